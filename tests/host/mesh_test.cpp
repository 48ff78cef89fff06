// The C++ mirror of the mesh clean-up (sfm::clean_mesh and sfm::write_mesh_ply of sfm_ops.hpp) on a caller's mesh, for
// tests/test_mesh_gpu.py, which compares the file written here with the bytes of Python's writer.
//   mesh_test in.bin out.ply
// in.bin:  int32 nv, nt, min_component, keep_largest, iterations, normals; double cell, lambda, mu; double xyz[nv][3]; uint8 bgr[nv][3];
//          int32 tri[nt][3]
#include <cstdio>
#include <vector>

#include "../../sfm_opencv_amd/host/sfm_ops.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[6];
    double p[3];
    if (fread(h, 4, 6, f) != 6 || fread(p, 8, 3, f) != 3 || h[0] < 0 || h[1] < 0) return 2;
    const size_t nv = (size_t)h[0], nt = (size_t)h[1];
    std::vector<sfm::Point3d> pts(nv), normals;
    std::vector<sfm::Vec3b> colors(nv);
    std::vector<int32_t> tris(nt * 3);
    if (nv && (fread(&pts[0].x, 24, nv, f) != nv || fread(&colors[0].v[0], 3, nv, f) != nv)) return 2;
    if (nt && fread(tris.data(), 12, nt, f) != nt) return 2;
    fclose(f);
    const int n = sfm::clean_mesh(pts, colors, tris, h[2], h[3] != 0, p[0], h[4], p[1], p[2], h[5] ? &normals : nullptr);
    if (n < 0) return 1;
    sfm::write_mesh_ply(argv[2], pts, colors, tris, h[5] ? &normals : nullptr);
    printf("clean mesh: %zu vertices, %d triangles\n", pts.size(), n);
    return 0;
}
