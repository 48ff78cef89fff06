// The C++ mirror of the dense mesh (sfm::dense_mesh_for_all and sfm::write_mesh_ply of sfm_ops.hpp) on a caller's views, for
// tests/test_tsdf_gpu.py, which compares the file written here with the bytes of Python's writer.
//   tsdf_test in.bin out.ply
// in.bin:  int32 n_img, rows, cols, channels, n_src, planes, radius, min_sources, min_consistent, n_sparse; double wmin, wmax, min_score,
//          rel_tol, voxel (unused); int32 dims[3], min_weight, voxels; double origin[3], voxel (0: the volume comes from the sparse points
//          and `voxels`), trunc_voxels; double K4[4]; double ext[n_img][6]; double sparse[n_sparse][3]; the images
#include <cstdio>
#include <vector>

#include "../../sfm_opencv_amd/host/sfm_ops.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[10], m[5];
    double p[5], q[5], K4[4];
    if (fread(h, 4, 10, f) != 10 || fread(p, 8, 5, f) != 5 || fread(m, 4, 5, f) != 5 || fread(q, 8, 5, f) != 5 || fread(K4, 8, 4, f) != 4) return 2;
    const int n_img = h[0], rows = h[1], cols = h[2], channels = h[3], n_sparse = h[9];
    sfm::Mat intrinsic(4, 1, sfm::CV_64F);
    for (int i = 0; i < 4; ++i) intrinsic.at<double>(i) = K4[i];
    std::vector<sfm::Mat> ext(n_img, sfm::Mat(6, 1, sfm::CV_64F));
    for (int i = 0; i < n_img; ++i)
        if (fread(ext[i].ptr<double>(), 8, 6, f) != 6) return 2;
    std::vector<sfm::Point3d> sparse(n_sparse);
    if (n_sparse && fread(&sparse[0].x, 24, n_sparse, f) != (size_t)n_sparse) return 2;
    const size_t bytes = (size_t)rows * cols * channels;
    std::vector<std::vector<uint8_t>> img(n_img, std::vector<uint8_t>(bytes));
    std::vector<const uint8_t*> images;
    for (int i = 0; i < n_img; ++i) {
        if (fread(img[i].data(), 1, bytes, f) != bytes) return 2;
        images.push_back(img[i].data());
    }
    fclose(f);
    sfm::DenseOptions opt;
    opt.n_src = h[4]; opt.planes = h[5]; opt.radius = h[6]; opt.min_sources = h[7]; opt.min_consistent = h[8];
    opt.wmin = p[0]; opt.wmax = p[1]; opt.min_score = p[2]; opt.rel_tol = p[3];
    for (int a = 0; a < 3; ++a) { opt.mesh_dims[a] = m[a]; opt.mesh_origin[a] = q[a]; }
    opt.mesh_min_weight = m[3]; opt.mesh_voxel = q[3]; opt.mesh_trunc_voxels = q[4];
    if (m[4] > 0) opt.mesh_voxels = m[4];
    std::vector<sfm::Point3d> pts;
    std::vector<sfm::Vec3b> colors;
    std::vector<int32_t> tris;
    const int n = sfm::dense_mesh_for_all(images, rows, cols, channels, intrinsic, ext, sparse, opt, pts, colors, tris);
    if (n < 0) return 1;
    sfm::write_mesh_ply(argv[2], pts, colors, tris);
    printf("dense mesh: %zu vertices, %d triangles\n", pts.size(), n);
    return 0;
}
