// The C++ mirror of the dense step with the semi-global path switched on (sfm::DenseOptions::sgm of sfm_ops.hpp) on a caller's views, for
// tests/test_sgm_gpu.py, which compares the file written here with Python's arrays.
//   sgm_test in.bin out.bin
// in.bin:  int32 n_img, rows, cols, channels, n_src, planes, radius, min_sources, min_consistent, P1, P2, paths, max_cost; double wmin,
//          wmax, rel_tol, cost_scale; double K4[4]; double ext[n_img][6]; the images
// out.bin: int32 n; double xyz[n][3]; uint8 bgr[n][3]
#include <cstdio>
#include <vector>

#include "../../sfm_opencv_amd/host/sfm_ops.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[13];
    double p[4], K4[4];
    if (fread(h, 4, 13, f) != 13 || fread(p, 8, 4, f) != 4 || fread(K4, 8, 4, f) != 4) return 2;
    const int n_img = h[0], rows = h[1], cols = h[2], channels = h[3];
    sfm::Mat intrinsic(4, 1, sfm::CV_64F);
    for (int i = 0; i < 4; ++i) intrinsic.at<double>(i) = K4[i];
    std::vector<sfm::Mat> ext(n_img, sfm::Mat(6, 1, sfm::CV_64F));
    for (int i = 0; i < n_img; ++i)
        if (fread(ext[i].ptr<double>(), 8, 6, f) != 6) return 2;
    const size_t bytes = (size_t)rows * cols * channels;
    std::vector<std::vector<uint8_t>> img(n_img, std::vector<uint8_t>(bytes));
    std::vector<const uint8_t*> images;
    for (int i = 0; i < n_img; ++i) {
        if (fread(img[i].data(), 1, bytes, f) != bytes) return 2;
        images.push_back(img[i].data());
    }
    fclose(f);
    sfm::DenseOptions opt;
    if (opt.sgm) return 3;                                               // the default is the winner per pixel
    opt.n_src = h[4]; opt.planes = h[5]; opt.radius = h[6]; opt.min_sources = h[7]; opt.min_consistent = h[8];
    opt.sgm = true; opt.sgm_P1 = h[9]; opt.sgm_P2 = h[10]; opt.sgm_paths = h[11]; opt.sgm_max_cost = h[12];
    opt.wmin = p[0]; opt.wmax = p[1]; opt.rel_tol = p[2]; opt.sgm_cost_scale = p[3];
    std::vector<sfm::Point3d> pts;
    std::vector<sfm::Vec3b> colors;
    const int n = sfm::dense_cloud_for_all(images, rows, cols, channels, intrinsic, ext, {}, opt, pts, colors);
    if (n < 0) return 1;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t n32 = n;
    fwrite(&n32, 4, 1, o);
    if (n) { fwrite(&pts[0].x, 24, n, o); fwrite(&colors[0].v[0], 3, n, o); }
    fclose(o);
    printf("dense cloud (sgm): %d points\n", n);
    return 0;
}
