// The C++ mirror of the dense step (sfm::dense_cloud_for_all of sfm_ops.hpp) on a caller's views, for tests/test_dense_gpu.py, which
// compares the file written here with Python's arrays; "range" only prints sfm::dense_depth_range of the first view (no GPU call).
//   dense_test cloud|range in.bin out.bin
// in.bin:  int32 n_img, rows, cols, channels, n_src, planes, radius, min_sources, min_consistent, n_sparse; double wmin, wmax, min_score,
//          rel_tol, voxel; double K4[4]; double ext[n_img][6]; double sparse[n_sparse][3]; the images
// out.bin: cloud: int32 n; double xyz[n][3]; uint8 bgr[n][3]        range: double wmin, wmax
#include <cstdio>
#include <vector>

#include "../../sfm_opencv_amd/host/sfm_ops.hpp"

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const std::string mode = argv[1];
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    int32_t h[10];
    double p[5], K4[4];
    if (fread(h, 4, 10, f) != 10 || fread(p, 8, 5, f) != 5 || fread(K4, 8, 4, f) != 4) return 2;
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
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 2;
    if (mode == "range") {
        double w[2] = { 0.0, 0.0 };
        if (!sfm::dense_depth_range(sparse, ext[0].ptr<double>(), w[0], w[1])) return 1;
        fwrite(w, 8, 2, o);
        fclose(o);
        return 0;
    }
    sfm::DenseOptions opt;
    opt.n_src = h[4]; opt.planes = h[5]; opt.radius = h[6]; opt.min_sources = h[7]; opt.min_consistent = h[8];
    opt.wmin = p[0]; opt.wmax = p[1]; opt.min_score = p[2]; opt.rel_tol = p[3]; opt.voxel = p[4];
    std::vector<sfm::Point3d> pts;
    std::vector<sfm::Vec3b> colors;
    const int n = sfm::dense_cloud_for_all(images, rows, cols, channels, intrinsic, ext, sparse, opt, pts, colors);
    if (n < 0) return 1;
    const int32_t n32 = n;
    fwrite(&n32, 4, 1, o);
    if (n) { fwrite(&pts[0].x, 24, n, o); fwrite(&colors[0].v[0], 3, n, o); }
    fclose(o);
    printf("dense cloud: %d points\n", n);
    return 0;
}
