// The C++ mirror of the view selection (sfm::select_views of sfm_ops.hpp) on a caller's sparse model, for tests/test_select_gpu.py, which
// compares the file written here with Python's arrays.
//   select_test in.bin out.bin
// in.bin:  int32 n_views, n_pt, n_obs, n_src; double min_angle_deg; double ext[n_views][6]; double pts[n_pt][3]; int32 obs_cam[n_obs];
//          int32 obs_pt[n_obs]
// out.bin: int32 shared[n_views][n_views], score[n_views][n_views], sources[n_views][n_src], n_scored[n_views]; double wrange[n_views][2];
//          int32 n_depth[n_views]
#include <cstdio>
#include <vector>

#include "../../sfm_opencv_amd/host/sfm_ops.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[4];
    double deg;
    if (fread(h, 4, 4, f) != 4 || fread(&deg, 8, 1, f) != 1) return 2;
    const int n_views = h[0], n_pt = h[1], n_obs = h[2], n_src = h[3];
    if (n_views < 0 || n_pt < 0 || n_obs < 0) return 2;
    std::vector<sfm::Mat> ext(n_views, sfm::Mat(6, 1, sfm::CV_64F));
    for (int i = 0; i < n_views; ++i)
        if (fread(ext[i].ptr<double>(), 8, 6, f) != 6) return 2;
    std::vector<sfm::Point3d> pts(n_pt);
    if (n_pt && fread(&pts[0].x, 24, n_pt, f) != (size_t)n_pt) return 2;
    std::vector<int32_t> obs_cam(n_obs), obs_pt(n_obs);
    if (n_obs && (fread(obs_cam.data(), 4, n_obs, f) != (size_t)n_obs || fread(obs_pt.data(), 4, n_obs, f) != (size_t)n_obs)) return 2;
    fclose(f);
    sfm::SelectedViews sel;
    if (!sfm::select_views(ext, pts, obs_cam, obs_pt, n_src, deg, sel)) return 1;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(sel.shared.data(), 4, sel.shared.size(), o); fwrite(sel.score.data(), 4, sel.score.size(), o); fwrite(sel.sources.data(), 4, sel.sources.size(), o);
    fwrite(sel.n_scored.data(), 4, sel.n_scored.size(), o); fwrite(sel.wrange.data(), 8, sel.wrange.size(), o); fwrite(sel.n_depth.data(), 4, sel.n_depth.size(), o);
    fclose(o);
    printf("select_views: %d views, %d sources each\n", sel.n_views, sel.n_src);
    return 0;
}
