// The C++ mirror of the track builder (sfm::build_tracks_for_all of sfm_ops.hpp) on a caller's key points and match lists, for
// tests/test_tracks_gpu.py, which compares the file written here with Python's arrays.
//   tracks_test in.bin out.bin
// in.bin:  int32 n_img, n_pairs, min_len, keep_first; int32 n_kp[n_img]; sfm_keypoint kp[sum n_kp]; int32 pairs[n_pairs][2];
//          int32 counts[n_pairs]; then every pair's sfm_dmatch list
// out.bin: int32 stats[8]; int32 track_of[sum n_kp]; int32 obs_cam[n_obs], obs_pt[n_obs], obs_kp[n_obs]; double obs_uv[n_obs][2];
//          int32 track_len[n_tracks]; int32 counts_out[n_pairs]; then every pair's filtered list
#include <cstdio>
#include <vector>

#include "../../sfm_opencv_amd/host/sfm_ops.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[4];
    if (fread(h, 4, 4, f) != 4) return 2;
    const int n_img = h[0], n_pairs = h[1];
    if (n_img < 0 || n_pairs < 0) return 2;
    std::vector<int32_t> n_kp(n_img), pr(2 * (size_t)n_pairs), counts(n_pairs);
    if (n_img && fread(n_kp.data(), 4, n_img, f) != (size_t)n_img) return 2;
    std::vector<std::vector<sfm::KeyPoint>> kp(n_img);
    for (int i = 0; i < n_img; ++i) {
        if (n_kp[i] < 0) return 2;
        kp[i].resize(n_kp[i]);
        if (n_kp[i] && fread(kp[i].data(), sizeof(sfm::KeyPoint), n_kp[i], f) != (size_t)n_kp[i]) return 2;
    }
    if (n_pairs && (fread(pr.data(), 8, n_pairs, f) != (size_t)n_pairs || fread(counts.data(), 4, n_pairs, f) != (size_t)n_pairs)) return 2;
    std::vector<std::pair<int, int>> pairs(n_pairs);
    std::vector<std::vector<sfm::DMatch>> lists(n_pairs);
    for (int q = 0; q < n_pairs; ++q) {
        if (counts[q] < 0) return 2;
        pairs[q] = { pr[2 * q], pr[2 * q + 1] };
        lists[q].resize(counts[q]);
        if (counts[q] && fread(lists[q].data(), sizeof(sfm::DMatch), counts[q], f) != (size_t)counts[q]) return 2;
    }
    fclose(f);
    sfm::Tracks t;
    if (!sfm::build_tracks_for_all(kp, pairs, lists, h[2], h[3] != 0, t)) return 1;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(t.stats, 4, 8, o);
    for (const auto& idx : t.correspond_struct_idx) fwrite(idx.data(), 4, idx.size(), o);
    fwrite(t.obs_cam.data(), 4, t.obs_cam.size(), o); fwrite(t.obs_pt.data(), 4, t.obs_pt.size(), o); fwrite(t.obs_kp.data(), 4, t.obs_kp.size(), o);
    fwrite(t.obs_uv.data(), 8, t.obs_uv.size(), o); fwrite(t.track_len.data(), 4, t.track_len.size(), o);
    for (const auto& m : t.matches_for_all) { const int32_t c = (int32_t)m.size(); fwrite(&c, 4, 1, o); }
    for (const auto& m : t.matches_for_all) fwrite(m.data(), sizeof(sfm::DMatch), m.size(), o);
    fclose(o);
    printf("tracks: %d of length >= %d over %d observations\n", t.stats[0], h[2], t.stats[1]);
    return 0;
}
