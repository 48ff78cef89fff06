// sfm_ops.hpp -- host-side mirror of the reference's hot-path interface (header-only C++17, no OpenCV).
//
// The reference (OpenCV_SFM/NViewReconstuct.cpp, "NView") has no plugin API: its boundary is the free functions
// declared at NView:35-138.  This header gives the same function names, argument order and error behaviour on POD
// mirrors of the OpenCV types, implemented over the C-ABI of libsfmhip.so (include/sfmhip.h).  A maintainer of the
// reference keeps his cv:: types and uses the shims shown in INTEGRATION.md; code without OpenCV uses this header.
#pragma once
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/sfmhip.h"

namespace sfm {

// ---- POD mirrors (layouts identical to the cv:: types they replace) ------------------------------------------
struct Point2f { float x = 0, y = 0; };
struct Point2d { double x = 0, y = 0; };
struct Point3f { float x = 0, y = 0, z = 0; };
struct Point3d { double x = 0, y = 0, z = 0; Point3d() = default; Point3d(double a, double b, double c) : x(a), y(b), z(c) {}
                 Point3d(const Point3f& p) : x(p.x), y(p.y), z(p.z) {} };
struct Vec3b { uint8_t v[3] = { 0, 0, 0 }; uint8_t& operator[](int i) { return v[i]; } const uint8_t& operator[](int i) const { return v[i]; } };
struct KeyPoint { Point2f pt; float size = 0, angle = -1, response = 0; int octave = 0, class_id = -1; };   // 28 bytes
struct DMatch { int queryIdx = -1, trainIdx = -1, imgIdx = -1; float distance = 0; };                          // 16 bytes
static_assert(sizeof(KeyPoint) == sizeof(sfm_keypoint) && sizeof(DMatch) == sizeof(sfm_dmatch), "layout");

enum { CV_8U = 0, CV_32F = 5, CV_64F = 6 };
// minimal row-major matrix: descriptors (CV_8U / CV_32F), 3x3 R, 3x1 T, 6x1 extrinsic, 4x1 intrinsic, 3x3 K (CV_64F)
struct Mat {
    int rows = 0, cols = 0, type = CV_64F;
    std::vector<uint8_t> buf;
    Mat() = default;
    Mat(int r, int c, int t) : rows(r), cols(c), type(t), buf((size_t)r * c * elem(t), 0) {}
    static size_t elem(int t) { return t == CV_8U ? 1 : (t == CV_32F ? 4 : 8); }
    bool empty() const { return rows == 0 || cols == 0; }
    template <typename T> T* ptr(int r = 0) { return reinterpret_cast<T*>(buf.data()) + (size_t)r * cols; }
    template <typename T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(buf.data()) + (size_t)r * cols; }
    template <typename T> T& at(int r, int c = 0) { return ptr<T>(r)[c]; }
    template <typename T> const T& at(int r, int c = 0) const { return ptr<T>(r)[c]; }
    static Mat eye3() { Mat m(3, 3, CV_64F); m.at<double>(0, 0) = m.at<double>(1, 1) = m.at<double>(2, 2) = 1.0; return m; }
};

struct Pt3DPly { float x = 0, y = 0, z = 0, nx = 0, ny = 0, nz = 0; uint8_t r = 0, g = 0, b = 0; };   // NView:21-32

// ---- context -------------------------------------------------------------------------------------------------
inline sfmhip_ctx* context(int device = 0)
{
    static sfmhip_ctx* ctx = nullptr;
    if (!ctx) {
        const int rc = sfmhip_create(device, &ctx);
        if (rc != SFMHIP_OK) { printf("[Err]: sfmhip_create failed (%d): no usable MI355X device, and there is no CPU fallback.\n", rc); ctx = nullptr; }
    }
    return ctx;
}

// Devices match_features_for_all() spreads its image pairs over (sfmhip_match_pairs_multi: contiguous blocks of the chain, every block
// uploaded over its own device's PCIe link, no exchange) and bundle_adjustment() its points (one context each; the reduced-system
// sums go over RCCL inside the library, sfmhip_ba_solve_multi).  Default: the one context above.  Listing a device twice gives two
// contexts on it: the one-card rehearsal.
inline std::vector<sfmhip_ctx*>& ba_contexts()
{
    static std::vector<sfmhip_ctx*> v;
    return v;
}
inline bool set_ba_devices(const std::vector<int>& devices)
{
    std::vector<sfmhip_ctx*>& v = ba_contexts();
    for (size_t i = 1; i < v.size(); ++i) sfmhip_destroy(v[i]);
    v.clear();
    for (size_t i = 0; i < devices.size(); ++i) {
        sfmhip_ctx* c = nullptr;
        if (i == 0) c = context(devices[0]);
        else if (sfmhip_create(devices[i], &c) != SFMHIP_OK) c = nullptr;
        if (!c) { printf("[Err]: no context on device %d\n", devices[i]); for (size_t k = 1; k < v.size(); ++k) sfmhip_destroy(v[k]); v.clear(); return false; }
        v.push_back(c);
    }
    return true;
}

// ---- matching (NView:873-913, 850-871) ---------------------------------------------------------------------------
// CV_8U rows -> NORM_HAMMING2 (the live configuration, NView:876); CV_32F rows -> NORM_L2 (TwoViewReconstruct.cpp:159)
inline void match_features(const Mat& query, const Mat& train, std::vector<DMatch>& matches, bool cross_check = false)
{
    if (cross_check) {          // the one pair through sfmhip_match_pairs_ex, which carries the flag (this context only, as below)
        matches.clear();
        sfmhip_ctx* c = context();
        if (!c || query.rows == 0) return;
        sfmhip_descset* sets[2] = { nullptr, nullptr };
        const Mat* m[2] = { &query, &train };
        int rc = SFMHIP_OK;
        for (int i = 0; i < 2 && rc == SFMHIP_OK; ++i)
            rc = m[i]->type == CV_8U ? sfmhip_descset_create_hamming2_host(c, m[i]->ptr<uint8_t>(), m[i]->rows, m[i]->cols, (size_t)m[i]->cols, &sets[i])
                                     : sfmhip_descset_create_l2_host(c, m[i]->ptr<float>(), m[i]->rows, m[i]->cols, (size_t)m[i]->cols, &sets[i]);
        std::vector<DMatch> out((size_t)query.rows);
        const int32_t pr[2] = { 0, 1 };
        int32_t cnt = 0;
        if (rc == SFMHIP_OK)
            rc = sfmhip_match_pairs_ex(c, sets, 2, pr, 1, 0.6, 10.0f, 5.0f, SFMHIP_MATCH_MUTUAL, reinterpret_cast<sfm_dmatch*>(out.data()), query.rows, &cnt);
        for (auto* s : sets) sfmhip_descset_destroy(s);
        if (rc != SFMHIP_OK) { printf("[Err]: match_features: %s\n", sfmhip_last_error(c)); return; }
        out.resize((size_t)cnt);
        matches.swap(out);
        return;
    }
    matches.clear();
    sfmhip_ctx* ctx = context();
    if (!ctx || query.rows == 0) return;
    std::vector<DMatch> out((size_t)query.rows);
    int n = 0, rc;
    if (query.type == CV_8U)
        rc = sfmhip_match_features_hamming2(ctx, query.ptr<uint8_t>(), query.rows, train.ptr<uint8_t>(), train.rows, query.cols,
                                            (size_t)query.cols, (size_t)train.cols, reinterpret_cast<sfm_dmatch*>(out.data()), &n);
    else
        rc = sfmhip_match_features_l2(ctx, query.ptr<float>(), query.rows, train.ptr<float>(), train.rows, query.cols,
                                      (size_t)query.cols, (size_t)train.cols, reinterpret_cast<sfm_dmatch*>(out.data()), &n);
    if (rc != SFMHIP_OK) { printf("[Err]: match_features: %s\n", sfmhip_last_error(ctx)); return; }
    out.resize((size_t)n);
    matches.swap(out);
}

// one batched launch sequence for the whole chain instead of N-1 serial calls.  cross_check: keep a match i -> j only if i is also
// the nearest query of j (SFMHIP_MATCH_MUTUAL; not in the reference, which runs the ratio test only)
inline void match_features_for_all(const std::vector<Mat>& descriptor_for_all, std::vector<std::vector<DMatch>>& matches_for_all, bool cross_check = false)
{
    const int flags = cross_check ? SFMHIP_MATCH_MUTUAL : 0;
    matches_for_all.clear();
    sfmhip_ctx* ctx = context();
    const int n = (int)descriptor_for_all.size();
    if (!ctx || n < 2) return;
    std::vector<sfmhip_descset*> sets((size_t)n, nullptr);
    int max_rows = 1, rc = SFMHIP_OK;
    // all images in one call (one pass of the staging threads, one transfer stream, one preparation launch) when they share a type
    // and a row length -- what extract_features produces; image by image otherwise
    bool uniform = true;
    for (int i = 0; i < n; ++i) {
        const Mat& d = descriptor_for_all[i];
        max_rows = d.rows > max_rows ? d.rows : max_rows;
        uniform = uniform && d.type == descriptor_for_all[0].type && d.cols == descriptor_for_all[0].cols && d.cols > 0;
    }
    if (uniform && ba_contexts().size() > 1) {
        // several devices (--gpus=): the chain in contiguous blocks over the contexts, host matrices straight into the one call
        std::vector<int32_t> rows((size_t)n), pairs, counts((size_t)n - 1, 0);
        std::vector<const void*> ptrs((size_t)n);
        for (int i = 0; i < n; ++i) { rows[i] = descriptor_for_all[i].rows; ptrs[i] = descriptor_for_all[i].buf.data(); }
        for (int i = 0; i + 1 < n; ++i) { printf("Matching images %d - %d\n", i, i + 1); pairs.push_back(i); pairs.push_back(i + 1); }
        std::vector<DMatch> out((size_t)(n - 1) * max_rows);
        const bool ham = descriptor_for_all[0].type == CV_8U;
        rc = sfmhip_match_pairs_multi_ex(ba_contexts().data(), (int)ba_contexts().size(), ham ? SFMHIP_DESC_HAMMING2_U8 : SFMHIP_DESC_L2_F32, ptrs.data(), rows.data(),
                                         descriptor_for_all[0].cols, nullptr, n, pairs.data(), n - 1, 0.6, 10.0f, 5.0f, flags,
                                         reinterpret_cast<sfm_dmatch*>(out.data()), max_rows, counts.data());
        if (rc != SFMHIP_OK) { printf("[Err]: match_features_for_all: %s\n", sfmhip_last_error(ctx)); return; }
        for (int i = 0; i + 1 < n; ++i) {
            matches_for_all.emplace_back(out.begin() + (size_t)i * max_rows, out.begin() + (size_t)i * max_rows + counts[i]);
            if (counts[i] == 0) printf("[Warning]: zero matches between %d and %d.\n", i, i + 1);
        }
        return;
    }
    if (uniform) {
        std::vector<int32_t> rows((size_t)n);
        for (int i = 0; i < n; ++i) rows[i] = descriptor_for_all[i].rows;
        if (descriptor_for_all[0].type == CV_8U) {
            std::vector<const uint8_t*> ptrs((size_t)n);
            for (int i = 0; i < n; ++i) ptrs[i] = descriptor_for_all[i].ptr<uint8_t>();
            rc = sfmhip_descsets_create_hamming2_host(ctx, ptrs.data(), rows.data(), descriptor_for_all[0].cols, nullptr, n, sets.data());
        } else {
            std::vector<const float*> ptrs((size_t)n);
            for (int i = 0; i < n; ++i) ptrs[i] = descriptor_for_all[i].ptr<float>();
            rc = sfmhip_descsets_create_l2_host(ctx, ptrs.data(), rows.data(), descriptor_for_all[0].cols, nullptr, n, sets.data());
        }
    } else {
        for (int i = 0; i < n && rc == SFMHIP_OK; ++i) {
            const Mat& d = descriptor_for_all[i];
            rc = d.type == CV_8U ? sfmhip_descset_create_hamming2_host(ctx, d.ptr<uint8_t>(), d.rows, d.cols, (size_t)d.cols, &sets[i])
                                 : sfmhip_descset_create_l2_host(ctx, d.ptr<float>(), d.rows, d.cols, (size_t)d.cols, &sets[i]);
        }
    }
    std::vector<int32_t> pairs, counts((size_t)n - 1, 0);
    for (int i = 0; i + 1 < n; ++i) { printf("Matching images %d - %d\n", i, i + 1); pairs.push_back(i); pairs.push_back(i + 1); }
    std::vector<DMatch> out((size_t)(n - 1) * max_rows);
    if (rc == SFMHIP_OK)
        rc = sfmhip_match_pairs_ex(ctx, sets.data(), n, pairs.data(), n - 1, 0.6, 10.0f, 5.0f, flags,
                                   reinterpret_cast<sfm_dmatch*>(out.data()), max_rows, counts.data());
    for (auto* s : sets) sfmhip_descset_destroy(s);
    if (rc != SFMHIP_OK) { printf("[Err]: match_features_for_all: %s\n", sfmhip_last_error(ctx)); return; }
    for (int i = 0; i + 1 < n; ++i) {
        matches_for_all.emplace_back(out.begin() + (size_t)i * max_rows, out.begin() + (size_t)i * max_rows + counts[i]);
        if (counts[i] == 0) printf("[Warning]: zero matches between %d and %d.\n", i, i + 1);
    }
}

// the rows (x1, y1, x2, y2) of every pair's matches on coordinates normalised by K, in blocks of `stride` rows (the longest list)
inline void pair_rows_for_all(const Mat& K, const std::vector<std::vector<KeyPoint>>& key_points_for_all,
                              const std::vector<std::vector<DMatch>>& matches_for_all, std::vector<double>& corr, std::vector<int32_t>& rows, size_t& stride)
{
    const size_t n_pairs = matches_for_all.size();
    const double fx = K.at<double>(0, 0), fy = K.at<double>(1, 1), cx = K.at<double>(0, 2), cy = K.at<double>(1, 2);
    stride = 0;
    for (const auto& m : matches_for_all) stride = m.size() > stride ? m.size() : stride;
    corr.assign(n_pairs * stride * 4, 0.0);
    rows.assign(n_pairs, 0);
    for (size_t i = 0; i < n_pairs; ++i) {
        const auto& m = matches_for_all[i];
        rows[i] = (int32_t)m.size();
        double* r = corr.data() + i * stride * 4;
        for (size_t k = 0; k < m.size(); ++k, r += 4) {
            const KeyPoint& a = key_points_for_all[i][(size_t)m[k].queryIdx];
            const KeyPoint& b = key_points_for_all[i + 1][(size_t)m[k].trainIdx];
            r[0] = ((double)a.pt.x - cx) / fx; r[1] = ((double)a.pt.y - cy) / fy;
            r[2] = ((double)b.pt.x - cx) / fx; r[3] = ((double)b.pt.y - cy) / fy;
        }
    }
}
// the elements of m whose flag is set, in their order
inline void keep_masked(std::vector<DMatch>& m, const uint8_t* keep)
{
    size_t w = 0;
    for (size_t k = 0; k < m.size(); ++k)
        if (keep[k]) m[w++] = m[k];
    m.resize(w);
}

// ---- two-view geometric verification (extension; what colmap / OpenMVG run between matching and reconstruction; the reference rejects
// epipolar outliers for its first pair only, inside findEssentialMat, NView:1032) -- matches_for_all[i] joins images i and i + 1.  The key
// points are normalised by K, the threshold is px pixels (t = px / (0.5 (fx + fy))), all pairs run in one call of sfmhip_verify_pairs
// (where the definition is).  A pair whose model keeps at least min_inliers matches is replaced by the kept ones, in their order; any
// other pair keeps its matches as they are, with a warning, so the chain cannot break.  counts[i] = the matches kept by the model of
// pair i (0: none); F (may be null): 9 doubles per pair on normalised coordinates, NaN where there is no model.  Returns 0, -1 on error.
inline int verify_matches_for_all(const Mat& K, const std::vector<std::vector<KeyPoint>>& key_points_for_all,
                                  std::vector<std::vector<DMatch>>& matches_for_all, std::vector<int32_t>& counts, const double px = 1.0,
                                  const int hypotheses = 1024, const int rounds = 3, const int min_inliers = 15, const uint64_t seed = 0,
                                  std::vector<double>* F = nullptr)
{
    const int n_pairs = (int)matches_for_all.size();
    counts.assign((size_t)n_pairs, 0);
    if (F) F->assign((size_t)n_pairs * 9, std::nan(""));
    sfmhip_ctx* ctx = context();
    if (!ctx || (int)key_points_for_all.size() < n_pairs + 1) return -1;
    if (n_pairs == 0) return 0;
    const double fx = K.at<double>(0, 0), fy = K.at<double>(1, 1);
    size_t stride = 0;
    std::vector<double> corr;
    std::vector<int32_t> rows;
    pair_rows_for_all(K, key_points_for_all, matches_for_all, corr, rows, stride);
    std::vector<uint8_t> mask((size_t)n_pairs * stride, 0);
    if (sfmhip_verify_pairs(ctx, corr.data(), (int)stride, rows.data(), n_pairs, px / (0.5 * (fx + fy)), hypotheses, rounds, seed, min_inliers, mask.data(),
                            counts.data(), F ? F->data() : nullptr, nullptr) != SFMHIP_OK) {
        printf("[Err]: verify_matches_for_all: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    for (int i = 0; i < n_pairs; ++i) {
        auto& m = matches_for_all[(size_t)i];
        if (counts[(size_t)i] == 0) {
            printf("[Warning]: pair %d: no epipolar model with %d matches, the %zu matches are kept as they are.\n", i, min_inliers, m.size());
            continue;
        }
        keep_masked(m, mask.data() + (size_t)i * stride);
    }
    return 0;
}

// ---- the same with a homography RANSAC beside the epipolar one and the F/H selection of sfmhip_two_view_geometry (where the definition
// is): px pixels for F, px_h pixels for the homography (a transfer distance carries the noise of both images).  kind[i]: 0 no model
// (the pair keeps its matches, with a warning), 1 general (the pair keeps F's inliers), 2 planar or panoramic (it keeps the
// homography's; its two-view pose is ill-determined and a warning says so).  counts[i]: the matches kept by the selected model;
// counts2: (cF, cH) per pair.  Returns 0, -1 on error.
inline int two_view_geometry_for_all(const Mat& K, const std::vector<std::vector<KeyPoint>>& key_points_for_all,
                                     std::vector<std::vector<DMatch>>& matches_for_all, std::vector<int32_t>& kind, std::vector<int32_t>& counts,
                                     std::vector<int32_t>& counts2, const double px = 1.0, const double px_h = 2.0, const int hypotheses = 1024,
                                     const int rounds = 3, const double hf_ratio = 0.8, const int min_inliers = 15, const uint64_t seed = 0,
                                     std::vector<double>* F = nullptr, std::vector<double>* Hm = nullptr)
{
    const int n_pairs = (int)matches_for_all.size();
    kind.assign((size_t)n_pairs, 0); counts.assign((size_t)n_pairs, 0); counts2.assign((size_t)n_pairs * 2, 0);
    if (F) F->assign((size_t)n_pairs * 9, std::nan(""));
    if (Hm) Hm->assign((size_t)n_pairs * 9, std::nan(""));
    sfmhip_ctx* ctx = context();
    if (!ctx || (int)key_points_for_all.size() < n_pairs + 1) return -1;
    if (n_pairs == 0) return 0;
    const double f = 0.5 * (K.at<double>(0, 0) + K.at<double>(1, 1));
    size_t stride = 0;
    std::vector<double> corr;
    std::vector<int32_t> rows;
    pair_rows_for_all(K, key_points_for_all, matches_for_all, corr, rows, stride);
    std::vector<uint8_t> mask((size_t)n_pairs * stride, 0);
    if (sfmhip_two_view_geometry(ctx, corr.data(), (int)stride, rows.data(), n_pairs, px / f, px_h / f, hypotheses, rounds, seed, min_inliers, hf_ratio,
                                 kind.data(), mask.data(), counts.data(), counts2.data(), F ? F->data() : nullptr, Hm ? Hm->data() : nullptr,
                                 nullptr) != SFMHIP_OK) {
        printf("[Err]: two_view_geometry_for_all: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    for (int i = 0; i < n_pairs; ++i) {
        auto& m = matches_for_all[(size_t)i];
        if (kind[(size_t)i] == 0) {
            printf("[Warning]: pair %d: no two-view model with %d matches, the %zu matches are kept as they are.\n", i, min_inliers, m.size());
            continue;
        }
        if (kind[(size_t)i] == 2)
            printf("[Warning]: pair %d: planar or panoramic (H explains %d matches, F %d): its two-view pose is ill-determined.\n", i,
                   (int)counts2[2 * (size_t)i + 1], (int)counts2[2 * (size_t)i]);
        keep_masked(m, mask.data() + (size_t)i * stride);
    }
    return 0;
}

// ---- find_transform (NView:1022-1060) for every consecutive pair on the device: two_view_geometry_for_all as above (the lists are
// filtered in the same way, kind / counts / counts2 mean the same), and then sfmhip_relative_pose (where the definition is) on the pairs of
// kind 1 with F's inlier mask and F, both calls over all pairs at once.  poses[i]: ok applies find_transform's own gates (more than 15
// inliers, n_front / n_inl >= 0.7) and requires kind 1; a pair of kind 0 or 2 is reported without a pose (reason says why).  kept is a
// flag per match of the list AS IT CAME IN, set for the final inliers in front of both cameras (bit 1 of mask_out), and matches those
// elements in their order: the re-taken set is usually larger than the RANSAC's.  Returns 0, -1 on error.
struct RelativePose {
    bool ok = false; const char* reason = ""; int kind = 0; Mat R, T;
    int cand = -1, n4[4] = { 0, 0, 0, 0 }, n_used = 0, n_inl = 0, n_front = 0, n_angle = 0;
    double sv[3] = { std::nan(""), std::nan(""), std::nan("") };
    std::vector<uint8_t> kept; std::vector<DMatch> matches;
};
inline int relative_pose_for_all(const Mat& K, const std::vector<std::vector<KeyPoint>>& key_points_for_all,
                                 std::vector<std::vector<DMatch>>& matches_for_all, std::vector<int32_t>& kind, std::vector<int32_t>& counts,
                                 std::vector<int32_t>& counts2, std::vector<RelativePose>& poses, const double px = 1.0, const double px_h = 2.0,
                                 const int hypotheses = 1024, const int rounds = 3, const double hf_ratio = 0.8, const int min_inliers = 15,
                                 const uint64_t seed = 0, const int pose_rounds = 3, const int pose_iters = 10, const double max_depth = 50.0,
                                 const double min_angle_deg = 2.0)
{
    const int n_pairs = (int)matches_for_all.size();
    kind.assign((size_t)n_pairs, 0); counts.assign((size_t)n_pairs, 0); counts2.assign((size_t)n_pairs * 2, 0);
    poses.assign((size_t)n_pairs, RelativePose());
    sfmhip_ctx* ctx = context();
    if (!ctx || (int)key_points_for_all.size() < n_pairs + 1) return -1;
    if (n_pairs == 0) return 0;
    const double f = 0.5 * (K.at<double>(0, 0) + K.at<double>(1, 1));
    size_t stride = 0;
    std::vector<double> corr, F((size_t)n_pairs * 9), pose((size_t)n_pairs * 12), quality((size_t)n_pairs * 5);
    std::vector<int32_t> rows, info((size_t)n_pairs * 10);
    pair_rows_for_all(K, key_points_for_all, matches_for_all, corr, rows, stride);
    std::vector<uint8_t> mask((size_t)n_pairs * stride, 0), mask_out((size_t)n_pairs * stride, 0);
    if (sfmhip_two_view_geometry(ctx, corr.data(), (int)stride, rows.data(), n_pairs, px / f, px_h / f, hypotheses, rounds, seed, min_inliers, hf_ratio,
                                 kind.data(), mask.data(), counts.data(), counts2.data(), F.data(), nullptr, nullptr) != SFMHIP_OK) {
        printf("[Err]: relative_pose_for_all: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    // a pair of another kind gets no pose: without rows it ends with status 0
    std::vector<int32_t> pose_rows(rows);
    for (int i = 0; i < n_pairs; ++i)
        if (kind[(size_t)i] != 1) pose_rows[(size_t)i] = 0;
    if (sfmhip_relative_pose(ctx, corr.data(), (int)stride, pose_rows.data(), n_pairs, mask.data(), F.data(), px / f, pose_rounds, pose_iters, max_depth,
                             min_angle_deg * 3.14159265358979323846 / 180.0, pose.data(), info.data(), quality.data(), mask_out.data()) != SFMHIP_OK) {
        printf("[Err]: relative_pose_for_all: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    for (int i = 0; i < n_pairs; ++i) {
        auto& m = matches_for_all[(size_t)i];
        RelativePose& p = poses[(size_t)i];
        const int32_t* in = &info[10 * (size_t)i];
        p.kind = kind[(size_t)i];
        p.kept.assign(m.size(), 0);
        if (p.kind != 1) p.reason = p.kind == 2 ? "planar or panoramic" : "no two-view model";
        else {
            p.cand = in[1]; p.n_used = in[6]; p.n_inl = in[7]; p.n_front = in[8]; p.n_angle = in[9];
            for (int k = 0; k < 4; ++k) p.n4[k] = in[2 + k];
            for (int k = 0; k < 3; ++k) p.sv[k] = quality[5 * (size_t)i + k];
            if (in[0] != 1) p.reason = "no candidate has a match in front";
            else {
                p.R = Mat(3, 3, CV_64F); p.T = Mat(3, 1, CV_64F);
                std::copy(&pose[12 * (size_t)i], &pose[12 * (size_t)i] + 9, p.R.ptr<double>());
                std::copy(&pose[12 * (size_t)i] + 9, &pose[12 * (size_t)i] + 12, p.T.ptr<double>());
                for (size_t k = 0; k < m.size(); ++k)
                    if (mask_out[(size_t)i * stride + k] & 2) { p.kept[k] = 1; p.matches.push_back(m[k]); }
                if (p.n_inl <= 15) p.reason = "15 inliers or fewer";
                else if ((double)p.n_front < 0.7 * (double)p.n_inl) p.reason = "fewer than 0.7 of the inliers in front";
                else p.ok = true;
            }
        }
        if (kind[(size_t)i] == 0) {
            printf("[Warning]: pair %d: no two-view model with %d matches, the %zu matches are kept as they are.\n", i, min_inliers, m.size());
            continue;
        }
        if (kind[(size_t)i] == 2)
            printf("[Warning]: pair %d: planar or panoramic (H explains %d matches, F %d): its two-view pose is ill-determined.\n", i,
                   (int)counts2[2 * (size_t)i + 1], (int)counts2[2 * (size_t)i]);
        keep_masked(m, mask.data() + (size_t)i * stride);
    }
    return 0;
}

inline void get_matched_points(const std::vector<KeyPoint>& p1, const std::vector<KeyPoint>& p2, const std::vector<DMatch> matches,
                               std::vector<Point2f>& out_p1, std::vector<Point2f>& out_p2)
{
    out_p1.clear(); out_p2.clear();
    for (const auto& m : matches) { out_p1.push_back(p1[m.queryIdx].pt); out_p2.push_back(p2[m.trainIdx].pt); }
}
inline void get_matched_colors(const std::vector<Vec3b>& c1, const std::vector<Vec3b>& c2, const std::vector<DMatch> matches,
                               std::vector<Vec3b>& out_c1, std::vector<Vec3b>& out_c2)
{
    out_c1.clear(); out_c2.clear();
    for (const auto& m : matches) { out_c1.push_back(c1[m.queryIdx]); out_c2.push_back(c2[m.trainIdx]); }
}

// ---- triangulation (NView:1117-1159) ---------------------------------------------------------------------------
// proj = float(K) * [float(R) | float(T)] as a float32 product with double accumulation (cv::gemm on CV_32F [3P])
inline void projection_matrix(const Mat& K, const Mat& R, const Mat& T, float P[12])
{
    float fK[9], RT[12];
    for (int i = 0; i < 9; ++i) fK[i] = (float)K.ptr<double>()[i];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) RT[4 * r + c] = (float)R.at<double>(r, c); RT[4 * r + 3] = (float)T.at<double>(r, 0); }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += (double)fK[3 * r + k] * (double)RT[4 * k + c];
            P[4 * r + c] = (float)s;
        }
}

inline int reconstruct(const Mat& K, Mat& R1, Mat& T1, Mat& R2, Mat& T2, std::vector<Point2f>& pts2d_1, std::vector<Point2f>& pts2d_2,
                       std::vector<Point3d>& structure)
{
    if (pts2d_1.size() == 0 || pts2d_2.size() == 0) { printf("[Err]: empty 2d points.\n"); return -1; }
    sfmhip_ctx* ctx = context();
    if (!ctx) return -1;
    float P1[12], P2[12];
    projection_matrix(K, R1, T1, P1); projection_matrix(K, R2, T2, P2);
    const int n = (int)pts2d_1.size();
    structure.clear(); structure.resize((size_t)n);
    const int rc = sfmhip_triangulate2_f32(ctx, P1, P2, &pts2d_1[0].x, &pts2d_2[0].x, n, nullptr, &structure[0].x);
    if (rc != SFMHIP_OK) { printf("[Err]: reconstruct: %s\n", sfmhip_last_error(ctx)); structure.clear(); return -1; }
    return 0;
}

// TwoViewReconstruct.cpp:231-250: first camera at the origin (proj1 = float(K) [I | 0]), second [R | T]; the result stays
// HOMOGENEOUS -- `structure` is the 4 x N CV_32F matrix cv::triangulatePoints fills (one column per point); the division
// by w happens when the file is written (TwoViewReconstruct.cpp:341-346).  void like the reference: errors only print.
inline void reconstruct(Mat& K, Mat& R, Mat& T, std::vector<Point2f>& p1, std::vector<Point2f>& p2, Mat& structure)
{
    const int n = (int)p1.size();
    structure = Mat(4, n, CV_32F);
    sfmhip_ctx* ctx = context();
    if (!ctx || n == 0 || p2.size() != p1.size()) { if (n == 0) structure = Mat(); return; }
    Mat R0 = Mat::eye3(), T0(3, 1, CV_64F);
    float P1[12], P2[12];
    projection_matrix(K, R0, T0, P1); projection_matrix(K, R, T, P2);
    const int rc = sfmhip_triangulate2_f32(ctx, P1, P2, &p1[0].x, &p2[0].x, n, structure.ptr<float>(), nullptr);
    if (rc != SFMHIP_OK) { printf("[Err]: reconstruct: %s\n", sfmhip_last_error(ctx)); structure = Mat(); }
}

// ---- track bookkeeping (host, integer; NView:959-983, 1246-1301) --------------------------------------------------
inline void init_correspondence(const std::vector<std::vector<KeyPoint>>& key_points_for_all, const std::vector<DMatch>& matches01,
                                const std::vector<uint8_t>& mask, std::vector<std::vector<int>>& correspond_struct_idx)
{
    correspond_struct_idx.clear();
    correspond_struct_idx.resize(key_points_for_all.size());
    for (size_t i = 0; i < key_points_for_all.size(); ++i) correspond_struct_idx[i].resize(key_points_for_all[i].size(), -1);
    int idx = 0;
    for (size_t i = 0; i < matches01.size(); ++i) {
        if (!mask.empty() && mask[i] == 0) continue;
        correspond_struct_idx[0][matches01[i].queryIdx] = idx;
        correspond_struct_idx[1][matches01[i].trainIdx] = idx;
        ++idx;
    }
    printf("Total %d 3D points from the first two frames' valid keypoint matches.\n", idx);
}
inline void get_obj_pts_and_img_pts(const std::vector<DMatch>& matches, const std::vector<int>& struct_indices,
                                    const std::vector<Point3d>& structure, const std::vector<KeyPoint>& key_points,
                                    std::vector<Point3f>& object_points, std::vector<Point2f>& image_points)
{
    object_points.clear(); image_points.clear();
    for (const auto& m : matches) {
        const int si = struct_indices[m.queryIdx];
        if (si < 0) continue;
        object_points.push_back(Point3f{ (float)structure[si].x, (float)structure[si].y, (float)structure[si].z });
        image_points.push_back(key_points[m.trainIdx].pt);
    }
}
inline void fuse_structure(const std::vector<DMatch>& matches, std::vector<int>& struct_indices, std::vector<int>& next_struct_indices,
                           std::vector<Point3d>& structure, std::vector<Point3d>& next_structure,
                           std::vector<Vec3b>& colors, std::vector<Vec3b>& next_colors)
{
    for (size_t i = 0; i < matches.size(); ++i) {
        const int q = matches[i].queryIdx, t = matches[i].trainIdx;
        const int si = struct_indices[q];
        if (si >= 0) { next_struct_indices[t] = si; continue; }
        structure.push_back(next_structure[i]);
        colors.push_back(next_colors[i]);
        struct_indices[q] = next_struct_indices[t] = (int)structure.size() - 1;
    }
}
inline void maskout_2d_pts_pair(const std::vector<uint8_t>& mask, std::vector<Point2f>& a, std::vector<Point2f>& b)
{
    std::vector<Point2f> ca = a, cb = b; a.clear(); b.clear();
    for (size_t i = 0; i < mask.size(); ++i) if (mask[i] > 0) { a.push_back(ca[i]); b.push_back(cb[i]); }
}
inline void maskout_colors(const std::vector<uint8_t>& mask, std::vector<Vec3b>& c)
{
    std::vector<Vec3b> cc = c; c.clear();
    for (size_t i = 0; i < mask.size(); ++i) if (mask[i] > 0) c.push_back(cc[i]);
}

// cv::Rodrigues 3x3 -> 3x1 (NView:1480) and back
inline void Rodrigues(const Mat& R, Mat& r)
{
    r = Mat(3, 1, CV_64F);
    const double* m = R.ptr<double>();
    double c = (m[0] + m[4] + m[8] - 1.0) * 0.5; c = c > 1 ? 1 : (c < -1 ? -1 : c);
    const double th = std::acos(c);
    double w[3] = { m[7] - m[5], m[2] - m[6], m[3] - m[1] };
    if (th < 1e-12) { for (int i = 0; i < 3; ++i) r.at<double>(i) = 0.5 * w[i]; return; }
    if (M_PI - th < 1e-6) {
        double A[3] = { (m[0] + 1) * 0.5, (m[4] + 1) * 0.5, (m[8] + 1) * 0.5 };
        int k = A[0] >= A[1] ? (A[0] >= A[2] ? 0 : 2) : (A[1] >= A[2] ? 1 : 2);
        double ax[3], d = std::sqrt(A[k] > 0 ? A[k] : 0);
        for (int i = 0; i < 3; ++i) ax[i] = ((m[3 * k + i] + (i == k ? 1.0 : 0.0)) * 0.5) / d;
        const double nn = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        for (int i = 0; i < 3; ++i) r.at<double>(i) = th * ax[i] / nn;
        return;
    }
    const double s = th / (2.0 * std::sin(th));
    for (int i = 0; i < 3; ++i) r.at<double>(i) = s * w[i];
}

// cv::Rodrigues 3x1 -> 3x3 (NView:1418): R = cos(th) I + (1 - cos(th)) r r' + sin(th) [r]x, r = v / |v| [3P]
inline void Rodrigues_vec(const Mat& rvec, Mat& R)
{
    R = Mat::eye3();
    const double x = rvec.at<double>(0), y = rvec.at<double>(1), z = rvec.at<double>(2);
    const double th = std::sqrt(x * x + y * y + z * z);
    if (th < 2.220446049250313e-16) return;
    const double c = std::cos(th), s = std::sin(th), c1 = 1.0 - c, rx = x / th, ry = y / th, rz = z / th;
    double* m = R.ptr<double>();
    m[0] = c + c1 * rx * rx;       m[1] = c1 * rx * ry - s * rz;  m[2] = c1 * rx * rz + s * ry;
    m[3] = c1 * rx * ry + s * rz;  m[4] = c + c1 * ry * ry;       m[5] = c1 * ry * rz - s * rx;
    m[6] = c1 * rx * rz - s * ry;  m[7] = c1 * ry * rz + s * rx;  m[8] = c + c1 * rz * rz;
}

// ---- image registration (cv::solvePnPRansac, NView:1415) for many views in one call of sfmhip_register_views (where the definition is):
// obj_pts_list[q] / img_pts_list[q] are the structure points and their pixel observations in view q.  The observations are normalised
// by K, the threshold is px pixels, the pose comes out of the winning P (sfmhip_pose_from_projection) and is polished on the inliers by
// the motion-only bundle adjustment: one camera, every point constant, intrinsics fixed.  A view is not ok -- reason says why, the mask
// and count are still reported -- where no model reaches min_inliers, P is no rotation, or sv_ratio exceeds sv_ratio_max (coplanar
// points: the DLT's P is not a pose there; the measured ranges are in DESIGN.md 4c).  Returns 0, -1 on error.
struct RegisteredView { bool ok = false; const char* reason = ""; Mat R, T; std::vector<uint8_t> mask; int count = 0; double sv_ratio = std::nan(""); };
inline int register_views_for_all(const Mat& K, const std::vector<std::vector<Point3f>>& obj_pts_list, const std::vector<std::vector<Point2f>>& img_pts_list,
                                  std::vector<RegisteredView>& views, const double px = 2.0, const int hypotheses = 1024, const int rounds = 3,
                                  const int min_inliers = 6, const uint64_t seed = 0, const double sv_ratio_max = 2.0)
{
    const int n = (int)obj_pts_list.size();
    views.assign((size_t)n, RegisteredView());
    sfmhip_ctx* ctx = context();
    if (!ctx || img_pts_list.size() != obj_pts_list.size()) return -1;
    if (n == 0) return 0;
    const double fx = K.at<double>(0, 0), fy = K.at<double>(1, 1), cx = K.at<double>(0, 2), cy = K.at<double>(1, 2);
    size_t stride = 0;
    for (int q = 0; q < n; ++q) {
        if (obj_pts_list[(size_t)q].size() != img_pts_list[(size_t)q].size()) return -1;
        stride = std::max(stride, obj_pts_list[(size_t)q].size());
    }
    std::vector<double> corr((size_t)n * stride * 5, 0.0), P((size_t)n * 12);
    std::vector<int32_t> rows((size_t)n), counts((size_t)n);
    std::vector<uint8_t> mask((size_t)n * stride, 0);
    for (int q = 0; q < n; ++q) {
        const auto& X = obj_pts_list[(size_t)q]; const auto& x = img_pts_list[(size_t)q];
        rows[(size_t)q] = (int32_t)X.size();
        double* r = corr.data() + (size_t)q * stride * 5;
        for (size_t k = 0; k < X.size(); ++k, r += 5) {
            r[0] = X[k].x; r[1] = X[k].y; r[2] = X[k].z; r[3] = ((double)x[k].x - cx) / fx; r[4] = ((double)x[k].y - cy) / fy;
        }
    }
    if (sfmhip_register_views(ctx, corr.data(), (int)stride, rows.data(), n, px / (0.5 * (fx + fy)), hypotheses, rounds, seed, min_inliers, mask.data(),
                              counts.data(), P.data(), nullptr) != SFMHIP_OK) {
        printf("[Err]: register_views_for_all: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    for (int q = 0; q < n; ++q) {
        RegisteredView& v = views[(size_t)q];
        const size_t m = (size_t)rows[(size_t)q];
        v.mask.assign(mask.begin() + (size_t)q * stride, mask.begin() + (size_t)q * stride + m);
        v.count = counts[(size_t)q];
        if (v.count == 0) { v.reason = "no model"; continue; }
        double R[9], t[3];
        const int rc = sfmhip_pose_from_projection(&P[12 * (size_t)q], R, t, &v.sv_ratio);
        if (rc == SFMHIP_OK && !(v.sv_ratio <= sv_ratio_max)) { v.reason = "coplanar points"; continue; }
        if (rc != SFMHIP_OK) { v.reason = v.sv_ratio > sv_ratio_max ? "coplanar points" : "no rotation"; continue; }
        v.R = Mat(3, 3, CV_64F); v.T = Mat(3, 1, CV_64F);
        std::copy(R, R + 9, v.R.ptr<double>());
        for (int a = 0; a < 3; ++a) v.T.at<double>(a) = t[a];
        v.ok = true;
        // the refinement: sfmhip_ba_solve_ex over the inliers with the points constant
        Mat rvec;
        Rodrigues(v.R, rvec);
        double K4[4] = { fx, fy, cx, cy }, ext[6] = { rvec.at<double>(0), rvec.at<double>(1), rvec.at<double>(2), t[0], t[1], t[2] };
        std::vector<double> pts, uv;
        std::vector<int32_t> oc, op;
        for (size_t k = 0; k < m; ++k)
            if (v.mask[k]) {
                const Point3f& X = obj_pts_list[(size_t)q][k]; const Point2f& x = img_pts_list[(size_t)q][k];
                op.push_back((int32_t)oc.size()); oc.push_back(0);
                pts.push_back(X.x); pts.push_back(X.y); pts.push_back(X.z); uv.push_back(x.x); uv.push_back(x.y);
            }
        const std::vector<uint8_t> cam_const(1, 0), pt_const(oc.size(), 1);
        sfm_ba_options o; sfmhip_ba_default_options(&o);
        o.fix_first_camera = 0; o.fix_intrinsics = 1;
        sfm_ba_summary s; std::memset(&s, 0, sizeof s);
        if (sfmhip_ba_solve_ex(ctx, K4, ext, 1, pts.data(), (int)oc.size(), oc.data(), op.data(), uv.data(), (int)oc.size(), cam_const.data(), pt_const.data(),
                               &o, &s) == SFMHIP_OK && s.termination != SFMHIP_BA_FAILURE && std::isfinite(ext[0] + ext[1] + ext[2] + ext[3] + ext[4] + ext[5])) {
            for (int a = 0; a < 3; ++a) { rvec.at<double>(a) = ext[a]; v.T.at<double>(a) = ext[3 + a]; }
            Rodrigues_vec(rvec, v.R);
        }
    }
    return 0;
}

// ---- bundle adjustment (NView:1162-1244): in place on intrinsic (4x1), extrinsics (6x1 each), structure -----------
// const_cameras / const_points: indices of blocks held constant (ceres::Problem::SetParameterBlockConstant; camera 0 stays constant
// as in the reference unless the options say otherwise) -- local / windowed BA, motion-only, structure-only (sfmhip_ba_solve_ex).
// Empty sets: the reference's problem.  An index out of range is an error: "[Err]" line, nothing optimised, parameters unchanged.
inline void bundle_adjustment(Mat& intrinsic, std::vector<Mat>& extrinsics, std::vector<std::vector<int>>& inds_2d_to_3d,
                              std::vector<std::vector<KeyPoint>>& key_points_for_all, std::vector<Point3d>& pts3d,
                              const std::vector<int>& const_cameras, const std::vector<int>& const_points)
{
    sfmhip_ctx* ctx = context();
    if (!ctx) { printf("Bundle Adjustment failed.\n"); return; }
    std::vector<int32_t> oc, op; std::vector<double> uv;
    for (size_t img = 0; img < inds_2d_to_3d.size(); ++img)
        for (size_t k = 0; k < inds_2d_to_3d[img].size(); ++k) {
            const int id = inds_2d_to_3d[img][k];
            if (id < 0) continue;
            oc.push_back((int32_t)img); op.push_back(id);
            uv.push_back((double)key_points_for_all[img][k].pt.x); uv.push_back((double)key_points_for_all[img][k].pt.y);   // Point2d observed (NView:1199)
        }
    const int nc = (int)extrinsics.size();
    std::vector<double> ext((size_t)6 * nc);
    for (int c = 0; c < nc; ++c) std::memcpy(&ext[6 * (size_t)c], extrinsics[c].ptr<double>(), 6 * sizeof(double));
    std::vector<uint8_t> cmask, pmask;          // empty set: NULL mask
    for (int c : const_cameras) {
        if (c < 0 || c >= nc) { printf("[Err]: bundle_adjustment: constant camera %d out of range (%d cameras).\n", c, nc); return; }
        cmask.resize((size_t)nc, 0); cmask[c] = 1;
    }
    for (int p : const_points) {
        if (p < 0 || p >= (int)pts3d.size()) { printf("[Err]: bundle_adjustment: constant point %d out of range (%d points).\n", p, (int)pts3d.size()); return; }
        pmask.resize(pts3d.size(), 0); pmask[p] = 1;
    }
    const uint8_t* cm = cmask.empty() ? nullptr : cmask.data();
    const uint8_t* pm = pmask.empty() ? nullptr : pmask.data();
    sfm_ba_options o; sfmhip_ba_default_options(&o);
    sfm_ba_summary s; std::memset(&s, 0, sizeof s);
    const std::vector<sfmhip_ctx*>& many = ba_contexts();
    const int rc = many.size() > 1
        ? sfmhip_ba_solve_multi_ex(many.data(), (int)many.size(), intrinsic.ptr<double>(), ext.data(), nc, pts3d.empty() ? nullptr : &pts3d[0].x,
                                   (int)pts3d.size(), oc.data(), op.data(), uv.data(), (int)oc.size(), cm, pm, &o, &s)
        : sfmhip_ba_solve_ex(ctx, intrinsic.ptr<double>(), ext.data(), nc, pts3d.empty() ? nullptr : &pts3d[0].x, (int)pts3d.size(),
                             oc.data(), op.data(), uv.data(), (int)oc.size(), cm, pm, &o, &s);
    if (rc != SFMHIP_OK || s.termination == SFMHIP_BA_FAILURE) { printf("Bundle Adjustment failed.\n"); return; }
    for (int c = 0; c < nc; ++c) std::memcpy(extrinsics[c].ptr<double>(), &ext[6 * (size_t)c], 6 * sizeof(double));
    printf("\nBundle Adjustment statistics (approximated RMSE):\n #views: %d\n #residuals: %d\n Initial RMSE(pixel): %g\n"
           " Final   RMSE(pixel): %g\n Time (s): %g\n\n", nc, s.num_residuals,
           std::sqrt(s.initial_cost / (s.num_residuals > 0 ? s.num_residuals : 1)),
           std::sqrt(s.final_cost / (s.num_residuals > 0 ? s.num_residuals : 1)), s.total_time_s);
}
inline void bundle_adjustment(Mat& intrinsic, std::vector<Mat>& extrinsics, std::vector<std::vector<int>>& inds_2d_to_3d,
                              std::vector<std::vector<KeyPoint>>& key_points_for_all, std::vector<Point3d>& pts3d)
{
    bundle_adjustment(intrinsic, extrinsics, inds_2d_to_3d, key_points_for_all, pts3d, std::vector<int>(), std::vector<int>());
}

// ---- normals (NView:551-599) ------------------------------------------------------------------------------------
inline int estimate_normals(const std::vector<Point3d>& pts3d, const int K, std::vector<Point3d>& normals)
{
    sfmhip_ctx* ctx = context();
    normals.resize(pts3d.size());
    if (!ctx) return -1;
    if (pts3d.empty()) return 0;
    return sfmhip_estimate_normals(ctx, &pts3d[0].x, (int)pts3d.size(), K, &normals[0].x) == SFMHIP_OK ? 0 : -1;
}

// ---- statistical outlier removal (extension, NOT reference behaviour: pcl::StatisticalOutlierRemoval / Open3D's
// remove_statistical_outlier) -- keep[i] = 1 where the mean distance of point i to its K nearest neighbours is at most
// mean + std_ratio * standard deviation of those means over the cloud.  Returns the number of points kept, -1 on error.
inline int filter_outliers(const std::vector<Point3d>& pts3d, const int K, const double std_ratio, std::vector<unsigned char>& keep)
{
    sfmhip_ctx* ctx = context();
    keep.assign(pts3d.size(), 0);
    if (!ctx) return -1;
    if (pts3d.empty()) return 0;
    if (sfmhip_statistical_outliers(ctx, &pts3d[0].x, (int)pts3d.size(), K, std_ratio, SFMHIP_POINTS_AUTO, keep.data(), nullptr, nullptr) != SFMHIP_OK) {
        printf("[Err]: filter_outliers: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    int kept = 0;
    for (unsigned char k : keep) kept += k ? 1 : 0;
    return kept;
}

// ---- radius outlier removal (extension; modelled on pcl::RadiusOutlierRemoval / Open3D's remove_radius_outlier) -- keep[i] = 1 where
// point i has at least min_neighbors OTHER points within distance r (sfmhip_radius_outliers).  Returns the number kept, -1 on error.
inline int filter_radius_outliers(const std::vector<Point3d>& pts3d, const double r, const int min_neighbors, std::vector<unsigned char>& keep)
{
    sfmhip_ctx* ctx = context();
    keep.assign(pts3d.size(), 0);
    if (!ctx) return -1;
    if (pts3d.empty()) return 0;
    if (sfmhip_radius_outliers(ctx, &pts3d[0].x, (int)pts3d.size(), r, min_neighbors, SFMHIP_POINTS_AUTO, keep.data(), nullptr) != SFMHIP_OK) {
        printf("[Err]: filter_radius_outliers: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    int kept = 0;
    for (unsigned char k : keep) kept += k ? 1 : 0;
    return kept;
}

// ---- largest-cluster filter (extension; modelled on pcl::EuclideanClusterExtraction / Open3D's cluster_dbscan followed by "keep the
// largest") -- keep[i] = 1 where point i belongs to the cluster with the most points (sfmhip_largest_cluster: clusters are the connected
// components, at distance r, of the points with at least min_points points within r of them, themselves included, plus the border
// points they adopt).  Returns the number kept, -1 on error; n_clusters: the number of clusters found.
inline int filter_largest_cluster(const std::vector<Point3d>& pts3d, const double r, const int min_points, std::vector<unsigned char>& keep,
                                  int* n_clusters = nullptr)
{
    sfmhip_ctx* ctx = context();
    keep.assign(pts3d.size(), 0);
    if (n_clusters) *n_clusters = 0;
    if (!ctx) return -1;
    if (pts3d.empty()) return 0;
    int kept = 0;
    if (sfmhip_largest_cluster(ctx, &pts3d[0].x, (int)pts3d.size(), r, min_points, SFMHIP_POINTS_AUTO, keep.data(), nullptr, n_clusters, &kept) != SFMHIP_OK) {
        printf("[Err]: filter_largest_cluster: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    return kept;
}

// ---- RANSAC plane segmentation (extension; modelled on Open3D's segment_plane / pcl::SACSegmentation with SACMODEL_PLANE) -- up to
// max_planes planes peeled off one after another (sfmhip_segment_planes, where the definition is): labels[i] = the plane of point i or
// -1; planes[k] = the least-squares plane (a, b, c, d) of the inliers of plane k, d >= 0; counts[k] = its number of points.  Returns the
// number of planes found, -1 on error.
struct Plane4d { double a = 0, b = 0, c = 0, d = 0; };
inline int segment_planes(const std::vector<Point3d>& pts3d, const double threshold, const int max_planes, const int min_inliers,
                          std::vector<int32_t>& labels, std::vector<Plane4d>& planes, std::vector<int32_t>& counts,
                          const int hypotheses = 1024, const uint64_t seed = 0)
{
    sfmhip_ctx* ctx = context();
    labels.assign(pts3d.size(), -1);
    planes.clear(); counts.clear();
    if (!ctx) return -1;
    if (pts3d.empty()) return 0;
    const size_t cap = max_planes > 0 ? (size_t)max_planes : 0;
    std::vector<Plane4d> ransac(cap), refined(cap);
    std::vector<int32_t> cnt(cap);
    int n_planes = 0;
    if (sfmhip_segment_planes(ctx, &pts3d[0].x, (int)pts3d.size(), threshold, hypotheses, seed, min_inliers, max_planes, labels.data(), &n_planes,
                              cap ? &ransac[0].a : nullptr, cap ? &refined[0].a : nullptr, cnt.data(), nullptr) != SFMHIP_OK) {
        printf("[Err]: segment_planes: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    planes.assign(refined.begin(), refined.begin() + n_planes);
    counts.assign(cnt.begin(), cnt.begin() + n_planes);
    return n_planes;
}

// ---- voxel-grid down-sampling (extension; sfmhip_voxel_downsample) -- one centroid per occupied voxel of edge `voxel`, in ascending
// voxel order; a voxel's colour is, per channel, the rounded mean (2 * sum + count) / (2 * count) in integers over its points (colors
// may be shorter than pts3d: out_colors is then left empty).  Returns the number of voxels, -1 on error.
inline int voxel_downsample(const std::vector<Point3d>& pts3d, const std::vector<Vec3b>& colors, const double voxel,
                            std::vector<Point3d>& out_pts, std::vector<Vec3b>& out_colors)
{
    sfmhip_ctx* ctx = context();
    out_pts.clear(); out_colors.clear();
    if (!ctx) return -1;
    if (pts3d.empty()) return 0;
    const int n = (int)pts3d.size();
    std::vector<Point3d> cen(pts3d.size());
    std::vector<int32_t> counts(pts3d.size()), voxel_of(pts3d.size());
    int nv = 0;
    if (sfmhip_voxel_downsample(ctx, &pts3d[0].x, n, voxel, &cen[0].x, counts.data(), voxel_of.data(), &nv, nullptr) != SFMHIP_OK) {
        printf("[Err]: voxel_downsample: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    out_pts.assign(cen.begin(), cen.begin() + nv);
    if (colors.size() >= pts3d.size()) {
        std::vector<long long> sum((size_t)nv * 3, 0);
        for (int i = 0; i < n; ++i)
            if (voxel_of[i] >= 0)
                for (int ch = 0; ch < 3; ++ch) sum[(size_t)voxel_of[i] * 3 + ch] += colors[i][ch];
        out_colors.resize(nv);
        for (int v = 0; v < nv; ++v)
            for (int ch = 0; ch < 3; ++ch) out_colors[v][ch] = (unsigned char)((2 * sum[(size_t)v * 3 + ch] + counts[v]) / (2 * (long long)counts[v]));
    }
    return nv;
}

// ---- dense cloud (extension; sfmhip_plane_sweep, sfmhip_depth_consistency, sfmhip_depth_to_points) -- the dense step after the bundle
// adjustment, the mirror of api.dense_cloud_for_all: every view is swept against the n_src views with the nearest camera centres (equal
// distances: the lower index), its depth map is checked against theirs, the kept pixels become coloured world points, the views' points
// follow each other in view order; voxel > 0: voxel_downsample on the result.  images: rows x cols x channels bytes each, dense.
// intrinsic: 4 x 1 (fx, fy, cx, cy); extrinsics: 6 x 1 (angle-axis, t) per view, as bundle_adjustment leaves them.  The inverse-depth
// range of a view is [wmin, wmax] where wmin < wmax are given, else dense_depth_range of the sparse points.  Returns the number of
// points, -1 on error.
struct DenseOptions {
    int n_src = 2, planes = 64, radius = 2, min_sources = 1;
    double wmin = 0.0, wmax = 0.0, min_score = 0.5, rel_tol = 0.01;
    int min_consistent = -1;               // < 0: min(2, n_src)
    double voxel = 0.0;
    // semi-global aggregation of the sweep's costs before the winner is taken (sfmhip_plane_sweep_sgm; at most 256 planes, min_score is
    // not used); off: the winner per pixel
    bool sgm = false;
    double sgm_cost_scale = 262144.0;
    int sgm_P1 = 512, sgm_P2 = 4096, sgm_paths = 8, sgm_max_cost = 65535;
    // the mesh (dense_mesh_for_all): the volume is (mesh_dims, mesh_origin, mesh_voxel) where mesh_voxel > 0, else tsdf_bounds of the sparse
    // points with mesh_voxels voxels along its longest side; truncation at mesh_trunc_voxels voxels; a voxel counts with mesh_min_weight views
    int mesh_voxels = 128, mesh_min_weight = 2;
    double mesh_trunc_voxels = 4.0, mesh_margin = 0.1;
    int mesh_dims[3] = { 0, 0, 0 };
    double mesh_origin[3] = { 0.0, 0.0, 0.0 }, mesh_voxel = 0.0;
    // the clean-up of the mesh (clean_mesh), every step off by default and run in this order: the components with at least
    // mesh_min_component triangles (0: off) / only the largest; vertex clustering on cells of mesh_simplify_voxels voxels (0: off);
    // mesh_smooth_iterations Taubin pairs of steps (lambda, then mu), Laplacian steps where mu == 0 (0: off); vertex normals
    int mesh_min_component = 0;
    bool mesh_keep_largest = false;
    double mesh_simplify_voxels = 0.0;
    int mesh_smooth_iterations = 0;
    double mesh_smooth_lambda = 0.5, mesh_smooth_mu = -0.53;
    bool mesh_normals = false;
    // the bundle adjustment's observation lists into sparse_pts (empty: the sources are the nearest camera centres and the range comes from
    // the whole cloud, as before): the sources and every view's range come from select_views, pairs counted from min_angle_deg on
    std::vector<int32_t> obs_cam, obs_pt;
    double min_angle_deg = 1.0;
};
// numpy.percentile(z, q) with its default linear interpolation, z sorted ascending
inline double dense_percentile(const std::vector<double>& z, const double q)
{
    const double pos = q / 100.0 * (double)(z.size() - 1);
    const size_t lo = (size_t)std::floor(pos), hi = std::min(lo + 1, z.size() - 1);
    const double t = pos - (double)lo, a = z[lo], b = z[hi];
    return t >= 0.5 ? b - (b - a) * (1.0 - t) : a + (b - a) * t;
}
// the inverses of the 98th and 2nd percentile of the sparse points' depths z > 0 in the view, the interval widened by a quarter of its
// length at both ends (the lower end no lower than half the 98th percentile's inverse); false with fewer than two points in front
inline bool dense_depth_range(const std::vector<Point3d>& sparse_pts, const double ext6[6], double& wmin, double& wmax)
{
    const double K1[4] = { 1.0, 1.0, 0.0, 0.0 };
    double Rinv[9], c[3];
    if (sfmhip_sweep_geometry(K1, ext6, nullptr, 0, nullptr, nullptr, nullptr, nullptr, Rinv, c) != SFMHIP_OK) return false;
    std::vector<double> z;
    for (const Point3d& p : sparse_pts) {
        const double v = ((p.x - c[0]) * Rinv[2] + (p.y - c[1]) * Rinv[5]) + (p.z - c[2]) * Rinv[8];
        if (std::isfinite(v) && v > 0.0) z.push_back(v);
    }
    if (z.size() < 2) return false;
    std::sort(z.begin(), z.end());
    const double wlo = 1.0 / dense_percentile(z, 98.0), whi = 1.0 / dense_percentile(z, 2.0);
    double span = whi - wlo;
    if (!(span > 0.0)) span = 0.5 * wlo;
    wmin = std::max(wlo - 0.25 * span, 0.5 * wlo);
    wmax = whi + 0.25 * span;
    return true;
}
// ---- view selection (extension; sfmhip_select_views, where the definition is), the mirror of api.select_views: the covisibility counts of
// the views (shared, score: n_views x n_views), every view's n_src sources ranked by the sparse points shared under at least min_angle_deg
// (sources: n_views x n_src; n_scored of them by score, the rest by centre distance), and every view's inverse-depth range from the n_depth
// points it sees in front of it (wrange: n_views x 2, zeros where n_depth < 2).  false on error.
struct SelectedViews {
    int n_views = 0, n_src = 0;
    std::vector<int32_t> shared, score, sources, n_scored, n_depth;
    std::vector<double> wrange;
};
inline bool select_views(const std::vector<Mat>& extrinsics, const std::vector<Point3d>& pts, const std::vector<int32_t>& obs_cam, const std::vector<int32_t>& obs_pt,
                         const int n_src, const double min_angle_deg, SelectedViews& out)
{
    sfmhip_ctx* ctx = context();
    const int n = (int)extrinsics.size();
    if (!ctx || n < 2 || n_src < 1 || obs_cam.size() != obs_pt.size() || !(min_angle_deg >= 0.0 && min_angle_deg <= 90.0)) return false;
    std::vector<double> ext((size_t)n * 6);
    for (int i = 0; i < n; ++i) std::memcpy(&ext[6 * (size_t)i], extrinsics[i].ptr<double>(), 6 * sizeof(double));
    const double c = std::cos(min_angle_deg * (M_PI / 180.0));
    out.n_views = n; out.n_src = n_src;
    out.shared.assign((size_t)n * n, 0); out.score.assign((size_t)n * n, 0); out.sources.assign((size_t)n * n_src, 0);
    out.n_scored.assign(n, 0); out.n_depth.assign(n, 0); out.wrange.assign((size_t)n * 2, 0.0);
    const int rc = sfmhip_select_views(ctx, ext.data(), n, pts.empty() ? nullptr : &pts[0].x, (int)pts.size(), obs_cam.empty() ? nullptr : obs_cam.data(),
                                       obs_pt.empty() ? nullptr : obs_pt.data(), (int)obs_cam.size(), c * c, n_src, out.shared.data(), out.score.data(),
                                       out.sources.data(), out.n_scored.data(), out.wrange.data(), out.n_depth.data());
    if (rc != SFMHIP_OK) printf("[Err]: select_views: %s\n", sfmhip_last_error(ctx));
    return rc == SFMHIP_OK;
}
// ---- tracks from pairwise matches (extension; sfmhip_build_tracks, where the definition is), the mirror of api.tracks_for_all: the
// connected components of the match graph over any pair list.  pairs: (query image, train image) of every list of matches_for_all, empty:
// the chain (i, i + 1).  correspond_struct_idx[img][kp] = track or -1, as bundle_adjustment takes it; the observation lists are in (track,
// image) order; matches_for_all comes back reduced to the elements between two observations of a track.  false on error.
struct Tracks {
    std::vector<std::vector<int>> correspond_struct_idx;
    std::vector<int32_t> obs_cam, obs_pt, obs_kp, track_len;
    std::vector<double> obs_uv;
    int32_t stats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    std::vector<std::vector<DMatch>> matches_for_all;
};
inline bool build_tracks_for_all(const std::vector<std::vector<KeyPoint>>& key_points_for_all, const std::vector<std::pair<int, int>>& pairs,
                                 const std::vector<std::vector<DMatch>>& matches_for_all, const int min_len, const bool keep_first, Tracks& out)
{
    static_assert(sizeof(KeyPoint) == sizeof(sfm_keypoint) && sizeof(DMatch) == sizeof(sfm_dmatch), "layouts of include/sfmhip.h");
    sfmhip_ctx* ctx = context();
    const int n_img = (int)key_points_for_all.size();
    std::vector<int32_t> pr;
    if (pairs.empty()) for (int i = 0; i + 1 < n_img; ++i) { pr.push_back(i); pr.push_back(i + 1); }
    else for (const auto& p : pairs) { pr.push_back(p.first); pr.push_back(p.second); }
    const size_t P = pr.size() / 2;
    if (!ctx || n_img < 1 || matches_for_all.size() != P) return false;
    std::vector<int32_t> n_kp(n_img), counts(P);
    std::vector<const sfm_keypoint*> kp(n_img);
    size_t n = 0, S = 0;
    for (int i = 0; i < n_img; ++i) {
        n_kp[i] = (int32_t)key_points_for_all[i].size(); n += key_points_for_all[i].size();
        kp[i] = key_points_for_all[i].empty() ? nullptr : (const sfm_keypoint*)key_points_for_all[i].data();
    }
    for (size_t q = 0; q < P; ++q) { counts[q] = (int32_t)matches_for_all[q].size(); S = std::max(S, matches_for_all[q].size()); }
    std::vector<DMatch> m(P * S), mo(P * S);
    for (size_t q = 0; q < P; ++q) std::copy(matches_for_all[q].begin(), matches_for_all[q].end(), m.begin() + q * S);
    std::vector<int32_t> track_of(n), counts_out(P, 0);
    out.obs_cam.assign(n, 0); out.obs_pt.assign(n, 0); out.obs_kp.assign(n, 0); out.track_len.assign(n / 2, 0); out.obs_uv.assign(2 * n, 0.0);
    const int rc = sfmhip_build_tracks(ctx, n_img, n_kp.data(), pr.data(), (int)P, (const sfm_dmatch*)m.data(), (int)S, counts.data(), kp.data(), min_len,
                                       keep_first ? SFMHIP_TRACKS_KEEP_FIRST : SFMHIP_TRACKS_DROP_CONFLICTS, track_of.data(), out.obs_cam.data(), out.obs_pt.data(),
                                       out.obs_kp.data(), out.obs_uv.data(), out.track_len.data(), (sfm_dmatch*)mo.data(), counts_out.data(), out.stats);
    if (rc != SFMHIP_OK) { printf("[Err]: build_tracks_for_all: %s\n", sfmhip_last_error(ctx)); return false; }
    const size_t n_tracks = (size_t)out.stats[0], n_obs = (size_t)out.stats[1];
    out.obs_cam.resize(n_obs); out.obs_pt.resize(n_obs); out.obs_kp.resize(n_obs); out.obs_uv.resize(2 * n_obs); out.track_len.resize(n_tracks);
    out.correspond_struct_idx.assign(n_img, std::vector<int>());
    size_t at = 0;
    for (int i = 0; i < n_img; ++i) { out.correspond_struct_idx[i].assign(track_of.begin() + at, track_of.begin() + at + n_kp[i]); at += (size_t)n_kp[i]; }
    out.matches_for_all.assign(P, std::vector<DMatch>());
    for (size_t q = 0; q < P; ++q) out.matches_for_all[q].assign(mo.begin() + q * S, mo.begin() + q * S + counts_out[q]);
    return true;
}
struct DenseGeo { float A[72], b[24]; double Rrel[72], trel[24], Rinv[9], c[3]; };
// what dense_cloud_for_all and dense_mesh_for_all share: the sources of every view (the nearest camera centres, or select_views' where
// opt.obs_cam is given), its geometry arrays and its depth map (the plane sweep, or its semi-global form); false on error, with the message printed under the caller's name
inline bool dense_depth_maps(sfmhip_ctx* ctx, const char* who, const std::vector<const uint8_t*>& images, const int rows, const int cols, const int channels,
                             const Mat& intrinsic, const std::vector<Mat>& extrinsics, const std::vector<Point3d>& sparse_pts, const DenseOptions& opt, int& n_src,
                             std::vector<std::vector<int>>& sources, std::vector<DenseGeo>& geo, std::vector<std::vector<float>>& depth)
{
    const int n_img = (int)images.size();
    if (!ctx || n_img < 2 || extrinsics.size() != images.size() || rows < 1 || cols < 1) return false;
    n_src = std::min(opt.n_src, n_img - 1);
    if (n_src < 1 || n_src > 8) return false;
    const double* K4 = intrinsic.ptr<double>();
    const double K1[4] = { 1.0, 1.0, 0.0, 0.0 };
    const size_t npx = (size_t)rows * cols, ld = (size_t)cols * channels;
    // the sources of every view: the nearest camera centres
    std::vector<double> cen((size_t)n_img * 3);
    for (int i = 0; i < n_img; ++i)
        if (sfmhip_sweep_geometry(K1, extrinsics[i].ptr<double>(), nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &cen[3 * (size_t)i]) != SFMHIP_OK) return false;
    sources.assign(n_img, std::vector<int>());
    SelectedViews sel;
    const bool by_model = !opt.obs_cam.empty();
    if (by_model && !select_views(extrinsics, sparse_pts, opt.obs_cam, opt.obs_pt, n_src, opt.min_angle_deg, sel)) return false;
    for (int i = 0; i < n_img; ++i) {
        if (by_model) {
            sources[i].assign(sel.sources.begin() + (size_t)i * n_src, sel.sources.begin() + (size_t)(i + 1) * n_src);
            continue;
        }
        std::vector<std::pair<double, int>> d;
        for (int j = 0; j < n_img; ++j) {
            if (j == i) continue;
            const double dx = cen[3 * j] - cen[3 * i], dy = cen[3 * j + 1] - cen[3 * i + 1], dz = cen[3 * j + 2] - cen[3 * i + 2];
            d.emplace_back(std::sqrt((dx * dx + dy * dy) + dz * dz), j);
        }
        std::stable_sort(d.begin(), d.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
        for (int k = 0; k < n_src; ++k) sources[i].push_back(d[k].second);
    }
    geo.assign(n_img, DenseGeo());
    depth.assign(n_img, std::vector<float>(npx));
    std::vector<int32_t> plane(npx);
    std::vector<float> score(npx);
    std::vector<uint16_t> win_cost(opt.sgm ? npx : 0);
    for (int i = 0; i < n_img; ++i) {
        double e[48];
        const uint8_t* src[8];
        for (int k = 0; k < n_src; ++k) { std::memcpy(e + 6 * k, extrinsics[sources[i][k]].ptr<double>(), 6 * sizeof(double)); src[k] = images[sources[i][k]]; }
        DenseGeo& g = geo[i];
        if (sfmhip_sweep_geometry(K4, extrinsics[i].ptr<double>(), e, n_src, g.A, g.b, g.Rrel, g.trel, g.Rinv, g.c) != SFMHIP_OK) return false;
        double wmin = opt.wmin, wmax = opt.wmax;
        bool have = wmin < wmax;
        if (!have && by_model && sel.n_depth[i] >= 2) { wmin = sel.wrange[2 * (size_t)i]; wmax = sel.wrange[2 * (size_t)i + 1]; have = true; }
        if (!have && (by_model || !dense_depth_range(sparse_pts, extrinsics[i].ptr<double>(), wmin, wmax))) {
            printf("[Err]: %s: no depth range for view %d\n", who, i);
            return false;
        }
        const int rc = opt.sgm ? sfmhip_plane_sweep_sgm(ctx, images[i], src, n_src, rows, cols, channels, ld, g.A, g.b, opt.planes, wmin, wmax, opt.radius, opt.min_sources,
                                                        opt.sgm_cost_scale, opt.sgm_P1, opt.sgm_P2, opt.sgm_paths, opt.sgm_max_cost, plane.data(), win_cost.data(),
                                                        depth[i].data())
                               : sfmhip_plane_sweep(ctx, images[i], src, n_src, rows, cols, channels, ld, g.A, g.b, opt.planes, wmin, wmax, opt.radius, opt.min_sources,
                                                    opt.min_score, plane.data(), score.data(), depth[i].data());
        if (rc != SFMHIP_OK) {
            printf("[Err]: %s: %s\n", who, sfmhip_last_error(ctx));
            return false;
        }
    }
    return true;
}
inline int dense_cloud_for_all(const std::vector<const uint8_t*>& images, const int rows, const int cols, const int channels, const Mat& intrinsic,
                               const std::vector<Mat>& extrinsics, const std::vector<Point3d>& sparse_pts, const DenseOptions& opt,
                               std::vector<Point3d>& out_pts, std::vector<Vec3b>& out_colors)
{
    sfmhip_ctx* ctx = context();
    out_pts.clear(); out_colors.clear();
    int n_src = 0;
    std::vector<std::vector<int>> sources;
    std::vector<DenseGeo> geo;
    std::vector<std::vector<float>> depth;
    if (!dense_depth_maps(ctx, "dense_cloud_for_all", images, rows, cols, channels, intrinsic, extrinsics, sparse_pts, opt, n_src, sources, geo, depth)) return -1;
    const int n_img = (int)images.size(), min_consistent = opt.min_consistent < 0 ? std::min(2, n_src) : opt.min_consistent;
    const double* K4 = intrinsic.ptr<double>();
    const size_t npx = (size_t)rows * cols, ld = (size_t)cols * channels;
    std::vector<uint8_t> keep(npx);
    std::vector<Point3d> xyz(npx);
    std::vector<Vec3b> bgr(npx);
    std::vector<Point3d> pts;
    std::vector<Vec3b> cols_out;
    for (int i = 0; i < n_img; ++i) {
        const float* ds[8];
        for (int k = 0; k < n_src; ++k) ds[k] = depth[sources[i][k]].data();
        const DenseGeo& g = geo[i];
        int32_t n = 0;
        if (sfmhip_depth_consistency(ctx, depth[i].data(), ds, n_src, rows, cols, K4, g.Rrel, g.trel, opt.rel_tol, min_consistent, nullptr, keep.data()) != SFMHIP_OK ||
            sfmhip_depth_to_points(ctx, depth[i].data(), keep.data(), images[i], rows, cols, channels, ld, K4, g.Rinv, g.c, &xyz[0].x, &bgr[0].v[0], (int)npx, &n) != SFMHIP_OK) {
            printf("[Err]: dense_cloud_for_all: %s\n", sfmhip_last_error(ctx));
            return -1;
        }
        pts.insert(pts.end(), xyz.begin(), xyz.begin() + n);
        cols_out.insert(cols_out.end(), bgr.begin(), bgr.begin() + n);
    }
    if (opt.voxel > 0.0 && !pts.empty()) return voxel_downsample(pts, cols_out, opt.voxel, out_pts, out_colors);
    out_pts.swap(pts); out_colors.swap(cols_out);
    return (int)out_pts.size();
}

// ---- dense mesh (extension; sfmhip_tsdf_integrate, sfmhip_tsdf_mesh), the mirror of api.tsdf_bounds and api.dense_mesh_for_all
// (dims, origin, voxel) of a volume around the sparse cloud: per axis the 2nd and 98th percentile of the finite points, widened by `margin`
// of the interval at both ends; the voxel is the longest side over `voxels`, the other axes take the voxels that cover their side (at
// least 2), centred on it; false with fewer than two finite points or a cloud without extent
inline bool tsdf_bounds(const std::vector<Point3d>& sparse_pts, const int voxels, const double margin, int dims[3], double origin[3], double& voxel)
{
    std::vector<double> ax[3];
    for (const Point3d& p : sparse_pts)
        if (std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z)) { ax[0].push_back(p.x); ax[1].push_back(p.y); ax[2].push_back(p.z); }
    if (ax[0].size() < 2 || voxels < 1) return false;
    double lo[3], hi[3], side = 0.0;
    for (int a = 0; a < 3; ++a) {
        std::sort(ax[a].begin(), ax[a].end());
        const double l = dense_percentile(ax[a], 2.0), h = dense_percentile(ax[a], 98.0), span = h - l;
        lo[a] = l - margin * span; hi[a] = h + margin * span;
        side = std::max(side, hi[a] - lo[a]);
    }
    if (!(side > 0.0)) return false;
    voxel = side / (double)voxels;
    for (int a = 0; a < 3; ++a) {
        dims[a] = std::max((int)std::ceil((hi[a] - lo[a]) / voxel - 1e-9), 2);
        origin[a] = 0.5 * (lo[a] + hi[a]) - 0.5 * (double)dims[a] * voxel;
    }
    return true;
}
// The clean-up of a triangle mesh in place, the mirror of the five sfmhip_mesh_* calls in the order api.dense_mesh_for_all runs them:
// min_component >= 1 or keep_largest: sfmhip_mesh_filter_components; cell > 0: sfmhip_mesh_simplify on cells of that edge; iterations > 0:
// sfmhip_mesh_smooth; normals != nullptr: sfmhip_mesh_vertex_normals into it.  Returns the number of triangles, -1 on error.
inline int clean_mesh(std::vector<Point3d>& pts, std::vector<Vec3b>& colors, std::vector<int32_t>& tris, const int min_component, const bool keep_largest,
                      const double cell, const int iterations, const double lambda, const double mu, std::vector<Point3d>* normals)
{
    sfmhip_ctx* ctx = context();
    if (pts.size() != colors.size() || tris.size() % 3 != 0) return -1;
    auto fail = [&]() { printf("[Err]: clean_mesh: %s\n", sfmhip_last_error(ctx)); return -1; };
    // a call that writes a new mesh into arrays of the old one's size
    auto rebuilt = [&](auto&& call) {
        const int nv = (int)pts.size(), nt = (int)(tris.size() / 3);
        std::vector<Point3d> p2(nv); std::vector<Vec3b> c2(nv); std::vector<int32_t> t2((size_t)nt * 3);
        int mv = 0, mt = 0;
        if (call(nv ? &pts[0].x : nullptr, nv ? &colors[0].v[0] : nullptr, nv, tris.data(), nt, nv ? &p2[0].x : nullptr, nv ? &c2[0].v[0] : nullptr, t2.data(), &mv, &mt) !=
            SFMHIP_OK)
            return false;
        p2.resize(mv); c2.resize(mv); t2.resize((size_t)mt * 3);
        pts.swap(p2); colors.swap(c2); tris.swap(t2);
        return true;
    };
    if (min_component >= 1 || keep_largest) {
        if (!rebuilt([&](const double* x, const uint8_t* c, int nv, const int32_t* t, int nt, double* xo, uint8_t* co, int32_t* to, int* mv, int* mt) {
                return sfmhip_mesh_filter_components(ctx, x, c, nv, t, nt, std::max(min_component, 1), keep_largest ? 1 : 0, xo, co, to, nullptr, mv, mt);
            }))
            return fail();
    }
    if (cell > 0.0) {
        if (!rebuilt([&](const double* x, const uint8_t* c, int nv, const int32_t* t, int nt, double* xo, uint8_t* co, int32_t* to, int* mv, int* mt) {
                return sfmhip_mesh_simplify(ctx, x, c, nv, t, nt, cell, xo, co, to, nullptr, mv, mt);
            }))
            return fail();
    }
    const int nv = (int)pts.size(), nt = (int)(tris.size() / 3);
    if (iterations > 0 && nv > 0) {
        std::vector<Point3d> p2(nv);
        if (sfmhip_mesh_smooth(ctx, &pts[0].x, nv, tris.data(), nt, iterations, lambda, mu, &p2[0].x) != SFMHIP_OK) return fail();
        pts.swap(p2);
    }
    if (normals) {
        normals->assign(nv, Point3d());
        if (nv > 0 && sfmhip_mesh_vertex_normals(ctx, &pts[0].x, nv, tris.data(), nt, &(*normals)[0].x) != SFMHIP_OK) return fail();
    }
    return nt;
}

// The dense surface after the bundle adjustment: dense_cloud_for_all's depth maps and keep masks (same arguments), every view fused into
// one truncated signed distance volume, 8 views per call, and the volume meshed by marching tetrahedra (once for the counts, once into
// arrays of that size), then cleaned up as the mesh_* options say (clean_mesh; out_normals is filled where opt.mesh_normals is set and it is
// given).  out_tris: three vertex numbers per triangle.  Returns the number of triangles, -1 on error.
inline int dense_mesh_for_all(const std::vector<const uint8_t*>& images, const int rows, const int cols, const int channels, const Mat& intrinsic,
                              const std::vector<Mat>& extrinsics, const std::vector<Point3d>& sparse_pts, const DenseOptions& opt,
                              std::vector<Point3d>& out_pts, std::vector<Vec3b>& out_colors, std::vector<int32_t>& out_tris,
                              std::vector<Point3d>* out_normals = nullptr)
{
    sfmhip_ctx* ctx = context();
    out_pts.clear(); out_colors.clear(); out_tris.clear();
    int n_src = 0;
    std::vector<std::vector<int>> sources;
    std::vector<DenseGeo> geo;
    std::vector<std::vector<float>> depth;
    if (!dense_depth_maps(ctx, "dense_mesh_for_all", images, rows, cols, channels, intrinsic, extrinsics, sparse_pts, opt, n_src, sources, geo, depth)) return -1;
    const int n_img = (int)images.size(), min_consistent = opt.min_consistent < 0 ? std::min(2, n_src) : opt.min_consistent;
    const double* K4 = intrinsic.ptr<double>();
    const size_t npx = (size_t)rows * cols, ld = (size_t)cols * channels;
    int dims[3] = { opt.mesh_dims[0], opt.mesh_dims[1], opt.mesh_dims[2] };
    double origin[3] = { opt.mesh_origin[0], opt.mesh_origin[1], opt.mesh_origin[2] }, voxel = opt.mesh_voxel;
    if (!(voxel > 0.0) && !tsdf_bounds(sparse_pts, opt.mesh_voxels, opt.mesh_margin, dims, origin, voxel)) {
        printf("[Err]: dense_mesh_for_all: no volume\n");
        return -1;
    }
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || (double)dims[0] * dims[1] * dims[2] > 268435456.0) return -1;
    std::vector<std::vector<uint8_t>> keep(n_img, std::vector<uint8_t>(npx));
    std::vector<double> R((size_t)n_img * 9), t((size_t)n_img * 3);
    for (int i = 0; i < n_img; ++i) {
        const float* ds[8];
        for (int k = 0; k < n_src; ++k) ds[k] = depth[sources[i][k]].data();
        const DenseGeo& g = geo[i];
        if (sfmhip_depth_consistency(ctx, depth[i].data(), ds, n_src, rows, cols, K4, g.Rrel, g.trel, opt.rel_tol, min_consistent, nullptr, keep[i].data()) != SFMHIP_OK) {
            printf("[Err]: dense_mesh_for_all: %s\n", sfmhip_last_error(ctx));
            return -1;
        }
        for (int r = 0; r < 3; ++r)                                      // world to camera: the transpose of Rinv, and the pose's t
            for (int c = 0; c < 3; ++c) R[9 * (size_t)i + 3 * r + c] = g.Rinv[3 * c + r];
        std::memcpy(&t[3 * (size_t)i], extrinsics[i].ptr<double>() + 3, 3 * sizeof(double));
    }
    const size_t nvox = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<int32_t> dsum(nvox, 0), wsum(nvox, 0);
    std::vector<uint32_t> csum(nvox * 3, 0);
    for (int i0 = 0; i0 < n_img; i0 += 8) {
        const int n = std::min(8, n_img - i0);
        const float* dp[8]; const uint8_t* kp[8]; const uint8_t* ip[8];
        for (int k = 0; k < n; ++k) { dp[k] = depth[i0 + k].data(); kp[k] = keep[i0 + k].data(); ip[k] = images[i0 + k]; }
        if (sfmhip_tsdf_integrate(ctx, dims, origin, voxel, opt.mesh_trunc_voxels * voxel, dp, kp, ip, n, rows, cols, channels, ld, K4, &R[9 * (size_t)i0], &t[3 * (size_t)i0],
                                  dsum.data(), wsum.data(), csum.data()) != SFMHIP_OK) {
            printf("[Err]: dense_mesh_for_all: %s\n", sfmhip_last_error(ctx));
            return -1;
        }
    }
    int32_t nv = 0, nt = 0;
    if (sfmhip_tsdf_mesh(ctx, dims, origin, voxel, dsum.data(), wsum.data(), csum.data(), opt.mesh_min_weight, nullptr, nullptr, 0, nullptr, 0, &nv, &nt) != SFMHIP_OK) {
        printf("[Err]: dense_mesh_for_all: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    out_pts.resize(nv); out_colors.resize(nv); out_tris.resize((size_t)nt * 3);
    if (nv > 0 && nt > 0 &&
        sfmhip_tsdf_mesh(ctx, dims, origin, voxel, dsum.data(), wsum.data(), csum.data(), opt.mesh_min_weight, &out_pts[0].x, &out_colors[0].v[0], nv, out_tris.data(), nt, &nv,
                         &nt) != SFMHIP_OK) {
        printf("[Err]: dense_mesh_for_all: %s\n", sfmhip_last_error(ctx));
        return -1;
    }
    const bool want_normals = opt.mesh_normals && out_normals;
    if (opt.mesh_min_component >= 1 || opt.mesh_keep_largest || opt.mesh_simplify_voxels > 0.0 || opt.mesh_smooth_iterations > 0 || want_normals)
        return clean_mesh(out_pts, out_colors, out_tris, opt.mesh_min_component, opt.mesh_keep_largest, opt.mesh_simplify_voxels * voxel, opt.mesh_smooth_iterations,
                          opt.mesh_smooth_lambda, opt.mesh_smooth_mu, want_normals ? out_normals : nullptr);
    return nt;
}

// ---- outputs (NView:186-338) ------------------------------------------------------------------------------------
namespace detail {
// fs::doubleToString [3P] + the "%.16e" of the Windows CRT the reference's files were written with (exact decimal ties
// round half away from zero; glibc rounds them to even)
// fs::floatToString [3P]: "%.8e" of the float (integral values as "3."), same CRT rounding rule
inline std::string etoa(double v, int frac_digits);
inline std::string ftoa(float v)
{
    char buf[64];
    if (std::isnan(v)) return ".Nan";
    if (std::isinf(v)) return v < 0 ? "-.Inf" : ".Inf";
    if (std::fabs(v) < 2147483648.0f && (float)(long long)std::llround((double)v) == v) { snprintf(buf, sizeof buf, "%lld.", (long long)std::llround((double)v)); return buf; }
    return etoa((double)v, 8);
}
inline std::string dtoa(double v)
{
    char buf[512];
    if (std::isnan(v)) return ".Nan";
    if (std::isinf(v)) return v < 0 ? "-.Inf" : ".Inf";
    if (std::fabs(v) < 2147483648.0 && (double)(long long)std::llround(v) == v) { snprintf(buf, sizeof buf, "%lld.", (long long)std::llround(v)); return buf; }
    return etoa(v, 16);
}
// "%.<frac_digits>e" with exact decimal ties rounded half away from zero
inline std::string etoa(double v, int frac_digits)
{
    char buf[512];
    snprintf(buf, sizeof buf, "%.60e", v);          // glibc prints the exact expansion
    std::string s(buf);
    const size_t epos = s.find('e');
    std::string mant = s.substr(0, epos), ex = s.substr(epos + 1);
    const bool neg = mant[0] == '-';
    if (neg) mant = mant.substr(1);
    std::string digits; digits += mant[0]; digits += mant.substr(2);          // d.ddddd -> "ddddd..."
    int e10 = std::atoi(ex.c_str());
    const int nd = frac_digits + 1;
    const bool up = digits[nd] >= '5';                                          // >= half -> away from zero (exact ties included)
    std::string dn = digits.substr(0, nd);
    if (up) {
        int i = nd - 1;
        while (i >= 0) { if (dn[i] == '9') { dn[i] = '0'; --i; } else { dn[i]++; break; } }
        if (i < 0) { dn = "1" + dn.substr(0, nd - 1); ++e10; }
    }
    snprintf(buf, sizeof buf, "%s%c.%se%c%02d", neg ? "-" : "", dn[0], dn.substr(1).c_str(), e10 < 0 ? '-' : '+', e10 < 0 ? -e10 : e10);
    return buf;
}
struct Emitter {
    std::string out, cur;
    void line(const std::string& s) { out += s; out += '\n'; }
    void flow(const std::string& prefix, const std::vector<std::string>& tok, size_t indent)
    {
        cur = prefix + "[";
        bool first = true;
        for (const auto& t : tok) {
            if (!first) cur += ",";
            if (cur.size() + t.size() > 71 && cur.size() > indent) { line(cur); cur.assign(indent, ' '); }
            else cur += " ";
            cur += t; first = false;
        }
        cur += " ]"; line(cur); cur.clear();
    }
};
}  // namespace detail

inline void save_structure(std::string file_name, std::vector<Mat>& rotations, std::vector<Mat>& motions,
                           std::vector<Point3d>& structure, std::vector<Vec3b>& colors)
{
    detail::Emitter e;
    e.line("%YAML:1.0"); e.line("---");
    e.line("Camera Count: " + std::to_string(rotations.size()));
    e.line("Point Count: " + std::to_string(structure.size()));
    auto mats = [&](const char* name, std::vector<Mat>& ms) {
        e.line(std::string(name) + ":");
        for (auto& m : ms) {
            e.line("   - !!opencv-matrix"); e.line("      rows: " + std::to_string(m.rows)); e.line("      cols: " + std::to_string(m.cols)); e.line("      dt: d");
            std::vector<std::string> tok;
            for (int i = 0; i < m.rows * m.cols; ++i) tok.push_back(detail::dtoa(m.ptr<double>()[i]));
            e.flow("      data: ", tok, 10);
        }
    };
    mats("Rotations", rotations); mats("Motions", motions);
    e.line("Points:");
    for (const auto& p : structure) e.flow("   - ", { detail::dtoa(p.x), detail::dtoa(p.y), detail::dtoa(p.z) }, 7);
    e.line("Colors:");
    for (const auto& c : colors) e.flow("   - ", { std::to_string(c[0]), std::to_string(c[1]), std::to_string(c[2]) }, 7);
    std::ofstream f(file_name, std::ios::out | std::ios::binary);
    f << e.out;
}

// TwoViewReconstruct.cpp:313-356: `structure` is the homogeneous 4 x N float matrix; each column is divided by its w in
// float32 (Mat_<float> c; c /= c(3)) and written as a Point3f, i.e. "%.8e" tokens (fs::floatToString [3P])
inline void save_structure(std::string file_name, std::vector<Mat>& rotations, std::vector<Mat>& motions, Mat& structure,
                           std::vector<Vec3b>& colors)
{
    detail::Emitter e;
    e.line("%YAML:1.0"); e.line("---");
    e.line("Camera Count: " + std::to_string(rotations.size()));
    e.line("Point Count: " + std::to_string(structure.cols));
    auto mats = [&](const char* name, std::vector<Mat>& ms) {
        e.line(std::string(name) + ":");
        for (auto& m : ms) {
            e.line("   - !!opencv-matrix"); e.line("      rows: " + std::to_string(m.rows)); e.line("      cols: " + std::to_string(m.cols)); e.line("      dt: d");
            std::vector<std::string> tok;
            for (int i = 0; i < m.rows * m.cols; ++i) tok.push_back(detail::dtoa(m.ptr<double>()[i]));
            e.flow("      data: ", tok, 10);
        }
    };
    mats("Rotations", rotations); mats("Motions", motions);
    e.line("Points:");
    for (int i = 0; i < structure.cols; ++i) {
        const float w = structure.at<float>(3, i);
        // cv::Mat /= scalar multiplies by the reciprocal taken in double and rounds to float [3P]
        const double rw = 1.0 / (double)w;
        const float x = (float)((double)structure.at<float>(0, i) * rw), y = (float)((double)structure.at<float>(1, i) * rw),
                    z = (float)((double)structure.at<float>(2, i) * rw);
        e.flow("   - ", { detail::ftoa(x), detail::ftoa(y), detail::ftoa(z) }, 7);
    }
    e.line("Colors:");
    for (const auto& c : colors) e.flow("   - ", { std::to_string(c[0]), std::to_string(c[1]), std::to_string(c[2]) }, 7);
    std::ofstream f(file_name, std::ios::out | std::ios::binary);
    f << e.out;
}

inline int get_ply_pts3d(const std::vector<Point3d>& pts3d, const std::vector<Point3d>& normals, const std::vector<Vec3b>& colors,
                         std::vector<Pt3DPly>& pts3d_ply)
{
    if (pts3d.size() != normals.size() || pts3d.size() != colors.size()) { printf("[Err]: items size not equal.\n"); return -1; }
    pts3d_ply.resize(pts3d.size());
    for (size_t i = 0; i < pts3d.size(); ++i) {
        Pt3DPly p;
        p.x = (float)pts3d[i].x; p.y = (float)pts3d[i].y; p.z = (float)pts3d[i].z;
        p.nx = (float)normals[i].x; p.ny = (float)normals[i].y; p.nz = (float)normals[i].z;
        p.b = colors[i][0]; p.g = colors[i][1]; p.r = colors[i][2];
        pts3d_ply[i] = p;
    }
    printf("Total %zd 3D points.\n", pts3d.size());
    return 0;
}

inline void write_ply_binary(const std::string& path, const std::vector<Pt3DPly>& points)
{
    auto bad = [](const Pt3DPly& p) { return std::isnan(p.x) || std::isnan(p.y) || std::isnan(p.z) || std::isnan(p.nx) || std::isnan(p.ny) || std::isnan(p.nz); };
    size_t valid = 0;
    for (const auto& p : points) if (!bad(p)) ++valid;
    std::ofstream f(path, std::ios::out | std::ios::binary);
    assert(f.is_open());
    f << "ply\nformat binary_little_endian 1.0\nelement vertex " << valid << "\nproperty float x\nproperty float y\nproperty float z\n"
         "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n";
    for (const auto& p : points) {
        if (bad(p)) continue;
        f.write((const char*)&p.x, 4); f.write((const char*)&p.y, 4); f.write((const char*)&p.z, 4);
        f.write((const char*)&p.nx, 4); f.write((const char*)&p.ny, 4); f.write((const char*)&p.nz, 4);
        f.write((const char*)&p.r, 1); f.write((const char*)&p.g, 1); f.write((const char*)&p.b, 1);
    }
}

// a triangle mesh as a binary little-endian .ply: write_ply_binary's vertex element (the colours (b, g, r) rows written red, green, blue),
// then `element face` with a uchar count of 3 and three int32 per face.  Without normals the nx ny nz fields are zero and the file is
// what it has always been; with them (one per vertex) they are written as floats and the header carries a comment line that says so
// (formats.MESH_NORMALS_COMMENT in the Python writer, which this mirrors byte for byte)
inline void write_mesh_ply(const std::string& path, const std::vector<Point3d>& pts, const std::vector<Vec3b>& colors, const std::vector<int32_t>& tris,
                           const std::vector<Point3d>* normals = nullptr)
{
    assert(pts.size() == colors.size() && tris.size() % 3 == 0 && (!normals || normals->size() == pts.size()));
    std::ofstream f(path, std::ios::out | std::ios::binary);
    assert(f.is_open());
    f << "ply\nformat binary_little_endian 1.0\n" << (normals ? "comment normals area-weighted per vertex\n" : "") << "element vertex " << pts.size()
      << "\nproperty float x\nproperty float y\nproperty float z\n"
         "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
         "element face " << tris.size() / 3 << "\nproperty list uchar int vertex_indices\nend_header\n";
    for (size_t i = 0; i < pts.size(); ++i) {
        const float v[6] = { (float)pts[i].x, (float)pts[i].y, (float)pts[i].z, normals ? (float)(*normals)[i].x : 0.0f, normals ? (float)(*normals)[i].y : 0.0f,
                             normals ? (float)(*normals)[i].z : 0.0f };
        const uint8_t rgb[3] = { colors[i][2], colors[i][1], colors[i][0] };
        f.write((const char*)v, 24); f.write((const char*)rgb, 3);
    }
    const uint8_t three = 3;
    for (size_t i = 0; i < tris.size(); i += 3) { f.write((const char*)&three, 1); f.write((const char*)&tris[i], 12); }
}

}  // namespace sfm
