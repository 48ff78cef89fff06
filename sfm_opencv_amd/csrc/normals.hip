// normals.hip -- point-cloud normals for the .ply writer ("next" row 8f-1; replaces estimate_normals
// NViewReconstuct.cpp:551-599 and PCAFitPlane 601-690).
//
// The reference pushes ALL other points into a priority_queue per point (O(N^2 log N) on the host) and pops the
// K nearest; here one thread per point streams the cloud through LDS tiles and keeps a sorted top-16 in
// registers (ordering: distance, then index -- any order among equal distances is a valid K-set for the
// reference).  Then the plane fit of PCAFitPlane: mean of the K neighbours, covariance / K, eigenvector of the
// smallest eigenvalue (cyclic Jacobi instead of Eigen::EigenSolver), flipped when n . mean > 0 (NView:672),
// normalised.  fp64 throughout, no FMA contraction so distances compare exactly like the host's.
// The contract with oracle/orc_normals.c (tests/test_normals_fit_gpu.py: equal in every bit): both sides are compiled with
// -ffp-contract=off, fp64 sqrt and division are the correctly rounded ones on both, and plane_fit / eig3_min keep the oracle's order.
#include "common.hpp"
#pragma clang fp contract(off)
#include "eig3.hpp"

#define KMAX 16
#define NTILE 256

// plane fit of point i on the neighbours bi[0 .. K) (-1: none), in that order
__device__ __forceinline__ void plane_fit(const double* __restrict__ pts, const int (&bi)[KMAX], int K, int i, double* __restrict__ normals)
{
    int cnt = 0;
    double mean[3] = { 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K && bi[k] >= 0) {
            mean[0] += pts[3 * (size_t)bi[k]]; mean[1] += pts[3 * (size_t)bi[k] + 1]; mean[2] += pts[3 * (size_t)bi[k] + 2];
            ++cnt;
        }
    if (cnt == 0) { normals[3 * (size_t)i] = NAN; normals[3 * (size_t)i + 1] = NAN; normals[3 * (size_t)i + 2] = NAN; return; }
    mean[0] /= (double)cnt; mean[1] /= (double)cnt; mean[2] /= (double)cnt;
    double C[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K && bi[k] >= 0) {
            const double d[3] = { pts[3 * (size_t)bi[k]] - mean[0], pts[3 * (size_t)bi[k] + 1] - mean[1], pts[3 * (size_t)bi[k] + 2] - mean[2] };
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) C[3 * a + b] += d[a] * d[b];
        }
#pragma unroll
    for (int a = 0; a < 9; ++a) C[a] /= (double)cnt;
    double v[3];
    eig3_min(C, v);
    if (v[0] * mean[0] + v[1] * mean[1] + v[2] * mean[2] > 0.0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
    const double nn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    normals[3 * (size_t)i] = v[0] / nn; normals[3 * (size_t)i + 1] = v[1] / nn; normals[3 * (size_t)i + 2] = v[2] / nn;
}

__global__ __launch_bounds__(NTILE) void normals_kernel(const double* __restrict__ pts, int n, int K, double* __restrict__ normals)
{
    __shared__ double tx[NTILE], ty[NTILE], tz[NTILE];
    const int i = blockIdx.x * NTILE + threadIdx.x;
    const bool active = i < n;
    const double px = active ? pts[3 * (size_t)i] : 0.0, py = active ? pts[3 * (size_t)i + 1] : 0.0, pz = active ? pts[3 * (size_t)i + 2] : 0.0;
    double bd[KMAX]; int bi[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { bd[k] = INFINITY; bi[k] = -1; }
    // Squared-distance gate in front of the exact test: sqrt(d2) < bd[last] is impossible once d2 > bd[last]^2 (1 + 2^-50) (the real
    // root then exceeds bd[last], and rounding is monotone), so the fp64 square root -- two thirds of the instructions of a candidate --
    // is taken only by candidates that can still enter the list.  Same K-sets, same order, bit for bit (round 3: 113 -> see profiles/).
    double gate2 = INFINITY;
    for (int base = 0; base < n; base += NTILE) {
        const int j0 = base + threadIdx.x;
        __syncthreads();
        if (j0 < n) { tx[threadIdx.x] = pts[3 * (size_t)j0]; ty[threadIdx.x] = pts[3 * (size_t)j0 + 1]; tz[threadIdx.x] = pts[3 * (size_t)j0 + 2]; }
        __syncthreads();
        const int cnt = n - base < NTILE ? n - base : NTILE;
        for (int t = 0; t < cnt; ++t) {
            const int j = base + t;
            const double dx = px - tx[t], dy = py - ty[t], dz = pz - tz[t];
            const double d2 = dx * dx + dy * dy + dz * dz;
            if (!(d2 <= gate2)) continue;
            const double d = sqrt(d2);
            if (j != i && d < bd[KMAX - 1]) {
                bd[KMAX - 1] = d; bi[KMAX - 1] = j;
#pragma unroll
                for (int k = KMAX - 1; k > 0; --k) {
                    if (bd[k] < bd[k - 1]) {
                        const double td = bd[k]; bd[k] = bd[k - 1]; bd[k - 1] = td;
                        const int ti = bi[k]; bi[k] = bi[k - 1]; bi[k - 1] = ti;
                    }
                }
                gate2 = bd[KMAX - 1] * bd[KMAX - 1] * (1.0 + 0x1p-50);       // inf while the list is not full
            }
        }
    }
    if (!active) return;
    plane_fit(pts, bi, K, i, normals);
}

// the same fit on a neighbour table (sfm_points_knn_enqueue): the grid search finds the K-sets, in the order of the sweep above
__global__ __launch_bounds__(NTILE) void normals_from_knn_kernel(const double* __restrict__ pts, const int32_t* __restrict__ idx, int n, int K, double* __restrict__ normals)
{
    const int i = blockIdx.x * NTILE + threadIdx.x;
    if (i >= n) return;
    int bi[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) bi[k] = k < K ? idx[(size_t)i * K + k] : -1;
    plane_fit(pts, bi, K, i, normals);
}

// radius-limited ("hybrid") neighbourhoods: an entry of the table farther than r is no neighbour (plane_fit skips -1)
__global__ __launch_bounds__(256) void normals_radius_mask_kernel(int32_t* __restrict__ idx, const double* __restrict__ dist, size_t total, double r)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < total && dist[t] > r) idx[t] = -1;
}

int sfm_normals_from_knn_enqueue(sfmhip_ctx* ctx, const double* d_pts, const int32_t* d_idx, int n, int K, double* d_normals)
{
    hipLaunchKernelGGL(normals_from_knn_kernel, dim3(ceil_div(n, NTILE)), dim3(NTILE), 0, ctx->stream, d_pts, d_idx, n, K, d_normals);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

extern "C" int sfmhip_estimate_normals_ex(sfmhip_ctx* ctx, const double* pts, int n, int K, int method, double* normals)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_estimate_normals");
    SFM_ARG_CHECK(ctx, ctx && n >= 0 && K >= 1 && K <= KMAX);
    SFM_ARG_CHECK(ctx, points_method_ok(method));
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, pts && normals);
    if (method == SFMHIP_POINTS_AUTO) method = sfm_points_auto_method(n);
    SfmPoolHold hold(ctx);
    double *d_p = nullptr, *d_n = nullptr; int32_t* d_idx = nullptr;
    int rc = sfm_upload_async(ctx, hold, pts, 3 * (size_t)n, d_p);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * 24, (void**)&d_n);
    if (rc == SFMHIP_OK && method == SFMHIP_POINTS_GRID) rc = hold.get((size_t)n * K * sizeof(int32_t), (void**)&d_idx);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    if (method == SFMHIP_POINTS_GRID) {
        rc = sfm_points_knn_enqueue(ctx, d_p, n, K, method, d_idx, nullptr);
        if (rc == SFMHIP_OK) rc = sfm_normals_from_knn_enqueue(ctx, d_p, d_idx, n, K, d_n);
        if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    } else {
        hipLaunchKernelGGL(normals_kernel, dim3(ceil_div(n, NTILE)), dim3(NTILE), 0, ctx->stream, d_p, n, K, d_n);
        SFM_HIP_TRY(ctx, hipGetLastError());
    }
    return sfm_finish(ctx, hipMemcpyAsync(normals, d_n, (size_t)n * 24, hipMemcpyDeviceToHost, ctx->stream));
}

extern "C" int sfmhip_estimate_normals(sfmhip_ctx* ctx, const double* pts, int n, int K, double* normals)
{
    return sfmhip_estimate_normals_ex(ctx, pts, n, K, SFMHIP_POINTS_AUTO, normals);
}

extern "C" int sfmhip_estimate_normals_hybrid(sfmhip_ctx* ctx, const double* pts, int n, int K, double r, int method, double* normals)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_estimate_normals_hybrid");
    SFM_ARG_CHECK(ctx, ctx && n >= 0 && K >= 1 && K <= KMAX && std::isfinite(r) && r >= 0.0);
    SFM_ARG_CHECK(ctx, points_method_ok(method));
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, pts && normals);
    SfmPoolHold hold(ctx);
    double *d_p = nullptr, *d_n = nullptr, *d_dist = nullptr; int32_t* d_idx = nullptr;
    const size_t total = (size_t)n * K;
    int rc = sfm_upload_async(ctx, hold, pts, 3 * (size_t)n, d_p);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * 24, (void**)&d_n);
    if (rc == SFMHIP_OK) rc = hold.get(total * sizeof(int32_t), (void**)&d_idx);
    if (rc == SFMHIP_OK) rc = hold.get(total * sizeof(double), (void**)&d_dist);
    if (rc == SFMHIP_OK) rc = sfm_points_knn_enqueue(ctx, d_p, n, K, method, d_idx, d_dist);
    if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(normals_radius_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_idx, (const double*)d_dist, total, r);
        rc = sfm_normals_from_knn_enqueue(ctx, d_p, d_idx, n, K, d_n);
    }
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    return sfm_finish(ctx, hipMemcpyAsync(normals, d_n, (size_t)n * 24, hipMemcpyDeviceToHost, ctx->stream));
}
