// planes.hip -- RANSAC plane segmentation of a 3-D point cloud, one plane or several peeled off one after another (Open3D segment_plane,
// PCL SACSegmentation with SACMODEL_PLANE; the definition is in sfmhip.h at sfmhip_segment_planes and is followed to the letter here:
// the labels, counts and winners are integer decisions on prescribed fp64 values, the same for every run and launch geometry).
//
// A round p, everything on the device and on one stream:
//   plane_flag_kernel / scan / plane_scatter_kernel   the ACTIVE list: the finite points that still carry label -1, packed in ascending
//                                                     original index into rows of four doubles (x, y, z, 0); its length m stays in the state
//   plane_hyp_kernel                                  one thread per hypothesis: the triple from splitmix64, the plane, a valid bit
//   plane_score_kernel                                the H x m part: count of the active points within t of every hypothesis
//   plane_winner_kernel                               one workgroup: the valid hypothesis with the largest count, the smallest h among
//                                                     equals; writes the plane / count / winner of the round or raises the stop flag
//   plane_label_kernel                                the winner's inliers get label p (plane_residual, the function the scoring used)
//   plane_refit_tile_kernel / plane_refit_top_kernel  (where the refined plane is wanted) mean, then covariance of the points labelled p
//                                                     in fixed-order trees, eig3_min, the same sign rule
// All max_planes rounds are enqueued; the stop flag and m live in device memory, and after the stop every kernel of a round leaves at
// once (the launches cover an upper bound, n points).
//
// plane_score_kernel is the scoring loop of ransac.hpp, which explains its shape, with PlaneModel: a lane keeps its plane in 8 VGPRs, and
// per point a wave issues 3 fp64 mul + 3 fp64 add (contraction is off: the residual is the prescribed formula), a compare on |e| and a
// conditional add: eight VALU instructions, which is what bounds the kernel (measured and accounted for in DESIGN.md 4b; a variant with
// two hypotheses per lane, half the LDS reads per residual, was 3 % faster and was not kept).  The sampler and the winner reduction are
// ransac.hpp's too; what is here is the plane: its active list, its three-point hypothesis, its residual, what a round writes, the refit.
#include "common.hpp"
#include "sortscan.hpp"
#pragma clang fp contract(off)
#include "eig3.hpp"
#include "ransac.hpp"

#define REFIT_TILE 4096
#define PLANES_H_MAX 65536
#define PLANES_MAX 64

// what the rounds share, in device memory
struct PlaneState {
    int stop;                 // raised by the round that finds no plane; every later kernel leaves at once
    int m;                    // length of the active list of the current round
    int pad[2];
    double wplane[4];         // the winner's plane of the current round as computed (before the sign rule)
    double mean[3], cnt;      // refit: mean and number of the points labelled with the current round
};
__device__ __forceinline__ bool round_dead(const PlaneState* s) { return s->stop || s->m < 3; }

// THE residual: scoring and labelling both call this, so the number of points labelled equals the winner's count by construction
__device__ __forceinline__ double plane_residual(double a, double b, double c, double d, double x, double y, double z)
{
    return ((a * x + b * y) + c * z) + d;
}
__device__ __forceinline__ bool plane_inlier(double a, double b, double c, double d, double x, double y, double z, double t)
{
    return fabs(plane_residual(a, b, c, d, x, y, z)) <= t;               // false for a NaN residual (an invalid hypothesis)
}
// what the scoring loop of ransac.hpp needs to know about a plane
struct PlaneModel {
    typedef double4 Row;
    static constexpr int NPAR = 4, UNROLL = 8;
    static __device__ __forceinline__ bool inlier(const double (&P)[4], const double4& q, double t) { return plane_inlier(P[0], P[1], P[2], P[3], q.x, q.y, q.z, t); }
};
// all four components negated when d < 0
__device__ __forceinline__ void plane_store_signed(double* __restrict__ out, double a, double b, double c, double d)
{
    const bool neg = d < 0.0;
    out[0] = neg ? -a : a; out[1] = neg ? -b : b; out[2] = neg ? -c : c; out[3] = neg ? -d : d;
}

// labels -1, the per-plane outputs at their "no plane" values, the state cleared
__global__ __launch_bounds__(256) void plane_init_kernel(int32_t* __restrict__ labels, int n, int max_planes, int32_t* __restrict__ n_planes,
                                                         double* __restrict__ planes, double* __restrict__ refined, int32_t* __restrict__ counts,
                                                         int32_t* __restrict__ winner, PlaneState* __restrict__ state)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) labels[t] = -1;
    if (t < 4 * max_planes) { planes[t] = NAN; if (refined) refined[t] = NAN; }
    if (t < max_planes) { if (counts) counts[t] = 0; if (winner) winner[t] = -1; }
    if (t == 0) { *n_planes = 0; state->stop = 0; state->m = 0; }
}

// n + 1 entries: 1 for a finite point that is still unlabelled; the exclusive scan turns them into positions in the active list
__global__ __launch_bounds__(256) void plane_flag_kernel(const double* __restrict__ pts, const int32_t* __restrict__ labels, int n,
                                                         const PlaneState* __restrict__ state, pu32* __restrict__ flag)
{
    if (state->stop) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    pu32 f = 0u;
    if (i < n && labels[i] == -1) {
        const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        f = isfinite(x) && isfinite(y) && isfinite(z) ? 1u : 0u;
    }
    flag[i] = f;
}
__global__ __launch_bounds__(256) void plane_scatter_kernel(const double* __restrict__ pts, int n, const pu32* __restrict__ excl, PlaneState* __restrict__ state,
                                                            double4* __restrict__ act)
{
    if (state->stop) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) state->m = (int)excl[n];
    if (i >= n) return;
    const pu32 at = excl[i];
    if (excl[i + 1] != at) act[at] = make_double4(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], 0.0);
}

// hypothesis h of round p: hyp[4 h ..] = (a, b, c, d), NaN where it is invalid (it then counts nobody); its counter cleared
__global__ __launch_bounds__(256) void plane_hyp_kernel(const double4* __restrict__ act, const PlaneState* __restrict__ state, int p, int H, pu64 seed,
                                                        double* __restrict__ hyp, int32_t* __restrict__ hvalid, int32_t* __restrict__ hcnt)
{
    if (round_dead(state)) return;
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    pu64 u[3];
    ransac_sample_distinct<3>(seed, (pu64)p * (pu64)H + (pu64)h, (pu64)state->m, u);
    const double4 p0 = act[u[0]], p1 = act[u[1]], p2 = act[u[2]];
    const double e1x = p1.x - p0.x, e1y = p1.y - p0.y, e1z = p1.z - p0.z;
    const double e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
    const double mx = e1y * e2z - e1z * e2y, my = e1z * e2x - e1x * e2z, mz = e1x * e2y - e1y * e2x;
    const double s = sqrt((mx * mx + my * my) + mz * mz);
    const bool valid = isfinite(s) && s > 0.0;
    double a = NAN, b = NAN, c = NAN, d = NAN;
    if (valid) {
        a = mx / s; b = my / s; c = mz / s;
        d = -((a * p0.x + b * p0.y) + c * p0.z);
    }
    hyp[4 * (size_t)h] = a; hyp[4 * (size_t)h + 1] = b; hyp[4 * (size_t)h + 2] = c; hyp[4 * (size_t)h + 3] = d;
    hvalid[h] = valid ? 1 : 0;
    hcnt[h] = 0;
}

// the H x m part: ransac_score over the active list
__global__ __launch_bounds__(256) void plane_score_kernel(const double4* __restrict__ act, const PlaneState* __restrict__ state, const double* __restrict__ hyp,
                                                          int H, double t, int32_t* __restrict__ hcnt)
{
    __shared__ double4 tile[SCORE_CHUNK];
    if (round_dead(state)) return;                                       // uniform over the grid
    const int h = blockIdx.x * 256 + threadIdx.x;
    ransac_score<PlaneModel>(tile, act, state->m, h < H ? hyp + 4 * (size_t)h : nullptr, t, hcnt + h);
}

// one workgroup: argmax of (count, then the smallest h) over the valid hypotheses; the round's outputs, or the stop flag
__global__ __launch_bounds__(256) void plane_winner_kernel(PlaneState* __restrict__ state, int p, int H, int min_inliers, const double* __restrict__ hyp,
                                                           const int32_t* __restrict__ hvalid, const int32_t* __restrict__ hcnt, int32_t* __restrict__ n_planes,
                                                           double* __restrict__ planes, int32_t* __restrict__ counts, int32_t* __restrict__ winner)
{
    __shared__ pu64 sb[256];
    if (state->stop) return;
    const pu64 w = ransac_block_winner(hvalid, hcnt, state->m < 3 ? 0 : H, sb);      // a round without three active points: no hypothesis
    if (threadIdx.x != 0) return;
    if (!w || ransac_key_count(w) < min_inliers) { state->stop = 1; return; }
    const int cnt = ransac_key_count(w), h = ransac_key_h(w);
    const double a = hyp[4 * (size_t)h], b = hyp[4 * (size_t)h + 1], c = hyp[4 * (size_t)h + 2], d = hyp[4 * (size_t)h + 3];
    state->wplane[0] = a; state->wplane[1] = b; state->wplane[2] = c; state->wplane[3] = d;
    plane_store_signed(planes + 4 * (size_t)p, a, b, c, d);
    if (counts) counts[p] = cnt;
    if (winner) winner[p] = h;
    *n_planes = p + 1;
}

// the winner's inliers among the points the round's active list was made of
__global__ __launch_bounds__(256) void plane_label_kernel(const double* __restrict__ pts, int n, const PlaneState* __restrict__ state, int p, double t,
                                                          int32_t* __restrict__ labels)
{
    if (state->stop) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || labels[i] != -1) return;
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
    if (plane_inlier(state->wplane[0], state->wplane[1], state->wplane[2], state->wplane[3], x, y, z, t)) labels[i] = p;
}

// ------------------------------------------------------------------------------------------------
// the refined plane: least squares over the points labelled p.  Two passes of (tile partials, one workgroup over the tiles), every sum a
// fixed-order tree.  pass 0: (sum x, sum y, sum z, count) -> mean;  pass 1: the six sums of products of (x - mean) -> covariance / count,
// eig3_min, normalised, d = -(n . mean), the sign rule of the RANSAC plane.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void block_tree_sum6(double (&v)[6], double (*sv)[256])
{
#pragma unroll
    for (int k = 0; k < 6; ++k) sv[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int k = 0; k < 6; ++k) sv[k][threadIdx.x] += sv[k][threadIdx.x + off];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = sv[k][0];
}
__global__ __launch_bounds__(256) void plane_refit_tile_kernel(const double* __restrict__ pts, const int32_t* __restrict__ labels, int n, int p, int pass,
                                                               const PlaneState* __restrict__ state, double* __restrict__ partial)
{
    __shared__ double sv[6][256];
    if (state->stop) return;
    const double mx = pass ? state->mean[0] : 0.0, my = pass ? state->mean[1] : 0.0, mz = pass ? state->mean[2] : 0.0;
    double v[6] = { 0, 0, 0, 0, 0, 0 };
    for (int r = 0; r < REFIT_TILE / 256; ++r) {
        const size_t i = (size_t)blockIdx.x * REFIT_TILE + (size_t)r * 256 + threadIdx.x;
        if (i < (size_t)n && labels[i] == p) {
            const double x = pts[3 * i] - mx, y = pts[3 * i + 1] - my, z = pts[3 * i + 2] - mz;
            if (pass) { v[0] += x * x; v[1] += x * y; v[2] += x * z; v[3] += y * y; v[4] += y * z; v[5] += z * z; }
            else { v[0] += x; v[1] += y; v[2] += z; v[3] += 1.0; }
        }
    }
    block_tree_sum6(v, sv);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) partial[6 * (size_t)blockIdx.x + k] = v[k];
}
__global__ __launch_bounds__(256) void plane_refit_top_kernel(const double* __restrict__ partial, int nt, int p, int pass, PlaneState* __restrict__ state,
                                                              double* __restrict__ refined)
{
    __shared__ double sv[6][256];
    if (state->stop) return;
    double v[6] = { 0, 0, 0, 0, 0, 0 };
    for (int t = threadIdx.x; t < nt; t += 256)
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] += partial[6 * (size_t)t + k];
    block_tree_sum6(v, sv);
    if (threadIdx.x != 0) return;
    if (pass == 0) {
        state->mean[0] = v[0] / v[3]; state->mean[1] = v[1] / v[3]; state->mean[2] = v[2] / v[3]; state->cnt = v[3];
        return;
    }
    const double cnt = state->cnt;
    const double C[9] = { v[0] / cnt, v[1] / cnt, v[2] / cnt, v[1] / cnt, v[3] / cnt, v[4] / cnt, v[2] / cnt, v[4] / cnt, v[5] / cnt };
    double e[3];
    eig3_min(C, e);
    const double nn = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    const double a = e[0] / nn, b = e[1] / nn, c = e[2] / nn;
    const double d = -((a * state->mean[0] + b * state->mean[1]) + c * state->mean[2]);
    plane_store_signed(refined + 4 * (size_t)p, a, b, c, d);
}

__global__ __launch_bounds__(256) void plane_keep_kernel(const int32_t* __restrict__ labels, int n, uint8_t* __restrict__ keep)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keep[i] = labels[i] == 0 ? 1 : 0;
}

// every round on the context's stream; d_refined / d_counts / d_winner may be null
static int planes_enqueue(sfmhip_ctx* ctx, const double* d_pts, int n, double t, int H, pu64 seed, int min_inliers, int max_planes, int32_t* d_labels,
                          int32_t* d_n_planes, double* d_planes, double* d_refined, int32_t* d_counts, int32_t* d_winner)
{
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)n;
    const int nb = ceil_div(n, 256), nb1 = ceil_div(n + 1, 256), hb = ceil_div(H, 256), nt = ceil_div(n, REFIT_TILE);
    const int gy = ransac_score_grid_y(n, hb);
    SfmCarve carve;
    const size_t o_state = carve(sizeof(PlaneState)), o_act = carve(N * sizeof(double4)), o_hyp = carve((size_t)H * 4 * sizeof(double)),
                 o_val = carve((size_t)H * 4), o_cnt = carve((size_t)H * 4), o_part = carve(d_refined ? (size_t)6 * nt * sizeof(double) : 0);
    SfmScan F(carve, N + 1);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    F.bind(w);
    PlaneState* state = (PlaneState*)(w + o_state);
    pu32* flag = F.data;
    double4* act = (double4*)(w + o_act);
    double* hyp = (double*)(w + o_hyp);
    int32_t *hvalid = (int32_t*)(w + o_val), *hcnt = (int32_t*)(w + o_cnt);
    double* part = (double*)(w + o_part);
    hipLaunchKernelGGL(plane_init_kernel, dim3(ceil_div(std::max(n, 4 * max_planes), 256)), dim3(256), 0, st, d_labels, n, max_planes, d_n_planes, d_planes,
                       d_refined, d_counts, d_winner, state);
    for (int p = 0; p < max_planes; ++p) {
        hipLaunchKernelGGL(plane_flag_kernel, dim3(nb1), dim3(256), 0, st, d_pts, (const int32_t*)d_labels, n, (const PlaneState*)state, flag);
        F.scan(st, N + 1);
        hipLaunchKernelGGL(plane_scatter_kernel, dim3(nb), dim3(256), 0, st, d_pts, n, (const pu32*)flag, state, act);
        hipLaunchKernelGGL(plane_hyp_kernel, dim3(hb), dim3(256), 0, st, (const double4*)act, (const PlaneState*)state, p, H, seed, hyp, hvalid, hcnt);
        hipLaunchKernelGGL(plane_score_kernel, dim3(hb, gy), dim3(256), 0, st, (const double4*)act, (const PlaneState*)state, (const double*)hyp, H, t, hcnt);
        hipLaunchKernelGGL(plane_winner_kernel, dim3(1), dim3(256), 0, st, state, p, H, min_inliers, (const double*)hyp, (const int32_t*)hvalid,
                           (const int32_t*)hcnt, d_n_planes, d_planes, d_counts, d_winner);
        hipLaunchKernelGGL(plane_label_kernel, dim3(nb), dim3(256), 0, st, d_pts, n, (const PlaneState*)state, p, t, d_labels);
        if (d_refined)
            for (int pass = 0; pass < 2; ++pass) {
                hipLaunchKernelGGL(plane_refit_tile_kernel, dim3(nt), dim3(256), 0, st, d_pts, (const int32_t*)d_labels, n, p, pass, (const PlaneState*)state, part);
                hipLaunchKernelGGL(plane_refit_top_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nt, p, pass, state, d_refined);
            }
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

static inline bool planes_args_ok(const sfmhip_ctx* ctx, int n, double t, int H, int min_inliers, int max_planes)
{
    return ctx && n >= 0 && std::isfinite(t) && t >= 0.0 && H >= 1 && H <= PLANES_H_MAX && min_inliers >= 3 && max_planes >= 1 && max_planes <= PLANES_MAX;
}

// the segmentation of a host cloud and, where keep is given, the mask of plane 0: the body of the two host entry points
static int planes_host(sfmhip_ctx* ctx, const double* pts, int n, double t, int H, pu64 seed, int min_inliers, int max_planes, int32_t* labels, int* n_planes,
                       double* planes, double* refined, int32_t* counts, int32_t* winner, uint8_t* keep)
{
    SfmPoolHold hold(ctx);
    double* d_p = nullptr; int32_t* d_lab = nullptr; uint8_t* d_keep = nullptr; char* d_head = nullptr;
    // n_planes, then planes, refined, counts, winner
    const size_t o_pl = 256, o_rf = o_pl + align256((size_t)max_planes * 32), o_ct = o_rf + align256((size_t)max_planes * 32),
                 o_wn = o_ct + align256((size_t)max_planes * 4), head_bytes = o_wn + align256((size_t)max_planes * 4);
    int rc = sfm_upload_async(ctx, hold, pts, 3 * (size_t)n, d_p);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * sizeof(int32_t), (void**)&d_lab);
    if (rc == SFMHIP_OK && keep) rc = hold.get((size_t)n, (void**)&d_keep);
    if (rc == SFMHIP_OK) rc = hold.get(head_bytes, (void**)&d_head);
    if (rc == SFMHIP_OK)
        rc = planes_enqueue(ctx, d_p, n, t, H, seed, min_inliers, max_planes, d_lab, (int32_t*)d_head, (double*)(d_head + o_pl),
                            refined ? (double*)(d_head + o_rf) : nullptr, (int32_t*)(d_head + o_ct), (int32_t*)(d_head + o_wn));
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    if (keep) {
        hipLaunchKernelGGL(plane_keep_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const int32_t*)d_lab, n, d_keep);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, st);
    }
    int32_t np = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&np, d_head, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && labels) e = hipMemcpyAsync(labels, d_lab, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(planes, d_head + o_pl, (size_t)max_planes * 32, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && refined) e = hipMemcpyAsync(refined, d_head + o_rf, (size_t)max_planes * 32, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && counts) e = hipMemcpyAsync(counts, d_head + o_ct, (size_t)max_planes * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && winner) e = hipMemcpyAsync(winner, d_head + o_wn, (size_t)max_planes * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    rc = sfm_finish(ctx, e);
    if (rc == SFMHIP_OK && n_planes) *n_planes = np;
    return rc;
}

extern "C" {

int sfmhip_segment_planes_dev(sfmhip_ctx* ctx, const double* d_pts, int n, double t, int H, uint64_t seed, int min_inliers, int max_planes, int32_t* d_labels,
                              int32_t* d_n_planes, double* d_planes, double* d_refined, int32_t* d_counts, int32_t* d_winner)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_segment_planes_dev");
    SFM_ARG_CHECK(ctx, planes_args_ok(ctx, n, t, H, min_inliers, max_planes));
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, d_pts && d_labels && d_n_planes && d_planes);
    return planes_enqueue(ctx, d_pts, n, t, H, (pu64)seed, min_inliers, max_planes, d_labels, d_n_planes, d_planes, d_refined, d_counts, d_winner);
}

int sfmhip_segment_planes(sfmhip_ctx* ctx, const double* pts, int n, double t, int H, uint64_t seed, int min_inliers, int max_planes, int32_t* labels,
                          int* n_planes, double* planes, double* refined, int32_t* counts, int32_t* winner)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_segment_planes");
    SFM_ARG_CHECK(ctx, planes_args_ok(ctx, n, t, H, min_inliers, max_planes));
    if (n == 0) { if (n_planes) *n_planes = 0; return SFMHIP_OK; }
    SFM_ARG_CHECK(ctx, pts && labels && n_planes && planes);
    return planes_host(ctx, pts, n, t, H, (pu64)seed, min_inliers, max_planes, labels, n_planes, planes, refined, counts, winner, nullptr);
}

int sfmhip_segment_plane(sfmhip_ctx* ctx, const double* pts, int n, double t, int H, uint64_t seed, int min_inliers, double plane[4], uint8_t* keep, int* count,
                         double refined[4])
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_segment_plane");
    SFM_ARG_CHECK(ctx, planes_args_ok(ctx, n, t, H, min_inliers, 1));
    if (n == 0) { if (count) *count = 0; return SFMHIP_OK; }
    SFM_ARG_CHECK(ctx, pts && plane && keep);
    int32_t cnt = 0;
    const int rc = planes_host(ctx, pts, n, t, H, (pu64)seed, min_inliers, 1, nullptr, nullptr, plane, refined, &cnt, nullptr, keep);
    if (rc == SFMHIP_OK && count) *count = cnt;
    return rc;
}

}
