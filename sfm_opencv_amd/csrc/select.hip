// select.hip -- what the dense stage needs from the sparse model (sfmhip_select_views): the covisibility matrices of the views, every
// view's source views ranked by the sparse points it shares with them under a sufficient triangulation angle, and every view's
// inverse-depth range from the points it sees.  The definition is in include/sfmhip.h and restated in tests/select_ref.py; every output
// is integer counts or fp64 evaluated in the written order with contraction off, so the outputs are the same bits for every run and
// launch geometry.
//
// How it runs, all on the context's stream, nothing synchronises:
//   1. select_key_kernel        (point << 12 | view) per observation; an observation that does not count gets the key past all others
//   2. SfmSort                  one sort groups the observations by point, the views of a point ascending
//   3. sfm_enqueue_run_heads    a key equal to its left neighbour is a repeated (point, view) pair: it takes part in nothing below
//   4. select_geo_kernel        Rinv and c of the views, computed on the host, arrive as kernel arguments
//      select_ray_kernel        a = X - c and z per distinct pair; the keys of the depth lists
//   5. select_pair_kernel       a thread per pair walks the later views of its point: sum over the tracks of L (L - 1) / 2 visits.  The
//                               adds of a wave's visits are settled by ballot first (as mesh_cc_sizes_kernel settles its labels): in a
//                               two-view scene every visit of a wave lands on one counter and leaves as one add
//   6. select_mirror_kernel     the pair kernel counts i < j only; the lower triangles are copies
//   7. select_rank_kernel       one wave per view over its row of the score matrix, one selection round per source
//   8. SfmSort twice            by the bit pattern of z (positive doubles order as unsigned integers), then stably by view: every view's
//                               depths in ascending order, no second sort in the library
//   9. select_range_kernel      a thread per view finds its segment by bisection and reads the two order statistics
// Integer atomics only: any order of the adds gives the same counts.
#include "sortscan.hpp"

#include <cmath>

#pragma clang fp contract(off)

typedef unsigned long long vu64;
typedef unsigned int vu32;

#define SEL_VIEW_BITS 12
#define SEL_VIEWS_MAX (1 << SEL_VIEW_BITS)
#define SEL_SRC_MAX 8
#define SEL_SETTLE_ROUNDS 4
#define SEL_GEO_VIEWS 32

struct __attribute__((aligned(32))) SelRay { double a0, a1, a2, z; };

__device__ __forceinline__ bool sel_finite(double x) { return ((vu64)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

__global__ __launch_bounds__(256) void select_key_kernel(const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_pt, const double* __restrict__ pts,
                                                         size_t n, int n_views, int n_pt, vu64* __restrict__ keys)
{
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n) return;
    const int cam = obs_cam[o], pt = obs_pt[o];
    bool ok = cam >= 0 && cam < n_views && pt >= 0 && pt < n_pt;
    if (ok) {
        const double* X = pts + 3 * (size_t)pt;
        ok = sel_finite(X[0]) && sel_finite(X[1]) && sel_finite(X[2]);
    }
    keys[o] = ok ? ((vu64)pt << SEL_VIEW_BITS | (vu64)cam) : ((vu64)n_pt << SEL_VIEW_BITS);
}

// The geometry reaches the device as kernel arguments, SEL_GEO_VIEWS views a launch: a copy from the caller's pageable memory would make
// the _dev form wait for the stream.
struct SelGeoChunk { double g[SEL_GEO_VIEWS * 12]; };
__global__ __launch_bounds__(128) void select_geo_kernel(const SelGeoChunk chunk, int count, double* __restrict__ out)
{
    const int t = (int)(blockIdx.x * 128u + threadIdx.x);
    if (t < count) out[t] = chunk.g[t];
}

// geo: twelve doubles per view, Rinv (row-major) and c of sfmhip_sweep_geometry
__global__ __launch_bounds__(256) void select_ray_kernel(const vu64* __restrict__ keys, const vu32* __restrict__ head, const double* __restrict__ pts,
                                                         const double* __restrict__ geo, size_t n, int n_views, SelRay* __restrict__ ray,
                                                         vu64* __restrict__ zkey, vu32* __restrict__ zview)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    SelRay r = { 0.0, 0.0, 0.0, 0.0 };
    vu64 zk = ~0ull; vu32 zv = (vu32)n_views;
    if (head[e]) {
        const vu64 k = keys[e];
        const int i = (int)(k & (SEL_VIEWS_MAX - 1));
        const double* X = pts + 3 * (size_t)(k >> SEL_VIEW_BITS);
        const double* g = geo + 12 * (size_t)i;
        r.a0 = X[0] - g[9]; r.a1 = X[1] - g[10]; r.a2 = X[2] - g[11];
        r.z = (r.a0 * g[2] + r.a1 * g[5]) + r.a2 * g[8];
        if (r.z > 0) { zk = (vu64)__double_as_longlong(r.z); zv = (vu32)i; }
    }
    ray[e] = r; zkey[e] = zk; zview[e] = zv;
}

// The wave's visits of this trip: a lane with `on` adds one to shared[idx] and, with `scored`, one to score[idx].  Up to
// SEL_SETTLE_ROUNDS distinct counters are settled by ballot, one add each; lanes still open after that add for themselves.
__device__ __forceinline__ void sel_settle(vu32 idx, bool on, bool scored, int lane, int32_t* __restrict__ shared, int32_t* __restrict__ score)
{
    bool open = on;
    for (int round = 0; round < SEL_SETTLE_ROUNDS; ++round) {
        const vu64 m = __ballot(open);
        if (!m) return;                                                    // uniform over the wave
        const int leader = __ffsll((long long)m) - 1;
        const vu32 idx0 = (vu32)__shfl((int)idx, leader);
        const bool same = open && idx == idx0;
        const vu64 ms = __ballot(same), mc = __ballot(same && scored);
        if (lane == leader) {
            atomicAdd(shared + idx0, (int32_t)__popcll(ms));
            if (mc) atomicAdd(score + idx0, (int32_t)__popcll(mc));
        }
        if (same) open = false;
    }
    if (open) {
        atomicAdd(shared + idx, 1);
        if (scored) atomicAdd(score + idx, 1);
    }
}

// One thread per sorted entry.  A distinct pair (point, view i) visits the later entries of its point, whatever their number: trip t looks
// at entry e + t, and the wave leaves the loop when none of its lanes has a later entry of its point left.  The views of a point ascend,
// so every visit is a pair i < j and lands in the upper triangles.
__global__ __launch_bounds__(256) void select_pair_kernel(const vu64* __restrict__ keys, const vu32* __restrict__ head, const SelRay* __restrict__ ray, size_t n,
                                                          int n_views, double cos2_min, int32_t* __restrict__ shared, int32_t* __restrict__ score)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool go = e < n && head[e] != 0;
    vu64 pt = 0; int i = 0; double na = 0.0;
    SelRay a = { 0.0, 0.0, 0.0, 0.0 };
    if (go) {
        const vu64 k = keys[e];
        pt = k >> SEL_VIEW_BITS; i = (int)(k & (SEL_VIEWS_MAX - 1));
        a = ray[e];
        na = (a.a0 * a.a0 + a.a1 * a.a1) + a.a2 * a.a2;
    }
    for (size_t t = 1;; ++t) {
        const size_t f = e + t;
        vu64 kf = 0;
        if (go) {
            go = f < n;
            if (go) { kf = keys[f]; go = (kf >> SEL_VIEW_BITS) == pt; }
        }
        if (!__ballot(go)) break;
        const bool on = go && head[f] != 0;
        bool scored = false; vu32 idx = 0;
        if (on) {
            const SelRay b = ray[f];
            const double d = (a.a0 * b.a0 + a.a1 * b.a1) + a.a2 * b.a2;
            const double nb = (b.a0 * b.a0 + b.a1 * b.a1) + b.a2 * b.a2;
            scored = a.z > 0 && b.z > 0 && (d <= 0 || d * d <= cos2_min * (na * nb));
            idx = (vu32)i * (vu32)n_views + (vu32)(kf & (SEL_VIEWS_MAX - 1));
        }
        sel_settle(idx, on, scored, lane, shared, score);
    }
}

__global__ __launch_bounds__(256) void select_mirror_kernel(int32_t* __restrict__ shared, int32_t* __restrict__ score, int n_views)
{
    const vu32 t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (vu32)n_views * (vu32)n_views) return;
    const vu32 i = t / (vu32)n_views, j = t % (vu32)n_views;
    if (i > j) { shared[t] = shared[j * (vu32)n_views + i]; score[t] = score[j * (vu32)n_views + i]; }
}

// One wave per view i.  A round takes the least (a, j) behind the last one taken, lexicographically; first with a = 2^32 - 1 - score over
// the views of positive score (score descending, index ascending), then, when those run out, with a = the bits of the squared centre
// distance over the views of score zero (a non-negative double orders like its bits).  A lane looks at the columns lane, lane + 64, ...
__global__ __launch_bounds__(256) void select_rank_kernel(const int32_t* __restrict__ score, const double* __restrict__ geo, int n_views, int n_src,
                                                          int32_t* __restrict__ sources, int32_t* __restrict__ n_scored)
{
    const int lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= n_views) return;                                              // uniform over the wave
    const int32_t* row = score + (size_t)i * n_views;
    const double cx = geo[12 * (size_t)i + 9], cy = geo[12 * (size_t)i + 10], cz = geo[12 * (size_t)i + 11];
    bool by_score = true, first = true;
    vu64 pa = 0; vu32 pj = 0;
    int taken = 0, scored = 0;
    while (taken < n_src) {
        vu64 ba = ~0ull; vu32 bj = ~0u;
        for (int j = lane; j < n_views; j += 64) {
            if (j == i) continue;
            const int32_t s = row[j];
            vu64 av;
            if (by_score) {
                if (s <= 0) continue;
                av = (vu64)(0xffffffffu - (vu32)s);
            } else {
                if (s > 0) continue;
                const double dx = geo[12 * (size_t)j + 9] - cx, dy = geo[12 * (size_t)j + 10] - cy, dz = geo[12 * (size_t)j + 11] - cz;
                av = (vu64)__double_as_longlong((dx * dx + dy * dy) + dz * dz);
            }
            if (!(first || av > pa || (av == pa && (vu32)j > pj))) continue;
            if (av < ba || (av == ba && (vu32)j < bj)) { ba = av; bj = (vu32)j; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const vu64 oa = (vu64)__shfl_xor((long long)ba, off);
            const vu32 oj = (vu32)__shfl_xor((int)bj, off);
            if (oa < ba || (oa == ba && oj < bj)) { ba = oa; bj = oj; }
        }
        if (bj == ~0u) {                                                   // uniform: every lane holds the wave's result
            if (!by_score) break;                                          // cannot happen: n_src <= n_views - 1
            by_score = false; first = true;
            continue;
        }
        if (lane == 0) sources[(size_t)i * n_src + taken] = (int32_t)bj;
        pa = ba; pj = bj; first = false;
        ++taken;
        if (by_score) ++scored;
    }
    if (lane == 0) n_scored[i] = scored;
}

__device__ __forceinline__ size_t sel_lower_bound(const vu64* __restrict__ k, size_t n, vu64 v)
{
    size_t lo = 0, hi = n;
    while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (k[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

// views: the view of every entry in front of its camera (n_views: none), ascending; perm: the entry's place in zsorted, the ascending
// bit patterns of the depths.  Within a view the places ascend, because the second sort is stable.
__global__ __launch_bounds__(256) void select_range_kernel(const vu64* __restrict__ views, const vu32* __restrict__ perm, const vu64* __restrict__ zsorted, size_t n,
                                                           int n_views, double* __restrict__ wrange, int32_t* __restrict__ n_depth)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n_views) return;
    const size_t lo = sel_lower_bound(views, n, (vu64)i), hi = sel_lower_bound(views, n, (vu64)i + 1);
    const size_t m = hi - lo;
    if (n_depth) n_depth[i] = (int32_t)m;
    if (!wrange) return;
    double w0 = 0.0, w1 = 0.0;
    if (m >= 2) {
        const double zlo = __longlong_as_double((long long)zsorted[perm[lo + (2 * (m - 1)) / 100]]);
        const double zhi = __longlong_as_double((long long)zsorted[perm[lo + (98 * (m - 1) + 99) / 100]]);
        const double wlo = 1.0 / zhi, whi = 1.0 / zlo;
        double span = whi - wlo;
        if (!(span > 0)) span = 0.5 * wlo;
        const double x = wlo - 0.25 * span, y = 0.5 * wlo;
        w0 = y > x ? y : x;
        w1 = whi + 0.25 * span;
    }
    wrange[2 * (size_t)i] = w0; wrange[2 * (size_t)i + 1] = w1;
}

__global__ __launch_bounds__(256) void select_widen_kernel(const vu32* __restrict__ in, size_t n, vu64* __restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] = in[e];
}

static inline int sel_bit_length(vu64 x) { int b = 0; while (x) { ++b; x >>= 1; } return b; }
static inline unsigned sel_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

static bool select_args_ok(const sfmhip_ctx* ctx, const double* ext6, int n_views, const double* pts, int n_pt, const int32_t* obs_cam, const int32_t* obs_pt, int n_obs,
                           double cos2_min, int n_src)
{
    return ctx && ext6 && n_views >= 2 && n_views <= SEL_VIEWS_MAX && n_src >= 1 && n_src <= std::min(SEL_SRC_MAX, n_views - 1) && std::isfinite(cos2_min) &&
           cos2_min >= 0.0 && cos2_min <= 1.0 && n_pt >= 0 && n_obs >= 0 && (n_pt == 0 || pts) && (n_obs == 0 || (obs_cam && obs_pt));
}

// Rinv and c of every view through the host body of sfmhip_sweep_geometry; false where a pose or a centre is not finite
static bool select_geometry(const double* ext6, int n_views, std::vector<double>& geo)
{
    static const double K1[4] = { 1.0, 1.0, 0.0, 0.0 };
    geo.resize(12 * (size_t)n_views);
    for (int i = 0; i < n_views; ++i) {
        const double* e = ext6 + 6 * (size_t)i;
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(e[k])) return false;
        double* g = &geo[12 * (size_t)i];
        if (sfmhip_sweep_geometry(K1, e, nullptr, 0, nullptr, nullptr, nullptr, nullptr, g, g + 9) != SFMHIP_OK) return false;
        if (!(std::isfinite(g[9]) && std::isfinite(g[10]) && std::isfinite(g[11]))) return false;
    }
    return true;
}

// everything on device arrays but geo (host, 12 doubles per view); any output may be null.  The temporaries are taken before anything is
// enqueued: a failed allocation leaves the outputs alone.
static int select_enqueue(sfmhip_ctx* ctx, const std::vector<double>& geo, int n_views, const double* d_pts, int n_pt, const int32_t* d_obs_cam, const int32_t* d_obs_pt,
                          int n_obs, double cos2_min, int n_src, int32_t* d_shared, int32_t* d_score, int32_t* d_sources, int32_t* d_n_scored, double* d_wrange,
                          int32_t* d_n_depth)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)n_obs, V = (size_t)n_views, VV = V * V;
    SfmCarve carve;
    const size_t o_geo = carve(V * 12 * sizeof(double)), o_shared = carve(d_shared ? 0 : VV * 4), o_score = carve(d_score ? 0 : VV * 4);
    const size_t o_sources = carve(d_sources ? 0 : V * SEL_SRC_MAX * 4), o_nscored = carve(d_n_scored ? 0 : V * 4);
    const size_t o_head = carve((n + 1) * 4), o_ray = carve(n * sizeof(SelRay));
    SfmSort S(carve, n), T(carve, n);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    S.bind(w); T.bind(w);
    double* d_geo = (double*)(w + o_geo);
    int32_t* shared = d_shared ? d_shared : (int32_t*)(w + o_shared);
    int32_t* score = d_score ? d_score : (int32_t*)(w + o_score);
    int32_t* sources = d_sources ? d_sources : (int32_t*)(w + o_sources);
    int32_t* n_scored = d_n_scored ? d_n_scored : (int32_t*)(w + o_nscored);
    vu32* head = (vu32*)(w + o_head);
    SelRay* ray = (SelRay*)(w + o_ray);

    for (int v0 = 0; v0 < n_views; v0 += SEL_GEO_VIEWS) {
        const int count = 12 * std::min(SEL_GEO_VIEWS, n_views - v0);
        SelGeoChunk chunk;
        std::memcpy(chunk.g, &geo[12 * (size_t)v0], (size_t)count * sizeof(double));
        hipLaunchKernelGGL(select_geo_kernel, dim3((unsigned)((count + 127) / 128)), dim3(128), 0, st, chunk, count, d_geo + 12 * (size_t)v0);
    }
    SFM_HIP_TRY(ctx, hipMemsetAsync(shared, 0, VV * 4, st));
    SFM_HIP_TRY(ctx, hipMemsetAsync(score, 0, VV * 4, st));
    int side = 0;
    if (n > 0) {
        hipLaunchKernelGGL(select_key_kernel, dim3(sel_blocks(n)), dim3(256), 0, st, d_obs_cam, d_obs_pt, d_pts, n, n_views, n_pt, S.k[0]);
        // every key lies below 2^bits and the bits above are zero, so the passes the sort rounds up to see nothing else
        const vu64 none = (vu64)n_pt << SEL_VIEW_BITS;
        side = S.sort(st, n, 0, sel_bit_length(none), true);
        sfm_enqueue_run_heads(st, S.k[side], n, none, head);
        hipLaunchKernelGGL(select_ray_kernel, dim3(sel_blocks(n)), dim3(256), 0, st, (const vu64*)S.k[side], (const vu32*)head, d_pts, (const double*)d_geo, n, n_views, ray,
                           S.k[side ^ 1], S.v[side ^ 1]);
        hipLaunchKernelGGL(select_pair_kernel, dim3(sel_blocks(n)), dim3(256), 0, st, (const vu64*)S.k[side], (const vu32*)head, (const SelRay*)ray, n, n_views, cos2_min,
                           shared, score);
    }
    hipLaunchKernelGGL(select_mirror_kernel, dim3(sel_blocks(VV)), dim3(256), 0, st, shared, score, n_views);
    hipLaunchKernelGGL(select_rank_kernel, dim3((unsigned)((n_views + 3) / 4)), dim3(256), 0, st, (const int32_t*)score, (const double*)d_geo, n_views, n_src, sources,
                       n_scored);
    if (d_wrange || d_n_depth) {
        int side_z = 0, side_v = 0;
        if (n > 0) {
            // the pair kernel is done with the point keys: their side is the sort's other side from here on
            side_z = S.sort(st, n, side ^ 1, 64, false);
            hipLaunchKernelGGL(select_widen_kernel, dim3(sel_blocks(n)), dim3(256), 0, st, (const vu32*)S.v[side_z], n, T.k[0]);
            side_v = T.sort(st, n, 0, sel_bit_length((vu64)n_views), true);
        }
        hipLaunchKernelGGL(select_range_kernel, dim3(sel_blocks(V)), dim3(256), 0, st, (const vu64*)T.k[side_v], (const vu32*)T.v[side_v], (const vu64*)S.k[side_z], n, n_views,
                           d_wrange, d_n_depth);
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

extern "C" {

int sfmhip_select_views_dev(sfmhip_ctx* ctx, const double* ext6, int n_views, const double* d_pts, int n_pt, const int32_t* d_obs_cam, const int32_t* d_obs_pt, int n_obs,
                            double cos2_min, int n_src, int32_t* d_shared, int32_t* d_score, int32_t* d_sources, int32_t* d_n_scored, double* d_wrange, int32_t* d_n_depth)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_select_views_dev");
    SFM_ARG_CHECK(ctx, select_args_ok(ctx, ext6, n_views, d_pts, n_pt, d_obs_cam, d_obs_pt, n_obs, cos2_min, n_src));
    std::vector<double> geo;
    SFM_ARG_CHECK(ctx, select_geometry(ext6, n_views, geo));
    return select_enqueue(ctx, geo, n_views, d_pts, n_pt, d_obs_cam, d_obs_pt, n_obs, cos2_min, n_src, d_shared, d_score, d_sources, d_n_scored, d_wrange, d_n_depth);
}

int sfmhip_select_views(sfmhip_ctx* ctx, const double* ext6, int n_views, const double* pts, int n_pt, const int32_t* obs_cam, const int32_t* obs_pt, int n_obs,
                        double cos2_min, int n_src, int32_t* shared, int32_t* score, int32_t* sources, int32_t* n_scored, double* wrange, int32_t* n_depth)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_select_views");
    SFM_ARG_CHECK(ctx, select_args_ok(ctx, ext6, n_views, pts, n_pt, obs_cam, obs_pt, n_obs, cos2_min, n_src));
    for (int o = 0; o < n_obs; ++o) SFM_ARG_CHECK(ctx, obs_cam[o] >= 0 && obs_cam[o] < n_views && obs_pt[o] >= 0 && obs_pt[o] < n_pt);
    std::vector<double> geo;
    SFM_ARG_CHECK(ctx, select_geometry(ext6, n_views, geo));
    const size_t n = (size_t)n_obs, V = (size_t)n_views, VV = V * V, P = (size_t)n_pt;
    SfmCarve carve;
    const size_t o_pts = carve(P * 24), o_cam = carve(n * 4), o_pt = carve(n * 4), o_shared = carve(shared ? VV * 4 : 0), o_score = carve(score ? VV * 4 : 0),
                 o_sources = carve(sources ? V * (size_t)n_src * 4 : 0), o_nscored = carve(n_scored ? V * 4 : 0), o_wrange = carve(wrange ? V * 16 : 0),
                 o_ndepth = carve(n_depth ? V * 4 : 0);
    SfmPoolHold hold(ctx);
    char* d = nullptr;
    int rc = hold.get(carve.bytes ? carve.bytes : 256, (void**)&d);
    if (rc != SFMHIP_OK) return rc;
    if (P) rc = sfm_upload(ctx, d + o_pts, pts, P * 24);
    if (rc == SFMHIP_OK && n) rc = sfm_upload(ctx, d + o_cam, obs_cam, n * 4);
    if (rc == SFMHIP_OK && n) rc = sfm_upload(ctx, d + o_pt, obs_pt, n * 4);
    if (rc == SFMHIP_OK)
        rc = select_enqueue(ctx, geo, n_views, (const double*)(d + o_pts), n_pt, (const int32_t*)(d + o_cam), (const int32_t*)(d + o_pt), n_obs, cos2_min, n_src,
                            shared ? (int32_t*)(d + o_shared) : nullptr, score ? (int32_t*)(d + o_score) : nullptr, sources ? (int32_t*)(d + o_sources) : nullptr,
                            n_scored ? (int32_t*)(d + o_nscored) : nullptr, wrange ? (double*)(d + o_wrange) : nullptr, n_depth ? (int32_t*)(d + o_ndepth) : nullptr);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipError_t e = hipSuccess;
    if (shared) e = hipMemcpyAsync(shared, d + o_shared, VV * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && score) e = hipMemcpyAsync(score, d + o_score, VV * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && sources) e = hipMemcpyAsync(sources, d + o_sources, V * (size_t)n_src * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && n_scored) e = hipMemcpyAsync(n_scored, d + o_nscored, V * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && wrange) e = hipMemcpyAsync(wrange, d + o_wrange, V * 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && n_depth) e = hipMemcpyAsync(n_depth, d + o_ndepth, V * 4, hipMemcpyDeviceToHost, ctx->stream);
    return sfm_finish(ctx, e);
}

}  // extern "C"
