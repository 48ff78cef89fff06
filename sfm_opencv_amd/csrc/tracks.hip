// tracks.hip -- feature tracks from pairwise match lists (sfmhip_build_tracks): the connected components of the match graph over any pair
// list, OpenMVG's conflict rule (or its repair), a length filter, and the observation lists that triangulation and bundle adjustment take.
// The definition is in include/sfmhip.h and restated in tests/tracks_ref.py.  Integer work only; every output is a function of the set of
// valid edges, so the same bytes come out for any order of the pairs or elements, any duplication, every run and every launch geometry.
//
// How it runs, all on the context's stream, nothing synchronises; n = n_feat:
//   1. tracks_init_kernel      parent[g] = g; img_of[g] by bisection in off[]
//   2. tracks_link_kernel      a thread per (pair, slot): validation against the pair table, cluster_unite (unionfind.hpp).  The ignored
//                              elements of a wave leave as one add, settled by ballot
//   3. tracks_flatten_kernel   root[g] = cluster_find, as the key of
//   4. SfmSort                 one stable sort by root with identity values: a component is a run, its features ascending
//   5. sfm_enqueue_run_heads, tracks_first_kernel      per record: head of its component; first of its image
//   6. SfmScan twice           H numbers the components, F counts the first-of-image records: a component's length is F[end] - F[start],
//                              its conflicts are the rest of the run -- nobody walks a component
//   7. tracks_cstart_kernel    the start of every run, the end of the last
//      tracks_comp_kernel      a thread per component: conflicting, short, track; a wave's three counts leave by ballot into its own slot
//   8. SfmScan                 T numbers the tracks by ascending root
//      tracks_keep_kernel, SfmScan      O numbers the kept records: the observations in (track, g) order
//   9. tracks_scatter_kernel   track_of, obs_*, obs_uv, track_len; the longest track by at most one atomicMax a wave
//      tracks_stats_kernel     one wave adds the waves' counts in a fixed order
//  10. tracks_filter_kernel    a workgroup per pair: the elements between two kept observations, compacted in order
// The only atomics besides those of unionfind.hpp: the add of the ignored elements and the max of the lengths, both on integers.
#include "sortscan.hpp"
#include "unionfind.hpp"

typedef unsigned long long tu64;
typedef unsigned int tu32;

#define TRK_IMG_MAX 65536

struct __attribute__((aligned(16))) TrkPair { int32_t off_a, off_b, n_a, n_b; };      // all zero: no element of the pair is valid

__device__ __forceinline__ int trk_clamp_count(int c, int stride) { return c < 0 ? 0 : (c > stride ? stride : c); }

__global__ __launch_bounds__(256) void tracks_init_kernel(const tu32* __restrict__ off, int n_img, size_t n, tu32* __restrict__ parent, int32_t* __restrict__ img_of)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    parent[g] = (tu32)g;
    int lo = 0, hi = n_img;                                                // off[lo] <= g < off[hi]: the image is never an empty one
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= (tu32)g) lo = mid; else hi = mid; }
    img_of[g] = lo;
}

// ctl[0]: ignored elements, ctl[1]: a union hit CLUSTER_RETRY_CAP
__global__ __launch_bounds__(256) void tracks_link_kernel(const TrkPair* __restrict__ tbl, const sfm_dmatch* __restrict__ matches, int max_per_pair,
                                                          const int32_t* __restrict__ counts, size_t total, tu32* __restrict__ parent, tu32* __restrict__ ctl)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool valid = false, ignored = false;
    tu32 ga = 0, gb = 0;
    if (t < total) {
        const size_t q = t / (size_t)max_per_pair;
        const int i = (int)(t - q * (size_t)max_per_pair);
        if (i < trk_clamp_count(counts[q], max_per_pair)) {
            const TrkPair p = tbl[q];
            const sfm_dmatch mm = matches[t];
            valid = (tu32)mm.queryIdx < (tu32)p.n_a && (tu32)mm.trainIdx < (tu32)p.n_b;
            ignored = !valid;
            ga = (tu32)p.off_a + (tu32)mm.queryIdx; gb = (tu32)p.off_b + (tu32)mm.trainIdx;
        }
    }
    const tu64 mi = __ballot(ignored);
    if (mi && lane == __ffsll((long long)mi) - 1) atomicAdd(ctl, (tu32)__popcll(mi));
    if (valid) (void)cluster_unite(parent, ga, gb, ctl + 1);
}

__global__ __launch_bounds__(256) void tracks_flatten_kernel(tu32* __restrict__ parent, size_t n, tu64* __restrict__ keys)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g < n) keys[g] = (tu64)cluster_find(parent, (tu32)g);
}

// n + 1 flags: record r is the first of its image in its component (head: the run heads, not yet scanned)
__global__ __launch_bounds__(256) void tracks_first_kernel(const tu32* __restrict__ val, const int32_t* __restrict__ img_of, const tu32* __restrict__ head, size_t n,
                                                           tu32* __restrict__ first)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    first[r] = (r < n && (head[r] || img_of[val[r]] != img_of[val[r - 1]])) ? 1u : 0u;
}

// H: the scanned run heads.  cstart[c] = first record of component c, cstart[n_comp] = n
__global__ __launch_bounds__(256) void tracks_cstart_kernel(const tu32* __restrict__ H, size_t n, tu32* __restrict__ cstart)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    if (r == n) cstart[H[n]] = (tu32)n;
    else if (H[r + 1] != H[r]) cstart[H[r]] = (tu32)r;
}

// a thread per component (n + 1 threads: the flags behind the last component are zero).  wsum: three counts per wave of the launch --
// components of two features or more, conflicting ones, short ones
__global__ __launch_bounds__(256) void tracks_comp_kernel(const tu32* __restrict__ H, const tu32* __restrict__ F, const tu32* __restrict__ cstart, size_t n, int min_len,
                                                          int keep_first, tu32* __restrict__ keepc, tu32* __restrict__ wsum)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool multi = false, conflict = false, shrt = false, track = false;
    if (c < (size_t)H[n]) {
        const tu32 s = cstart[c], e = cstart[c + 1];
        const tu32 size = e - s, len = F[e] - F[s];
        multi = size >= 2u;
        conflict = len < size;
        const bool survives = multi && (keep_first || !conflict);
        track = survives && len >= (tu32)min_len;
        shrt = survives && !track;
    }
    if (c <= n) keepc[c] = track ? 1u : 0u;
    const tu64 bm = __ballot(multi), bc = __ballot(conflict), bs = __ballot(shrt);
    if ((threadIdx.x & 63) == 0) {
        tu32* w = wsum + 3 * ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6));
        w[0] = (tu32)__popcll(bm); w[1] = (tu32)__popcll(bc); w[2] = (tu32)__popcll(bs);
    }
}

// n + 1 flags: record r is an observation (H, F, T scanned)
__global__ __launch_bounds__(256) void tracks_keep_kernel(const tu32* __restrict__ H, const tu32* __restrict__ F, const tu32* __restrict__ T, size_t n,
                                                          tu32* __restrict__ keepr)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    bool keep = false;
    if (r < n) {
        const tu32 c = H[r + 1] - 1u;
        keep = F[r + 1] != F[r] && T[c + 1] != T[c];
    }
    keepr[r] = keep ? 1u : 0u;
}

struct TrkOut { int32_t *track_of, *obs_cam, *obs_pt, *obs_kp, *track_len; double* obs_uv; };

__global__ __launch_bounds__(256) void tracks_scatter_kernel(const tu32* __restrict__ val, const int32_t* __restrict__ img_of, const tu32* __restrict__ off,
                                                             const tu32* __restrict__ H, const tu32* __restrict__ F, const tu32* __restrict__ T,
                                                             const tu32* __restrict__ O, const tu32* __restrict__ cstart,
                                                             const sfm_keypoint* const* __restrict__ kp, size_t n, TrkOut out, int32_t* __restrict__ longest)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    int len = 0;
    if (r < n) {
        const tu32 g = val[r], c = H[r + 1] - 1u;
        const tu32 tid = T[c];
        const bool track = T[c + 1] != tid, kept = track && F[r + 1] != F[r];
        if (out.track_of) out.track_of[g] = kept ? (int32_t)tid : -1;
        if (kept) {
            const tu32 o = O[r];
            const int img = img_of[g];
            const tu32 k = g - off[img];
            if (out.obs_cam) out.obs_cam[o] = img;
            if (out.obs_pt) out.obs_pt[o] = (int32_t)tid;
            if (out.obs_kp) out.obs_kp[o] = (int32_t)k;
            if (out.obs_uv) {
                const sfm_keypoint* p = kp[img] + k;
                out.obs_uv[2 * (size_t)o] = (double)p->x; out.obs_uv[2 * (size_t)o + 1] = (double)p->y;
            }
        }
        if (track && H[r + 1] != H[r]) {                                   // the component's head: its length
            len = (int)(F[cstart[c + 1]] - F[r]);
            if (out.track_len) out.track_len[tid] = len;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(len, o); len = t > len ? t : len; }
    // the maximum only grows: a wave that reads a value no smaller than its own has nothing to add (at 250 K tracks of length <= 6 all
    // but a handful of the 15 K waves leave it at the load)
    if ((threadIdx.x & 63) == 0 && len > __hip_atomic_load(longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(longest, len);
}

// one wave.  stats[6] is the scatter kernel's; a union that gave up: n_tracks = -1
__global__ __launch_bounds__(64) void tracks_stats_kernel(const tu32* __restrict__ wsum, size_t n_waves, const tu32* __restrict__ n_tracks, const tu32* __restrict__ n_obs,
                                                          const tu32* __restrict__ ctl, int32_t* __restrict__ stats)
{
    tu32 a = 0, b = 0, c = 0;
    for (size_t w = threadIdx.x; w < n_waves; w += 64) { a += wsum[3 * w]; b += wsum[3 * w + 1]; c += wsum[3 * w + 2]; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { a += (tu32)__shfl_xor((int)a, o); b += (tu32)__shfl_xor((int)b, o); c += (tu32)__shfl_xor((int)c, o); }
    if (threadIdx.x == 0) {
        const tu32 err = ctl[1];
        stats[0] = err ? -1 : (int32_t)*n_tracks; stats[1] = (int32_t)*n_obs;
        stats[2] = (int32_t)a; stats[3] = (int32_t)b; stats[4] = (int32_t)c;
        stats[5] = (int32_t)ctl[0]; stats[7] = err ? 1 : 0;
    }
}

// ordered compaction inside a workgroup of 256 threads, as twoview.hip's block_rank: the flagged threads below this one, and their number
__device__ __forceinline__ int trk_block_rank(bool f, int* sw, int& total)
{
    const tu64 b = __ballot(f);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                                     // the previous call's readers are done with sw
    if (lane == 0) sw[wave] = __popcll(b);
    __syncthreads();
    int below = __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) below += sw[w];
    total = (sw[0] + sw[1]) + (sw[2] + sw[3]);
    return below;
}

// one workgroup per pair: the valid elements whose two features are kept observations (an edge joins them: of one track), in their order
__global__ __launch_bounds__(256) void tracks_filter_kernel(const TrkPair* __restrict__ tbl, const sfm_dmatch* __restrict__ matches, int max_per_pair,
                                                            const int32_t* __restrict__ counts, const int32_t* __restrict__ track_of,
                                                            sfm_dmatch* __restrict__ out, int32_t* __restrict__ counts_out)
{
    __shared__ int sw[4];
    const size_t q = blockIdx.x;
    const int cnt = trk_clamp_count(counts[q], max_per_pair);
    const TrkPair p = tbl[q];
    int m = 0;
    for (int base = 0; base < cnt; base += 256) {
        const int i = base + (int)threadIdx.x;
        sfm_dmatch mm = { 0, 0, 0, 0.f };
        bool f = false;
        if (i < cnt) {
            mm = matches[q * max_per_pair + i];
            f = (tu32)mm.queryIdx < (tu32)p.n_a && (tu32)mm.trainIdx < (tu32)p.n_b;
            if (f) f = track_of[(tu32)p.off_a + (tu32)mm.queryIdx] >= 0 && track_of[(tu32)p.off_b + (tu32)mm.trainIdx] >= 0;
        }
        int total;
        const int r = trk_block_rank(f, sw, total);
        if (f && out) out[q * max_per_pair + m + r] = mm;
        m += total;
    }
    if (threadIdx.x == 0 && counts_out) counts_out[q] = m;
}

static inline int trk_bit_length(tu64 x) { int b = 0; while (x) { ++b; x >>= 1; } return b; }
static inline unsigned trk_blocks(size_t n) { return (unsigned)((n + 255) / 256); }
static inline bool trk_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    return a && b && na && nb && (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}

struct TrkArgs {
    int n_img; const int32_t* n_kp; const int32_t* pairs; int n_pairs; const sfm_dmatch* matches; int max_per_pair; const int32_t* counts;
    const sfm_keypoint* const* kp; int min_len; int flags;
    int32_t *track_of, *obs_cam, *obs_pt, *obs_kp; double* obs_uv; int32_t* track_len; sfm_dmatch* matches_out; int32_t *counts_out, *stats;
};

// the argument rules of both forms; off: the exclusive prefix sums of n_kp, n_img + 1 entries
static bool tracks_args_ok(const sfmhip_ctx* ctx, const TrkArgs& a, std::vector<tu32>& off)
{
    if (!ctx || !a.n_kp || a.n_img < 1 || a.n_img > TRK_IMG_MAX || a.n_pairs < 0 || a.max_per_pair < 0 || a.min_len < 2) return false;
    if (a.flags & ~SFMHIP_TRACKS_KEEP_FIRST) return false;
    if (a.n_pairs > 0 && (!a.pairs || ((!a.matches || !a.counts) && a.max_per_pair > 0))) return false;
    if (a.obs_uv && !a.kp) return false;
    off.resize((size_t)a.n_img + 1);
    tu64 sum = 0;
    for (int i = 0; i < a.n_img; ++i) {
        if (a.n_kp[i] < 0) return false;
        if (a.obs_uv && a.n_kp[i] > 0 && !a.kp[i]) return false;
        off[(size_t)i] = (tu32)sum;
        sum += (tu64)a.n_kp[i];
        if (sum >= 0x80000000ull) return false;
    }
    off[(size_t)a.n_img] = (tu32)sum;
    const size_t n = (size_t)sum, PS = (size_t)a.n_pairs * (size_t)a.max_per_pair, P = (size_t)a.n_pairs;
    const void* o[9] = { a.track_of, a.obs_cam, a.obs_pt, a.obs_kp, a.obs_uv, a.track_len, a.matches_out, a.counts_out, a.stats };
    const size_t b[9] = { n * 4, n * 4, n * 4, n * 4, n * 16, (n / 2) * 4, PS * sizeof(sfm_dmatch), P * 4, 8 * 4 };
    for (int i = 0; i < 9; ++i) {
        for (int j = i + 1; j < 9; ++j)
            if (trk_overlap(o[i], b[i], o[j], b[j])) return false;
        if (trk_overlap(o[i], b[i], a.matches, PS * sizeof(sfm_dmatch)) || trk_overlap(o[i], b[i], a.counts, P * 4)) return false;
    }
    return true;
}

// Everything on device arrays but n_kp, pairs and the pointer table kp (host; consumed before this returns).  Every block is taken before a
// kernel or a write to an output is enqueued: a failed allocation leaves the outputs alone.
static int tracks_enqueue(sfmhip_ctx* ctx, const TrkArgs& a, const std::vector<tu32>& off)
{
    hipStream_t st = ctx->stream;
    const int n_img = a.n_img;
    const size_t n = (size_t)off[(size_t)n_img], P = (size_t)a.n_pairs, S = (size_t)a.max_per_pair;
    if (n == 0 || P == 0) {                                                // no edge: no track, and the statistics are zero
        if (a.track_of && n) SFM_HIP_TRY(ctx, hipMemsetAsync(a.track_of, 0xff, n * 4, st));
        if (a.counts_out && P) SFM_HIP_TRY(ctx, hipMemsetAsync(a.counts_out, 0, P * 4, st));
        if (a.stats) SFM_HIP_TRY(ctx, hipMemsetAsync(a.stats, 0, 8 * 4, st));
        return SFMHIP_OK;
    }
    std::vector<TrkPair> tbl(P);
    for (size_t q = 0; q < P; ++q) {
        const int ia = a.pairs[2 * q], ib = a.pairs[2 * q + 1];
        TrkPair p = { 0, 0, 0, 0 };
        if (ia >= 0 && ia < n_img && ib >= 0 && ib < n_img && ia != ib) p = { (int32_t)off[(size_t)ia], (int32_t)off[(size_t)ib], a.n_kp[ia], a.n_kp[ib] };
        tbl[q] = p;
    }
    const size_t n_waves = (size_t)trk_blocks(n + 1) * 4;
    SfmCarve carve;
    const size_t o_parent = carve(n * 4), o_img = carve(n * 4), o_cstart = carve((n + 1) * 4), o_wsum = carve(n_waves * 12), o_ctl = carve(16), o_stats = carve(a.stats ? 0 : 32),
                 o_trackof = carve(a.track_of ? 0 : n * 4);
    SfmSort R(carve, n);
    SfmScan H(carve, n + 1), F(carve, n + 1), T(carve, n + 1), O(carve, n + 1);
    SfmPoolHold hold(ctx);
    TrkPair* d_tbl = nullptr; tu32* d_off = nullptr; const sfm_keypoint** d_kp = nullptr; char* w = nullptr;
    int rc = sfm_upload_async(ctx, hold, tbl.data(), P, d_tbl);            // pageable sources: consumed when the calls return
    if (rc == SFMHIP_OK) rc = sfm_upload_async(ctx, hold, off.data(), off.size(), d_off);
    if (rc == SFMHIP_OK && a.obs_uv) rc = sfm_upload_async(ctx, hold, a.kp, (size_t)n_img, d_kp);
    if (rc == SFMHIP_OK) rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    R.bind(w); H.bind(w); F.bind(w); T.bind(w); O.bind(w);
    tu32 *parent = (tu32*)(w + o_parent), *cstart = (tu32*)(w + o_cstart), *wsum = (tu32*)(w + o_wsum), *ctl = (tu32*)(w + o_ctl);
    int32_t* img_of = (int32_t*)(w + o_img);
    int32_t* stats = a.stats ? a.stats : (int32_t*)(w + o_stats);
    int32_t* track_of = a.track_of ? a.track_of : (int32_t*)(w + o_trackof);
    const bool filter = a.matches_out || a.counts_out;

    SFM_HIP_TRY(ctx, hipMemsetAsync(ctl, 0, 16, st));
    SFM_HIP_TRY(ctx, hipMemsetAsync(stats, 0, 32, st));
    hipLaunchKernelGGL(tracks_init_kernel, dim3(trk_blocks(n)), dim3(256), 0, st, (const tu32*)d_off, n_img, n, parent, img_of);
    if (S > 0)
        hipLaunchKernelGGL(tracks_link_kernel, dim3(trk_blocks(P * S)), dim3(256), 0, st, (const TrkPair*)d_tbl, a.matches, a.max_per_pair, a.counts, P * S, parent, ctl);
    hipLaunchKernelGGL(tracks_flatten_kernel, dim3(trk_blocks(n)), dim3(256), 0, st, parent, n, R.k[0]);
    // every key lies below n and the bits above are zero, so the passes the sort rounds up to see nothing else
    const int side = R.sort(st, n, 0, trk_bit_length((tu64)n), true);
    const tu32* val = R.v[side];
    sfm_enqueue_run_heads(st, R.k[side], n, ~0ull, H.data);
    hipLaunchKernelGGL(tracks_first_kernel, dim3(trk_blocks(n + 1)), dim3(256), 0, st, val, (const int32_t*)img_of, (const tu32*)H.data, n, F.data);
    H.scan(st, n + 1);
    F.scan(st, n + 1);
    hipLaunchKernelGGL(tracks_cstart_kernel, dim3(trk_blocks(n + 1)), dim3(256), 0, st, (const tu32*)H.data, n, cstart);
    hipLaunchKernelGGL(tracks_comp_kernel, dim3(trk_blocks(n + 1)), dim3(256), 0, st, (const tu32*)H.data, (const tu32*)F.data, (const tu32*)cstart, n, a.min_len,
                       (a.flags & SFMHIP_TRACKS_KEEP_FIRST) ? 1 : 0, T.data, wsum);
    T.scan(st, n + 1);
    hipLaunchKernelGGL(tracks_keep_kernel, dim3(trk_blocks(n + 1)), dim3(256), 0, st, (const tu32*)H.data, (const tu32*)F.data, (const tu32*)T.data, n, O.data);
    O.scan(st, n + 1);
    const TrkOut out = { (a.track_of || filter) ? track_of : nullptr, a.obs_cam, a.obs_pt, a.obs_kp, a.track_len, a.obs_uv };
    hipLaunchKernelGGL(tracks_scatter_kernel, dim3(trk_blocks(n)), dim3(256), 0, st, val, (const int32_t*)img_of, (const tu32*)d_off, (const tu32*)H.data,
                       (const tu32*)F.data, (const tu32*)T.data, (const tu32*)O.data, (const tu32*)cstart, (const sfm_keypoint* const*)d_kp, n, out, stats + 6);
    hipLaunchKernelGGL(tracks_stats_kernel, dim3(1), dim3(64), 0, st, (const tu32*)wsum, n_waves, (const tu32*)T.data + n, (const tu32*)O.data + n, (const tu32*)ctl,
                       stats);
    if (filter) {
        if (S > 0)
            hipLaunchKernelGGL(tracks_filter_kernel, dim3((unsigned)P), dim3(256), 0, st, (const TrkPair*)d_tbl, a.matches, a.max_per_pair, a.counts,
                               (const int32_t*)track_of, a.matches_out, a.counts_out);
        else if (a.counts_out) SFM_HIP_TRY(ctx, hipMemsetAsync(a.counts_out, 0, P * 4, st));
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

extern "C" {

int sfmhip_build_tracks_dev(sfmhip_ctx* ctx, int n_img, const int32_t* n_kp, const int32_t* pairs, int n_pairs, const sfm_dmatch* d_matches, int max_per_pair,
                            const int32_t* d_counts, const sfm_keypoint* const* d_kp, int min_len, int flags, int32_t* d_track_of, int32_t* d_obs_cam,
                            int32_t* d_obs_pt, int32_t* d_obs_kp, double* d_obs_uv, int32_t* d_track_len, sfm_dmatch* d_matches_out, int32_t* d_counts_out,
                            int32_t* d_stats)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_build_tracks_dev");
    const TrkArgs a = { n_img, n_kp, pairs, n_pairs, d_matches, max_per_pair, d_counts, d_kp, min_len, flags, d_track_of, d_obs_cam, d_obs_pt, d_obs_kp,
                        d_obs_uv, d_track_len, d_matches_out, d_counts_out, d_stats };
    std::vector<tu32> off;
    SFM_ARG_CHECK(ctx, tracks_args_ok(ctx, a, off));
    return tracks_enqueue(ctx, a, off);
}

int sfmhip_build_tracks(sfmhip_ctx* ctx, int n_img, const int32_t* n_kp, const int32_t* pairs, int n_pairs, const sfm_dmatch* matches, int max_per_pair,
                        const int32_t* counts, const sfm_keypoint* const* kp, int min_len, int flags, int32_t* track_of, int32_t* obs_cam, int32_t* obs_pt,
                        int32_t* obs_kp, double* obs_uv, int32_t* track_len, sfm_dmatch* matches_out, int32_t* counts_out, int32_t* stats)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_build_tracks");
    const TrkArgs h = { n_img, n_kp, pairs, n_pairs, matches, max_per_pair, counts, kp, min_len, flags, track_of, obs_cam, obs_pt, obs_kp, obs_uv, track_len,
                        matches_out, counts_out, stats };
    std::vector<tu32> off;
    SFM_ARG_CHECK(ctx, tracks_args_ok(ctx, h, off));
    const size_t n = (size_t)off[(size_t)n_img], P = (size_t)n_pairs, PS = P * (size_t)max_per_pair;
    const bool want_filter = matches_out || counts_out;      // a pair's count is needed for its prefix, asked for or not
    SfmCarve carve;
    const size_t o_m = carve(PS * sizeof(sfm_dmatch)), o_c = carve(P * 4), o_kp = carve(obs_uv ? n * sizeof(sfm_keypoint) : 0), o_trackof = carve(track_of ? n * 4 : 0),
                 o_cam = carve(obs_cam ? n * 4 : 0), o_pt = carve(obs_pt ? n * 4 : 0), o_okp = carve(obs_kp ? n * 4 : 0), o_uv = carve(obs_uv ? n * 16 : 0),
                 o_len = carve(track_len ? (n / 2) * 4 : 0), o_mo = carve(matches_out ? PS * sizeof(sfm_dmatch) : 0), o_co = carve(want_filter ? P * 4 : 0), o_stats = carve(32);
    SfmPoolHold hold(ctx);
    char* d = nullptr;
    int rc = hold.get(carve.bytes, (void**)&d);
    if (rc != SFMHIP_OK) return rc;
    if (PS) rc = sfm_upload(ctx, d + o_m, matches, PS * sizeof(sfm_dmatch));
    if (rc == SFMHIP_OK && P && max_per_pair > 0) rc = sfm_upload(ctx, d + o_c, counts, P * 4);
    std::vector<const sfm_keypoint*> kp_tbl;
    if (obs_uv) {
        kp_tbl.resize((size_t)n_img);
        for (int i = 0; i < n_img && rc == SFMHIP_OK; ++i) {
            kp_tbl[(size_t)i] = (const sfm_keypoint*)(d + o_kp) + off[(size_t)i];
            if (n_kp[i] > 0) rc = sfm_upload(ctx, (void*)kp_tbl[(size_t)i], kp[i], (size_t)n_kp[i] * sizeof(sfm_keypoint));
        }
    }
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    const TrkArgs a = { n_img, n_kp, pairs, n_pairs, (const sfm_dmatch*)(d + o_m), max_per_pair, (const int32_t*)(d + o_c), obs_uv ? kp_tbl.data() : nullptr, min_len,
                        flags, track_of ? (int32_t*)(d + o_trackof) : nullptr, obs_cam ? (int32_t*)(d + o_cam) : nullptr, obs_pt ? (int32_t*)(d + o_pt) : nullptr,
                        obs_kp ? (int32_t*)(d + o_okp) : nullptr, obs_uv ? (double*)(d + o_uv) : nullptr, track_len ? (int32_t*)(d + o_len) : nullptr,
                        matches_out ? (sfm_dmatch*)(d + o_mo) : nullptr, want_filter ? (int32_t*)(d + o_co) : nullptr, (int32_t*)(d + o_stats) };
    rc = tracks_enqueue(ctx, a, off);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    int32_t st8[8];
    std::vector<int32_t> co(want_filter ? P : 0);
    hipError_t e = hipMemcpyAsync(st8, d + o_stats, 32, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && want_filter && P) e = hipMemcpyAsync(co.data(), d + o_co, P * 4, hipMemcpyDeviceToHost, ctx->stream);
    rc = sfm_finish(ctx, e);
    if (rc != SFMHIP_OK) return rc;
    if (st8[7]) { ctx->last_error = "sfmhip_build_tracks: a union gave up after CLUSTER_RETRY_CAP trips"; return SFMHIP_E_NUMERIC; }
    // only the written prefixes come back
    const size_t n_tracks = (size_t)st8[0], n_obs = (size_t)st8[1];
    std::vector<sfm_dmatch> mo;
    if (track_of && n) e = hipMemcpyAsync(track_of, d + o_trackof, n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && obs_cam && n_obs) e = hipMemcpyAsync(obs_cam, d + o_cam, n_obs * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && obs_pt && n_obs) e = hipMemcpyAsync(obs_pt, d + o_pt, n_obs * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && obs_kp && n_obs) e = hipMemcpyAsync(obs_kp, d + o_okp, n_obs * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && obs_uv && n_obs) e = hipMemcpyAsync(obs_uv, d + o_uv, n_obs * 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && track_len && n_tracks) e = hipMemcpyAsync(track_len, d + o_len, n_tracks * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && matches_out && PS) {
        mo.resize(PS);
        e = hipMemcpyAsync(mo.data(), d + o_mo, PS * sizeof(sfm_dmatch), hipMemcpyDeviceToHost, ctx->stream);
    }
    rc = sfm_finish(ctx, e);
    if (rc != SFMHIP_OK) return rc;
    if (matches_out && PS) {
        for (size_t q = 0; q < P; ++q) {
            const size_t c = (size_t)co[q];
            if (c) std::memcpy(matches_out + q * (size_t)max_per_pair, mo.data() + q * (size_t)max_per_pair, c * sizeof(sfm_dmatch));
        }
    }
    if (counts_out && P) std::memcpy(counts_out, co.data(), P * 4);
    if (stats) std::memcpy(stats, st8, 32);
    return SFMHIP_OK;
}

}  // extern "C"
