// sortscan.hip -- the exclusive prefix sum and the stable radix sort that every list of the library goes through (bundle-adjustment
// set-up, the grids, voxels and clusters of points.hip, planes.hip, sift.hip, akaze.hip, dense.hip, tsdf.hip, mesh.hip), and the marker
// of run heads in sorted keys.  The contract is stated in sortscan.hpp.  Everything is HBM-bound integer work in plain coalesced passes;
// the only structured kernel is the radix scatter (per-wave match-any ranking, so that the sort is stable).
#include "sortscan.hpp"

typedef unsigned long long su64;
typedef unsigned int su32;

// ------------------------------------------------------------------------------------------------
// exclusive prefix sum of 32-bit counters, in place: tile scan -> scan of the tile totals -> add
// ------------------------------------------------------------------------------------------------
#define SCAN_ITEMS 16
#define SCAN_TILE (256 * SCAN_ITEMS)

__device__ __forceinline__ su32 sfm_wave_incl_scan(su32 v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const su32 t = __shfl_up(v, off); if (lane >= off) v += t; }
    return v;
}

// 256 threads: exclusive prefix of v over the workgroup, the workgroup's total in *total
__device__ __forceinline__ su32 sfm_block_excl_scan(su32 v, su32* total, su32* sm)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const su32 incl = sfm_wave_incl_scan(v, lane);
    if (lane == 63) sm[wave] = incl;
    __syncthreads();
    su32 wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const su32 s = sm[w]; if (w < wave) wbase += s; tot += s; }
    __syncthreads();
    *total = tot;
    return wbase + incl - v;
}

__global__ __launch_bounds__(256) void sfm_scan_tile_kernel(su32* __restrict__ data, size_t n, su32* __restrict__ bsum)
{
    __shared__ su32 sm[4];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    su32 x[SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) { x[j] = base + j < n ? data[base + j] : 0u; sum += x[j]; }
    su32 tot;
    su32 run = sfm_block_excl_scan(sum, &tot, sm);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) { if (base + j < n) data[base + j] = run; run += x[j]; }
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one workgroup: exclusive scan of the tile totals (64-bit carry: *total64 tells the caller whether 32 bits sufficed)
__global__ __launch_bounds__(256) void sfm_scan_top_kernel(su32* __restrict__ bsum, int nb, su64* __restrict__ total64)
{
    __shared__ su32 sm[4];
    su64 carry = 0;
    for (int base = 0; base < nb; base += 256) {
        const int i = base + threadIdx.x;
        const su32 v = i < nb ? bsum[i] : 0u;
        su32 tot;
        const su32 ex = sfm_block_excl_scan(v, &tot, sm);
        if (i < nb) bsum[i] = (su32)(carry + ex);
        carry += tot;
    }
    if (threadIdx.x == 0 && total64) *total64 = carry;
}

__global__ __launch_bounds__(256) void sfm_scan_add_kernel(su32* __restrict__ data, size_t n, const su32* __restrict__ bsum)
{
    const su32 add = bsum[blockIdx.x];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) { const size_t i = base + (size_t)j * 256 + threadIdx.x; if (i < n) data[i] += add; }
}

static inline size_t scan_tiles(size_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
size_t SfmScan::bsum_words(size_t n) { return scan_tiles(n); }

void sfm_enqueue_scan(hipStream_t st, su32* data, size_t n, su32* bsum, su64* total64)
{
    if (n == 0) { if (total64) (void)hipMemsetAsync(total64, 0, sizeof(su64), st); return; }
    const int nb = (int)scan_tiles(n);
    hipLaunchKernelGGL(sfm_scan_tile_kernel, dim3(nb), dim3(256), 0, st, data, n, bsum);
    hipLaunchKernelGGL(sfm_scan_top_kernel, dim3(1), dim3(256), 0, st, bsum, nb, total64);
    hipLaunchKernelGGL(sfm_scan_add_kernel, dim3(nb), dim3(256), 0, st, data, n, (const su32*)bsum);
}

// ------------------------------------------------------------------------------------------------
// stable LSD radix sort of (64-bit key, 32-bit value) pairs, 8 bits per pass
//   tile = 4 waves x RS_ROUNDS x 64 consecutive elements; a wave owns a contiguous piece of the tile and walks it 64
//   elements at a time, ranking equal digits with a match-any over eight ballots, so equal keys keep their order.
// ------------------------------------------------------------------------------------------------
#define RS_ROUNDS 16
#define RS_TILE (256 * RS_ROUNDS)

__global__ __launch_bounds__(256) void sfm_sort_hist_kernel(const su64* __restrict__ keys, size_t n, int shift, su32* __restrict__ hist, int nblocks)
{
    __shared__ su32 cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * RS_TILE;
#pragma unroll 4
    for (int r = 0; r < RS_ROUNDS; ++r) {
        const size_t i = base + (size_t)r * 256 + threadIdx.x;
        if (i < n) atomicAdd(&cnt[(su32)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = cnt[threadIdx.x];      // digit-major: one scan over the whole table gives the offsets
}

__global__ __launch_bounds__(256) void sfm_sort_scatter_kernel(const su64* __restrict__ kin, const su32* __restrict__ vin, su64* __restrict__ kout,
                                                               su32* __restrict__ vout, size_t n, int shift, const su32* __restrict__ off, int nblocks)
{
    __shared__ su32 wcnt[4][256];
    __shared__ su32 wbase[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const size_t w0 = (size_t)blockIdx.x * RS_TILE + (size_t)wave * (64 * RS_ROUNDS);
    su64 k[RS_ROUNDS]; su32 v[RS_ROUNDS], rk[RS_ROUNDS];
    const su64 lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        const size_t i = w0 + (size_t)r * 64 + lane;
        const bool valid = i < n;
        k[r] = valid ? kin[i] : 0ull;
        v[r] = valid ? (vin ? vin[i] : (su32)i) : 0u;
        const su32 d = (su32)(k[r] >> shift) & 255u;
        su64 m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) { const bool bit = (d >> b) & 1u; const su64 bal = __ballot(bit); m &= bit ? bal : ~bal; }
        rk[r] = 0;
        if (valid) {
            // every lane of the group reads the wave's running count of this digit, then the group's last lane advances it
            // (one wave, program order: the read of all lanes precedes the write)
            const su32 prev = wcnt[wave][d];
            rk[r] = prev + (su32)__popcll(m & lt);
            if ((m >> lane) == 1ull) wcnt[wave][d] = prev + (su32)__popcll(m);
        }
    }
    __syncthreads();
    {
        su32 run = off[(size_t)tid * nblocks + blockIdx.x];
#pragma unroll
        for (int w = 0; w < 4; ++w) { wbase[w][tid] = run; run += wcnt[w][tid]; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        const size_t i = w0 + (size_t)r * 64 + lane;
        if (i < n) {
            const su32 d = (su32)(k[r] >> shift) & 255u;
            const size_t pos = (size_t)wbase[wave][d] + rk[r];
            kout[pos] = k[r]; vout[pos] = v[r];
        }
    }
}

static inline size_t sort_tiles(size_t n) { return (n + RS_TILE - 1) / RS_TILE; }
size_t SfmSort::hist_words(size_t n) { return (size_t)256 * sort_tiles(n); }
size_t SfmSort::bsum_words(size_t n) { return scan_tiles(hist_words(n)); }

int SfmSort::sort(hipStream_t st, size_t n, int cur, int bits, bool identity_vals) const
{
    if (n == 0) return cur;
    const int passes = bits <= 0 ? 1 : (bits + 7) / 8;
    const int nblocks = (int)sort_tiles(n);
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(sfm_sort_hist_kernel, dim3(nblocks), dim3(256), 0, st, (const su64*)k[cur], n, 8 * p, hist, nblocks);
        sfm_enqueue_scan(st, hist, (size_t)256 * nblocks, bsum, nullptr);
        hipLaunchKernelGGL(sfm_sort_scatter_kernel, dim3(nblocks), dim3(256), 0, st, (const su64*)k[cur],
                           (p == 0 && identity_vals) ? (const su32*)nullptr : (const su32*)v[cur], k[cur ^ 1], v[cur ^ 1], n, 8 * p,
                           (const su32*)hist, nblocks);
        cur ^= 1;
    }
    return cur;
}

// run heads of sorted keys
__global__ __launch_bounds__(256) void sfm_run_head_kernel(const su64* __restrict__ keys, size_t n, su64 limit, su32* __restrict__ flag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    flag[i] = (i < n && keys[i] < limit && (i == 0 || keys[i - 1] != keys[i])) ? 1u : 0u;      // n + 1 entries: the scan leaves the count in flag[n]
}

void sfm_enqueue_run_heads(hipStream_t st, const su64* keys, size_t n, su64 limit, su32* flag)
{
    hipLaunchKernelGGL(sfm_run_head_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, keys, n, limit, flag);
}

// ------------------------------------------------------------------------------------------------
// the two primitives on host arrays, for the tests of the contract of sortscan.hpp
// ------------------------------------------------------------------------------------------------
extern "C" {

int sfmhip_debug_sort_pairs(sfmhip_ctx* ctx, const uint64_t* keys, const uint32_t* vals, size_t n, int bits, uint64_t* keys_out, uint32_t* vals_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_debug_sort_pairs");
    SFM_ARG_CHECK(ctx, ctx && bits >= 0 && bits <= 64 && n <= 0x7fffffffull && (n == 0 || (keys && keys_out && vals_out)));
    SFM_ARG_CHECK(ctx, !ranges_overlap(keys_out, n * 8, keys, n * 8) && !ranges_overlap(keys_out, n * 8, vals, n * 4) &&
                           !ranges_overlap(vals_out, n * 4, keys, n * 8) && !ranges_overlap(vals_out, n * 4, vals, n * 4) &&
                           !ranges_overlap(keys_out, n * 8, vals_out, n * 4));
    SfmCarve carve;
    SfmSort S(carve, n);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    S.bind(w);
    hipStream_t st = ctx->stream;
    hipError_t e = n ? hipMemcpyAsync(S.k[0], keys, n * 8, hipMemcpyHostToDevice, st) : hipSuccess;
    if (e == hipSuccess && n && vals) e = hipMemcpyAsync(S.v[0], vals, n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const int side = S.sort(st, n, 0, bits, vals == nullptr);
        e = hipGetLastError();
        if (e == hipSuccess && n) e = hipMemcpyAsync(keys_out, S.k[side], n * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && n) e = hipMemcpyAsync(vals_out, S.v[side], n * 4, hipMemcpyDeviceToHost, st);
    }
    return sfm_finish(ctx, e);
}

int sfmhip_debug_scan_u32(sfmhip_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out, uint64_t* total64_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_debug_scan_u32");
    SFM_ARG_CHECK(ctx, ctx && n <= 0x7fffffffull && (n == 0 || (in && out)));
    SFM_ARG_CHECK(ctx, !ranges_overlap(out, n * 4, in, n * 4) && !ranges_overlap(total64_out, 8, in, n * 4) && !ranges_overlap(total64_out, 8, out, n * 4));
    SfmCarve carve;
    SfmScan S(carve, n);
    const size_t o_total = carve(sizeof(uint64_t));
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    S.bind(w);
    unsigned long long* total = (unsigned long long*)(w + o_total);
    hipStream_t st = ctx->stream;
    hipError_t e = n ? hipMemcpyAsync(S.data, in, n * 4, hipMemcpyHostToDevice, st) : hipSuccess;
    if (e == hipSuccess) {
        S.scan(st, n, total);
        e = hipGetLastError();
        if (e == hipSuccess && n) e = hipMemcpyAsync(out, S.data, n * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && total64_out) e = hipMemcpyAsync(total64_out, total, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    }
    return sfm_finish(ctx, e);
}

}  // extern "C"
