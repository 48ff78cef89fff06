// ba_setup.hpp -- construction of a bundle-adjustment problem ON THE DEVICE (included by ba.hip only: its kernels have external linkage).
//
// bundle_adjustment() of the reference is ONE call that builds the ceres::Problem and solves it
// (NViewReconstuct.cpp:1169-1224), and the "Time (s)" it prints covers both (NView:1239).  What has to be built here
// before the first LM iteration are orderings of the observation list:
//   * observations grouped by point, a point's observations by ascending camera (ties: caller's order);
//   * points stored sorted by the list of cameras that see them (lexicographic, ties: caller's order), so that the
//     per-camera and per-camera-pair walks of the kernels gather from runs of neighbouring records;
//   * a camera-ordered copy of (point slot, pixel);
//   * for every pair of free cameras that share points, the list of observation pairs, cut into chunks.
// Rounds 1-2 did this with std::sort / std::stable_sort on one host thread: 0.2 s at C4 (200 cameras / 1.2M observations)
// and 1.3 s at C5 (1000 / 8M) -- ten to a hundred times the LM loop it prepares.  All of it is now a handful of
// stable LSD radix sorts, prefix sums and gather kernels on the GPU; the host only sees per-camera-pair counts.
// The resulting tables are identical, entry by entry, to the ones the host code produced (tests/test_ba_setup_gpu.py
// restates the orderings in numpy), so the iteration results stay bit-identical.
//
// Everything here is HBM-bound integer work on a few hundred MB at most, in plain coalesced passes: the key, starts, slot, fill,
// pair, items and crange kernels.  The sorts, the scans and the run heads between them are the library's own (sortscan.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sortscan.hpp"

typedef unsigned long long su64;
typedef unsigned int su32;

// ------------------------------------------------------------------------------------------------
// the set-up passes
// ------------------------------------------------------------------------------------------------
static inline int setup_bit_width(su64 x) { int b = 0; while (x) { ++b; x >>= 1; } return b; }

// observation k -> key (point << cb | camera); flags[0] |= 1 on an index out of range (the key then stays inside the tables)
__global__ __launch_bounds__(256) void setup_obs_key_kernel(const int* __restrict__ rc, const int* __restrict__ rp, int nobs, int nc, int np, int cb,
                                                            su64* __restrict__ keys, int* __restrict__ flags)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nobs) return;
    const int c = rc[k], p = rp[k];
    if (c < 0 || c >= nc || p < 0 || p >= np) { atomicOr(flags, 1); keys[k] = 0; return; }
    keys[k] = ((su64)p << cb) | (su64)c;
}

// keys sorted; v(i) = keys[i] >> shift < nvals.  starts[v] = first i with v(i) >= v, for v = 0 .. nvals (starts[nvals] = n): the
// CSR offsets of the sorted list without counters or atomics (an atomic per observation on its camera's counter -- 8,000 per
// address at C5 -- made this pass 10 ms; as boundaries of the sorted keys it is one coalesced read)
__global__ __launch_bounds__(256) void setup_starts_kernel(const su64* __restrict__ keys, size_t n, int shift, su64 nvals, su32* __restrict__ starts)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    const su64 cur = i < n ? keys[i] >> shift : nvals;
    su64 v = i > 0 ? (keys[i - 1] >> shift) + 1 : 0;
    for (; v <= cur && v <= nvals; ++v) starts[v] = (su32)i;
}

// max over p of st[p + 1] - st[p] (the longest track): one atomic per workgroup
__global__ __launch_bounds__(256) void setup_max_kernel(const su32* __restrict__ st, int n, su32* __restrict__ out)
{
    __shared__ su32 sm[4];
    su32 x = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) x = max(x, st[i + 1] - st[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = max(x, (su32)__shfl_xor(x, off));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) { x = max(max(sm[0], sm[1]), max(sm[2], sm[3])); if (x) atomicMax(out, x); }
}

// Sort key of a point for one group of positions [j0, j0 + npos) of its ascending camera list: fields of b bits,
// earlier positions in the higher bits, camera + 1 (0 = the list has ended: a prefix sorts first).
__global__ __launch_bounds__(256) void setup_ptkey_kernel(const su32* __restrict__ order, int np, const su32* __restrict__ st,
                                                          const su64* __restrict__ obs_keys, su64 cam_mask, int j0, int npos, int b, su64* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const su32 p = order ? order[i] : (su32)i;
    const su32 base = st[p], m = st[p + 1] - base;
    su64 key = 0;
    for (int j = j0; j < j0 + npos; ++j) key = (key << b) | ((su32)j < m ? (obs_keys[base + j] & cam_mask) + 1ull : 0ull);
    out[i] = key;
}

// slot of every point, and the per-slot observation counts (scanned into pt_start by the caller)
__global__ __launch_bounds__(256) void setup_slot_kernel(const su32* __restrict__ order, int np, const su32* __restrict__ st, int* __restrict__ slot,
                                                         su32* __restrict__ cnt_slot)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= np) return;
    const su32 p = order[s];
    slot[p] = s; cnt_slot[s] = st[p + 1] - st[p];
}

// observations into their final order: by slot, inside a point by (camera, caller's index)
__global__ __launch_bounds__(256) void setup_fill_obs_kernel(const su64* __restrict__ obs_keys, const su32* __restrict__ obs_k, int nobs, int cb,
                                                             const su32* __restrict__ st, const int* __restrict__ slot, const int* __restrict__ pt_start,
                                                             const double2* __restrict__ ruv, int* __restrict__ ocam, int* __restrict__ opt,
                                                             double2* __restrict__ ouv, su64* __restrict__ cam_keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nobs) return;
    const su64 key = obs_keys[i];
    const su32 p = (su32)(key >> cb);
    const int cam = (int)(key & ((1ull << cb) - 1ull));
    const int s = slot[p];
    const int q = pt_start[s] + (int)((su32)i - st[p]);
    ocam[q] = cam; opt[q] = s; ouv[q] = ruv[obs_k[i]];
    cam_keys[q] = (su64)cam;
}

// dst[slot[p]] = src[p] (to_slot) or dst[p] = src[slot[p]] (back to the caller's order), 3 doubles per point
__global__ __launch_bounds__(256) void setup_permute_pts_kernel(const double* __restrict__ src, const int* __restrict__ slot, int np, double* __restrict__ dst, int to_slot)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    const size_t a = 3 * (size_t)p, b = 3 * (size_t)slot[p];
    const size_t from = to_slot ? a : b, to = to_slot ? b : a;
    dst[to] = src[from]; dst[to + 1] = src[from + 1]; dst[to + 2] = src[from + 2];
}

// camera-ordered copy of (point slot, pixel): q_sorted = observation indices sorted by camera (stable)
__global__ __launch_bounds__(256) void setup_cam_copy_kernel(const su32* __restrict__ q_sorted, int nobs, const int* __restrict__ opt, const double2* __restrict__ ouv,
                                                             int* __restrict__ cam_pt, double2* __restrict__ cam_uv)
{
    const int at = blockIdx.x * 256 + threadIdx.x;
    if (at >= nobs) return;
    const su32 q = q_sorted[at];
    cam_pt[at] = opt[q]; cam_uv[at] = ouv[q];
}

// observation pairs of a point between free cameras: a point's observations are in ascending camera order and the constant
// cameras are numbered first (sfmhip_ba_create_ex renumbers them), so those of constant cameras lead; with m others there are
// m (m - 1) / 2 pairs.  A constant point (ptfix, per slot; null: none) has no pairs at all.
__device__ __forceinline__ int setup_lead_fixed(const int* __restrict__ ocam, int lo, int hi, int nfix, const unsigned char* __restrict__ ptfix, int s)
{
    if (ptfix && ptfix[s]) return hi - lo;
    int z = 0;
    if (nfix) while (lo + z < hi && ocam[lo + z] < nfix) ++z;
    return z;
}
// total64 (zeroed by the caller): the number of pairs in 64 bits.  The per-point counters and the tile sums of the scan behind them are
// 32 bits wide and WRAP for absurd inputs (4096 points of 1449 observations each in one tile); the caller rejects the problem on this
// sum before it looks at anything the scan produced.
__global__ __launch_bounds__(256) void setup_pair_count_kernel(const int* __restrict__ pt_start, const int* __restrict__ ocam, int np, int nfix,
                                                               const unsigned char* __restrict__ ptfix, su32* __restrict__ npair, su64* __restrict__ total64)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    su64 c = 0;
    if (s < np) {
        const int lo = pt_start[s], hi = pt_start[s + 1];
        const su64 m = (su64)(hi - lo - setup_lead_fixed(ocam, lo, hi, nfix, ptfix, s));
        c = m * (m - (m ? 1 : 0)) / 2;
        npair[s] = c > 0xffffffffull ? 0xffffffffu : (su32)c;
    }
    su64 v = c;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off);
        v += ((su64)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)total64, (unsigned long long)v);
}

// thread per observation i: its pairs (i, j > i) in the order "for i, for j" of the point -- key = ca * nc + cb with ca >= cb,
// raw = (observation of ca, observation of cb)
__global__ __launch_bounds__(256) void setup_pair_gen_kernel(const int* __restrict__ pt_start, const int* __restrict__ ocam, const int* __restrict__ opt, int nobs,
                                                             int nfix, const unsigned char* __restrict__ ptfix, int nc, const su32* __restrict__ pair_off,
                                                             su64* __restrict__ keys, int2* __restrict__ raw)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nobs) return;
    const int s = opt[q], lo = pt_start[s], hi = pt_start[s + 1];
    const int z = setup_lead_fixed(ocam, lo, hi, nfix, ptfix, s);
    const long long a = (long long)q - (lo + z), m = (long long)hi - lo - z;
    if (a < 0) return;
    size_t id = (size_t)pair_off[s] + (size_t)(a * (2 * m - a - 1) / 2);
    const int ci = ocam[q];
    for (int j = q + 1; j < hi; ++j, ++id) {
        const int cj = ocam[j];                   // cj >= ci
        if (ci < cj) { keys[id] = (su64)cj * (su64)nc + (su64)ci; raw[id] = make_int2(j, q); }
        else         { keys[id] = (su64)ci * (su64)nc + (su64)cj; raw[id] = make_int2(q, j); }
    }
}

// constant points back into the caller's order with the bits given at create (the LM state may hold a -0 as +0): out[p] = pts0[slot[p]]
__global__ __launch_bounds__(256) void setup_restore_fixed_pts_kernel(const double* __restrict__ pts0, const int* __restrict__ slot, const unsigned char* __restrict__ ptfix,
                                                                      int np, double* __restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    const int s = slot[p];
    if (ptfix[s]) { out[3 * (size_t)p] = pts0[3 * (size_t)s]; out[3 * (size_t)p + 1] = pts0[3 * (size_t)s + 1]; out[3 * (size_t)p + 2] = pts0[3 * (size_t)s + 2]; }
}

// per-slot constant-point flags from the caller's order: flags_slot[slot[p]] = flags[p]
__global__ __launch_bounds__(256) void setup_slot_flags_kernel(const unsigned char* __restrict__ flags, const int* __restrict__ slot, int np, unsigned char* __restrict__ flags_slot)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < np) flags_slot[slot[p]] = flags[p] ? 1 : 0;
}

// run starts of the sorted pair keys: run heads -> (scan) -> compaction
__global__ __launch_bounds__(256) void setup_compact_kernel(const su64* __restrict__ keys, const su32* __restrict__ rank, size_t n, su64* __restrict__ blk_key,
                                                            su32* __restrict__ blk_first)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    if (t == 0 || keys[t] != keys[t - 1]) { blk_key[rank[t]] = keys[t]; blk_first[rank[t]] = (su32)t; }
}

// items of the pair kernels, in sorted order: [observation i, observation j, point slot, 0]
__global__ __launch_bounds__(256) void setup_items_kernel(const su32* __restrict__ id_sorted, const int2* __restrict__ raw, const int* __restrict__ opt, size_t n,
                                                          int4* __restrict__ items)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int2 r = raw[id_sorted[t]];
    items[t] = make_int4(r.x, r.y, opt[r.x], 0);
}

// lowest and highest camera among the observations of every block of 256 points (the back-substitution stages them in LDS)
__global__ __launch_bounds__(256) void setup_crange_kernel(const int* __restrict__ pt_start, const int* __restrict__ ocam, int np, int* __restrict__ crange)
{
    __shared__ int slo[4], shi[4];
    const int b = blockIdx.x;
    const int q0 = pt_start[min(np, b * 256)], q1 = pt_start[min(np, (b + 1) * 256)];
    int lo = INT_MAX, hi = -1;
    for (int q = q0 + threadIdx.x; q < q1; q += 256) { const int c = ocam[q]; lo = min(lo, c); hi = max(hi, c); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_xor(lo, off)); hi = max(hi, __shfl_xor(hi, off)); }
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        crange[2 * (size_t)b] = min(min(slo[0], slo[1]), min(slo[2], slo[3]));
        crange[2 * (size_t)b + 1] = max(max(shi[0], shi[1]), max(shi[2], shi[3]));
    }
}
