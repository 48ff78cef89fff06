// ransac.hpp -- what the RANSAC engines of planes.hip and twoview.hip share, and nothing that knows a model: the counter-based sampler, the
// H x m scoring loop and the winner reduction, each prescribed bit for bit by sfmhip.h.  Include it below `#pragma clang fp contract(off)`.
//
// The shape of the scoring loop.  LANES OWN HYPOTHESES: a workgroup of 256 threads takes 256 hypotheses (blockIdx.x) and a sequence of
// chunks of SCORE_CHUNK rows (blockIdx.y, then a stride of gridDim.y chunks); a lane keeps its model (2 NPAR VGPRs) and its count in
// registers; the chunk is staged in LDS as rows of the model's type (M::Row: four doubles, or the padded five of the absolute pose), and
// every lane reads the SAME row at the same time: identical addresses are a broadcast, without bank conflicts.  Per row a wave issues the model's residual (contraction is off: it is the prescribed formula),
// a compare and a conditional add, and these VALU instructions are what bounds the kernel (the accounts are with the models).  A wave none
// of whose lanes has a hypothesis (H = 65: three waves of the second block) only helps with the staging.  Counts: one integer atomicAdd
// per lane at the very end, so a counter takes at most gridDim.y adds per round, from different workgroups at different times; integer
// sums are exact in any order.
#pragma once
#include "common.hpp"

#define SCORE_CHUNK 512          // rows staged per pass of the scoring loop (16 KB of LDS for rows of four doubles, 24 KB for rows of six)
#define SCORE_MAX_WG 2048        // workgroups of a scoring kernel (per pair) at most, 8 per CU of the MI355X; beyond that a workgroup strides over chunks

typedef unsigned long long pu64;
typedef unsigned int pu32;

// gridDim.y of a scoring launch over at most `rows` rows and hb blocks of 256 hypotheses
static inline int ransac_score_grid_y(int rows, int hb) { return std::max(1, std::min(ceil_div(rows, SCORE_CHUNK), SCORE_MAX_WG / hb)); }

__device__ __forceinline__ pu64 splitmix64(pu64 seed, pu64 c)
{
    pu64 z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the K distinct positions in [0, m), m >= K, that hypothesis g draws, in draw order: draw k is splitmix64(seed, K g + k) mod (m - k),
// moved past the earlier draws in ascending order (srt: the ones chosen so far, ascending)
template <int K>
__device__ __forceinline__ void ransac_sample_distinct(pu64 seed, pu64 g, pu64 m, pu64 (&u)[K])
{
    pu64 srt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        pu64 v = splitmix64(seed, (pu64)K * g + (pu64)k) % (m - (pu64)k);
#pragma unroll
        for (int j = 0; j < k; ++j) v += v >= srt[j] ? 1ull : 0ull;
        u[k] = srt[k] = v;
#pragma unroll
        for (int j = k; j > 0; --j) {
            const pu64 lo = srt[j] < srt[j - 1] ? srt[j] : srt[j - 1], hi = srt[j] < srt[j - 1] ? srt[j - 1] : srt[j];
            srt[j - 1] = lo; srt[j] = hi;
        }
    }
}

// The scoring loop of one workgroup (the shape is explained at the top): the number of rows[0 .. m) that this lane's model accepts, added
// to *counter.  Every thread of the workgroup calls it.  tile: SCORE_CHUNK rows of LDS; model: the lane's M::NPAR parameters, or null for
// a lane without a hypothesis.  M supplies Row (the type of a staged row), NPAR, UNROLL (of the row loop) and
// inlier(const double (&P)[NPAR], const Row& row, double thr).
template <class M>
__device__ __forceinline__ void ransac_score(typename M::Row* tile, const typename M::Row* __restrict__ rows, int m, const double* __restrict__ model,
                                             double thr, int32_t* __restrict__ counter)
{
    if ((int)blockIdx.y * SCORE_CHUNK >= m) return;                      // uniform over the workgroup; m >= 1 behind it
    const int nchunks = (m - 1) / SCORE_CHUNK + 1;
    const bool live = model != nullptr;
    const bool wave_live = __any(live);                                  // uniform over the wave
    double P[M::NPAR];
#pragma unroll
    for (int j = 0; j < M::NPAR; ++j) P[j] = live ? model[j] : NAN;
    int count = 0;
    for (int c = blockIdx.y; c < nchunks; c += gridDim.y) {              // chunk numbers and the rows of a chunk fit an int for every m
        const typename M::Row* chunk = rows + (size_t)c * SCORE_CHUNK;
        const int cnt = m - c * SCORE_CHUNK < SCORE_CHUNK ? m - c * SCORE_CHUNK : SCORE_CHUNK;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SCORE_CHUNK / 256; ++k) {
            const int r = k * 256 + (int)threadIdx.x;
            if (r < cnt) tile[r] = chunk[r];
        }
        __syncthreads();
        if (!wave_live) continue;
#pragma unroll M::UNROLL
        for (int r = 0; r < cnt; ++r) {
            const typename M::Row row = tile[r];
            count += M::inlier(P, row, thr) ? 1 : 0;
        }
    }
    if (live && count) atomicAdd(counter, count);
}

// The winner of H hypotheses, one workgroup of 256 threads: the valid one with the largest count, the smallest h among equals, as the
// packed key ((count + 1) << 32) | (0xffffffff - h); 0: no valid hypothesis.  Every thread of the workgroup calls it and gets the key.
// sb: 256 entries of LDS.
__device__ __forceinline__ pu64 ransac_block_winner(const int32_t* __restrict__ hvalid, const int32_t* __restrict__ hcnt, int H, pu64* sb)
{
    pu64 best = 0ull;
    for (int h = threadIdx.x; h < H; h += 256) {
        if (!hvalid[h]) continue;
        const pu64 v = ((pu64)((pu32)hcnt[h] + 1u) << 32) | (pu64)(0xffffffffu - (pu32)h);      // a valid hypothesis: v > 0
        best = v > best ? v : best;
    }
    sb[threadIdx.x] = best;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off && sb[threadIdx.x + off] > sb[threadIdx.x]) sb[threadIdx.x] = sb[threadIdx.x + off];
        __syncthreads();
    }
    return sb[0];
}
__device__ __forceinline__ int ransac_key_count(pu64 key) { return (int)((pu32)(key >> 32) - 1u); }      // of a key > 0
__device__ __forceinline__ int ransac_key_h(pu64 key) { return (int)(0xffffffffu - (pu32)key); }
