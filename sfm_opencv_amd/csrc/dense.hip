// dense.hip -- dense depth from calibrated images: the plane sweep (sfmhip_plane_sweep), the consistency check between the depth maps of
// neighbouring views (sfmhip_depth_consistency) and the export of the kept pixels as coloured world points (sfmhip_depth_to_points), with
// the host helper that prepares their geometry (sfmhip_sweep_geometry); and the sweep's regularised form, the semi-global aggregation of
// its cost volume (sfmhip_sweep_costs, sfmhip_sgm_depth, sfmhip_plane_sweep_sgm).  The definition is in sfmhip.h at sfmhip_plane_sweep and is
// followed to the letter: the warp is prescribed float operation by operation, the samples and the window sums are integers, the scores
// are doubles formed from those integers in a fixed order.  Nothing here depends on the order of a sum, so the launch geometry is free.
//
// Kernels
//   dense_gray_kernel     every image of a call (the reference and its sources) becomes one dense gray plane, once: the sweep's gathers
//                         then touch a byte per tap instead of three, and no row stride
//   sweep_kernel<R>       a workgroup of 256 threads owns a tile of 32 x 16 reference pixels, two per thread (and walks the tiles of the
//                         image with the stride of the grid, which is sized by the CUs).  The reference values of tile + halo go to LDS
//                         once per tile as 16-bit values; a thread keeps Sr and vr of its windows in registers for the whole sweep.  Per
//                         (group of four planes, source) the threads write the warped samples of tile + halo to LDS (16 bits, 0xFFFF =
//                         not good), meet at ONE barrier (the sample area is double-buffered), and every thread takes its windows' Sw,
//                         Sww, Srw out of LDS.  The running best, its two neighbour scores and the pending-right flag are per-thread
//                         state.
//   sgm_cost_kernel<R>    sweep_kernel's sibling: the same scoring, but every plane's score leaves as a 16-bit cost (sfmhip_sweep_costs)
//   sgm_path_kernel<PPL>  the semi-global aggregation of that volume (sfmhip_sgm_depth): a launch per direction, a wave per line, lanes on
//                         the planes; unsigned integers only
//   sgm_winner_kernel     a wave per pixel: the first smallest sum among the scored planes, the sub-plane fit
//   consistency_kernel    one thread per pixel, fp64
//   points_count_kernel / points_write_kernel   the kept pixels of 256 consecutive pixels are counted per workgroup, the counts go through
//                         the exclusive scan of sortscan.hpp, and the second kernel ranks the pixels inside a workgroup by ballots: the
//                         rows come out in row-major order without an atomic.
#include "common.hpp"
#include "sortscan.hpp"
#include <cmath>
#pragma clang fp contract(off)

#define DENSE_SRC_MAX 8
#define DENSE_DIM_MAX 16384
#define SWEEP_TW 32
#define SWEEP_PX 2                            // pixels per thread
#define SWEEP_TH (8 * SWEEP_PX)
#define SWEEP_THREADS (SWEEP_TW * SWEEP_TH / SWEEP_PX)
#define SWEEP_RMAX 5
#define SWEEP_HW (SWEEP_TW + 2 * SWEEP_RMAX)
#define SWEEP_HH (SWEEP_TH + 2 * SWEEP_RMAX)
#define SWEEP_BAD 0xFFFFu
#define SWEEP_PLANES_MAX 4096
#define SWEEP_KB 4                            // planes warped per barrier

struct DenseImages { const uint8_t* img[DENSE_SRC_MAX + 1]; };

struct SweepParams {
    const uint8_t* ref;
    const uint8_t* src[DENSE_SRC_MAX];
    float A[DENSE_SRC_MAX][9], b[DENSE_SRC_MAX][3];
    double wmin, step, min_score;
    int n_src, rows, cols, D, r, min_sources;
};

struct ConsistencyParams {
    const float* src[DENSE_SRC_MAX];
    double R[DENSE_SRC_MAX][9], t[DENSE_SRC_MAX][3];
    double fx, fy, cx, cy, rel_tol;
    int n_src, rows, cols, min_consistent;
};

struct PointsParams { double fx, fy, cx, cy, Rinv[9], c[3]; };

// image blockIdx.y of the call as a dense gray plane: (1868 B + 9617 G + 4899 R + 8192) >> 14 for BGR, a copy for gray
__global__ __launch_bounds__(256) void dense_gray_kernel(DenseImages I, int rows, int cols, int channels, size_t ld, uint8_t* __restrict__ gray)
{
    const size_t npx = (size_t)rows * cols;
    const uint8_t* __restrict__ img = I.img[blockIdx.y];
    uint8_t* __restrict__ out = gray + npx * blockIdx.y;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const size_t y = i / (size_t)cols, x = i - y * (size_t)cols;
        const uint8_t* p = img + y * ld + x * (size_t)channels;
        out[i] = channels == 1 ? p[0] : (uint8_t)((1868u * p[0] + 9617u * p[1] + 4899u * p[2] + 8192u) >> 14);
    }
}

// what a thread keeps per pixel it owns for the whole sweep: the reference window's sums, the running best with its two neighbour
// scores and the pending-right flag
struct SweepPixel {
    double dvr, best, best_l, best_r, prev;
    uint32_t Sr;
    int best_k;
    bool in_image, valid, has_l, has_r, prev_ok, pending;
};

// R: the window radius (an instantiation per radius: the window's inner loop unrolls and the LDS addresses are immediates).  A thread
// owns SWEEP_PX pixels of its column, SWEEP_TH / SWEEP_PX rows apart.  SWEEP_KB planes are warped per barrier, so a thread has some
// 3 * SWEEP_KB * 4 gathers in flight and reads a reference value once for SWEEP_KB samples.
template <int R>
__global__ __launch_bounds__(SWEEP_THREADS) void sweep_kernel(SweepParams P, int tiles_x, int n_tiles, int32_t* __restrict__ plane, float* __restrict__ score,
                                                              float* __restrict__ depth)
{
    constexpr int SIDE = 2 * R + 1, HW = SWEEP_TW + 2 * R, NH = HW * (SWEEP_TH + 2 * R), NWIN = SIDE * SIDE, ROWS_APART = SWEEP_TH / SWEEP_PX;
    __shared__ uint16_t ref16[SWEEP_HH * SWEEP_HW];
    __shared__ uint16_t smp[2][SWEEP_KB][SWEEP_HH * SWEEP_HW];
    const int tid = threadIdx.x, tx = tid & (SWEEP_TW - 1), ty = tid / SWEEP_TW;
    const int rows = P.rows, cols = P.cols;
    const float cm1 = (float)(cols - 1), rm1 = (float)(rows - 1);
    int buf = 0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int x0 = (tile % tiles_x) * SWEEP_TW, y0 = (tile / tiles_x) * SWEEP_TH;
        __syncthreads();                                                 // the previous tile's windows have been read
#pragma unroll
        for (int i = tid; i < NH; i += SWEEP_THREADS) {
            const int hy = i / HW, hx = i - hy * HW, u = x0 - R + hx, v = y0 - R + hy;
            const bool in = u >= 0 && u < cols && v >= 0 && v < rows;
            ref16[i] = in ? (uint16_t)(P.ref[(size_t)v * cols + u] * 16u) : (uint16_t)0;
        }
        __syncthreads();
        const int u = x0 + tx;
        SweepPixel px[SWEEP_PX];
#pragma unroll
        for (int p = 0; p < SWEEP_PX; ++p) {
            SweepPixel& q = px[p];
            const int v = y0 + ty + p * ROWS_APART;
            q.in_image = u < cols && v < rows;
            q.valid = q.in_image && u - R >= 0 && u + R < cols && v - R >= 0 && v + R < rows;
            uint32_t Sr = 0, Srr = 0;
            if (q.valid) {
#pragma nounroll
                for (int dy = 0; dy < SIDE; ++dy)
#pragma unroll
                    for (int dx = 0; dx < SIDE; ++dx) {
                        const uint32_t g = ref16[(ty + p * ROWS_APART + dy) * HW + tx + dx];
                        Sr += g; Srr += g * g;
                    }
            }
            const int64_t vr = (int64_t)NWIN * (int64_t)Srr - (int64_t)Sr * (int64_t)Sr;
            q.valid = q.valid && vr > 0;
            q.dvr = (double)vr; q.Sr = Sr;
            q.best_k = -1; q.best = 0.0; q.best_l = 0.0; q.best_r = 0.0; q.prev = 0.0;
            q.has_l = false; q.has_r = false; q.prev_ok = false; q.pending = false;
        }
        for (int k0 = 0; k0 < P.D; k0 += SWEEP_KB) {
            float wf[SWEEP_KB];
            double sum[SWEEP_PX][SWEEP_KB];
            int cnt[SWEEP_PX][SWEEP_KB];
#pragma unroll
            for (int j = 0; j < SWEEP_KB; ++j) {
                wf[j] = (float)(P.wmin + (double)(k0 + j) * P.step);
#pragma unroll
                for (int p = 0; p < SWEEP_PX; ++p) { sum[p][j] = 0.0; cnt[p][j] = 0; }
            }
            for (int s = 0; s < P.n_src; ++s) {
                const float* __restrict__ A = P.A[s];
                const uint8_t* __restrict__ g = P.src[s];
                uint16_t (*S)[SWEEP_HH * SWEEP_HW] = smp[buf];
#pragma unroll
                for (int i = tid; i < NH; i += SWEEP_THREADS) {
                    const int hy = i / HW, hx = i - hy * HW, uu = x0 - R + hx, vv = y0 - R + hy;
                    const bool in = uu >= 0 && uu < cols && vv >= 0 && vv < rows;
                    const float fu = (float)uu, fv = (float)vv;
                    const float a0 = A[0] * fu + A[1] * fv, a1 = A[3] * fu + A[4] * fv, a2 = A[6] * fu + A[7] * fv;
#pragma unroll
                    for (int j = 0; j < SWEEP_KB; ++j) {
                        uint32_t val = SWEEP_BAD;
                        if (in && k0 + j < P.D) {
                            const float q0 = a0 + (A[2] + wf[j] * P.b[s][0]);
                            const float q1 = a1 + (A[5] + wf[j] * P.b[s][1]);
                            const float q2 = a2 + (A[8] + wf[j] * P.b[s][2]);
                            const float sx = q0 / q2, sy = q1 / q2;
                            if (q2 > 0.0f && sx >= 0.0f && sy >= 0.0f && sx < cm1 && sy < rm1) {
                                const int ix = (int)sx, iy = (int)sy;
                                const uint32_t fx = (uint32_t)(int)((sx - (float)ix) * 32.0f), fy = (uint32_t)(int)((sy - (float)iy) * 32.0f);
                                const uint8_t* t = g + (size_t)iy * cols + ix;
                                const uint32_t g00 = t[0], g01 = t[1], g10 = t[cols], g11 = t[cols + 1];
                                val = (g00 * (32u - fx) * (32u - fy) + g01 * fx * (32u - fy) + g10 * (32u - fx) * fy + g11 * fx * fy + 32u) >> 6;
                            }
                        }
                        S[j][i] = (uint16_t)val;
                    }
                }
                __syncthreads();                                         // one barrier per (plane group, source): the other buffer is filled next
#pragma unroll
                for (int p = 0; p < SWEEP_PX; ++p) {
                    if (!px[p].valid) continue;
                    uint32_t Sw[SWEEP_KB], Sww[SWEEP_KB], Srw[SWEEP_KB], any[SWEEP_KB];
#pragma unroll
                    for (int j = 0; j < SWEEP_KB; ++j) { Sw[j] = 0; Sww[j] = 0; Srw[j] = 0; any[j] = 0; }
#pragma nounroll
                    for (int dy = 0; dy < SIDE; ++dy)                    // a row of the window at a time: its loads fit the registers
#pragma unroll
                        for (int dx = 0; dx < SIDE; ++dx) {
                            const int at = (ty + p * ROWS_APART + dy) * HW + tx + dx;
                            const uint32_t gr = ref16[at];
#pragma unroll
                            for (int j = 0; j < SWEEP_KB; ++j) {
                                const uint32_t w = S[j][at];
                                any[j] |= w; Sw[j] += w; Sww[j] += w * w; Srw[j] += gr * w;
                            }
                        }
#pragma unroll
                    for (int j = 0; j < SWEEP_KB; ++j) {
                        if (any[j] & 0x8000u) continue;                  // a good sample is at most 4080; a plane past D - 1 is all bad
                        const int64_t vw = (int64_t)NWIN * (int64_t)Sww[j] - (int64_t)Sw[j] * (int64_t)Sw[j];
                        if (vw > 0) {
                            const int64_t cov = (int64_t)NWIN * (int64_t)Srw[j] - (int64_t)px[p].Sr * (int64_t)Sw[j];
                            sum[p][j] = sum[p][j] + (double)cov / sqrt(px[p].dvr * (double)vw);
                            ++cnt[p][j];
                        }
                    }
                }
                buf ^= 1;
            }
#pragma unroll
            for (int p = 0; p < SWEEP_PX; ++p) {
                SweepPixel& q = px[p];
#pragma unroll
                for (int j = 0; j < SWEEP_KB; ++j) {
                    const int k = k0 + j;
                    if (k >= P.D) break;
                    const bool ok = cnt[p][j] >= P.min_sources;
                    const double c = ok ? sum[p][j] / (double)cnt[p][j] : 0.0;
                    if (q.pending) { q.has_r = ok; q.best_r = c; q.pending = false; }
                    if (ok && (q.best_k < 0 || c > q.best)) { q.best = c; q.best_k = k; q.has_l = q.prev_ok; q.best_l = q.prev; q.has_r = false; q.pending = true; }
                    q.prev = c; q.prev_ok = ok;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < SWEEP_PX; ++p) {
            const SweepPixel& q = px[p];
            if (!q.in_image) continue;
            const size_t o = (size_t)(y0 + ty + p * ROWS_APART) * cols + u;
            if (q.best_k < 0 || q.best < P.min_score) { plane[o] = -1; score[o] = NAN; depth[o] = NAN; }
            else {
                double w = P.wmin + (double)q.best_k * P.step;
                if (q.has_l && q.has_r) {
                    const double den = (q.best_l - 2.0 * q.best) + q.best_r;
                    if (den < 0.0) w = w + ((0.5 * (q.best_l - q.best_r)) / den) * P.step;
                }
                plane[o] = q.best_k; score[o] = (float)q.best; depth[o] = (float)(1.0 / w);
            }
        }
    }
}

// sweep_kernel's sibling for sfmhip_sweep_costs: the same tiles, LDS areas, warp and window sums, statement by statement, with another
// ending -- per plane group a thread turns its SWEEP_KB plane scores into 16-bit costs and writes them, where the sweep keeps a running
// best.  (One body for both was tried: sweep_kernel<2> then took 127 or 156 registers for its 126, so the two stay apart.)
// A thread's SWEEP_KB costs lie 2 * D bytes from its neighbour's.  They are stored where they belong, as one 8-byte store when D is a
// multiple of SWEEP_KB and the volume is aligned to 8 bytes (cost_vec): the next plane groups fill the same lines while these are still
// in L2 (a tile's costs are 512 * D * 2 bytes), so the volume reaches memory once, and the kernel's time is in its LDS reads.
template <int R>
__global__ __launch_bounds__(SWEEP_THREADS) void sgm_cost_kernel(SweepParams P, int tiles_x, int n_tiles, double cost_scale, bool cost_vec, uint16_t* __restrict__ cost)
{
    constexpr int SIDE = 2 * R + 1, HW = SWEEP_TW + 2 * R, NH = HW * (SWEEP_TH + 2 * R), NWIN = SIDE * SIDE, ROWS_APART = SWEEP_TH / SWEEP_PX;
    __shared__ uint16_t ref16[SWEEP_HH * SWEEP_HW];
    __shared__ uint16_t smp[2][SWEEP_KB][SWEEP_HH * SWEEP_HW];
    const int tid = threadIdx.x, tx = tid & (SWEEP_TW - 1), ty = tid / SWEEP_TW;
    const int rows = P.rows, cols = P.cols;
    const float cm1 = (float)(cols - 1), rm1 = (float)(rows - 1);
    int buf = 0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int x0 = (tile % tiles_x) * SWEEP_TW, y0 = (tile / tiles_x) * SWEEP_TH;
        __syncthreads();                                                 // the previous tile's windows have been read
#pragma unroll
        for (int i = tid; i < NH; i += SWEEP_THREADS) {
            const int hy = i / HW, hx = i - hy * HW, u = x0 - R + hx, v = y0 - R + hy;
            const bool in = u >= 0 && u < cols && v >= 0 && v < rows;
            ref16[i] = in ? (uint16_t)(P.ref[(size_t)v * cols + u] * 16u) : (uint16_t)0;
        }
        __syncthreads();
        const int u = x0 + tx;
        double dvr[SWEEP_PX];
        uint32_t Sr_[SWEEP_PX];
        bool in_image[SWEEP_PX], valid[SWEEP_PX];
#pragma unroll
        for (int p = 0; p < SWEEP_PX; ++p) {
            const int v = y0 + ty + p * ROWS_APART;
            in_image[p] = u < cols && v < rows;
            valid[p] = in_image[p] && u - R >= 0 && u + R < cols && v - R >= 0 && v + R < rows;
            uint32_t Sr = 0, Srr = 0;
            if (valid[p]) {
#pragma nounroll
                for (int dy = 0; dy < SIDE; ++dy)
#pragma unroll
                    for (int dx = 0; dx < SIDE; ++dx) {
                        const uint32_t g = ref16[(ty + p * ROWS_APART + dy) * HW + tx + dx];
                        Sr += g; Srr += g * g;
                    }
            }
            const int64_t vr = (int64_t)NWIN * (int64_t)Srr - (int64_t)Sr * (int64_t)Sr;
            valid[p] = valid[p] && vr > 0;
            dvr[p] = (double)vr; Sr_[p] = Sr;
        }
        for (int k0 = 0; k0 < P.D; k0 += SWEEP_KB) {
            float wf[SWEEP_KB];
            double sum[SWEEP_PX][SWEEP_KB];
            int cnt[SWEEP_PX][SWEEP_KB];
#pragma unroll
            for (int j = 0; j < SWEEP_KB; ++j) {
                wf[j] = (float)(P.wmin + (double)(k0 + j) * P.step);
#pragma unroll
                for (int p = 0; p < SWEEP_PX; ++p) { sum[p][j] = 0.0; cnt[p][j] = 0; }
            }
            for (int s = 0; s < P.n_src; ++s) {
                const float* __restrict__ A = P.A[s];
                const uint8_t* __restrict__ g = P.src[s];
                uint16_t (*S)[SWEEP_HH * SWEEP_HW] = smp[buf];
#pragma unroll
                for (int i = tid; i < NH; i += SWEEP_THREADS) {
                    const int hy = i / HW, hx = i - hy * HW, uu = x0 - R + hx, vv = y0 - R + hy;
                    const bool in = uu >= 0 && uu < cols && vv >= 0 && vv < rows;
                    const float fu = (float)uu, fv = (float)vv;
                    const float a0 = A[0] * fu + A[1] * fv, a1 = A[3] * fu + A[4] * fv, a2 = A[6] * fu + A[7] * fv;
#pragma unroll
                    for (int j = 0; j < SWEEP_KB; ++j) {
                        uint32_t val = SWEEP_BAD;
                        if (in && k0 + j < P.D) {
                            const float q0 = a0 + (A[2] + wf[j] * P.b[s][0]);
                            const float q1 = a1 + (A[5] + wf[j] * P.b[s][1]);
                            const float q2 = a2 + (A[8] + wf[j] * P.b[s][2]);
                            const float sx = q0 / q2, sy = q1 / q2;
                            if (q2 > 0.0f && sx >= 0.0f && sy >= 0.0f && sx < cm1 && sy < rm1) {
                                const int ix = (int)sx, iy = (int)sy;
                                const uint32_t fx = (uint32_t)(int)((sx - (float)ix) * 32.0f), fy = (uint32_t)(int)((sy - (float)iy) * 32.0f);
                                const uint8_t* t = g + (size_t)iy * cols + ix;
                                const uint32_t g00 = t[0], g01 = t[1], g10 = t[cols], g11 = t[cols + 1];
                                val = (g00 * (32u - fx) * (32u - fy) + g01 * fx * (32u - fy) + g10 * (32u - fx) * fy + g11 * fx * fy + 32u) >> 6;
                            }
                        }
                        S[j][i] = (uint16_t)val;
                    }
                }
                __syncthreads();                                         // one barrier per (plane group, source): the other buffer is filled next
#pragma unroll
                for (int p = 0; p < SWEEP_PX; ++p) {
                    if (!valid[p]) continue;
                    uint32_t Sw[SWEEP_KB], Sww[SWEEP_KB], Srw[SWEEP_KB], any[SWEEP_KB];
#pragma unroll
                    for (int j = 0; j < SWEEP_KB; ++j) { Sw[j] = 0; Sww[j] = 0; Srw[j] = 0; any[j] = 0; }
#pragma nounroll
                    for (int dy = 0; dy < SIDE; ++dy)                    // a row of the window at a time: its loads fit the registers
#pragma unroll
                        for (int dx = 0; dx < SIDE; ++dx) {
                            const int at = (ty + p * ROWS_APART + dy) * HW + tx + dx;
                            const uint32_t gr = ref16[at];
#pragma unroll
                            for (int j = 0; j < SWEEP_KB; ++j) {
                                const uint32_t w = S[j][at];
                                any[j] |= w; Sw[j] += w; Sww[j] += w * w; Srw[j] += gr * w;
                            }
                        }
#pragma unroll
                    for (int j = 0; j < SWEEP_KB; ++j) {
                        if (any[j] & 0x8000u) continue;                  // a good sample is at most 4080; a plane past D - 1 is all bad
                        const int64_t vw = (int64_t)NWIN * (int64_t)Sww[j] - (int64_t)Sw[j] * (int64_t)Sw[j];
                        if (vw > 0) {
                            const int64_t cov = (int64_t)NWIN * (int64_t)Srw[j] - (int64_t)Sr_[p] * (int64_t)Sw[j];
                            sum[p][j] = sum[p][j] + (double)cov / sqrt(dvr[p] * (double)vw);
                            ++cnt[p][j];
                        }
                    }
                }
                buf ^= 1;
            }
#pragma unroll
            for (int p = 0; p < SWEEP_PX; ++p) {
                if (!in_image[p]) continue;
                uint32_t cv[SWEEP_KB];
#pragma unroll
                for (int j = 0; j < SWEEP_KB; ++j) {
                    const bool ok = cnt[p][j] >= P.min_sources;
                    const double c = ok ? sum[p][j] / (double)cnt[p][j] : 0.0;
                    const double t = (1.0 - c) * cost_scale;
                    const double qd = floor(t + 0.5);
                    cv[j] = !ok ? 65535u : qd < 0.0 ? 0u : qd > 65534.0 ? 65534u : (uint32_t)qd;
                }
                uint16_t* o = cost + ((size_t)(y0 + ty + p * ROWS_APART) * cols + u) * (size_t)P.D + k0;
                if (cost_vec) *(uint2*)o = make_uint2(cv[0] | cv[1] << 16, cv[2] | cv[3] << 16);
                else
#pragma unroll
                    for (int j = 0; j < SWEEP_KB; ++j)
                        if (k0 + j < P.D) o[j] = (uint16_t)cv[j];
            }
        }
    }
}

// ---- semi-global aggregation of the cost volume (sfmhip_sgm_depth): all of it unsigned 32-bit integers
#define SGM_PLANES_MAX 256
#define SGM_UNSEEN 65535u
#define SGM_NEVER 0x3FFFFFFFu                 // held for planes past D - 1: never a minimum, and + P1 does not wrap
#define SGM_WAVES 4                           // lines (path kernel) or pixels (winner kernel) per workgroup, one wave each
#define SGM_AHEAD 4                           // pixels of a line whose loads are in flight while the pixels before them are updated

__device__ __forceinline__ uint32_t sgm_wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// the line-th line of the direction (dy, dx): its first pixel (the one whose predecessor is outside) and its length.  Lines of a row or
// column direction are the rows or columns; a diagonal has one line per pixel of the row it enters by, then one per further pixel of
// the column it enters by.
__device__ __forceinline__ void sgm_line(const int line, const int rows, const int cols, const int dy, const int dx, int& y, int& x, int& n)
{
    const int ys = dy > 0 ? 0 : rows - 1, xs = dx > 0 ? 0 : cols - 1;
    if (dy == 0) { y = line; x = xs; }
    else if (dx == 0 || line < cols) { y = ys; x = line; }
    else { y = ys + dy * (line - cols + 1); x = xs; }
    const int ny = dy == 0 ? rows + cols : dy > 0 ? rows - y : y + 1, nx = dx == 0 ? rows + cols : dx > 0 ? cols - x : x + 1;
    n = min(ny, nx);
}

// One wave per line, its lanes on the planes: lane l holds the PPL = ceil(D / 64) planes l * PPL .. l * PPL + PPL - 1, so a plane's two
// neighbours are in the lane's own registers except at the ends of its run, where one value comes from the lane below and one from the
// lane above.  Per pixel: the wave minimum of the previous pixel's L, the two shifts, the update, and S (+)= L.  The loads of the next
// SGM_AHEAD pixels (costs, and S unless this is the first direction, which stores) are issued before the current SGM_AHEAD are updated:
// the recurrence waits for the cross-lane operations, not for memory.  Every (pixel, plane) of S is touched by exactly one lane of one
// wave per launch and the launches of a call follow each other on one stream, so S is a plain read-add-write and its value does not
// depend on the launch geometry.
template <int PPL>
__global__ __launch_bounds__(64 * SGM_WAVES) void sgm_path_kernel(const uint16_t* __restrict__ C, uint32_t* __restrict__ S, int rows, int cols, int D, int dy, int dx,
                                                                  uint32_t P1, uint32_t P2, int n_lines, int first)
{
    const int lane = threadIdx.x & 63, line = blockIdx.x * SGM_WAVES + (threadIdx.x >> 6), k0 = lane * PPL;
    if (line >= n_lines) return;
    int y, x, n;
    sgm_line(line, rows, cols, dy, dx, y, x, n);
    bool has[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) has[j] = k0 + j < D;
    const ptrdiff_t stride = ((ptrdiff_t)dy * cols + dx) * (ptrdiff_t)D;
    const uint16_t* c_at = C + ((size_t)y * cols + x) * (size_t)D + k0;
    uint32_t* s_at = S + ((size_t)y * cols + x) * (size_t)D + k0;
    uint32_t c[SGM_AHEAD][PPL], s[SGM_AHEAD][PPL], prev[PPL];
#pragma unroll
    for (int t = 0; t < SGM_AHEAD; ++t)
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const bool ld = t < n && has[j];
            c[t][j] = ld ? c_at[t * stride + j] : 0u;
            s[t][j] = ld && !first ? s_at[t * stride + j] : 0u;
        }
#pragma unroll
    for (int j = 0; j < PPL; ++j) prev[j] = SGM_NEVER;
    for (int i0 = 0; i0 < n; i0 += SGM_AHEAD) {
        uint32_t cn[SGM_AHEAD][PPL], sn[SGM_AHEAD][PPL];
#pragma unroll
        for (int t = 0; t < SGM_AHEAD; ++t)
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
                const bool ld = i0 + SGM_AHEAD + t < n && has[j];
                cn[t][j] = ld ? c_at[(SGM_AHEAD + t) * stride + j] : 0u;
                sn[t][j] = ld && !first ? s_at[(SGM_AHEAD + t) * stride + j] : 0u;
            }
#pragma unroll
        for (int t = 0; t < SGM_AHEAD; ++t) {
            if (i0 + t >= n) break;
            uint32_t cur[PPL];
            if (i0 + t == 0) {
#pragma unroll
                for (int j = 0; j < PPL; ++j) cur[j] = has[j] ? c[t][j] : SGM_NEVER;
            } else {
                uint32_t m = prev[0];
#pragma unroll
                for (int j = 1; j < PPL; ++j) m = min(m, prev[j]);
                m = sgm_wave_min(m);
                uint32_t below = (uint32_t)__shfl_up((int)prev[PPL - 1], 1), above = (uint32_t)__shfl_down((int)prev[0], 1);
                if (lane == 0) below = SGM_NEVER;
                if (lane == 63) above = SGM_NEVER;
                const uint32_t jump = m + P2;
#pragma unroll
                for (int j = 0; j < PPL; ++j) {
                    const uint32_t lo = j > 0 ? prev[j - 1] : below, hi = j < PPL - 1 ? prev[j + 1] : above;
                    const uint32_t best = min(min(prev[j], jump), min(lo, hi) + P1);
                    cur[j] = has[j] ? c[t][j] + (best - m) : SGM_NEVER;
                }
            }
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
                if (has[j]) s_at[t * stride + j] = s[t][j] + cur[j];
                prev[j] = cur[j];
            }
        }
#pragma unroll
        for (int t = 0; t < SGM_AHEAD; ++t)
#pragma unroll
            for (int j = 0; j < PPL; ++j) { c[t][j] = cn[t][j]; s[t][j] = sn[t][j]; }
        c_at += SGM_AHEAD * stride; s_at += SGM_AHEAD * stride;
    }
}

struct SgmWinnerParams {
    double wmin, step;
    int D, max_cost;
    int32_t* plane; uint16_t* cost; uint32_t* sum; float* depth;
};

// One wave per pixel, lanes on the planes: the key (S << 8 | k) of the seen planes (S < 2^20: eight directions of at most 2 * 65535) has
// its minimum at the smallest S and, among equals, the smallest k.  Lane 0 then fits and writes.
__global__ __launch_bounds__(64 * SGM_WAVES) void sgm_winner_kernel(const uint16_t* __restrict__ C, const uint32_t* __restrict__ S, size_t npx, SgmWinnerParams P)
{
    const int lane = threadIdx.x & 63;
    const size_t px = (size_t)blockIdx.x * SGM_WAVES + (threadIdx.x >> 6);
    if (px >= npx) return;
    const uint16_t* __restrict__ c = C + px * (size_t)P.D;
    const uint32_t* __restrict__ s = S + px * (size_t)P.D;
    uint32_t key = 0xFFFFFFFFu;
    for (int k = lane; k < P.D; k += 64)
        if (c[k] != SGM_UNSEEN) key = min(key, s[k] << 8 | (uint32_t)k);
    key = sgm_wave_min(key);
    if (lane != 0) return;
    const int k = key == 0xFFFFFFFFu ? 0 : (int)(key & 255u);
    const bool none = key == 0xFFFFFFFFu || (int)c[k] > P.max_cost;
    if (P.plane) P.plane[px] = none ? -1 : k;
    if (P.cost) P.cost[px] = none ? (uint16_t)SGM_UNSEEN : c[k];
    if (P.sum) P.sum[px] = none ? 0u : s[k];
    if (!P.depth) return;
    if (none) { P.depth[px] = NAN; return; }
    double w = P.wmin + (double)k * P.step;
    if (k > 0 && k < P.D - 1 && c[k - 1] != SGM_UNSEEN && c[k + 1] != SGM_UNSEEN) {
        const double sl = (double)s[k - 1], sk = (double)s[k], sr = (double)s[k + 1];
        const double den = (sl - 2.0 * sk) + sr;
        if (den > 0.0) w = w + ((0.5 * (sl - sr)) / den) * P.step;
    }
    P.depth[px] = (float)(1.0 / w);
}

__global__ __launch_bounds__(256) void consistency_kernel(const float* __restrict__ depth, ConsistencyParams P, uint8_t* __restrict__ count, uint8_t* __restrict__ keep)
{
    const size_t npx = (size_t)P.rows * P.cols;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const size_t v = i / (size_t)P.cols, u = i - v * (size_t)P.cols;
        const float df = depth[i];
        int n = 0;
        if (isfinite(df)) {
            const double d = (double)df;
            const double X0 = (((double)u - P.cx) / P.fx) * d, X1 = (((double)v - P.cy) / P.fy) * d;
            for (int s = 0; s < P.n_src; ++s) {
                const double* R = P.R[s];
                const double Y0 = ((R[0] * X0 + R[1] * X1) + R[2] * d) + P.t[s][0];
                const double Y1 = ((R[3] * X0 + R[4] * X1) + R[5] * d) + P.t[s][1];
                const double Y2 = ((R[6] * X0 + R[7] * X1) + R[8] * d) + P.t[s][2];
                if (!(Y2 > 0.0)) continue;
                const double pu = floor(((P.fx * Y0) / Y2 + P.cx) + 0.5), pv = floor(((P.fy * Y1) / Y2 + P.cy) + 0.5);
                if (!(pu >= 0.0 && pu < (double)P.cols && pv >= 0.0 && pv < (double)P.rows)) continue;
                const float dsf = P.src[s][(size_t)pv * (size_t)P.cols + (size_t)pu];
                if (!isfinite(dsf)) continue;
                if (fabs((double)dsf - Y2) <= P.rel_tol * Y2) ++n;
            }
        }
        if (count) count[i] = (uint8_t)n;
        if (keep) keep[i] = isfinite(df) && n >= P.min_consistent ? 1 : 0;
    }
}

// a pixel is exported when its keep byte is set (and, so that no row is ever non-finite by construction of the caller, nothing else)
__global__ __launch_bounds__(256) void points_count_kernel(const uint8_t* __restrict__ keep, size_t npx, unsigned nb, unsigned* __restrict__ counts)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int c = __syncthreads_count(i < npx && keep[i] != 0);
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = (unsigned)c;
        if (blockIdx.x == 0) counts[nb] = 0;                             // becomes the total under the exclusive scan
    }
}

__global__ __launch_bounds__(256) void points_write_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ keep, const uint8_t* __restrict__ img, int rows,
                                                           int cols, int channels, size_t ld, PointsParams P, const unsigned* __restrict__ offs, unsigned nb,
                                                           double* __restrict__ xyz, uint8_t* __restrict__ bgr, int cap, int32_t* __restrict__ n_found)
{
    __shared__ unsigned wave_n[4];
    const size_t npx = (size_t)rows * cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool k = i < npx && keep[i] != 0;
    const unsigned long long m = __ballot(k);
    if (lane == 0) wave_n[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_found = (int32_t)offs[nb];
    if (!k) return;
    size_t at = offs[blockIdx.x] + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) at += wave_n[w];
    if (at >= (size_t)cap) return;
    const size_t v = i / (size_t)cols, u = i - v * (size_t)cols;
    const double d = (double)depth[i];
    const double X0 = (((double)u - P.cx) / P.fx) * d, X1 = (((double)v - P.cy) / P.fy) * d;
    if (xyz) {
        xyz[3 * at + 0] = ((P.Rinv[0] * X0 + P.Rinv[1] * X1) + P.Rinv[2] * d) + P.c[0];
        xyz[3 * at + 1] = ((P.Rinv[3] * X0 + P.Rinv[4] * X1) + P.Rinv[5] * d) + P.c[1];
        xyz[3 * at + 2] = ((P.Rinv[6] * X0 + P.Rinv[7] * X1) + P.Rinv[8] * d) + P.c[2];
    }
    if (bgr) {
        const uint8_t* p = img + v * ld + u * (size_t)channels;
        bgr[3 * at + 0] = p[0]; bgr[3 * at + 1] = channels == 1 ? p[0] : p[1]; bgr[3 * at + 2] = channels == 1 ? p[0] : p[2];
    }
}

static inline bool dense_image_ok(int rows, int cols, int channels, size_t ld)
{
    return rows >= 1 && rows <= DENSE_DIM_MAX && cols >= 1 && cols <= DENSE_DIM_MAX && (channels == 1 || channels == 3) && ld >= (size_t)cols * (size_t)channels;
}
static inline bool dense_pos_finite(double x) { return std::isfinite(x) && x > 0.0; }
static inline bool dense_all(const void* const* p, int n)
{
    for (int i = 0; i < n; ++i)
        if (!p[i]) return false;
    return true;
}
static inline bool sweep_args_ok(const sfmhip_ctx* ctx, const void* ref, const void* const* src, int n_src, int rows, int cols, int channels, size_t ld, const float* A,
                                 const float* b, int D, double wmin, double wmax, int r, int min_sources, double min_score)
{
    return ctx && ref && src && n_src >= 1 && n_src <= DENSE_SRC_MAX && dense_all(src, n_src) && dense_image_ok(rows, cols, channels, ld) && A && b && D >= 2 &&
           D <= SWEEP_PLANES_MAX && dense_pos_finite(wmin) && dense_pos_finite(wmax) && wmin < wmax && r >= 0 && r <= SWEEP_RMAX && min_sources >= 1 &&
           !std::isnan(min_score);
}
static inline int dense_grid(const sfmhip_ctx* ctx, size_t work_groups, int per_cu)
{
    return (int)std::max<size_t>(1, std::min(work_groups, (size_t)ctx->num_cus * (size_t)per_cu));
}
// the bytes of an image whose last row ends at its last pixel
static inline size_t dense_image_bytes(int rows, int cols, int channels, size_t ld) { return (size_t)(rows - 1) * ld + (size_t)cols * (size_t)channels; }

// the gray planes of a call (from the block cache, held by the caller's hold) and the parameters of the sweep's kernels
static int sweep_prepare(sfmhip_ctx* ctx, SfmPoolHold& hold, const uint8_t* d_ref, const uint8_t* const* d_src, int n_src, int rows, int cols, int channels, size_t ld,
                         const float* A, const float* b, int D, double wmin, double wmax, int r, int min_sources, double min_score, SweepParams& P)
{
    const size_t npx = (size_t)rows * cols;
    uint8_t* d_gray = nullptr;
    const int rc = hold.get(&d_gray, npx * (size_t)(n_src + 1));
    if (rc != SFMHIP_OK) return rc;
    DenseImages I = {};
    I.img[0] = d_ref;
    for (int s = 0; s < n_src; ++s) I.img[s + 1] = d_src[s];
    hipLaunchKernelGGL(dense_gray_kernel, dim3(dense_grid(ctx, (npx + 255) / 256, 16), n_src + 1), dim3(256), 0, ctx->stream, I, rows, cols, channels, ld, d_gray);
    P = {};
    P.ref = d_gray;
    for (int s = 0; s < n_src; ++s) {
        P.src[s] = d_gray + npx * (size_t)(s + 1);
        std::memcpy(P.A[s], A + 9 * s, 9 * sizeof(float));
        std::memcpy(P.b[s], b + 3 * s, 3 * sizeof(float));
    }
    P.wmin = wmin; P.step = (wmax - wmin) / (double)(D - 1); P.min_score = min_score;
    P.n_src = n_src; P.rows = rows; P.cols = cols; P.D = D; P.r = r; P.min_sources = min_sources;
    return SFMHIP_OK;
}

// KERNEL<r> for the window radius r of the call
#define SWEEP_LAUNCH(KERNEL, r, grid, ...)                                                                                       \
    switch (r) {                                                                                                                 \
    case 0: hipLaunchKernelGGL(KERNEL<0>, grid, dim3(SWEEP_THREADS), 0, ctx->stream, __VA_ARGS__); break;                        \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(SWEEP_THREADS), 0, ctx->stream, __VA_ARGS__); break;                        \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(SWEEP_THREADS), 0, ctx->stream, __VA_ARGS__); break;                        \
    case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(SWEEP_THREADS), 0, ctx->stream, __VA_ARGS__); break;                        \
    case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(SWEEP_THREADS), 0, ctx->stream, __VA_ARGS__); break;                        \
    default: hipLaunchKernelGGL(KERNEL<5>, grid, dim3(SWEEP_THREADS), 0, ctx->stream, __VA_ARGS__); break;                       \
    }

// the gray planes, then the sweep, on the context's stream; the planes come from the block cache
static int sweep_enqueue(sfmhip_ctx* ctx, const uint8_t* d_ref, const uint8_t* const* d_src, int n_src, int rows, int cols, int channels, size_t ld, const float* A,
                         const float* b, int D, double wmin, double wmax, int r, int min_sources, double min_score, int32_t* d_plane, float* d_score, float* d_depth)
{
    SfmPoolHold hold(ctx);
    SweepParams P;
    const int rc = sweep_prepare(ctx, hold, d_ref, d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, min_score, P);
    if (rc != SFMHIP_OK) return rc;
    const int tiles_x = ceil_div(cols, SWEEP_TW), n_tiles = tiles_x * ceil_div(rows, SWEEP_TH);
    const dim3 grid(dense_grid(ctx, (size_t)n_tiles, 8));
    SWEEP_LAUNCH(sweep_kernel, r, grid, P, tiles_x, n_tiles, d_plane, d_score, d_depth)
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

// the gray planes, then the cost volume of the sweep (rows x cols x D uint16)
static int costs_enqueue(sfmhip_ctx* ctx, const uint8_t* d_ref, const uint8_t* const* d_src, int n_src, int rows, int cols, int channels, size_t ld, const float* A,
                         const float* b, int D, double wmin, double wmax, int r, int min_sources, double cost_scale, uint16_t* d_cost)
{
    SfmPoolHold hold(ctx);
    SweepParams P;
    const int rc = sweep_prepare(ctx, hold, d_ref, d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, 0.0, P);
    if (rc != SFMHIP_OK) return rc;
    const int tiles_x = ceil_div(cols, SWEEP_TW), n_tiles = tiles_x * ceil_div(rows, SWEEP_TH);
    const dim3 grid(dense_grid(ctx, (size_t)n_tiles, 8));
    const bool vec = D % SWEEP_KB == 0 && (uintptr_t)d_cost % 8 == 0;
    SWEEP_LAUNCH(sgm_cost_kernel, r, grid, P, tiles_x, n_tiles, cost_scale, vec, d_cost)
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

static inline bool sgm_args_ok(const sfmhip_ctx* ctx, int rows, int cols, int D, double wmin, double wmax, int P1, int P2, int paths, int max_cost)
{
    return ctx && rows >= 1 && rows <= DENSE_DIM_MAX && cols >= 1 && cols <= DENSE_DIM_MAX && D >= 2 && D <= SGM_PLANES_MAX && dense_pos_finite(wmin) &&
           dense_pos_finite(wmax) && wmin < wmax && P1 >= 0 && P1 <= P2 && P2 <= 65535 && (paths == 4 || paths == 8) && max_cost >= 0 && max_cost <= 65535;
}

// one launch per direction (the first stores S, the others add to it), then the winner; d_S: rows x cols x D uint32, the caller's
static int sgm_enqueue(sfmhip_ctx* ctx, const uint16_t* d_cost, int rows, int cols, int D, double wmin, double wmax, int P1, int P2, int paths, int max_cost,
                       int32_t* d_plane, uint16_t* d_wcost, uint32_t* d_sum, float* d_depth, uint32_t* d_S)
{
    static const int DIR[8][2] = { { 0, 1 }, { 0, -1 }, { 1, 0 }, { -1, 0 }, { 1, 1 }, { -1, -1 }, { 1, -1 }, { -1, 1 } };
    const int ppl = ceil_div(D, 64);
    for (int d = 0; d < paths; ++d) {
        const int dy = DIR[d][0], dx = DIR[d][1], n_lines = dy == 0 ? rows : dx == 0 ? cols : rows + cols - 1;
        const dim3 grid(ceil_div(n_lines, SGM_WAVES)), block(64 * SGM_WAVES);
        switch (ppl) {
        case 1: hipLaunchKernelGGL(sgm_path_kernel<1>, grid, block, 0, ctx->stream, d_cost, d_S, rows, cols, D, dy, dx, (uint32_t)P1, (uint32_t)P2, n_lines, d == 0); break;
        case 2: hipLaunchKernelGGL(sgm_path_kernel<2>, grid, block, 0, ctx->stream, d_cost, d_S, rows, cols, D, dy, dx, (uint32_t)P1, (uint32_t)P2, n_lines, d == 0); break;
        case 3: hipLaunchKernelGGL(sgm_path_kernel<3>, grid, block, 0, ctx->stream, d_cost, d_S, rows, cols, D, dy, dx, (uint32_t)P1, (uint32_t)P2, n_lines, d == 0); break;
        default: hipLaunchKernelGGL(sgm_path_kernel<4>, grid, block, 0, ctx->stream, d_cost, d_S, rows, cols, D, dy, dx, (uint32_t)P1, (uint32_t)P2, n_lines, d == 0); break;
        }
    }
    if (d_plane || d_wcost || d_sum || d_depth) {
        const size_t npx = (size_t)rows * cols;
        SgmWinnerParams W;
        W.wmin = wmin; W.step = (wmax - wmin) / (double)(D - 1); W.D = D; W.max_cost = max_cost;
        W.plane = d_plane; W.cost = d_wcost; W.sum = d_sum; W.depth = d_depth;
        hipLaunchKernelGGL(sgm_winner_kernel, dim3((unsigned)((npx + SGM_WAVES - 1) / SGM_WAVES)), dim3(64 * SGM_WAVES), 0, ctx->stream, d_cost, (const uint32_t*)d_S, npx, W);
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

// the reference image and its sources into one block of the hold; d_src[s]: where source s lies
static int dense_upload_images(sfmhip_ctx* ctx, SfmPoolHold& hold, const uint8_t* ref, const uint8_t* const* src, int n_src, size_t bytes, uint8_t*& d_img,
                               const uint8_t* (&d_src)[DENSE_SRC_MAX])
{
    const size_t img_stride = align256(bytes);
    int rc = hold.get(&d_img, img_stride * (size_t)(n_src + 1));
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d_img, ref, bytes);
    for (int s = 0; s < n_src && rc == SFMHIP_OK; ++s) {
        d_src[s] = d_img + img_stride * (size_t)(s + 1);
        rc = sfm_upload(ctx, d_img + img_stride * (size_t)(s + 1), src[s], bytes);
    }
    return rc;
}

static inline bool consistency_args_ok(const sfmhip_ctx* ctx, const void* depth, const void* const* src, int n_src, int rows, int cols, const double* K4, const double* Rrel,
                                       const double* trel, double rel_tol, int min_consistent)
{
    return ctx && depth && src && n_src >= 1 && n_src <= DENSE_SRC_MAX && dense_all(src, n_src) && rows >= 1 && rows <= DENSE_DIM_MAX && cols >= 1 &&
           cols <= DENSE_DIM_MAX && K4 && Rrel && trel && std::isfinite(rel_tol) && rel_tol >= 0.0 && min_consistent >= 0;
}
static int consistency_enqueue(sfmhip_ctx* ctx, const float* d_depth, const float* const* d_src, int n_src, int rows, int cols, const double* K4, const double* Rrel,
                               const double* trel, double rel_tol, int min_consistent, uint8_t* d_count, uint8_t* d_keep)
{
    ConsistencyParams P = {};
    for (int s = 0; s < n_src; ++s) {
        P.src[s] = d_src[s];
        std::memcpy(P.R[s], Rrel + 9 * s, 9 * sizeof(double));
        std::memcpy(P.t[s], trel + 3 * s, 3 * sizeof(double));
    }
    P.fx = K4[0]; P.fy = K4[1]; P.cx = K4[2]; P.cy = K4[3]; P.rel_tol = rel_tol;
    P.n_src = n_src; P.rows = rows; P.cols = cols; P.min_consistent = min_consistent;
    hipLaunchKernelGGL(consistency_kernel, dim3(dense_grid(ctx, ((size_t)rows * cols + 255) / 256, 16)), dim3(256), 0, ctx->stream, d_depth, P, d_count, d_keep);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

static inline bool points_args_ok(const sfmhip_ctx* ctx, const void* depth, const void* keep, const void* img, int rows, int cols, int channels, size_t ld, const double* K4,
                                  const double* Rinv, const double* c, const void* xyz, const void* bgr, int cap, const void* n_found)
{
    return ctx && depth && keep && dense_image_ok(rows, cols, channels, ld) && K4 && Rinv && c && cap >= 0 && n_found && (img || !bgr) && (cap == 0 || xyz || bgr);
}
static int points_enqueue(sfmhip_ctx* ctx, const float* d_depth, const uint8_t* d_keep, const uint8_t* d_img, int rows, int cols, int channels, size_t ld, const double* K4,
                          const double* Rinv, const double* c, double* d_xyz, uint8_t* d_bgr, int cap, int32_t* d_n_found)
{
    const size_t npx = (size_t)rows * cols, nb = (npx + 255) / 256;
    SfmCarve carve;
    SfmScan C(carve, nb + 1);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    C.bind(w);
    unsigned* counts = C.data;
    PointsParams P;
    P.fx = K4[0]; P.fy = K4[1]; P.cx = K4[2]; P.cy = K4[3];
    std::memcpy(P.Rinv, Rinv, sizeof(P.Rinv));
    std::memcpy(P.c, c, sizeof(P.c));
    hipLaunchKernelGGL(points_count_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_keep, npx, (unsigned)nb, counts);
    C.scan(ctx->stream, nb + 1);
    hipLaunchKernelGGL(points_write_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_depth, d_keep, d_img, rows, cols, channels, ld, P, (const unsigned*)counts,
                       (unsigned)nb, d_xyz, d_bgr, cap, d_n_found);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

// R of the BA parameterisation (angle-axis, world to camera): Rodrigues, the first-order form below an angle of 1e-15
static void dense_rotation(const double* w, double (&R)[9])
{
    const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    if (t2 > 1e-30) {
        const double th = std::sqrt(t2), x = w[0] / th, y = w[1] / th, z = w[2] / th, c = std::cos(th), s = std::sin(th), k = 1.0 - c;
        R[0] = c + k * x * x;     R[1] = k * x * y - s * z; R[2] = k * x * z + s * y;
        R[3] = k * x * y + s * z; R[4] = c + k * y * y;     R[5] = k * y * z - s * x;
        R[6] = k * x * z - s * y; R[7] = k * y * z + s * x; R[8] = c + k * z * z;
    } else {
        R[0] = 1.0; R[1] = -w[2]; R[2] = w[1]; R[3] = w[2]; R[4] = 1.0; R[5] = -w[0]; R[6] = -w[1]; R[7] = w[0]; R[8] = 1.0;
    }
}

extern "C" {

int sfmhip_sweep_geometry(const double K4[4], const double ext6_ref[6], const double* ext6_src, int n_src, float* A, float* b, double* Rrel, double* trel, double Rinv[9],
                          double c[3])
{
    if (!K4 || !ext6_ref || n_src < 0 || n_src > DENSE_SRC_MAX || (n_src > 0 && !ext6_src)) return SFMHIP_E_ARG;
    const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    if (!(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)) || fx == 0.0 || fy == 0.0) return SFMHIP_E_ARG;
    double Rr[9];
    dense_rotation(ext6_ref, Rr);
    const double* tr = ext6_ref + 3;
    for (int i = 0; i < 3; ++i) {
        if (Rinv)
            for (int j = 0; j < 3; ++j) Rinv[3 * i + j] = Rr[3 * j + i];
        if (c) c[i] = -((Rr[i] * tr[0] + Rr[3 + i] * tr[1]) + Rr[6 + i] * tr[2]);
    }
    for (int s = 0; s < n_src; ++s) {
        double Rs[9], M[9], t[3];
        dense_rotation(ext6_src + 6 * s, Rs);
        const double* ts = ext6_src + 6 * s + 3;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) M[3 * i + j] = (Rs[3 * i] * Rr[3 * j] + Rs[3 * i + 1] * Rr[3 * j + 1]) + Rs[3 * i + 2] * Rr[3 * j + 2];
        for (int i = 0; i < 3; ++i) t[i] = ts[i] - ((M[3 * i] * tr[0] + M[3 * i + 1] * tr[1]) + M[3 * i + 2] * tr[2]);
        if (Rrel) std::memcpy(Rrel + 9 * s, M, sizeof(M));
        if (trel) std::memcpy(trel + 3 * s, t, sizeof(t));
        // K M K^-1 and K t, K = [fx 0 cx; 0 fy cy; 0 0 1]
        double KM[9];
        for (int j = 0; j < 3; ++j) { KM[j] = fx * M[j] + cx * M[6 + j]; KM[3 + j] = fy * M[3 + j] + cy * M[6 + j]; KM[6 + j] = M[6 + j]; }
        if (A)
            for (int i = 0; i < 3; ++i) {
                const double m0 = KM[3 * i] / fx, m1 = KM[3 * i + 1] / fy;
                A[9 * s + 3 * i] = (float)m0; A[9 * s + 3 * i + 1] = (float)m1; A[9 * s + 3 * i + 2] = (float)((KM[3 * i + 2] - m0 * cx) - m1 * cy);
            }
        if (b) { b[3 * s] = (float)(fx * t[0] + cx * t[2]); b[3 * s + 1] = (float)(fy * t[1] + cy * t[2]); b[3 * s + 2] = (float)t[2]; }
    }
    return SFMHIP_OK;
}

int sfmhip_plane_sweep_dev(sfmhip_ctx* ctx, const uint8_t* d_ref, const uint8_t* const* d_src, int n_src, int rows, int cols, int channels, size_t ld, const float* A,
                           const float* b, int D, double wmin, double wmax, int r, int min_sources, double min_score, int32_t* d_plane, float* d_score, float* d_depth)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_plane_sweep_dev");
    SFM_ARG_CHECK(ctx, sweep_args_ok(ctx, d_ref, (const void* const*)d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, min_score));
    SFM_ARG_CHECK(ctx, d_plane && d_score && d_depth);
    return sweep_enqueue(ctx, d_ref, d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, min_score, d_plane, d_score, d_depth);
}

int sfmhip_plane_sweep(sfmhip_ctx* ctx, const uint8_t* ref, const uint8_t* const* src, int n_src, int rows, int cols, int channels, size_t ld, const float* A, const float* b,
                       int D, double wmin, double wmax, int r, int min_sources, double min_score, int32_t* plane, float* score, float* depth)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_plane_sweep");
    SFM_ARG_CHECK(ctx, sweep_args_ok(ctx, ref, (const void* const*)src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, min_score));
    SFM_ARG_CHECK(ctx, plane && score && depth);
    const size_t npx = (size_t)rows * cols, bytes = dense_image_bytes(rows, cols, channels, ld);
    SfmPoolHold hold(ctx);
    uint8_t* d_img = nullptr; char* d_out = nullptr;
    SfmCarve carve;
    const size_t o_plane = carve(npx * 4), o_score = carve(npx * 4), o_depth = carve(npx * 4);
    const uint8_t* d_src[DENSE_SRC_MAX] = {};
    int rc = dense_upload_images(ctx, hold, ref, src, n_src, bytes, d_img, d_src);
    if (rc == SFMHIP_OK) rc = hold.get(carve.bytes, (void**)&d_out);
    if (rc == SFMHIP_OK)
        rc = sweep_enqueue(ctx, d_img, d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, min_score, (int32_t*)(d_out + o_plane),
                           (float*)(d_out + o_score), (float*)(d_out + o_depth));
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipError_t e = hipMemcpyAsync(plane, d_out + o_plane, npx * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(score, d_out + o_score, npx * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(depth, d_out + o_depth, npx * 4, hipMemcpyDeviceToHost, ctx->stream);
    return sfm_finish(ctx, e);
}

int sfmhip_sweep_costs_dev(sfmhip_ctx* ctx, const uint8_t* d_ref, const uint8_t* const* d_src, int n_src, int rows, int cols, int channels, size_t ld, const float* A,
                           const float* b, int D, double wmin, double wmax, int r, int min_sources, double cost_scale, uint16_t* d_cost)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_sweep_costs_dev");
    SFM_ARG_CHECK(ctx, sweep_args_ok(ctx, d_ref, (const void* const*)d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, 0.0));
    SFM_ARG_CHECK(ctx, D <= SGM_PLANES_MAX && dense_pos_finite(cost_scale) && d_cost);
    return costs_enqueue(ctx, d_ref, d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, cost_scale, d_cost);
}

int sfmhip_sweep_costs(sfmhip_ctx* ctx, const uint8_t* ref, const uint8_t* const* src, int n_src, int rows, int cols, int channels, size_t ld, const float* A, const float* b,
                       int D, double wmin, double wmax, int r, int min_sources, double cost_scale, uint16_t* cost)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_sweep_costs");
    SFM_ARG_CHECK(ctx, sweep_args_ok(ctx, ref, (const void* const*)src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, 0.0));
    SFM_ARG_CHECK(ctx, D <= SGM_PLANES_MAX && dense_pos_finite(cost_scale) && cost);
    const size_t nvol = (size_t)rows * cols * (size_t)D, bytes = dense_image_bytes(rows, cols, channels, ld);
    SfmPoolHold hold(ctx);
    uint8_t* d_img = nullptr; uint16_t* d_cost = nullptr;
    const uint8_t* d_src[DENSE_SRC_MAX] = {};
    int rc = dense_upload_images(ctx, hold, ref, src, n_src, bytes, d_img, d_src);
    if (rc == SFMHIP_OK) rc = hold.get(&d_cost, nvol);
    if (rc == SFMHIP_OK) rc = costs_enqueue(ctx, d_img, d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, cost_scale, d_cost);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    return sfm_finish(ctx, hipMemcpyAsync(cost, d_cost, nvol * 2, hipMemcpyDeviceToHost, ctx->stream));
}

int sfmhip_sgm_depth_dev(sfmhip_ctx* ctx, const uint16_t* d_cost, int rows, int cols, int D, double wmin, double wmax, int P1, int P2, int paths, int max_cost,
                         int32_t* d_plane, uint16_t* d_win_cost, uint32_t* d_sum, float* d_depth, uint32_t* d_S)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_sgm_depth_dev");
    SFM_ARG_CHECK(ctx, d_cost && sgm_args_ok(ctx, rows, cols, D, wmin, wmax, P1, P2, paths, max_cost));
    SFM_ARG_CHECK(ctx, d_plane || d_win_cost || d_sum || d_depth);
    SfmPoolHold hold(ctx);
    if (!d_S) {
        const int rc = hold.get(&d_S, (size_t)rows * cols * (size_t)D);
        if (rc != SFMHIP_OK) return rc;
    }
    return sgm_enqueue(ctx, d_cost, rows, cols, D, wmin, wmax, P1, P2, paths, max_cost, d_plane, d_win_cost, d_sum, d_depth, d_S);
}

int sfmhip_sgm_depth(sfmhip_ctx* ctx, const uint16_t* cost, int rows, int cols, int D, double wmin, double wmax, int P1, int P2, int paths, int max_cost, int32_t* plane,
                     uint16_t* win_cost, uint32_t* sum, float* depth, uint32_t* S)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_sgm_depth");
    SFM_ARG_CHECK(ctx, cost && sgm_args_ok(ctx, rows, cols, D, wmin, wmax, P1, P2, paths, max_cost));
    SFM_ARG_CHECK(ctx, plane || win_cost || sum || depth);
    const size_t npx = (size_t)rows * cols, nvol = npx * (size_t)D;
    SfmPoolHold hold(ctx);
    uint16_t* d_cost = nullptr; uint32_t* d_S = nullptr; char* d_out = nullptr;
    SfmCarve carve;
    const size_t o_plane = carve(npx * 4), o_sum = carve(npx * 4), o_depth = carve(npx * 4), o_cost = carve(npx * 2);
    int rc = hold.get(&d_cost, nvol);
    if (rc == SFMHIP_OK) rc = hold.get(&d_S, nvol);
    if (rc == SFMHIP_OK) rc = hold.get(carve.bytes, (void**)&d_out);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d_cost, cost, nvol * 2);
    if (rc == SFMHIP_OK)
        rc = sgm_enqueue(ctx, d_cost, rows, cols, D, wmin, wmax, P1, P2, paths, max_cost, plane ? (int32_t*)(d_out + o_plane) : nullptr,
                         win_cost ? (uint16_t*)(d_out + o_cost) : nullptr, sum ? (uint32_t*)(d_out + o_sum) : nullptr, depth ? (float*)(d_out + o_depth) : nullptr, d_S);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipError_t e = hipSuccess;
    if (plane) e = hipMemcpyAsync(plane, d_out + o_plane, npx * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && win_cost) e = hipMemcpyAsync(win_cost, d_out + o_cost, npx * 2, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && sum) e = hipMemcpyAsync(sum, d_out + o_sum, npx * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && depth) e = hipMemcpyAsync(depth, d_out + o_depth, npx * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && S) e = hipMemcpyAsync(S, d_S, nvol * 4, hipMemcpyDeviceToHost, ctx->stream);
    return sfm_finish(ctx, e);
}

// the two volumes are taken before anything is enqueued: a failed allocation leaves the outputs alone
int sfmhip_plane_sweep_sgm_dev(sfmhip_ctx* ctx, const uint8_t* d_ref, const uint8_t* const* d_src, int n_src, int rows, int cols, int channels, size_t ld, const float* A,
                               const float* b, int D, double wmin, double wmax, int r, int min_sources, double cost_scale, int P1, int P2, int paths, int max_cost,
                               int32_t* d_plane, uint16_t* d_win_cost, float* d_depth)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_plane_sweep_sgm_dev");
    SFM_ARG_CHECK(ctx, sweep_args_ok(ctx, d_ref, (const void* const*)d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, 0.0));
    SFM_ARG_CHECK(ctx, dense_pos_finite(cost_scale) && sgm_args_ok(ctx, rows, cols, D, wmin, wmax, P1, P2, paths, max_cost));
    SFM_ARG_CHECK(ctx, d_plane && d_win_cost && d_depth);
    const size_t nvol = (size_t)rows * cols * (size_t)D;
    SfmPoolHold hold(ctx);
    uint16_t* d_cost = nullptr; uint32_t* d_S = nullptr;
    int rc = hold.get(&d_cost, nvol);
    if (rc == SFMHIP_OK) rc = hold.get(&d_S, nvol);
    if (rc == SFMHIP_OK) rc = costs_enqueue(ctx, d_ref, d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, cost_scale, d_cost);
    if (rc == SFMHIP_OK) rc = sgm_enqueue(ctx, d_cost, rows, cols, D, wmin, wmax, P1, P2, paths, max_cost, d_plane, d_win_cost, nullptr, d_depth, d_S);
    return rc;
}

int sfmhip_plane_sweep_sgm(sfmhip_ctx* ctx, const uint8_t* ref, const uint8_t* const* src, int n_src, int rows, int cols, int channels, size_t ld, const float* A,
                           const float* b, int D, double wmin, double wmax, int r, int min_sources, double cost_scale, int P1, int P2, int paths, int max_cost,
                           int32_t* plane, uint16_t* win_cost, float* depth)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_plane_sweep_sgm");
    SFM_ARG_CHECK(ctx, sweep_args_ok(ctx, ref, (const void* const*)src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, 0.0));
    SFM_ARG_CHECK(ctx, dense_pos_finite(cost_scale) && sgm_args_ok(ctx, rows, cols, D, wmin, wmax, P1, P2, paths, max_cost));
    SFM_ARG_CHECK(ctx, plane && win_cost && depth);
    const size_t npx = (size_t)rows * cols, nvol = npx * (size_t)D, bytes = dense_image_bytes(rows, cols, channels, ld);
    SfmPoolHold hold(ctx);
    uint8_t* d_img = nullptr; uint16_t* d_cost = nullptr; uint32_t* d_S = nullptr; char* d_out = nullptr;
    const uint8_t* d_src[DENSE_SRC_MAX] = {};
    SfmCarve carve;
    const size_t o_plane = carve(npx * 4), o_depth = carve(npx * 4), o_cost = carve(npx * 2);
    int rc = dense_upload_images(ctx, hold, ref, src, n_src, bytes, d_img, d_src);
    if (rc == SFMHIP_OK) rc = hold.get(&d_cost, nvol);
    if (rc == SFMHIP_OK) rc = hold.get(&d_S, nvol);
    if (rc == SFMHIP_OK) rc = hold.get(carve.bytes, (void**)&d_out);
    if (rc == SFMHIP_OK) rc = costs_enqueue(ctx, d_img, d_src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, cost_scale, d_cost);
    if (rc == SFMHIP_OK)
        rc = sgm_enqueue(ctx, d_cost, rows, cols, D, wmin, wmax, P1, P2, paths, max_cost, (int32_t*)(d_out + o_plane), (uint16_t*)(d_out + o_cost), nullptr,
                         (float*)(d_out + o_depth), d_S);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipError_t e = hipMemcpyAsync(plane, d_out + o_plane, npx * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(win_cost, d_out + o_cost, npx * 2, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(depth, d_out + o_depth, npx * 4, hipMemcpyDeviceToHost, ctx->stream);
    return sfm_finish(ctx, e);
}

int sfmhip_depth_consistency_dev(sfmhip_ctx* ctx, const float* d_depth, const float* const* d_depth_src, int n_src, int rows, int cols, const double K4[4],
                                 const double* Rrel, const double* trel, double rel_tol, int min_consistent, uint8_t* d_count, uint8_t* d_keep)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_depth_consistency_dev");
    SFM_ARG_CHECK(ctx, consistency_args_ok(ctx, d_depth, (const void* const*)d_depth_src, n_src, rows, cols, K4, Rrel, trel, rel_tol, min_consistent));
    SFM_ARG_CHECK(ctx, d_count || d_keep);
    return consistency_enqueue(ctx, d_depth, d_depth_src, n_src, rows, cols, K4, Rrel, trel, rel_tol, min_consistent, d_count, d_keep);
}

int sfmhip_depth_consistency(sfmhip_ctx* ctx, const float* depth, const float* const* depth_src, int n_src, int rows, int cols, const double K4[4], const double* Rrel,
                             const double* trel, double rel_tol, int min_consistent, uint8_t* count, uint8_t* keep)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_depth_consistency");
    SFM_ARG_CHECK(ctx, consistency_args_ok(ctx, depth, (const void* const*)depth_src, n_src, rows, cols, K4, Rrel, trel, rel_tol, min_consistent));
    SFM_ARG_CHECK(ctx, count || keep);
    const size_t npx = (size_t)rows * cols;
    SfmPoolHold hold(ctx);
    float* d_maps = nullptr; uint8_t* d_out = nullptr;
    int rc = hold.get(&d_maps, npx * (size_t)(n_src + 1));
    if (rc == SFMHIP_OK) rc = hold.get(&d_out, 2 * npx);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d_maps, depth, npx * 4);
    const float* d_src[DENSE_SRC_MAX] = {};
    for (int s = 0; s < n_src && rc == SFMHIP_OK; ++s) {
        d_src[s] = d_maps + npx * (size_t)(s + 1);
        rc = sfm_upload(ctx, d_maps + npx * (size_t)(s + 1), depth_src[s], npx * 4);
    }
    if (rc == SFMHIP_OK) rc = consistency_enqueue(ctx, d_maps, d_src, n_src, rows, cols, K4, Rrel, trel, rel_tol, min_consistent, d_out, d_out + npx);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipError_t e = hipSuccess;
    if (count) e = hipMemcpyAsync(count, d_out, npx, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && keep) e = hipMemcpyAsync(keep, d_out + npx, npx, hipMemcpyDeviceToHost, ctx->stream);
    return sfm_finish(ctx, e);
}

int sfmhip_depth_to_points_dev(sfmhip_ctx* ctx, const float* d_depth, const uint8_t* d_keep, const uint8_t* d_img, int rows, int cols, int channels, size_t ld,
                               const double K4[4], const double Rinv[9], const double c[3], double* d_xyz, uint8_t* d_bgr, int cap, int32_t* d_n_found)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_depth_to_points_dev");
    SFM_ARG_CHECK(ctx, points_args_ok(ctx, d_depth, d_keep, d_img, rows, cols, channels, ld, K4, Rinv, c, d_xyz, d_bgr, cap, d_n_found));
    return points_enqueue(ctx, d_depth, d_keep, d_img, rows, cols, channels, ld, K4, Rinv, c, d_xyz, d_bgr, cap, d_n_found);
}

int sfmhip_depth_to_points(sfmhip_ctx* ctx, const float* depth, const uint8_t* keep, const uint8_t* img, int rows, int cols, int channels, size_t ld, const double K4[4],
                           const double Rinv[9], const double c[3], double* xyz, uint8_t* bgr, int cap, int32_t* n_found)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_depth_to_points");
    SFM_ARG_CHECK(ctx, points_args_ok(ctx, depth, keep, img, rows, cols, channels, ld, K4, Rinv, c, xyz, bgr, cap, n_found));
    const size_t npx = (size_t)rows * cols, bytes = dense_image_bytes(rows, cols, channels, ld), C = (size_t)cap;
    SfmPoolHold hold(ctx);
    char* d = nullptr;
    SfmCarve carve;
    const size_t o_depth = carve(npx * 4), o_keep = carve(npx), o_img = carve(img ? bytes : 0), o_xyz = carve(C * 3 * sizeof(double)), o_bgr = carve(C * 3), o_n = carve(4);
    int rc = hold.get(carve.bytes, (void**)&d);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d + o_depth, depth, npx * 4);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d + o_keep, keep, npx);
    if (rc == SFMHIP_OK && img) rc = sfm_upload(ctx, d + o_img, img, bytes);
    if (rc == SFMHIP_OK)
        rc = points_enqueue(ctx, (const float*)(d + o_depth), (const uint8_t*)(d + o_keep), img ? (const uint8_t*)(d + o_img) : nullptr, rows, cols, channels, ld, K4, Rinv,
                            c, xyz ? (double*)(d + o_xyz) : nullptr, bgr ? (uint8_t*)(d + o_bgr) : nullptr, cap, (int32_t*)(d + o_n));
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    int32_t n = 0;
    hipError_t e = hipMemcpyAsync(&n, d + o_n, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    const size_t m = std::min((size_t)std::max(n, 0), C);
    if (e == hipSuccess && xyz && m) e = hipMemcpyAsync(xyz, d + o_xyz, m * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && bgr && m) e = hipMemcpyAsync(bgr, d + o_bgr, m * 3, hipMemcpyDeviceToHost, ctx->stream);
    const int rc2 = sfm_finish(ctx, e);
    if (rc2 == SFMHIP_OK) *n_found = n;
    return rc2;
}

}
