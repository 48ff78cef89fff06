// akaze.hip -- AKAZE feature extraction on the device: the FED nonlinear scale space, the determinant-of-Hessian detector with its
// suppression against the neighbouring sublevels, the sub-pixel fit, the dominant orientation and the 486-bit M-LDB rows of
// sfm_opencv_amd/host/sfm_akaze.hpp (akaze_detect_and_compute with Params at its defaults), restated as kernels.
//
// What is exact and what is not.  Everything up to the refined key points is plain IEEE float arithmetic evaluated here in the host's
// order with contraction off (float division and sqrtf are correctly rounded): every level array, kcontrast, the raw maxima, the
// suppression's survivors and their order, the refined x, y, size, response and the row order have the host's bits.  The orientation goes
// through atan2f, the descriptor through cosf / sinf of the device maths library: angle and descriptor bits agree with the host within a
// tolerance only (tests/test_akaze_gpu.py states it).  The sums of both are taken in the host's order by one lane each.
//
// One image, everything on ctx->stream, no host round trip on the enqueue path:
//   akaze_gray_kernel                    bytes -> float gray * (1 / 255)
//   akaze_blur_rows_kernel<R> / _cols_   blur() through LDS tiles, clamped border, taps from -R to R from 0.0f; R = 7 (sigma 1.6) and 4 (sigma 1)
//   akaze_hmax_kernel, akaze_hist_kernel, akaze_kcontrast_kernel      k_percentile: gradient magnitudes of the sigma-1 blur, their maximum
//                                        (integer atomics on the bit pattern), the 300-bin histogram (integer atomics), the scan and the two
//                                        0.03f fallbacks by one thread; kcontrast of every level stays on the device
//   akaze_half_kernel                    halfsample
//   akaze_flow_kernel                    scharr of Lsmooth and the Perona-Malik g2 conductivity
//   akaze_fed_kernel                     nld_step, a Jacobi step: one launch per step (166 for 16 levels), ping-pong between two arrays
//   akaze_deriv1_kernel, akaze_det_kernel    Lx, Ly and Ldet (the three second derivatives are evaluated in place, never stored)
//   akaze_maxima_kernel                  v > 0.001f and the eight strict comparisons inside the border; appended through a counter, then
//                                        ordered by (level, y, x) with one stable radix sort: the host's scan order
//   akaze_suppress_round_kernel, _publish_, akaze_suppress_kernel     the first pass of find_extrema in rounds (below): 32 rounds over all
//                                        workgroups, two launches each, then a one-workgroup loop for what is left
//   akaze_suppress2_kernel               its second pass, a thread per candidate; survivors ordered by slot = the host's `out`
//   akaze_subpixel_kernel                subpixel(); flag + scan + compact keeps the order; one stable sort on descending response
//   akaze_describe_kernel                a wave per row: main_orientation (samples by the lanes, each of the 42 windows summed in ascending k
//                                        by one lane) and mldb (each of the 29 cells summed in the host's k, l order by one lane, the 61 bytes
//                                        by 61 lanes); writes the sfm_keypoint beside the row
//
// The suppression.  find_extrema walks the raw maxima in scan order against a growing list aux; the first entry of aux whose level is the
// candidate's or one below and that lies within the candidate's size is the only one consulted (replaced if weaker, else the candidate is
// dropped).  Restated: every candidate has a slot -- its own index if appended, the slot of the entry it replaces otherwise -- and aux order is
// ascending slot; candidate c consults the alive entry of smallest slot among the earlier candidates of levels {l, l-1} within size_c.  c
// therefore depends only on earlier candidates of those levels within 2 size_c of it (a replacing f has size_f <= size_c and lies within
// size_f of something within size_c of c; one pixel more covers the float rounding).  A round resolves every candidate whose such
// predecessors were resolved in earlier rounds, reading only what those published.  The first 32 rounds are a pair of launches each
// (decide, publish) over all workgroups, with a device-side "nothing left" exit; what they leave (nothing on images: the 64201
// maxima of a 10 MP texture need 19 rounds) is finished by a loop with barriers inside ONE workgroup.  No workgroup ever waits on another.  A round resolves at least the
// earliest unresolved candidate, so n rounds are the bound of that loop.  Lists
// from images are sorted by y within a level, which bounds the neighbour scan to a window of rows; a caller's list (sfmhip_akaze_suppress)
// is scanned whole.
//
// Footprint.  Kept per level: Lt, Lx, Ly, Ldet (16 bytes per level pixel; 16 levels are 5.3 full-resolution sets of the four, 85 bytes per
// input pixel).  Transient: six full-resolution float arrays (24 bytes per pixel).  Lists: K = max(cap, 4096, pixels / 8) raw maxima at
// about 150 bytes each (two AkCand, an AkFit, three ints of suppression state, two key / value pairs of the sort, flag, list), 18 bytes
// per pixel where pixels / 8 decides.  Strict 3 x 3 maxima are never adjacent, so a level cannot hold more than a quarter of the pixels
// inside its border; the determinant of a Hessian taken from blurred levels comes nowhere near that (textures give one per hundred
// pixels, 64201 on 10 MP), and the flag below is what stands behind the estimate.  A list that
// would overflow raises a flag: the host entries return SFMHIP_E_ARG with a message, the enqueue-only entry leaves -1 in *d_n_found.
#include "common.hpp"
#include "sortscan.hpp"
#pragma clang fp contract(off)
#include <cmath>

typedef unsigned long long pu64;
typedef unsigned int pu32;

#define AK_MAXL 16
#define AK_NS 109                       // samples of main_orientation: i*i + j*j < 36
#define AK_NWIN 48                      // windows of main_orientation: 42 with the float accumulation of a1
#define AK_NBITS 486
#define AK_KBINS 300
#define AK_ROW_TILE 256
#define AK_ROW_ROWS 4
#define AK_COL_TW 64
#define AK_COL_TH 32
#define AK_COL_PER (AK_COL_TH / 4)
#define AK_UNRESOLVED (-2)
#define AK_DROPPED (-1)
#define AK_DEAD (-3)
#define AK_NONE (-4)
#define AK_PRE_ROUNDS 32                // rounds of the suppression that run over all workgroups before the one-workgroup loop

struct AkTaps { float k[15]; int r; };

// what the host knows from rows / cols alone, and the fixed tables; lives in device memory (indexed by values the kernels load)
struct AkTab {
    int n_levels;
    int rows[AK_MAXL], cols[AK_MAXL], octave[AK_MAXL], sigma_size[AK_MAXL], border[AK_MAXL];
    float size[AK_MAXL];                              // esigma * derivative_factor
    pu64 off[AK_MAXL];                                // float offset of the level's Lt; Lx, Ly, Ldet follow at multiples of rows * cols
    float g[AK_NS]; int di[AK_NS], dj[AK_NS];         // main_orientation: Gaussian weight and offsets of sample n
    float a1[AK_NWIN], a2[AK_NWIN]; int nwin;
    unsigned short pair[AK_NBITS + 2];                // bit dpos compares cell a (bits 0-4) with cell b (5-9) on channel ch (10-11)
};
struct AkCounters {
    pu32 n_raw, n_kept, n_fit, pad0; int overflow; pu32 hmax_bits, npoints; int pad;
    float kc[AK_MAXL];                                // kcontrast of every level
    int seg[AK_MAXL + 1];                             // first candidate of every level in the sorted list
    int hist[AK_KBINS];
    int rem[AK_PRE_ROUNDS];                           // suppression: round r left candidates unresolved
};
struct AkCand { float x, y, response; int level; };
struct AkFit { float x, y, size, response; int level, ok, pad0, pad1; };

__device__ __forceinline__ int ak_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int ak_fround(float v) { return (int)(v + (v >= 0 ? 0.5f : -0.5f)); }
__device__ __forceinline__ int ak_reflect101(int i, int n) { if (n == 1) return 0; while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i; return i; }

__global__ __launch_bounds__(256) void akaze_gray_kernel(const uint8_t* __restrict__ img, int rows, int cols, int ch, size_t ld, float* __restrict__ dst)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    const uint8_t* p = img + (size_t)y * ld + (size_t)x * ch;
    const float g = ch == 3 ? 0.114f * p[0] + 0.587f * p[1] + 0.299f * p[2] : (float)p[0];
    dst[(size_t)y * cols + x] = g * (1.0f / 255.0f);
}

// row pass of blur(): AK_ROW_ROWS row segments of AK_ROW_TILE pixels per workgroup, halo of R, every index clamped into the row
template <int R>
__global__ __launch_bounds__(AK_ROW_TILE) void akaze_blur_rows_kernel(const float* __restrict__ src, int H, int W, AkTaps T, float* __restrict__ dst)
{
    __shared__ float s[AK_ROW_ROWS][AK_ROW_TILE + 2 * R];
    const int y0 = blockIdx.y * AK_ROW_ROWS, x0 = blockIdx.x * AK_ROW_TILE;
#pragma unroll
    for (int rr = 0; rr < AK_ROW_ROWS; ++rr) {
        const float* row = src + (size_t)min(y0 + rr, H - 1) * W;
        for (int t = threadIdx.x; t < AK_ROW_TILE + 2 * R; t += AK_ROW_TILE) s[rr][t] = row[ak_clampi(x0 - R + t, 0, W - 1)];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
#pragma unroll
    for (int rr = 0; rr < AK_ROW_ROWS; ++rr) {
        if (y0 + rr >= H) break;
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i <= 2 * R; ++i) a += T.k[i] * s[rr][(int)threadIdx.x + i];
        dst[(size_t)(y0 + rr) * W + x] = a;
    }
}

// column pass of blur(): a tile of AK_COL_TW x AK_COL_TH pixels per workgroup, halo of R rows, every row index clamped
template <int R>
__global__ __launch_bounds__(256) void akaze_blur_cols_kernel(const float* __restrict__ src, int H, int W, AkTaps T, float* __restrict__ dst)
{
    __shared__ float s[AK_COL_TH + 2 * R][AK_COL_TW];
    const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6, x = blockIdx.x * AK_COL_TW + cx, y0 = blockIdx.y * AK_COL_TH;
    const int xs = min(x, W - 1);
    for (int t = ty; t < AK_COL_TH + 2 * R; t += 4) s[t][cx] = src[(size_t)ak_clampi(y0 - R + t, 0, H - 1) * W + xs];
    __syncthreads();
    if (x >= W) return;
    const int j0 = ty * AK_COL_PER;
#pragma unroll
    for (int j = 0; j < AK_COL_PER; ++j) {
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i <= 2 * R; ++i) a += T.k[i] * s[j0 + j + i][cx];
        const int y = y0 + j0 + j;
        if (y < H) dst[(size_t)y * W + x] = a;
    }
}

// scharr() at one pixel
__device__ __forceinline__ void ak_scharr_at(const float* __restrict__ s, int H, int W, int y, int x, float& gx, float& gy)
{
    const int ym = ak_reflect101(y - 1, H), yp = ak_reflect101(y + 1, H), xm = ak_reflect101(x - 1, W), xp = ak_reflect101(x + 1, W);
    const float* rm = s + (size_t)ym * W; const float* r0 = s + (size_t)y * W; const float* rp = s + (size_t)yp * W;
    gx = 3.0f * (rm[xp] - rm[xm]) + 10.0f * (r0[xp] - r0[xm]) + 3.0f * (rp[xp] - rp[xm]);
    gy = 3.0f * (rp[xm] - rm[xm]) + 10.0f * (rp[x] - rm[x]) + 3.0f * (rp[xp] - rm[xp]);
}

// k_percentile, first loop: the gradient magnitude of every interior pixel and their maximum (non-negative floats: the bit patterns order them)
__global__ __launch_bounds__(256) void akaze_hmax_kernel(const float* __restrict__ sm, int H, int W, float* __restrict__ mag, AkCounters* __restrict__ cnt)
{
    __shared__ pu32 smax;
    if (threadIdx.x == 0) smax = 0u;
    __syncthreads();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    pu32 bits = 0u;
    // a workgroup walks a column strip in steps of the grid: the one shared address sees a few thousand atomics, not one per 256 pixels
    for (int y = blockIdx.y * 4 + (threadIdx.x >> 6); y < H - 1; y += gridDim.y * 4) {
        if (x < 1 || x >= W - 1 || y < 1) continue;
        float gx, gy;
        ak_scharr_at(sm, H, W, y, x, gx, gy);
        const float m = sqrtf(gx * gx + gy * gy);
        mag[(size_t)y * W + x] = m;
        if (m > 0.0f) bits = max(bits, __float_as_uint(m));           // (a NaN never enters: std::max(hmax, NaN) keeps hmax)
    }
    for (int off = 32; off > 0; off >>= 1) bits = max(bits, (pu32)__shfl_xor((int)bits, off));
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(&smax, bits);
    __syncthreads();
    // one address for every workgroup: only those above the value seen so far go to it (a stale read is a smaller one, never a wrong skip)
    if (threadIdx.x == 0 && smax > cnt->hmax_bits) atomicMax(&cnt->hmax_bits, smax);
}

// ... second loop: the histogram of the non-zero magnitudes
__global__ __launch_bounds__(256) void akaze_hist_kernel(const float* __restrict__ mag, int H, int W, AkCounters* __restrict__ cnt)
{
    __shared__ int h[AK_KBINS];
    __shared__ pu32 np;
    const float hmax = __uint_as_float(cnt->hmax_bits);
    if (!(hmax > 0.0f)) return;
    for (int t = threadIdx.x; t < AK_KBINS; t += 256) h[t] = 0;
    if (threadIdx.x == 0) np = 0u;
    __syncthreads();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    for (int y = blockIdx.y * 4 + (threadIdx.x >> 6); y < H - 1; y += gridDim.y * 4) {
        if (x < 1 || x >= W - 1 || y < 1) continue;
        const float m = mag[(size_t)y * W + x];
        if (m != 0.0f) {
            int b = (int)floorf(AK_KBINS * (m / hmax));
            if (b >= AK_KBINS) b = AK_KBINS - 1;
            if (b >= 0) atomicAdd(&h[b], 1);
            atomicAdd(&np, 1u);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < AK_KBINS; t += 256) if (h[t]) atomicAdd(&cnt->hist[t], h[t]);
    if (threadIdx.x == 0 && np) atomicAdd(&cnt->npoints, np);
}

// ... the scan, the fallbacks, and the factor 0.75f of every new octave
__global__ void akaze_kcontrast_kernel(const AkTab* __restrict__ T, AkCounters* __restrict__ cnt)
{
    const float hmax = __uint_as_float(cnt->hmax_bits);
    float kc = 0.03f;
    if (hmax > 0.0f) {
        const pu64 npoints = cnt->npoints;
        const pu64 nthreshold = (pu64)((float)npoints * 0.7f);
        pu64 nel = 0; int k = 0;
        for (; nel < nthreshold && k < AK_KBINS; ++k) nel += (pu64)cnt->hist[k];
        kc = nel < nthreshold ? 0.03f : hmax * (float)k / (float)AK_KBINS;
    }
    cnt->kc[0] = kc;
    for (int i = 1; i < T->n_levels; ++i) {
        if (T->octave[i] > T->octave[i - 1]) kc *= 0.75f;
        cnt->kc[i] = kc;
    }
}

__global__ __launch_bounds__(256) void akaze_half_kernel(const float* __restrict__ s, int sH, int sW, float* __restrict__ d, int H, int W)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int y0 = min(2 * y, sH - 1), y1 = min(2 * y + 1, sH - 1), x0 = min(2 * x, sW - 1), x1 = min(2 * x + 1, sW - 1);
    d[(size_t)y * W + x] = 0.25f * (s[(size_t)y0 * sW + x0] + s[(size_t)y0 * sW + x1] + s[(size_t)y1 * sW + x0] + s[(size_t)y1 * sW + x1]);
}

__global__ __launch_bounds__(256) void akaze_flow_kernel(const float* __restrict__ smooth, int H, int W, const AkCounters* __restrict__ cnt, int level,
                                                         float* __restrict__ flow)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float kc = cnt->kc[level], ik2 = 1.0f / (kc * kc);
    float gx, gy;
    ak_scharr_at(smooth, H, W, y, x, gx, gy);
    flow[(size_t)y * W + x] = 1.0f / (1.0f + ik2 * (gx * gx + gy * gy));
}

// nld_step: the whole increment from the old L
__global__ __launch_bounds__(256) void akaze_fed_kernel(const float* __restrict__ L, const float* __restrict__ c, int H, int W, float tau, float* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t at = (size_t)y * W + x;
    const float l = L[at], cc = c[at];
    float a = 0.0f;
    if (x + 1 < W) a += (cc + c[at + 1]) * (L[at + 1] - l);
    if (x > 0) a -= (c[at - 1] + cc) * (l - L[at - 1]);
    if (y + 1 < H) a += (cc + c[at + W]) * (L[at + W] - l);
    if (y > 0) a -= (c[at - W] + cc) * (l - L[at - W]);
    const float step = 0.5f * tau * a;
    out[at] = l + step;
}

// deriv() at one pixel
__device__ __forceinline__ float ak_deriv_at(const float* __restrict__ s, int H, int W, int y, int x, int sc, float w, float norm, bool along_x)
{
    const int ym = ak_reflect101(y - sc, H), yp = ak_reflect101(y + sc, H), xm = ak_reflect101(x - sc, W), xp = ak_reflect101(x + sc, W);
    const float* rm = s + (size_t)ym * W; const float* r0 = s + (size_t)y * W; const float* rp = s + (size_t)yp * W;
    if (along_x) return norm * ((rm[xp] - rm[xm]) + w * (r0[xp] - r0[xm]) + (rp[xp] - rp[xm]));
    return norm * ((rp[xm] - rm[xm]) + w * (rp[x] - rm[x]) + (rp[xp] - rm[xp]));
}

__global__ __launch_bounds__(256) void akaze_deriv1_kernel(const float* __restrict__ smooth, int H, int W, int sc, float w, float norm, float* __restrict__ Lx,
                                                           float* __restrict__ Ly)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float ss = (float)sc;
    Lx[(size_t)y * W + x] = ak_deriv_at(smooth, H, W, y, x, sc, w, norm, true) * ss;
    Ly[(size_t)y * W + x] = ak_deriv_at(smooth, H, W, y, x, sc, w, norm, false) * ss;
}

__global__ __launch_bounds__(256) void akaze_det_kernel(const float* __restrict__ Lx, const float* __restrict__ Ly, int H, int W, int sc, float w, float norm,
                                                        float* __restrict__ Ldet)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float ss = (float)sc;
    const float xx = ak_deriv_at(Lx, H, W, y, x, sc, w, norm, true) * ss, yy = ak_deriv_at(Ly, H, W, y, x, sc, w, norm, false) * ss,
                xy = ak_deriv_at(Lx, H, W, y, x, sc, w, norm, false) * ss;
    Ldet[(size_t)y * W + x] = xx * yy - xy * xy;
}

// the scan of find_extrema on one level, without the suppression
__global__ __launch_bounds__(256) void akaze_maxima_kernel(const float* __restrict__ D, int H, int W, int border, int level, float ratio, AkCand* __restrict__ cand,
                                                           pu32 K, AkCounters* __restrict__ cnt)
{
    const int x = border + blockIdx.x * 64 + (threadIdx.x & 63), y = border + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W - border || y >= H - border) return;
    const float* p = D + (size_t)y * W + x;
    const float v = p[0];
    if (!(v > 0.001f)) return;
    if (!(v > p[-1] && v > p[1] && v > p[-W - 1] && v > p[-W] && v > p[-W + 1] && v > p[W - 1] && v > p[W] && v > p[W + 1])) return;
    const pu32 at = atomicAdd(&cnt->n_raw, 1u);
    if (at < K) { AkCand c; c.x = x * ratio; c.y = y * ratio; c.response = v; c.level = level; cand[at] = c; }
    else cnt->overflow = 1;
}

// (level, y, x): x and y are integers below 16384 held as floats
__global__ __launch_bounds__(256) void akaze_key_kernel(const AkCand* __restrict__ cand, pu32 K, const AkCounters* __restrict__ cnt, pu64* __restrict__ keys)
{
    const pu32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    pu64 key = 0xFFFFFFFFull;
    if (i < min(cnt->n_raw, K)) { const AkCand c = cand[i]; key = ((pu64)c.level << 28) | ((pu64)(pu32)c.y << 14) | (pu64)(pu32)c.x; }
    keys[i] = key;
}
__global__ __launch_bounds__(256) void akaze_gather_kernel(const AkCand* __restrict__ cand, const pu32* __restrict__ perm, pu32 K, const AkCounters* __restrict__ cnt,
                                                           AkCand* __restrict__ sorted)
{
    const pu32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < min(cnt->n_raw, K)) sorted[i] = cand[perm[i]];
}
// a caller's list for sfmhip_akaze_suppress
__global__ __launch_bounds__(256) void akaze_pack_kernel(const float* __restrict__ xyr, const int32_t* __restrict__ level, pu32 n, AkCounters* __restrict__ cnt,
                                                         AkCand* __restrict__ sorted)
{
    const pu32 i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) cnt->n_raw = n;
    if (i >= n) return;
    AkCand c; c.x = xyr[3 * (size_t)i]; c.y = xyr[3 * (size_t)i + 1]; c.response = xyr[3 * (size_t)i + 2]; c.level = level[i];
    sorted[i] = c;
}

// first index in [lo, hi) whose y is not below ylo (the list is sorted by y there)
__device__ __forceinline__ int ak_lower_y(const AkCand* __restrict__ c, int lo, int hi, float ylo)
{
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (c[mid].y < ylo) lo = mid + 1; else hi = mid; }
    return lo;
}

// One candidate of one round of the first pass of find_extrema (header comment).  false: a predecessor within reach is unresolved.  Else p is
// the candidate's slot or AK_DROPPED and v the entry it replaces (-1: none).  seg / size: the level starts and sizes (LDS or global)
__device__ __forceinline__ bool ak_decide(const AkCand* __restrict__ c, const int* seg, const float* size, int ysorted, const int* slot, int i, int& p, int& v)
{
    const AkCand ci = c[i];
    const int l = ci.level & (AK_MAXL - 1);
    const float sz = size[l], reach = 2.0f * sz + 1.0f, reach2 = reach * reach;
    int best = 0x7FFFFFFF, best_e = -1;
    for (int lv = max(l - 1, 0); lv <= l; ++lv) {
        const int end = min(seg[lv + 1], i);
        int e = seg[lv];
        if (ysorted) e = ak_lower_y(c, e, end, ci.y - reach);
        for (; e < end; ++e) {
            const AkCand ce = c[e];
            if (ysorted && ce.y > ci.y + reach) break;
            const float dx = ci.x - ce.x, dy = ci.y - ce.y, d2 = dx * dx + dy * dy;
            if (!(d2 <= reach2)) continue;
            const int st = slot[e];
            if (st == AK_UNRESOLVED) return false;
            if (d2 <= sz * sz && st >= 0 && st < best) { best = st; best_e = e; }
        }
    }
    if (best_e < 0) { p = i; v = -1; }
    else if (ci.response > c[best_e].response) { p = best; v = best_e; }
    else { p = AK_DROPPED; v = -1; }
    return true;
}

// the level starts, and every candidate unresolved
__global__ __launch_bounds__(256) void akaze_suppress_init_kernel(const AkCand* __restrict__ c, pu32 K, AkCounters* __restrict__ cnt, int* __restrict__ slot,
                                                                   int* __restrict__ pend)
{
    const int n = (int)min(cnt->n_raw, K);
    if (blockIdx.x == 0 && threadIdx.x <= AK_MAXL) {         // seg[l]: the first candidate whose level is not below l
        int lo = 0, hi = n;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (c[mid].level < (int)threadIdx.x) lo = mid + 1; else hi = mid; }
        cnt->seg[threadIdx.x] = lo;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) { slot[i] = AK_UNRESOLVED; pend[i] = AK_NONE; }
}

// Round `round` of the first AK_PRE_ROUNDS, over all workgroups, in two launches: every unresolved candidate whose predecessors the earlier
// rounds resolved decides (reading only what they published), then the decisions are published.  cnt->rem[r]: round r left something
// unresolved; once a round left nothing, the launches behind it return at once
__global__ __launch_bounds__(256) void akaze_suppress_round_kernel(const AkCand* __restrict__ c, pu32 K, AkCounters* __restrict__ cnt, const AkTab* __restrict__ T,
                                                                    int ysorted, const int* __restrict__ slot, int* __restrict__ pend, int* __restrict__ victim, int round)
{
    if (round > 0 && cnt->rem[round - 1] == 0) return;
    const int n = (int)min(cnt->n_raw, K);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (slot[i] != AK_UNRESOLVED) continue;
        int p, v;
        if (ak_decide(c, cnt->seg, T->size, ysorted, slot, i, p, v)) { pend[i] = p; victim[i] = v; }
        else cnt->rem[round] = 1;
    }
}
__global__ __launch_bounds__(256) void akaze_suppress_publish_kernel(pu32 K, const AkCounters* __restrict__ cnt, int* __restrict__ slot, int* __restrict__ pend,
                                                                      const int* __restrict__ victim, int round)
{
    if (round > 0 && cnt->rem[round - 1] == 0) return;
    const int n = (int)min(cnt->n_raw, K);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int p = pend[i];
        if (p == AK_NONE) continue;
        slot[i] = p; pend[i] = AK_NONE;                      // (a candidate resolved in this round is nobody's victim in it)
        if (victim[i] >= 0) slot[victim[i]] = AK_DEAD;
    }
}

// The rounds the launches above left over, in ONE workgroup with barriers: the loop that is bound to end (a round resolves the earliest
// unresolved candidate at least: n rounds at most).  Images need none of it; a chain of candidates that replace one another does.
// slot[i] = the candidate's slot, AK_DROPPED, or AK_DEAD once replaced
__global__ __launch_bounds__(1024) void akaze_suppress_kernel(const AkCand* __restrict__ c, pu32 K, AkCounters* __restrict__ cnt, const AkTab* __restrict__ T, int ysorted,
                                                              int* __restrict__ slot, int* __restrict__ pend, int* __restrict__ victim)
{
    __shared__ int seg[AK_MAXL + 1];
    __shared__ float size[AK_MAXL];
    __shared__ int remaining;
    const int n = (int)min(cnt->n_raw, K), tid = threadIdx.x;
    if (tid <= AK_MAXL) { seg[tid] = cnt->seg[tid]; if (tid < AK_MAXL) size[tid] = T->size[tid]; }
    __syncthreads();
    for (int round = 0; round < n; ++round) {
        if (tid == 0) remaining = 0;
        __syncthreads();
        for (int i = tid; i < n; i += 1024) {
            if (slot[i] != AK_UNRESOLVED) continue;
            int p, v;
            if (ak_decide(c, seg, size, ysorted, slot, i, p, v)) { pend[i] = p; victim[i] = v; }
            else remaining = 1;
        }
        __syncthreads();
        const int rem = remaining;
        for (int i = tid; i < n; i += 1024) {                // publish: the next round reads what this one decided
            const int p = pend[i];
            if (p == AK_NONE) continue;
            slot[i] = p; pend[i] = AK_NONE;
            if (victim[i] >= 0) slot[victim[i]] = AK_DEAD;
        }
        __syncthreads();
        if (!rem) break;
    }
}

// second pass: an entry goes if a later entry (a larger slot) of its level or the one above covers and beats it; key = slot of a survivor
__global__ __launch_bounds__(256) void akaze_suppress2_kernel(const AkCand* __restrict__ c, pu32 K, AkCounters* __restrict__ cnt, const AkTab* __restrict__ T, int ysorted,
                                                              const int* __restrict__ slot, pu64* __restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (int)K) return;
    const int n = (int)min(cnt->n_raw, K);
    pu64 key = 0xFFFFFFFFull;
    if (i < n && slot[i] >= 0) {
        const AkCand ci = c[i];
        const int l = ci.level & (AK_MAXL - 1), si = slot[i];
        bool keep = true;
        for (int lv = l; lv <= min(l + 1, AK_MAXL - 1) && keep; ++lv) {
            const float sz = T->size[lv];
            const int end = cnt->seg[lv + 1];
            int j = cnt->seg[lv];
            if (ysorted) j = ak_lower_y(c, j, end, ci.y - sz - 1.0f);
            for (; j < end; ++j) {
                const AkCand cj = c[j];
                if (ysorted && cj.y > ci.y + sz + 1.0f) break;
                if (slot[j] <= si) continue;
                const float dx = ci.x - cj.x, dy = ci.y - cj.y;
                if (dx * dx + dy * dy <= sz * sz && ci.response < cj.response) { keep = false; break; }
            }
        }
        if (keep) { key = (pu64)(pu32)si; atomicAdd(&cnt->n_kept, 1u); }
    }
    keys[i] = key;
}

// subpixel() on the survivors in aux order; flag[t] = 1 where the fit holds (K + 1 entries)
__global__ __launch_bounds__(256) void akaze_subpixel_kernel(const AkCand* __restrict__ c, const pu32* __restrict__ order, pu32 K, const AkCounters* __restrict__ cnt,
                                                             const AkTab* __restrict__ T, const float* __restrict__ lev, AkFit* __restrict__ fit, pu32* __restrict__ flag)
{
    const pu32 t = blockIdx.x * 256 + threadIdx.x;
    if (t > K) return;
    pu32 ok = 0u;
    if (t < min(cnt->n_kept, K)) {
        const AkCand cd = c[order[t]];
        const int l = cd.level & (AK_MAXL - 1), W = T->cols[l], H = T->rows[l];
        const float ratio = (float)(1 << T->octave[l]);
        const int x = ak_fround(cd.x / ratio), y = ak_fround(cd.y / ratio);
        AkFit f; f.x = cd.x; f.y = cd.y; f.size = T->size[l]; f.response = cd.response; f.level = l; f.ok = 0; f.pad0 = f.pad1 = 0;
        if (!(x < 1 || y < 1 || x + 1 >= W || y + 1 >= H)) {
            const float* D = lev + T->off[l] + 3 * (size_t)H * W + (size_t)y * W + x;
            const float Dx = 0.5f * (D[1] - D[-1]), Dy = 0.5f * (D[W] - D[-W]);
            const float Dxx = D[1] + D[-1] - 2.0f * D[0], Dyy = D[W] + D[-W] - 2.0f * D[0];
            const float Dxy = 0.25f * (D[W + 1] + D[-W - 1] - D[-W + 1] - D[W - 1]);
            const float det = Dxx * Dyy - Dxy * Dxy;
            if (det != 0.0f) {
                const float dx = (-Dyy * Dx + Dxy * Dy) / det, dy = (Dxy * Dx - Dxx * Dy) / det;
                if (fabsf(dx) <= 1.0f && fabsf(dy) <= 1.0f) {
                    f.x = (x + dx) * ratio + 0.5f * (ratio - 1.0f);
                    f.y = (y + dy) * ratio + 0.5f * (ratio - 1.0f);
                    f.size *= 2.0f;
                    f.ok = 1; ok = 1u;
                }
            }
        }
        fit[t] = f;
    }
    flag[t] = ok;
}
__global__ __launch_bounds__(256) void akaze_compact_kernel(const pu32* __restrict__ excl, pu32 K, AkCounters* __restrict__ cnt, pu32* __restrict__ list)
{
    const pu32 i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) cnt->n_fit = excl[K];
    if (i >= K) return;
    const pu32 at = excl[i];
    if (excl[i + 1] != at) list[at] = i;
}
// descending response (positive floats: the bit patterns order them); a row past the list keeps the largest key and stays behind
__global__ __launch_bounds__(256) void akaze_resp_key_kernel(const AkFit* __restrict__ fit, const pu32* __restrict__ list, pu32 K, const AkCounters* __restrict__ cnt,
                                                             pu64* __restrict__ keys)
{
    const pu32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    keys[i] = i < cnt->n_fit ? (pu64)(~__float_as_uint(fit[list[i]].response)) : 0xFFFFFFFFull;
}
__global__ void akaze_count_kernel(const AkCounters* __restrict__ cnt, int max_features, int32_t* __restrict__ n_found)
{
    pu32 n = cnt->n_fit;
    if (max_features > 0 && n > (pu32)max_features) n = (pu32)max_features;
    *n_found = cnt->overflow ? -1 : (int32_t)n;
}

// main_orientation + mldb + the sfm_keypoint: a wave per output row, four per workgroup
__global__ __launch_bounds__(256) void akaze_describe_kernel(const AkTab* __restrict__ T, const float* __restrict__ lev, const AkFit* __restrict__ fit,
                                                             const pu32* __restrict__ order, const int32_t* __restrict__ n_found, int cap, sfm_keypoint* __restrict__ kp,
                                                             uint8_t* __restrict__ desc)
{
    __shared__ float resX[4][AK_NS], resY[4][AK_NS], ang[4][AK_NS];
    __shared__ float wsx[4][AK_NWIN], wsy[4][AK_NWIN];
    __shared__ float vals[4][29][3];
    __shared__ float s_angle[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = min(*n_found, cap);
    const int nwin = min(T->nwin, AK_NWIN);
    for (int base = blockIdx.x * 4; base < n; base += gridDim.x * 4) {          // the same trip count for the four waves: barriers inside
        const int q = base + wave;
        const bool live = q < n;
        const AkFit c = fit[order[live ? q : base]];
        const int l = c.level & (AK_MAXL - 1), W = T->cols[l], H = T->rows[l];
        const size_t px = (size_t)H * W;
        const float *Lt = lev + T->off[l], *Lx = Lt + px, *Ly = Lt + 2 * px;
        const float ratio = (float)(1 << T->octave[l]), xf = c.x / ratio, yf = c.y / ratio;
        const int s = max(1, ak_fround(0.5f * c.size / ratio));
        for (int k = lane; k < AK_NS; k += 64) {
            const int iy = ak_fround(yf + T->dj[k] * s), ix = ak_fround(xf + T->di[k] * s);
            float rx = 0.0f, ry = 0.0f, a = 0.0f;
            if (!(iy < 0 || ix < 0 || iy >= H || ix >= W)) {
                const float g = T->g[k];
                rx = g * Lx[(size_t)iy * W + ix]; ry = g * Ly[(size_t)iy * W + ix];
                a = atan2f(ry, rx); if (a < 0) a += 6.28318530718f;
            }
            resX[wave][k] = rx; resY[wave][k] = ry; ang[wave][k] = a;
        }
        __syncthreads();
        if (lane < nwin) {
            const float a1 = T->a1[lane], a2 = T->a2[lane];
            float sx = 0.0f, sy = 0.0f;
            for (int k = 0; k < AK_NS; ++k) {
                const float a = ang[wave][k];
                if ((a1 < a2 && a1 < a && a < a2) || (a2 < a1 && ((a > 0 && a < a2) || (a > a1 && a < 6.28318530718f)))) { sx += resX[wave][k]; sy += resY[wave][k]; }
            }
            wsx[wave][lane] = sx; wsy[wave][lane] = sy;
        }
        __syncthreads();
        if (lane == 0) {
            float best = 0.0f; int bw = -1;
            for (int w = 0; w < nwin; ++w) { const float m = wsx[wave][w] * wsx[wave][w] + wsy[wave][w] * wsy[wave][w]; if (m > best) { best = m; bw = w; } }
            float angle = 0.0f;
            if (bw >= 0) { angle = atan2f(wsy[wave][bw], wsx[wave][bw]); if (angle < 0) angle += 6.28318530718f; }
            s_angle[wave] = angle;
        }
        __syncthreads();
        const float angle = s_angle[wave];
        const float co = cosf(angle), si = sinf(angle);
        if (lane < 29) {
            // cell `lane`: grid 0 = 2 x 2 of step 10, grid 1 = 3 x 3 of step 7, grid 2 = 4 x 4 of step 5
            const int grid = lane < 4 ? 0 : (lane < 13 ? 1 : 2), cell = lane - (grid == 0 ? 0 : (grid == 1 ? 4 : 13));
            const int nc = grid + 2, step = grid == 0 ? 10 : (grid == 1 ? 7 : 5);
            const int i0 = -10 + (cell / nc) * step, j0 = -10 + (cell % nc) * step;
            float di = 0, dx = 0, dy = 0; int ns = 0;
            for (int k = i0; k < i0 + step; ++k)
                for (int ll = j0; ll < j0 + step; ++ll) {
                    const float sy = yf + (ll * co * s + k * si * s), sx = xf + (-ll * si * s + k * co * s);
                    const int y1 = ak_fround(sy), x1 = ak_fround(sx);
                    if (x1 < 0 || y1 < 0 || x1 >= W || y1 >= H) continue;
                    const size_t at = (size_t)y1 * W + x1;
                    const float rx = Lx[at], ry = Ly[at];
                    di += Lt[at]; dx += -rx * si + ry * co; dy += rx * co + ry * si; ++ns;
                }
            if (ns > 0) { di /= ns; dx /= ns; dy /= ns; }
            vals[wave][lane][0] = di; vals[wave][lane][1] = dx; vals[wave][lane][2] = dy;
        }
        __syncthreads();
        if (live && lane < 61) {
            pu32 byte = 0u;
            for (int b = 0; b < 8; ++b) {
                const int dpos = 8 * lane + b;
                if (dpos >= AK_NBITS) break;                                 // bits 486 and 487 stay clear
                const pu32 p = T->pair[dpos];
                const int ch = (int)(p >> 10) & 3;
                if (vals[wave][p & 31u][ch] > vals[wave][(p >> 5) & 31u][ch]) byte |= 1u << b;
            }
            desc[(size_t)q * 61 + lane] = (uint8_t)byte;
        }
        if (live && lane == 63) {
            sfm_keypoint o;
            o.x = c.x; o.y = c.y; o.size = c.size; o.angle = angle * 57.29577951308232f; o.response = c.response;
            o.octave = T->octave[l]; o.class_id = l;
            kp[q] = o;
        }
        __syncthreads();
    }
}

// the three diagnostic stages of sfmhip_akaze_extrema: rows of {x, y, size, response} and {octave, level}
__global__ __launch_bounds__(256) void akaze_stage_out_kernel(int stage, const AkCand* __restrict__ c, const pu32* __restrict__ order, const AkFit* __restrict__ fit,
                                                              const pu32* __restrict__ list, pu32 K, const AkCounters* __restrict__ cnt, const AkTab* __restrict__ T,
                                                              int cap, float* __restrict__ xysr, int32_t* __restrict__ ol, int32_t* __restrict__ n_found)
{
    const pu32 i = blockIdx.x * 256 + threadIdx.x;
    const pu32 n = stage == 0 ? min(cnt->n_raw, K) : (stage == 1 ? min(cnt->n_kept, K) : cnt->n_fit);
    if (i == 0) *n_found = cnt->overflow ? -1 : (int32_t)n;
    if (i >= n || i >= (pu32)cap) return;
    float x, y, size, r; int l;
    if (stage == 2) { const AkFit f = fit[list[i]]; x = f.x; y = f.y; size = f.size; r = f.response; l = f.level; }
    else { const AkCand d = c[stage == 0 ? i : order[i]]; x = d.x; y = d.y; r = d.response; l = d.level & (AK_MAXL - 1); size = T->size[l]; }
    xysr[4 * (size_t)i] = x; xysr[4 * (size_t)i + 1] = y; xysr[4 * (size_t)i + 2] = size; xysr[4 * (size_t)i + 3] = r;
    ol[2 * (size_t)i] = T->octave[l]; ol[2 * (size_t)i + 1] = l;
}
__global__ __launch_bounds__(256) void akaze_kept_out_kernel(const pu32* __restrict__ order, pu32 K, const AkCounters* __restrict__ cnt, int32_t* __restrict__ kept,
                                                             int32_t* __restrict__ n_kept)
{
    const pu32 i = blockIdx.x * 256 + threadIdx.x;
    const pu32 n = min(cnt->n_kept, K);
    if (i == 0) *n_kept = (int32_t)n;
    if (i < n) kept[i] = (int32_t)order[i];
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct AkPlan {
    AkTab tab;
    std::vector<float> tau[AK_MAXL];
    AkTaps taps_base, taps_one;          // sigma 1.6f (radius 7) and 1.0 (radius 4)
    size_t px0 = 0, level_floats = 0;
    pu32 K = 0;
};

// blur()'s own tap table
static AkTaps akaze_taps(double sigma)
{
    AkTaps T;
    const int r = std::max(1, (int)std::ceil(4.0 * sigma));
    T.r = r;
    for (float& v : T.k) v = 0.0f;
    if (r > 7) return T;
    double s = 0;
    for (int i = -r; i <= r; ++i) { T.k[i + r] = (float)std::exp(-0.5 * i * i / (sigma * sigma)); s += T.k[i + r]; }
    for (int i = 0; i < 2 * r + 1; ++i) T.k[i] = (float)(T.k[i] / s);
    return T;
}

// fed_taus of sfm_akaze.hpp
static std::vector<float> akaze_fed_taus(float T, float tau_max = 0.25f)
{
    const int n = (int)(std::ceil(std::sqrt(3.0 * T / tau_max + 0.25) - 0.5 - 1.0e-8) + 0.5);
    if (n <= 0) return {};
    const double scale = 3.0 * T / (tau_max * (double)(n * (n + 1)));
    std::vector<float> tauh((size_t)n), tau((size_t)n);
    const double c = 1.0 / (4.0 * n + 2.0), d = scale * tau_max / 2.0;
    for (int k = 0; k < n; ++k) { const double h = std::cos(3.14159265358979323846 * (2.0 * k + 1.0) * c); tauh[(size_t)k] = (float)(d / (h * h)); }
    const int kappa = n / 2;
    int prime = n + 1;
    auto is_prime = [](int v) { if (v < 2) return false; for (int q = 2; q * q <= v; ++q) if (v % q == 0) return false; return true; };
    while (!is_prime(prime)) ++prime;
    for (int k = 0, l = 0; l < n; ++k) { const int idx = ((k + 1) * kappa) % prime - 1; if (idx >= 0 && idx < n) tau[(size_t)l++] = tauh[(size_t)idx]; if (k > 4 * prime) { tau = tauh; break; } }
    return tau;
}

static int akaze_fround(float v) { return (int)(v + (v >= 0 ? 0.5f : -0.5f)); }

// the tables that do not depend on the image: level sizes, main_orientation's weights and windows, mldb's comparison list
static void akaze_fixed_tables(AkTab& T)
{
    const float soffset = 1.6f, derivative_factor = 1.5f;
    for (int i = 0; i < AK_MAXL; ++i) {
        const int o = i / 4, s = i % 4;
        const float esigma = soffset * std::pow(2.0f, (float)s / 4 + o);
        T.size[i] = esigma * derivative_factor;
        T.octave[i] = o;
        T.sigma_size[i] = akaze_fround(esigma * derivative_factor / (float)(1 << o));
        T.border[i] = akaze_fround(12.0f * std::sqrt(2.0f) * T.sigma_size[i]) + 1;
        T.rows[i] = T.cols[i] = 0; T.off[i] = 0;
    }
    int n = 0;
    for (int i = -6; i <= 6; ++i)
        for (int j = -6; j <= 6; ++j) {
            if (i * i + j * j >= 36) continue;
            T.g[n] = std::exp(-(float)(i * i + j * j) / (2.0f * 2.5f * 2.5f)); T.di[n] = i; T.dj[n] = j; ++n;
        }
    T.nwin = 0;
    for (float a1 = 0.0f; a1 < 6.28318530718f && T.nwin < AK_NWIN; a1 += 0.15f) {
        T.a1[T.nwin] = a1;
        T.a2[T.nwin] = a1 + 1.0471975512f > 6.28318530718f ? a1 - 5.2359877560f : a1 + 1.0471975512f;
        ++T.nwin;
    }
    for (int w = T.nwin; w < AK_NWIN; ++w) T.a1[w] = T.a2[w] = 0.0f;
    int dpos = 0, first = 0;
    for (int grid = 0; grid < 3; ++grid) {
        const int nv = (grid + 2) * (grid + 2);
        for (int ch = 0; ch < 3; ++ch)
            for (int a = 0; a < nv; ++a)
                for (int b = a + 1; b < nv; ++b) T.pair[dpos++] = (unsigned short)((first + a) | ((first + b) << 5) | (ch << 10));
        first += nv;
    }
    for (; dpos < AK_NBITS + 2; ++dpos) T.pair[dpos] = 0;
}

static void akaze_plan(int rows, int cols, int cap, AkPlan& P)
{
    AkTab& T = P.tab;
    memset(&T, 0, sizeof T);
    akaze_fixed_tables(T);
    P.px0 = (size_t)rows * cols;
    P.taps_base = akaze_taps((double)1.6f);
    P.taps_one = akaze_taps(1.0);
    int n = 0;
    size_t off = 0;
    float etime_prev = 0.0f;
    for (int o = 0; o < 4; ++o) {
        const int r = rows >> o, c = cols >> o;
        if (r < 80 || c < 80) break;
        for (int s = 0; s < 4; ++s, ++n) {
            const float esigma = 1.6f * std::pow(2.0f, (float)s / 4 + o), etime = 0.5f * esigma * esigma;
            T.rows[n] = r; T.cols[n] = c; T.off[n] = off; off += 4 * (size_t)r * c;
            if (n > 0) P.tau[n] = akaze_fed_taus(etime - etime_prev);
            etime_prev = etime;
        }
    }
    T.n_levels = n;
    P.level_floats = off;
    P.K = (pu32)std::max<size_t>(std::max<size_t>((size_t)std::max(cap, 0), 4096), P.px0 / 8);
}

static bool akaze_image_args_ok(const uint8_t* img, int rows, int cols, int channels, size_t ld)
{
    return img && rows >= 1 && cols >= 1 && rows <= 16384 && cols <= 16384 && (channels == 1 || channels == 3) && ld >= (size_t)cols * channels;
}

static inline dim3 akaze_grid(int H, int W) { return dim3(ceil_div(W, 64), ceil_div(H, 4)); }

// blur(src, sigma) into dst through tmp; the two radii have an instance each
static void akaze_enqueue_blur(hipStream_t st, const float* src, int H, int W, const AkTaps& T, float* tmp, float* dst)
{
    const dim3 gr(ceil_div(W, AK_ROW_TILE), ceil_div(H, AK_ROW_ROWS)), gc(ceil_div(W, AK_COL_TW), ceil_div(H, AK_COL_TH));
    if (T.r == 7) {
        hipLaunchKernelGGL(akaze_blur_rows_kernel<7>, gr, dim3(AK_ROW_TILE), 0, st, src, H, W, T, tmp);
        hipLaunchKernelGGL(akaze_blur_cols_kernel<7>, gc, dim3(256), 0, st, (const float*)tmp, H, W, T, dst);
    } else {
        hipLaunchKernelGGL(akaze_blur_rows_kernel<4>, gr, dim3(AK_ROW_TILE), 0, st, src, H, W, T, tmp);
        hipLaunchKernelGGL(akaze_blur_cols_kernel<4>, gc, dim3(256), 0, st, (const float*)tmp, H, W, T, dst);
    }
}

// the device areas of one image
struct AkAreas {
    AkTab* tab; AkCounters* cnt; float* lev; float* buf[6];
    size_t o_tab, o_cnt, o_lev, o_buf[6];
    void carve(SfmCarve& c, const AkPlan& P)
    {
        o_tab = c(sizeof(AkTab)); o_cnt = c(sizeof(AkCounters)); o_lev = c(std::max<size_t>(P.level_floats, 1) * 4);
        for (int i = 0; i < 6; ++i) o_buf[i] = c(P.px0 * 4);
    }
    void bind(char* w)
    {
        tab = (AkTab*)(w + o_tab); cnt = (AkCounters*)(w + o_cnt); lev = (float*)(w + o_lev);
        for (int i = 0; i < 6; ++i) buf[i] = (float*)(w + o_buf[i]);
    }
};

// build_scale_space of a device image: the tables go up, the counters are cleared, every level's Lt, Lx, Ly, Ldet are left in A.lev.
// smooth_out (may be null): receives Lsmooth of level smooth_level
static int akaze_enqueue_scale_space(sfmhip_ctx* ctx, const AkPlan& P, const AkAreas& A, const uint8_t* d_img, int rows, int cols, int ch, size_t ld,
                                     float* smooth_out, int smooth_level)
{
    hipStream_t st = ctx->stream;
    const AkTab& T = P.tab;
    const int rc = sfm_upload(ctx, A.tab, &T, sizeof T);
    if (rc != SFMHIP_OK) return rc;
    SFM_HIP_TRY(ctx, hipMemsetAsync(A.cnt, 0, sizeof(AkCounters), st));
    if (T.n_levels == 0) return SFMHIP_OK;
    float *gray = A.buf[0], *tmp = A.buf[1], *smooth = A.buf[2], *flow = A.buf[3], *ping = A.buf[4], *half = A.buf[5];
    if (P.taps_base.r != 7 || P.taps_one.r != 4) { ctx->last_error = "akaze: a blur radius without a kernel instance"; return SFMHIP_E_NUMERIC; }
    hipLaunchKernelGGL(akaze_gray_kernel, akaze_grid(rows, cols), dim3(256), 0, st, d_img, rows, cols, ch, ld, gray);
    // k_percentile
    akaze_enqueue_blur(st, gray, rows, cols, P.taps_one, tmp, smooth);
    hipLaunchKernelGGL(akaze_hmax_kernel, dim3(ceil_div(cols, 64), std::min(ceil_div(rows, 4), 64)), dim3(256), 0, st, (const float*)smooth, rows, cols, flow, A.cnt);
    hipLaunchKernelGGL(akaze_hist_kernel, dim3(ceil_div(cols, 64), std::min(ceil_div(rows, 4), 64)), dim3(256), 0, st, (const float*)flow, rows, cols, A.cnt);
    hipLaunchKernelGGL(akaze_kcontrast_kernel, dim3(1), dim3(1), 0, st, (const AkTab*)A.tab, A.cnt);
    const float w = 10.0f / 3.0f;
    for (int i = 0; i < T.n_levels; ++i) {
        const int H = T.rows[i], W = T.cols[i], sc = T.sigma_size[i];
        const size_t px = (size_t)H * W;
        float *Lt = A.lev + T.off[i], *Lx = Lt + px, *Ly = Lt + 2 * px, *Ldet = Lt + 3 * px;
        const dim3 g = akaze_grid(H, W);
        const float* sm = smooth;
        if (i == 0) {
            akaze_enqueue_blur(st, gray, H, W, P.taps_base, tmp, Lt);
            sm = Lt;                                                            // ev[0].Lsmooth = ev[0].Lt
        } else {
            const float* src = A.lev + T.off[i - 1];                          // the previous level's Lt ...
            if (T.octave[i] > T.octave[i - 1]) {                               // ... or its 2 x 2 means
                hipLaunchKernelGGL(akaze_half_kernel, g, dim3(256), 0, st, src, T.rows[i - 1], T.cols[i - 1], half, H, W);
                src = half;
            }
            akaze_enqueue_blur(st, src, H, W, P.taps_one, tmp, smooth);
            hipLaunchKernelGGL(akaze_flow_kernel, g, dim3(256), 0, st, (const float*)smooth, H, W, (const AkCounters*)A.cnt, i, flow);
            // the steps alternate between Lt and ping so that the last one writes Lt
            const int ns = (int)P.tau[i].size();
            if (ns == 0) SFM_HIP_TRY(ctx, hipMemcpyAsync(Lt, src, px * 4, hipMemcpyDeviceToDevice, st));
            for (int k = 0; k < ns; ++k) {
                float* dst = ((ns - 1 - k) & 1) ? ping : Lt;
                hipLaunchKernelGGL(akaze_fed_kernel, g, dim3(256), 0, st, src, (const float*)flow, H, W, P.tau[i][(size_t)k], dst);
                src = dst;
            }
        }
        if (smooth_out && smooth_level == i) SFM_HIP_TRY(ctx, hipMemcpyAsync(smooth_out, sm, px * 4, hipMemcpyDeviceToDevice, st));
        const float norm = 1.0f / (2.0f * sc * (w + 2.0f));
        hipLaunchKernelGGL(akaze_deriv1_kernel, g, dim3(256), 0, st, sm, H, W, sc, w, norm, Lx, Ly);
        hipLaunchKernelGGL(akaze_det_kernel, g, dim3(256), 0, st, (const float*)Lx, (const float*)Ly, H, W, sc, w, norm, Ldet);
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

// the lists of one carve: candidates, suppression state, survivors (K rows each), the sort of K keys and the K + 1 flags of the fit
struct AkLists {
    AkCand *raw, *cand; int *slot, *pend, *victim; AkFit* fit; pu32* list;
    SfmSort keys; SfmScan flags;
    size_t o_raw, o_cand, o_slot, o_pend, o_victim, o_fit, o_list;
    void carve(SfmCarve& c, size_t K)
    {
        o_raw = c(K * sizeof(AkCand)); o_cand = c(K * sizeof(AkCand)); o_slot = c(K * 4); o_pend = c(K * 4); o_victim = c(K * 4);
        o_fit = c(K * sizeof(AkFit)); o_list = c(K * 4);
        keys.carve(c, K); flags.carve(c, K + 1);
    }
    void bind(char* w)
    {
        raw = (AkCand*)(w + o_raw); cand = (AkCand*)(w + o_cand); slot = (int*)(w + o_slot); pend = (int*)(w + o_pend); victim = (int*)(w + o_victim);
        fit = (AkFit*)(w + o_fit); list = (pu32*)(w + o_list);
        keys.bind(w); flags.bind(w);
    }
};

// both passes of find_extrema on the sorted list S.cand (its length in cnt->n_raw): afterwards the survivors' indices are in
// S.keys.v[returned side] in aux order, their number in cnt->n_kept
static int akaze_enqueue_suppress(hipStream_t st, AkLists& S, size_t K, AkCounters* cnt, const AkTab* tab, int ysorted)
{
    const int kb = ceil_div((int)K, 256), rb = std::min(kb, 2048);
    hipLaunchKernelGGL(akaze_suppress_init_kernel, dim3(rb), dim3(256), 0, st, (const AkCand*)S.cand, (pu32)K, cnt, S.slot, S.pend);
    for (int r = 0; r < AK_PRE_ROUNDS; ++r) {
        hipLaunchKernelGGL(akaze_suppress_round_kernel, dim3(rb), dim3(256), 0, st, (const AkCand*)S.cand, (pu32)K, cnt, tab, ysorted, (const int*)S.slot, S.pend, S.victim, r);
        hipLaunchKernelGGL(akaze_suppress_publish_kernel, dim3(rb), dim3(256), 0, st, (pu32)K, (const AkCounters*)cnt, S.slot, S.pend, (const int*)S.victim, r);
    }
    hipLaunchKernelGGL(akaze_suppress_kernel, dim3(1), dim3(1024), 0, st, (const AkCand*)S.cand, (pu32)K, cnt, tab, ysorted, S.slot, S.pend, S.victim);
    hipLaunchKernelGGL(akaze_suppress2_kernel, dim3(kb), dim3(256), 0, st, (const AkCand*)S.cand, (pu32)K, cnt, tab, ysorted, (const int*)S.slot, S.keys.k[0]);
    return S.keys.sort(st, K, 0, 32, true);
}

// find_extrema + subpixel: stage 0 stops after the ordered raw maxima, 1 after the suppression, 2 after the fit (S.list: the rows of S.fit that
// hold, in aux order; cnt->n_fit of them).  *order_side: the side of S.keys.v with the survivors of stage 1
static void akaze_enqueue_detect(sfmhip_ctx* ctx, const AkPlan& P, const AkAreas& A, AkLists& S, int stage, int* order_side)
{
    hipStream_t st = ctx->stream;
    const AkTab& T = P.tab;
    const size_t K = P.K;
    const int kb = ceil_div((int)K, 256), kb1 = ceil_div((int)K + 1, 256);
    for (int i = 0; i < T.n_levels; ++i) {
        const int H = T.rows[i], W = T.cols[i], b = T.border[i];
        if (H - 2 * b <= 0 || W - 2 * b <= 0) continue;
        hipLaunchKernelGGL(akaze_maxima_kernel, akaze_grid(H - 2 * b, W - 2 * b), dim3(256), 0, st, (const float*)(A.lev + T.off[i] + 3 * (size_t)H * W), H, W, b, i,
                           (float)(1 << T.octave[i]), S.raw, (pu32)K, A.cnt);
    }
    hipLaunchKernelGGL(akaze_key_kernel, dim3(kb), dim3(256), 0, st, (const AkCand*)S.raw, (pu32)K, (const AkCounters*)A.cnt, S.keys.k[0]);
    int side = S.keys.sort(st, K, 0, 32, true);
    hipLaunchKernelGGL(akaze_gather_kernel, dim3(kb), dim3(256), 0, st, (const AkCand*)S.raw, (const pu32*)S.keys.v[side], (pu32)K, (const AkCounters*)A.cnt, S.cand);
    *order_side = 0;
    if (stage < 1) return;
    side = akaze_enqueue_suppress(st, S, K, A.cnt, A.tab, 1);
    *order_side = side;
    if (stage < 2) return;
    hipLaunchKernelGGL(akaze_subpixel_kernel, dim3(kb1), dim3(256), 0, st, (const AkCand*)S.cand, (const pu32*)S.keys.v[side], (pu32)K, (const AkCounters*)A.cnt,
                       (const AkTab*)A.tab, (const float*)A.lev, S.fit, S.flags.data);
    S.flags.scan(st, K + 1);
    hipLaunchKernelGGL(akaze_compact_kernel, dim3(kb), dim3(256), 0, st, (const pu32*)S.flags.data, (pu32)K, A.cnt, S.list);
}

// everything behind sfmhip_akaze_extract_dev
static int akaze_enqueue(sfmhip_ctx* ctx, const uint8_t* d_img, int rows, int cols, int ch, size_t ld, int max_features, sfm_keypoint* d_kp, uint8_t* d_desc, int cap,
                         int32_t* d_n_found)
{
    hipStream_t st = ctx->stream;
    AkPlan P;
    akaze_plan(rows, cols, cap, P);
    if (P.tab.n_levels == 0) {                                   // an image without a level has no key point
        SFM_HIP_TRY(ctx, hipMemsetAsync(d_n_found, 0, sizeof(int32_t), st));
        return SFMHIP_OK;
    }
    const size_t K = P.K;
    SfmCarve carve;
    AkAreas A; AkLists S;
    A.carve(carve, P); S.carve(carve, K);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    A.bind(w); S.bind(w);
    rc = akaze_enqueue_scale_space(ctx, P, A, d_img, rows, cols, ch, ld, nullptr, -1);
    if (rc != SFMHIP_OK) return rc;
    int side = 0;
    akaze_enqueue_detect(ctx, P, A, S, 2, &side);
    // std::stable_sort on descending response over the rows that passed the fit, in aux order
    const int kb = ceil_div((int)K, 256);
    hipLaunchKernelGGL(akaze_resp_key_kernel, dim3(kb), dim3(256), 0, st, (const AkFit*)S.fit, (const pu32*)S.list, (pu32)K, (const AkCounters*)A.cnt, S.keys.k[0]);
    SFM_HIP_TRY(ctx, hipMemcpyAsync(S.keys.v[0], S.list, K * 4, hipMemcpyDeviceToDevice, st));
    side = S.keys.sort(st, K, 0, 32, false);
    hipLaunchKernelGGL(akaze_count_kernel, dim3(1), dim3(1), 0, st, (const AkCounters*)A.cnt, max_features, d_n_found);
    if (cap > 0) {
        const int db = (int)std::min<size_t>(ceil_div(cap, 4), (size_t)ctx->num_cus * 16);
        hipLaunchKernelGGL(akaze_describe_kernel, dim3(db), dim3(256), 0, st, (const AkTab*)A.tab, (const float*)A.lev, (const AkFit*)S.fit, (const pu32*)S.keys.v[side],
                           (const int32_t*)d_n_found, cap, d_kp, d_desc);
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

static int akaze_upload_image(sfmhip_ctx* ctx, SfmPoolHold& hold, const uint8_t* img, int rows, int cols, int ch, size_t ld, uint8_t** d_img)
{
    const size_t bytes = (size_t)(rows - 1) * ld + (size_t)cols * ch;
    const int rc = hold.get(bytes, (void**)d_img);
    if (rc != SFMHIP_OK) return rc;
    return sfm_upload(ctx, *d_img, img, bytes);
}
static int akaze_overflow(sfmhip_ctx* ctx)
{
    ctx->last_error = "akaze: the list of raw maxima overflowed (it holds max(cap, 4096, pixels / 8) rows); call again with a cap above pixels / 8";
    return SFMHIP_E_ARG;
}

extern "C" {

int sfmhip_akaze_extract_dev(sfmhip_ctx* ctx, const uint8_t* d_img, int rows, int cols, int channels, size_t ld, int max_features, sfm_keypoint* d_kp, uint8_t* d_desc,
                             int cap, int32_t* d_n_found)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_akaze_extract_dev");
    SFM_ARG_CHECK(ctx, akaze_image_args_ok(d_img, rows, cols, channels, ld) && cap >= 0 && max_features >= 0);
    SFM_ARG_CHECK(ctx, ctx && d_n_found && (cap == 0 || (d_kp && d_desc)));
    return akaze_enqueue(ctx, d_img, rows, cols, channels, ld, max_features, d_kp, d_desc, cap, d_n_found);
}

int sfmhip_akaze_extract(sfmhip_ctx* ctx, const uint8_t* img, int rows, int cols, int channels, size_t ld, int max_features, sfm_keypoint* kp, uint8_t* desc, int cap,
                         int32_t* n_found)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_akaze_extract");
    SFM_ARG_CHECK(ctx, akaze_image_args_ok(img, rows, cols, channels, ld) && cap >= 0 && max_features >= 0);
    SFM_ARG_CHECK(ctx, ctx && n_found && (cap == 0 || (kp && desc)));
    SfmPoolHold hold(ctx);
    uint8_t* d_img = nullptr; sfm_keypoint* d_kp = nullptr; uint8_t* d_desc = nullptr; int32_t* d_n = nullptr;
    int rc = akaze_upload_image(ctx, hold, img, rows, cols, channels, ld, &d_img);
    if (rc == SFMHIP_OK) rc = hold.get(&d_kp, (size_t)cap);
    if (rc == SFMHIP_OK) rc = hold.get(&d_desc, (size_t)cap * 61);
    if (rc == SFMHIP_OK) rc = hold.get(&d_n, 1);
    if (rc == SFMHIP_OK) rc = akaze_enqueue(ctx, d_img, rows, cols, channels, ld, max_features, d_kp, d_desc, cap, d_n);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    int32_t n = 0;
    hipError_t e = hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && n > 0 && cap > 0) {
        const size_t m = (size_t)std::min(n, cap);
        e = hipMemcpyAsync(kp, d_kp, m * sizeof(sfm_keypoint), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(desc, d_desc, m * 61, hipMemcpyDeviceToHost, ctx->stream);
    }
    rc = sfm_finish(ctx, e);
    if (rc != SFMHIP_OK) return rc;
    if (n < 0) return akaze_overflow(ctx);
    *n_found = n;
    return SFMHIP_OK;
}

int sfmhip_akaze_scale_space(sfmhip_ctx* ctx, const uint8_t* img, int rows, int cols, int channels, size_t ld, int level, int kind, float* out, int* out_rows,
                             int* out_cols, int* n_levels, float* kcontrast)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_akaze_scale_space");
    SFM_ARG_CHECK(ctx, akaze_image_args_ok(img, rows, cols, channels, ld) && kind >= 0 && kind <= 4 && level >= 0 && level < AK_MAXL);
    SFM_ARG_CHECK(ctx, ctx != nullptr);
    AkPlan P;
    akaze_plan(rows, cols, 0, P);
    if (n_levels) *n_levels = P.tab.n_levels;
    if (!out && !kcontrast && !out_rows && !out_cols) return SFMHIP_OK;          // the number of levels alone: an image may have none
    SFM_ARG_CHECK(ctx, level < P.tab.n_levels);
    const int H = P.tab.rows[level], W = P.tab.cols[level];
    const size_t px = (size_t)H * W;
    if (out_rows) *out_rows = H;
    if (out_cols) *out_cols = W;
    if (!out && !kcontrast) return SFMHIP_OK;
    SfmCarve carve;
    AkAreas A;
    A.carve(carve, P);
    const size_t o_sm = carve(px * 4);
    SfmPoolHold hold(ctx);
    uint8_t* d_img = nullptr; char* w = nullptr;
    int rc = akaze_upload_image(ctx, hold, img, rows, cols, channels, ld, &d_img);
    if (rc == SFMHIP_OK) rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    A.bind(w);
    float* d_sm = (float*)(w + o_sm);
    rc = akaze_enqueue_scale_space(ctx, P, A, d_img, rows, cols, channels, ld, d_sm, level);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    const int which[5] = { 0, -1, 1, 2, 3 };                  // Lt, Lsmooth, Lx, Ly, Ldet
    const float* src = kind == 1 ? d_sm : A.lev + P.tab.off[level] + (size_t)which[kind] * px;
    hipError_t e = hipSuccess;
    if (out) e = hipMemcpyAsync(out, src, px * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && kcontrast) e = hipMemcpyAsync(kcontrast, &A.cnt->kc[level], sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    return sfm_finish(ctx, e);
}

int sfmhip_akaze_extrema(sfmhip_ctx* ctx, const uint8_t* img, int rows, int cols, int channels, size_t ld, int stage, float* xysr, int32_t* ol, int cap, int32_t* n_found)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_akaze_extrema");
    SFM_ARG_CHECK(ctx, akaze_image_args_ok(img, rows, cols, channels, ld) && cap >= 0 && stage >= 0 && stage <= 2);
    SFM_ARG_CHECK(ctx, ctx && n_found && (cap == 0 || (xysr && ol)));
    AkPlan P;
    akaze_plan(rows, cols, cap, P);
    if (P.tab.n_levels == 0) { *n_found = 0; return SFMHIP_OK; }
    const size_t K = P.K;
    SfmCarve carve;
    AkAreas A; AkLists S;
    A.carve(carve, P); S.carve(carve, K);
    const size_t o_xysr = carve((size_t)cap * 16), o_ol = carve((size_t)cap * 8), o_n = carve(4);
    SfmPoolHold hold(ctx);
    uint8_t* d_img = nullptr; char* w = nullptr;
    int rc = akaze_upload_image(ctx, hold, img, rows, cols, channels, ld, &d_img);
    if (rc == SFMHIP_OK) rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    A.bind(w); S.bind(w);
    hipStream_t st = ctx->stream;
    rc = akaze_enqueue_scale_space(ctx, P, A, d_img, rows, cols, channels, ld, nullptr, -1);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    int side = 0;
    akaze_enqueue_detect(ctx, P, A, S, stage, &side);
    hipLaunchKernelGGL(akaze_stage_out_kernel, dim3(ceil_div((int)K, 256)), dim3(256), 0, st, stage, (const AkCand*)S.cand, (const pu32*)S.keys.v[side], (const AkFit*)S.fit,
                       (const pu32*)S.list, (pu32)K, (const AkCounters*)A.cnt, (const AkTab*)A.tab, cap, (float*)(w + o_xysr), (int32_t*)(w + o_ol), (int32_t*)(w + o_n));
    hipError_t e = hipGetLastError();
    int32_t n = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&n, w + o_n, sizeof n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && n > 0 && cap > 0) {
        const size_t m = (size_t)std::min(n, cap);
        e = hipMemcpyAsync(xysr, w + o_xysr, m * 16, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(ol, w + o_ol, m * 8, hipMemcpyDeviceToHost, st);
    }
    rc = sfm_finish(ctx, e);
    if (rc != SFMHIP_OK) return rc;
    if (n < 0) return akaze_overflow(ctx);
    *n_found = n;
    return SFMHIP_OK;
}

int sfmhip_akaze_suppress(sfmhip_ctx* ctx, const float* xyr, const int32_t* level, int n, int32_t* kept, int32_t* n_kept)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_akaze_suppress");
    SFM_ARG_CHECK(ctx, n >= 0 && n_kept && (n == 0 || (xyr && level && kept)));
    for (int i = 0; i < n; ++i) SFM_ARG_CHECK(ctx, level[i] >= 0 && level[i] < AK_MAXL && (i == 0 || level[i] >= level[i - 1]));
    SFM_ARG_CHECK(ctx, ctx != nullptr);
    if (n == 0) { *n_kept = 0; return SFMHIP_OK; }
    const size_t K = (size_t)n;
    AkTab T;
    memset(&T, 0, sizeof T);
    akaze_fixed_tables(T);
    T.n_levels = AK_MAXL;
    SfmCarve carve;
    AkLists S;
    const size_t o_tab = carve(sizeof(AkTab)), o_cnt = carve(sizeof(AkCounters)), o_xyr = carve(K * 12), o_lvl = carve(K * 4), o_kept = carve(K * 4), o_n = carve(4);
    S.carve(carve, K);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    S.bind(w);
    hipStream_t st = ctx->stream;
    AkCounters* cnt = (AkCounters*)(w + o_cnt);
    rc = sfm_upload(ctx, w + o_tab, &T, sizeof T);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, w + o_xyr, xyr, K * 12);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, w + o_lvl, level, K * 4);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipError_t e = hipMemsetAsync(cnt, 0, sizeof(AkCounters), st);
    const int kb = ceil_div(n, 256);
    hipLaunchKernelGGL(akaze_pack_kernel, dim3(kb), dim3(256), 0, st, (const float*)(w + o_xyr), (const int32_t*)(w + o_lvl), (pu32)n, cnt, S.cand);
    const int side = akaze_enqueue_suppress(st, S, K, cnt, (const AkTab*)(w + o_tab), 0);
    hipLaunchKernelGGL(akaze_kept_out_kernel, dim3(kb), dim3(256), 0, st, (const pu32*)S.keys.v[side], (pu32)K, (const AkCounters*)cnt, (int32_t*)(w + o_kept), (int32_t*)(w + o_n));
    if (e == hipSuccess) e = hipGetLastError();
    int32_t m = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&m, w + o_n, sizeof m, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && m > 0) e = hipMemcpyAsync(kept, w + o_kept, (size_t)std::min(m, n) * 4, hipMemcpyDeviceToHost, st);
    rc = sfm_finish(ctx, e);
    if (rc != SFMHIP_OK) return rc;
    *n_kept = m;
    return SFMHIP_OK;
}

}
