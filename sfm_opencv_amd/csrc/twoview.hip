// twoview.hip -- two-view geometric verification: an epipolar RANSAC over many image pairs in one call (what colmap and OpenMVG run between
// matching and reconstruction; the reference has it for its first pair only, inside findEssentialMat).  The definition is in sfmhip.h at
// sfmhip_verify_pairs and is followed to the letter here: the mask, count and winner are integer decisions on prescribed fp64 values and F
// is prescribed bit for bit, the same for every run, batch and launch geometry.  The sampler, the scoring loop and the winner reduction
// are ransac.hpp's, as in planes.hip.
//
// A round p, everything on the device and on one stream, every kernel over all pairs at once:
//   twoview_prep_kernel     (once) one workgroup per pair: L_0, the rows with four finite values, packed in ascending row index into rows
//                           of four doubles; the state of the pair; L_0 as the list round 0 samples from
//   twoview_hyp_kernel      one thread per (pair, hypothesis): the eight rows from splitmix64, the 8 x 9 system, Gaussian elimination with
//                           complete pivoting in registers, back-substitution, F or NaN, a valid bit
//   twoview_score_kernel    the pairs x H x |L_0| part: the number of rows of L_0 every hypothesis accepts
//   twoview_winner_kernel   one workgroup per pair: the valid hypothesis with the largest count, the smallest h among equals; it becomes
//                           the pair's model, or the pair's stop flag is raised
//   twoview_list_kernel     one workgroup per pair: the model's inliers among L_0 in ascending order, the list the next round samples from
//   twoview_final_kernel    (once) mask, count, winner and F of every pair, or their "no model" values
// All rounds are enqueued; the stop flag and the list length of a pair live in device memory, and once a pair has stopped every block of
// a later round that belongs to it leaves at once.
//
// twoview_score_kernel is the scoring loop of ransac.hpp, which explains its shape, over the rows of one pair (blockIdx.z): a lane keeps
// its F in 18 VGPRs, and per row a wave issues 16 fp64 multiplications and 15 additions for l, m, e and d (contraction is off: the
// residual is the prescribed formula), two more multiplications for e*e and t2*d, a compare and a conditional add: 35 VALU
// instructions, which is what bounds the kernel (the account is in DESIGN.md 4c).
//
// TWO MODELS share this file: the fundamental matrix above (EpipolarModel) and the four-point homography of sfmhip_verify_pairs_h
// (HomographyModel), which is also the null vector of an 8 x 9 system.  A model supplies the size of its sample (also the shortest list a
// round may sample from), the rows of the system a sampled row gives, and its inlier test; the hypothesis, scoring and per-pair kernels
// (winner, list, final) are one body each over it, and prep runs once per call whatever the number of models.  homography_hyp_kernel
// differs from twoview_hyp_kernel in the sample (four rows) and the design matrix; homography_score_kernel in the residual: 12
// multiplications, 9 additions, a compare and a conditional add per row, 23 VALU instructions against 35.  sfmhip_two_view_geometry
// runs both models over the same packed rows, one after the other through the same pairs x H hypothesis areas, and
// geometry_select_kernel then decides per pair which mask is the pair's (the rule is in sfmhip.h).
//
// A THIRD MODEL, the absolute pose of sfmhip_register_views (PoseModel), runs through the same bodies on its own: a "pair" is a view, a
// row is a 3-D point and its observation, five doubles, packed into rows of six (M::Row; RowIO says how a row of the caller's block is
// read), the system is 11 x 12 and the model twelve values.  The elimination is one body over the size of the system, null_vector<R, C>,
// and its 8 x 9 instance is what F and the homography ran before.  pnp_hyp_kernel keeps 132 doubles of matrix in the 512 registers of a
// single wave per SIMD (VGPRs and AGPRs, no scratch) and applies the model's orient step, the sign rule, to the null vector;
// pnp_score_kernel is ransac_score over rows of six doubles: 15 multiplications, 12 additions, two compares and a conditional add per row,
// 30 VALU instructions.
#include "common.hpp"
#pragma clang fp contract(off)
#include "ransac.hpp"
#include "svd3.hpp"
#include "twoview_rows.hpp"               // THE residual test of F and the clamp of a block's count, shared with relpose.hip

#define HYP_THREADS 64           // hypotheses per workgroup of twoview_hyp_kernel
#define TWOVIEW_H_MAX 65536
#define TWOVIEW_ROUNDS_MAX 8
#define TWOVIEW_PAIRS_PER_LAUNCH 32768      // gridDim.z of the scoring launch; a longer batch goes in slices (the pairs are independent)

// what the rounds of one pair share, in device memory
struct TwoViewState {
    int stop;                 // raised by the round that ends the pair; every later block of the pair leaves at once
    int m;                    // |L_p|, the length of the list the current round samples from
    int m0;                   // |L_0|, the rows every round scores
    int best;                 // the model's count, -1 while there is no model
    int winner;               // g = p * H + h of the model
    int pad[3];
    double F[12];             // the model: M::NPAR values (F, the homography, or the projection matrix)
};
template <class M> __device__ __forceinline__ bool round_dead(const TwoViewState* s) { return s->stop || s->m < M::SAMPLE; }

// THE transfer test of the homography model, under the same rule: the squared forward transfer distance against t^2 with the division by
// w^2 multiplied out.  False for a NaN H.
__device__ __forceinline__ bool homography_inlier(const double (&Hm)[9], double x1, double y1, double x2, double y2, double t2)
{
    const double u = (Hm[0] * x1 + Hm[1] * y1) + Hm[2];
    const double v = (Hm[3] * x1 + Hm[4] * y1) + Hm[5];
    const double w = (Hm[6] * x1 + Hm[7] * y1) + Hm[8];
    const double du = u - x2 * w;
    const double dv = v - y2 * w;
    return du * du + dv * dv <= t2 * (w * w);
}
// THE reprojection test of the absolute-pose model, under the same rule: the squared reprojection distance against t^2 with the division by
// w^2 multiplied out, and the point in front of the camera.  False for a NaN P.
__device__ __forceinline__ bool pose_inlier(const double (&P)[12], double X, double Y, double Z, double x, double y, double t2)
{
    const double u = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
    const double v = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
    const double w = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
    const double du = u - x * w;
    const double dv = v - y * w;
    return (w > 0.0) & (du * du + dv * dv <= t2 * (w * w));           // & for &&: both compares every row, no branch in the scoring loop
}
// a packed row of the absolute-pose model: the point, its observation, and padding to three 16-byte slots
struct alignas(16) PoseRow { double X, Y, Z, x, y, pad; };
// What a model supplies to the bodies that are templates over it.  Row: a packed row; SAMPLE: the rows a hypothesis draws, which is also
// the shortest list a round may sample from; design: the rows of the (NPAR - 1) x NPAR system that sample k gives (one for F, two for the
// homography and the pose); orient: what happens to the unit null vector before it is a model (the pose's sign rule; false: invalid);
// NPAR, UNROLL and inlier: for the scoring loop of ransac.hpp
struct EpipolarModel {
    typedef double4 Row;
    static constexpr int SAMPLE = 8, NPAR = 9, UNROLL = 4;
    static __device__ __forceinline__ void design(int k, const double4& r, double (&A)[8][9])
    {
        A[k][0] = r.z * r.x; A[k][1] = r.z * r.y; A[k][2] = r.z;
        A[k][3] = r.w * r.x; A[k][4] = r.w * r.y; A[k][5] = r.w;
        A[k][6] = r.x;       A[k][7] = r.y;       A[k][8] = 1.0;
    }
    static __device__ __forceinline__ bool inlier(const double (&F)[9], const double4& r, double t2) { return twoview_inlier(F, r.x, r.y, r.z, r.w, t2); }
    static __device__ __forceinline__ bool orient(double (&)[9], const double4&) { return true; }       // the elimination fixes the sign
};
struct HomographyModel {
    typedef double4 Row;
    static constexpr int SAMPLE = 4, NPAR = 9, UNROLL = 4;
    static __device__ __forceinline__ void design(int k, const double4& r, double (&A)[8][9])
    {
        A[2 * k][0] = r.x; A[2 * k][1] = r.y; A[2 * k][2] = 1.0; A[2 * k][3] = 0.0; A[2 * k][4] = 0.0; A[2 * k][5] = 0.0;
        A[2 * k][6] = -(r.z * r.x); A[2 * k][7] = -(r.z * r.y); A[2 * k][8] = -r.z;
        A[2 * k + 1][0] = 0.0; A[2 * k + 1][1] = 0.0; A[2 * k + 1][2] = 0.0; A[2 * k + 1][3] = r.x; A[2 * k + 1][4] = r.y; A[2 * k + 1][5] = 1.0;
        A[2 * k + 1][6] = -(r.w * r.x); A[2 * k + 1][7] = -(r.w * r.y); A[2 * k + 1][8] = -r.w;
    }
    static __device__ __forceinline__ bool inlier(const double (&Hm)[9], const double4& r, double t2) { return homography_inlier(Hm, r.x, r.y, r.z, r.w, t2); }
    static __device__ __forceinline__ bool orient(double (&)[9], const double4&) { return true; }
};
// The six-point DLT of sfmhip_register_views: two rows of the 11 x 12 system per sampled row (the twelfth is left out), the sign rule as
// the model's orient step, and the reprojection test with the point in front of the camera
struct PoseModel {
    typedef PoseRow Row;
    static constexpr int SAMPLE = 6, NPAR = 12, UNROLL = 4;
    static __device__ __forceinline__ void design(int k, const PoseRow& r, double (&A)[11][12])
    {
        A[2 * k][0] = r.X; A[2 * k][1] = r.Y; A[2 * k][2] = r.Z; A[2 * k][3] = 1.0; A[2 * k][4] = 0.0; A[2 * k][5] = 0.0; A[2 * k][6] = 0.0; A[2 * k][7] = 0.0;
        A[2 * k][8] = -(r.x * r.X); A[2 * k][9] = -(r.x * r.Y); A[2 * k][10] = -(r.x * r.Z); A[2 * k][11] = -r.x;
        if (2 * k + 1 < 11) {                                            // row 11 is left out; k is a constant wherever this is called, and the clamp below only keeps the instance k = 5 inside the array for the compiler
            double (&B)[12] = A[2 * k + 1 < 11 ? 2 * k + 1 : 0];
            B[0] = 0.0; B[1] = 0.0; B[2] = 0.0; B[3] = 0.0; B[4] = r.X; B[5] = r.Y; B[6] = r.Z; B[7] = 1.0;
            B[8] = -(r.y * r.X); B[9] = -(r.y * r.Y); B[10] = -(r.y * r.Z); B[11] = -r.y;
        }
    }
    static __device__ __forceinline__ bool inlier(const double (&P)[12], const PoseRow& r, double t2) { return pose_inlier(P, r.X, r.Y, r.Z, r.x, r.y, t2); }
    // step 7: the depth of sample row 0 decides the sign of P; false where it decides nothing
    static __device__ __forceinline__ bool orient(double (&P)[12], const PoseRow& r)
    {
        const double w0 = ((P[8] * r.X + P[9] * r.Y) + P[10] * r.Z) + P[11];
#pragma unroll
        for (int j = 0; j < 12; ++j) P[j] = w0 < 0.0 ? -P[j] : P[j];
        return w0 != 0.0 && isfinite(w0);
    }
};
// how the bodies that are one over the row type read a row of the caller's block: its NCOL doubles, and whether all of them are finite
template <class Row> struct RowIO;
template <> struct RowIO<double4> {
    static constexpr int NCOL = 4;
    static __device__ __forceinline__ double4 load(const double* p) { return make_double4(p[0], p[1], p[2], p[3]); }
    static __device__ __forceinline__ bool finite(const double4& r) { return isfinite(r.x) && isfinite(r.y) && isfinite(r.z) && isfinite(r.w); }
};
template <> struct RowIO<PoseRow> {
    static constexpr int NCOL = 5;
    static __device__ __forceinline__ PoseRow load(const double* p) { return PoseRow{ p[0], p[1], p[2], p[3], p[4], 0.0 }; }
    static __device__ __forceinline__ bool finite(const PoseRow& r) { return isfinite(r.X) && isfinite(r.Y) && isfinite(r.Z) && isfinite(r.x) && isfinite(r.y); }
};

// ordered compaction inside a workgroup of 256 threads: the number of flagged threads below this one, and how many there are in all.
// Every thread of the workgroup calls it; sw: four ints of LDS.
__device__ __forceinline__ int block_rank(bool f, int* sw, int& total)
{
    const pu64 b = __ballot(f);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                                     // the previous call's readers are done with sw
    if (lane == 0) sw[wave] = __popcll(b);
    __syncthreads();
    int below = __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) below += sw[w];
    total = (sw[0] + sw[1]) + (sw[2] + sw[3]);
    return below;
}

// one workgroup per pair: L_0 packed into act, the identity as the list of round 0, the state; state2 / list2: the same for a second
// model that runs over the same rows, or null
template <class Row>
__device__ __forceinline__ void prep_rows(const double* __restrict__ corr, int stride, const int32_t* __restrict__ counts, TwoViewState* __restrict__ state,
                                          Row* __restrict__ act, int32_t* __restrict__ list, TwoViewState* __restrict__ state2, int32_t* __restrict__ list2)
{
    __shared__ int sw[4];
    const size_t q = blockIdx.x;
    const int cnt = clamp_count(counts[q], stride);
    const double* rows = corr + RowIO<Row>::NCOL * (size_t)stride * q;
    int m = 0;
    for (int base = 0; base < cnt; base += 256) {
        const int i = base + (int)threadIdx.x;
        Row row = {};
        bool f = false;
        if (i < cnt) {
            row = RowIO<Row>::load(rows + RowIO<Row>::NCOL * (size_t)i);
            f = RowIO<Row>::finite(row);
        }
        int total;
        const int r = block_rank(f, sw, total);
        if (f) {
            act[q * stride + m + r] = row; list[q * stride + m + r] = m + r;
            if (list2) list2[q * stride + m + r] = m + r;
        }
        m += total;
    }
    if (threadIdx.x == 0) {
        TwoViewState* s = state + q;
        s->stop = 0; s->m = m; s->m0 = m; s->best = -1; s->winner = -1;
        if (state2) { s = state2 + q; s->stop = 0; s->m = m; s->m0 = m; s->best = -1; s->winner = -1; }
    }
}
__global__ __launch_bounds__(256) void twoview_prep_kernel(const double* __restrict__ corr, int stride, const int32_t* __restrict__ counts,
                                                           TwoViewState* __restrict__ state, double4* __restrict__ act, int32_t* __restrict__ list,
                                                           TwoViewState* __restrict__ state2, int32_t* __restrict__ list2)
{
    prep_rows<double4>(corr, stride, counts, state, act, list, state2, list2);
}
__global__ __launch_bounds__(256) void pnp_prep_kernel(const double* __restrict__ corr, int stride, const int32_t* __restrict__ counts,
                                                       TwoViewState* __restrict__ state, PoseRow* __restrict__ act, int32_t* __restrict__ list)
{
    prep_rows<PoseRow>(corr, stride, counts, state, act, list, nullptr, nullptr);
}

// The sampling-free part of a hypothesis, steps 2 to 6 of the definition: the unit null vector of the system A and its valid bit.
// The matrix stays in registers: every loop is unrolled, so every index is a constant, and the one thing the pivoting decides at
// run time, which row and which column trade places, is done with selects over the candidates (SWAP_IF).  The same values move as in an
// indexed swap, so the arithmetic is the prescribed one.  (With the matrix in LDS and indexed by the pivot the kernel waited on one
// dependent LDS access after another: 179 us for 199 x 1024 hypotheses against the figure in DESIGN.md 4c for this form.)
#define SWAP_IF(c, a, b) { const double ta_ = (a), tb_ = (b); (a) = (c) ? tb_ : ta_; (b) = (c) ? ta_ : tb_; }
// (the system is R x C with C = R + 1: 8 x 9 for F and the homography, 11 x 12 for the projection matrix; f: the unit null vector; the
// value is the valid bit)
template <int R, int C>
__device__ __forceinline__ bool null_vector(double (&A)[R][C], double (&f)[C])
{
    int perm[C];
#pragma unroll
    for (int j = 0; j < C; ++j) perm[j] = j;
    bool valid = true;                                                   // an invalid hypothesis goes on computing values nobody uses
#pragma unroll
    for (int k = 0; k < R; ++k) {
        int at = k * C + k;
        double best = -1.0;
#pragma unroll
        for (int i = k; i < R; ++i)
#pragma unroll
            for (int j = k; j < C; ++j) {
                const double v = fabs(A[i][j]);
                const bool gt = v > best;                                 // the first maximum; never true for a NaN
                best = gt ? v : best; at = gt ? i * C + j : at;
            }
        const int pi = at / C, pj = at - C * pi;
        // rows k and pi (the columns below k of the rows from k on are never read again), then columns k and pj in every row
#pragma unroll
        for (int i = k + 1; i < R; ++i)
#pragma unroll
            for (int j = k; j < C; ++j) SWAP_IF(pi == i, A[k][j], A[i][j]);
#pragma unroll
        for (int c = k + 1; c < C; ++c) {
#pragma unroll
            for (int i = 0; i < R; ++i) SWAP_IF(pj == c, A[i][k], A[i][c]);
            const int a = perm[k], b = perm[c];
            perm[k] = pj == c ? b : a; perm[c] = pj == c ? a : b;
        }
        const double piv = A[k][k];
        valid = valid && piv != 0.0 && isfinite(piv);
#pragma unroll
        for (int i = k + 1; i < R; ++i) {
            const double f = A[i][k] / piv;
#pragma unroll
            for (int j = k + 1; j < C; ++j) A[i][j] = A[i][j] - f * A[k][j];
        }
    }
    double z[C];
    z[C - 1] = 1.0;
#pragma unroll
    for (int k = R - 1; k >= 0; --k) {
        double sum = A[k][k + 1] * z[k + 1];
#pragma unroll
        for (int j = k + 2; j < C; ++j) sum = sum + A[k][j] * z[j];
        z[k] = -sum / A[k][k];
    }
#pragma unroll
    for (int j = 0; j < C; ++j) {                                        // f[perm[k]] = z[k]
        f[j] = 0.0;
#pragma unroll
        for (int k = 0; k < C; ++k) f[j] = perm[k] == j ? z[k] : f[j];
    }
    double ss = f[0] * f[0];
#pragma unroll
    for (int j = 1; j < C; ++j) ss = ss + f[j] * f[j];
    const double nrm = sqrt(ss);
#pragma unroll
    for (int j = 0; j < C; ++j) f[j] = f[j] / nrm;
    return valid && isfinite(nrm) && nrm > 0.0;
}
#undef SWAP_IF

// hypothesis h of round p of pair q: hyp[NPAR (q H + h) ..] = the model from M::SAMPLE distinct rows of L_p, NaN where it is invalid (it
// then counts nobody); its valid bit; its counter cleared
template <class M>
__device__ __forceinline__ void hypothesis(const typename M::Row* __restrict__ act, const int32_t* __restrict__ list, int stride,
                                           const TwoViewState* __restrict__ state, int p, int H, pu64 seed, double* __restrict__ hyp,
                                           int32_t* __restrict__ hvalid, int32_t* __restrict__ hcnt)
{
    const size_t q = blockIdx.y;
    const TwoViewState* s = state + q;
    if (round_dead<M>(s)) return;
    const int h = blockIdx.x * HYP_THREADS + threadIdx.x;
    if (h >= H) return;
    pu64 u[M::SAMPLE];
    ransac_sample_distinct<M::SAMPLE>(seed, (pu64)p * (pu64)H + (pu64)h, (pu64)s->m, u);
    double A[M::NPAR - 1][M::NPAR];
#pragma unroll
    for (int k = 0; k < M::SAMPLE; ++k) M::design(k, act[q * stride + (size_t)list[q * stride + u[k]]], A);
    const size_t first = q * stride + (size_t)list[q * stride + u[0]];  // sample row 0 is read again behind the elimination, not kept through it
    double f[M::NPAR];
    bool valid = null_vector(A, f);
    valid = M::orient(f, act[first]) && valid;
    const size_t at = q * (size_t)H + (size_t)h;
#pragma unroll
    for (int j = 0; j < M::NPAR; ++j) hyp[M::NPAR * at + j] = valid ? f[j] : NAN;
    hvalid[at] = valid ? 1 : 0;
    hcnt[at] = 0;
}
__global__ __launch_bounds__(HYP_THREADS) void twoview_hyp_kernel(const double4* __restrict__ act, const int32_t* __restrict__ list, int stride,
                                                                  const TwoViewState* __restrict__ state, int p, int H, pu64 seed,
                                                                  double* __restrict__ hyp, int32_t* __restrict__ hvalid, int32_t* __restrict__ hcnt)
{
    hypothesis<EpipolarModel>(act, list, stride, state, p, H, seed, hyp, hvalid, hcnt);
}
__global__ __launch_bounds__(HYP_THREADS) void homography_hyp_kernel(const double4* __restrict__ act, const int32_t* __restrict__ list, int stride,
                                                                     const TwoViewState* __restrict__ state, int p, int H, pu64 seed,
                                                                     double* __restrict__ hyp, int32_t* __restrict__ hvalid, int32_t* __restrict__ hcnt)
{
    hypothesis<HomographyModel>(act, list, stride, state, p, H, seed, hyp, hvalid, hcnt);
}
// one wave per SIMD: the 11 x 12 matrix is 264 registers and lives in VGPRs and AGPRs together
__global__ __launch_bounds__(HYP_THREADS) void pnp_hyp_kernel(const PoseRow* __restrict__ act, const int32_t* __restrict__ list, int stride,
                                                              const TwoViewState* __restrict__ state, int p, int H, pu64 seed,
                                                              double* __restrict__ hyp, int32_t* __restrict__ hvalid, int32_t* __restrict__ hcnt)
{
    hypothesis<PoseModel>(act, list, stride, state, p, H, seed, hyp, hvalid, hcnt);
}

// the pairs x H x |L_0| part: ransac_score over the rows of pair blockIdx.z
template <class M>
__device__ __forceinline__ void score_pair(typename M::Row* tile, const typename M::Row* __restrict__ act, int stride, const TwoViewState* __restrict__ state,
                                           const double* __restrict__ hyp, int H, double t2, int32_t* __restrict__ hcnt)
{
    const size_t q = blockIdx.z;
    const TwoViewState* s = state + q;
    if (round_dead<M>(s)) return;                                        // uniform over the workgroup
    const int h = blockIdx.x * 256 + threadIdx.x;
    const size_t at = q * (size_t)H + (size_t)h;
    ransac_score<M>(tile, act + q * stride, s->m0, h < H ? hyp + M::NPAR * at : nullptr, t2, hcnt + at);
}
__global__ __launch_bounds__(256) void twoview_score_kernel(const double4* __restrict__ act, int stride, const TwoViewState* __restrict__ state,
                                                            const double* __restrict__ hyp, int H, double t2, int32_t* __restrict__ hcnt)
{
    __shared__ double4 tile[SCORE_CHUNK];
    score_pair<EpipolarModel>(tile, act, stride, state, hyp, H, t2, hcnt);
}
__global__ __launch_bounds__(256) void homography_score_kernel(const double4* __restrict__ act, int stride, const TwoViewState* __restrict__ state,
                                                               const double* __restrict__ hyp, int H, double t2, int32_t* __restrict__ hcnt)
{
    __shared__ double4 tile[SCORE_CHUNK];
    score_pair<HomographyModel>(tile, act, stride, state, hyp, H, t2, hcnt);
}
__global__ __launch_bounds__(256) void pnp_score_kernel(const PoseRow* __restrict__ act, int stride, const TwoViewState* __restrict__ state,
                                                        const double* __restrict__ hyp, int H, double t2, int32_t* __restrict__ hcnt)
{
    __shared__ PoseRow tile[SCORE_CHUNK];
    score_pair<PoseModel>(tile, act, stride, state, hyp, H, t2, hcnt);
}
// the two kernels above of a model, for the host
template <class M> struct KernelsOf;
template <> struct KernelsOf<EpipolarModel> { static constexpr auto hyp = twoview_hyp_kernel; static constexpr auto score = twoview_score_kernel; };
template <> struct KernelsOf<HomographyModel> { static constexpr auto hyp = homography_hyp_kernel; static constexpr auto score = homography_score_kernel; };
template <> struct KernelsOf<PoseModel> { static constexpr auto hyp = pnp_hyp_kernel; static constexpr auto score = pnp_score_kernel; };

// one workgroup per pair: argmax of (count, then the smallest h) over the valid hypotheses; the pair's model, or its stop flag
template <class M>
__global__ __launch_bounds__(256) void twoview_winner_kernel(TwoViewState* __restrict__ state, int p, int H, const double* __restrict__ hyp,
                                                             const int32_t* __restrict__ hvalid, const int32_t* __restrict__ hcnt)
{
    __shared__ pu64 sb[256];
    const size_t q = blockIdx.x;
    TwoViewState* s = state + q;
    const int stop = s->stop, m = s->m;
    __syncthreads();                                                     // everybody has read the state before thread 0 may change it
    if (stop) return;
    if (m < M::SAMPLE) { if (threadIdx.x == 0) s->stop = 1; return; }
    const pu64 w = ransac_block_winner(hvalid + q * (size_t)H, hcnt + q * (size_t)H, H, sb);
    if (threadIdx.x != 0) return;
    if (!w) { s->stop = 1; return; }
    const int cnt = ransac_key_count(w), h = ransac_key_h(w);
    if (p > 0 && cnt <= s->best) { s->stop = 1; return; }
    s->best = cnt;
    s->winner = p * H + h;
    for (int j = 0; j < M::NPAR; ++j) s->F[j] = hyp[M::NPAR * (q * (size_t)H + h) + j];
}

// one workgroup per pair: L_{p+1}, the positions in L_0 of the model's inliers, ascending
template <class M>
__global__ __launch_bounds__(256) void twoview_list_kernel(const typename M::Row* __restrict__ act, int stride, TwoViewState* __restrict__ state, double t2,
                                                           int32_t* __restrict__ list)
{
    __shared__ int sw[4];
    const size_t q = blockIdx.x;
    TwoViewState* s = state + q;
    if (s->stop) return;
    const int m0 = s->m0;
    double F[M::NPAR];
#pragma unroll
    for (int j = 0; j < M::NPAR; ++j) F[j] = s->F[j];
    int m = 0;
    for (int base = 0; base < m0; base += 256) {
        const int i = base + (int)threadIdx.x;
        bool f = false;
        if (i < m0) f = M::inlier(F, act[q * stride + i], t2);
        int total;
        const int r = block_rank(f, sw, total);
        if (f) list[q * stride + m + r] = i;
        m += total;
    }
    if (threadIdx.x == 0) s->m = m;
}

// the outputs of pair blockIdx.y for one model; F_out / winner may be null
template <class M>
__global__ __launch_bounds__(256) void twoview_final_kernel(const double* __restrict__ corr, int stride, const int32_t* __restrict__ counts,
                                                            const TwoViewState* __restrict__ state, double t2, int min_inliers,
                                                            uint8_t* __restrict__ mask, int32_t* __restrict__ count_out, double* __restrict__ F_out,
                                                            int32_t* __restrict__ winner)
{
    const size_t q = blockIdx.y;
    const TwoViewState* s = state + q;
    const bool ok = s->best >= min_inliers;
    double F[M::NPAR];
#pragma unroll
    for (int j = 0; j < M::NPAR; ++j) F[j] = ok ? s->F[j] : NAN;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) { count_out[q] = ok ? s->best : 0; if (winner) winner[q] = ok ? s->winner : -1; }
        if (threadIdx.x < M::NPAR && F_out) F_out[M::NPAR * q + threadIdx.x] = F[threadIdx.x];
    }
    if (i >= stride) return;
    bool in = false;
    if (ok && i < clamp_count(counts[q], stride)) {
        const typename M::Row r = RowIO<typename M::Row>::load(corr + RowIO<typename M::Row>::NCOL * ((size_t)stride * q + (size_t)i));
        in = RowIO<typename M::Row>::finite(r) && M::inlier(F, r, t2);
    }
    mask[q * stride + i] = in ? 1 : 0;
}

// the model selection of sfmhip_two_view_geometry for pair blockIdx.y: kind from the two counts, the selected mask, and both models' counts
// and winners side by side; counts2 / winners may be null
__global__ __launch_bounds__(256) void geometry_select_kernel(int stride, const int32_t* __restrict__ cF, const int32_t* __restrict__ cH,
                                                              const int32_t* __restrict__ wF, const int32_t* __restrict__ wH,
                                                              const uint8_t* __restrict__ maskF, const uint8_t* __restrict__ maskH, double hf_ratio,
                                                              int32_t* __restrict__ kind, uint8_t* __restrict__ mask, int32_t* __restrict__ count_out,
                                                              int32_t* __restrict__ counts2, int32_t* __restrict__ winners)
{
    const size_t q = blockIdx.y;
    const int nf = cF[q], nh = cH[q];
    const int k = (nf == 0 && nh == 0) ? 0 : (nh > 0 && (double)nh >= hf_ratio * (double)nf) ? 2 : 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        kind[q] = k;
        count_out[q] = k == 2 ? nh : k == 1 ? nf : 0;
        if (counts2) { counts2[2 * q] = nf; counts2[2 * q + 1] = nh; }
        if (winners) { winners[2 * q] = wF[q]; winners[2 * q + 1] = wH[q]; }
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= stride) return;
    mask[q * stride + i] = k == 2 ? maskH[q * stride + i] : k == 1 ? maskF[q * stride + i] : 0;
}

// ---- match lists: key points through sfm_dmatch into rows, and the surviving elements back out ------------------------------------------
struct TwoViewKp { const sfm_keypoint* a; const sfm_keypoint* b; };

__global__ __launch_bounds__(256) void twoview_gather_kernel(const TwoViewKp* __restrict__ kp, const sfm_dmatch* __restrict__ matches, int max_per_pair,
                                                             const int32_t* __restrict__ counts, double fx, double fy, double cx, double cy,
                                                             double* __restrict__ corr)
{
    const size_t q = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= clamp_count(counts[q], max_per_pair)) return;
    const sfm_dmatch mm = matches[q * max_per_pair + i];
    double x1 = NAN, y1 = NAN, x2 = NAN, y2 = NAN;                        // an element without a partner: a row that is never sampled nor kept
    if (mm.queryIdx >= 0 && mm.trainIdx >= 0) {
        const sfm_keypoint a = kp[q].a[mm.queryIdx], b = kp[q].b[mm.trainIdx];
        x1 = ((double)a.x - cx) / fx; y1 = ((double)a.y - cy) / fy;
        x2 = ((double)b.x - cx) / fx; y2 = ((double)b.y - cy) / fy;
    }
    double* r = corr + 4 * (q * max_per_pair + i);
    r[0] = x1; r[1] = y1; r[2] = x2; r[3] = y2;
}

// one workgroup per pair: the elements whose mask is set, in their order
__global__ __launch_bounds__(256) void twoview_compact_kernel(const sfm_dmatch* __restrict__ matches, int max_per_pair, const int32_t* __restrict__ counts,
                                                              const uint8_t* __restrict__ mask, sfm_dmatch* __restrict__ out)
{
    __shared__ int sw[4];
    const size_t q = blockIdx.x;
    const int cnt = clamp_count(counts[q], max_per_pair);
    int m = 0;
    for (int base = 0; base < cnt; base += 256) {
        const int i = base + (int)threadIdx.x;
        const bool f = i < cnt && mask[q * max_per_pair + i];
        sfm_dmatch mm = { 0, 0, 0, 0.f };
        if (f) mm = matches[q * max_per_pair + i];
        int total;
        const int r = block_rank(f, sw, total);
        if (f) out[q * max_per_pair + m + r] = mm;
        m += total;
    }
}

// what a call computes, and where its outputs go
enum { GEOM_F = 1, GEOM_H = 2, GEOM_BOTH = 3, GEOM_P = 4 };      // GEOM_P: the absolute pose of sfmhip_register_views, alone, on rows of five
static inline size_t geom_ncol(int models) { return models == GEOM_P ? 5 : 4; }        // doubles in a row of the caller's block
static inline size_t geom_npar(int models) { return models == GEOM_P ? 12 : 9; }       // doubles in a model
struct GeomOut {
    uint8_t* mask; int32_t* count;           // the model's (GEOM_F, GEOM_H, GEOM_P) or the selected one's (GEOM_BOTH)
    double* F; int32_t* winF;                // may be null; GEOM_P: P (twelve values per view) and its winner, with t_f as the threshold
    double* Hm; int32_t* winH;               // may be null
    int32_t* kind; int32_t* counts2; int32_t* winners;      // GEOM_BOTH only; counts2, winners (n x 2 each) may be null
};
static GeomOut geom_out_at(const GeomOut& o, int models, size_t q0, size_t stride)
{
    GeomOut r = o;
    r.mask = o.mask + stride * q0; r.count = o.count + q0;
    if (o.F) r.F = o.F + geom_npar(models) * q0;
    if (o.winF) r.winF = o.winF + q0;
    if (o.Hm) r.Hm = o.Hm + 9 * q0;
    if (o.winH) r.winH = o.winH + q0;
    if (o.kind) r.kind = o.kind + q0;
    if (o.counts2) r.counts2 = o.counts2 + 2 * q0;
    if (o.winners) r.winners = o.winners + 2 * q0;
    return r;
}
struct GeomParams { double t_f, t_h; int H, rounds; pu64 seed; int min_inliers; double hf_ratio; };

// the scratch areas the rounds of one model work in
struct RoundAreas { TwoViewState* state; void* act; int32_t* list; double* hyp; int32_t *hvalid, *hcnt; };

// every round of one model over n_pairs pairs, then its final kernel
template <class M>
static void enqueue_model(hipStream_t st, const RoundAreas& a, const double* d_corr, int stride, const int32_t* d_counts, int n_pairs, double t,
                          const GeomParams& g, uint8_t* d_mask, int32_t* d_count_out, double* d_model, int32_t* d_winner)
{
    const int H = g.H, hb = ceil_div(H, 256), gy = ransac_score_grid_y(stride, hb);
    const double t2 = t * t;
    for (int p = 0; p < g.rounds; ++p) {
        hipLaunchKernelGGL(KernelsOf<M>::hyp, dim3(ceil_div(H, HYP_THREADS), n_pairs), dim3(HYP_THREADS), 0, st,
                           (const typename M::Row*)a.act, (const int32_t*)a.list, stride, (const TwoViewState*)a.state, p, H, g.seed, a.hyp, a.hvalid, a.hcnt);
        hipLaunchKernelGGL(KernelsOf<M>::score, dim3(hb, gy, n_pairs), dim3(256), 0, st, (const typename M::Row*)a.act, stride,
                           (const TwoViewState*)a.state, (const double*)a.hyp, H, t2, a.hcnt);
        hipLaunchKernelGGL(twoview_winner_kernel<M>, dim3(n_pairs), dim3(256), 0, st, a.state, p, H, (const double*)a.hyp, (const int32_t*)a.hvalid,
                           (const int32_t*)a.hcnt);
        if (p + 1 < g.rounds)
            hipLaunchKernelGGL(twoview_list_kernel<M>, dim3(n_pairs), dim3(256), 0, st, (const typename M::Row*)a.act, stride, a.state, t2, a.list);
    }
    hipLaunchKernelGGL(twoview_final_kernel<M>, dim3(std::max(1, ceil_div(stride, 256)), n_pairs), dim3(256), 0, st, d_corr, stride, d_counts,
                       (const TwoViewState*)a.state, t2, g.min_inliers, d_mask, d_count_out, d_model, d_winner);
}

// up to TWOVIEW_PAIRS_PER_LAUNCH pairs on the context's stream: prep once, then the model(s), then (GEOM_BOTH) the selection.  The two
// models of GEOM_BOTH have a state and a list each and share the packed rows and the pairs x H hypothesis, valid and counter areas.
static int twoview_enqueue_slice(sfmhip_ctx* ctx, int models, const double* d_corr, int stride, const int32_t* d_counts, int n_pairs, const GeomParams& g,
                                 const GeomOut& o)
{
    hipStream_t st = ctx->stream;
    const size_t P = (size_t)n_pairs, S = (size_t)stride, H = (size_t)g.H;
    const bool both = models == GEOM_BOTH;
    SfmCarve carve;
    const size_t o_state = carve(P * sizeof(TwoViewState)), o_act = carve(P * S * (models == GEOM_P ? sizeof(PoseRow) : sizeof(double4))), o_list = carve(P * S * 4),
                 o_hyp = carve(P * H * geom_npar(models) * sizeof(double)), o_val = carve(P * H * 4), o_cnt = carve(P * H * 4);
    const size_t o_state2 = carve(both ? P * sizeof(TwoViewState) : 0), o_list2 = carve(both ? P * S * 4 : 0), o_maskF = carve(both ? P * S : 0),
                 o_maskH = carve(both ? P * S : 0), o_head = carve(both ? 4 * align256(P * 4) : 0);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    RoundAreas a = { (TwoViewState*)(w + o_state), w + o_act, (int32_t*)(w + o_list), (double*)(w + o_hyp), (int32_t*)(w + o_val),
                     (int32_t*)(w + o_cnt) };
    RoundAreas a2 = a;
    a2.state = (TwoViewState*)(w + o_state2); a2.list = (int32_t*)(w + o_list2);
    if (models == GEOM_P) {
        hipLaunchKernelGGL(pnp_prep_kernel, dim3(n_pairs), dim3(256), 0, st, d_corr, stride, d_counts, a.state, (PoseRow*)a.act, a.list);
        enqueue_model<PoseModel>(st, a, d_corr, stride, d_counts, n_pairs, g.t_f, g, o.mask, o.count, o.F, o.winF);
        SFM_HIP_TRY(ctx, hipGetLastError());
        return SFMHIP_OK;
    }
    hipLaunchKernelGGL(twoview_prep_kernel, dim3(n_pairs), dim3(256), 0, st, d_corr, stride, d_counts, a.state, (double4*)a.act, a.list,
                       both ? a2.state : (TwoViewState*)nullptr, both ? a2.list : (int32_t*)nullptr);
    if (models == GEOM_F)
        enqueue_model<EpipolarModel>(st, a, d_corr, stride, d_counts, n_pairs, g.t_f, g, o.mask, o.count, o.F, o.winF);
    else if (models == GEOM_H)
        enqueue_model<HomographyModel>(st, a, d_corr, stride, d_counts, n_pairs, g.t_h, g, o.mask, o.count, o.Hm, o.winH);
    else {
        uint8_t *maskF = (uint8_t*)(w + o_maskF), *maskH = (uint8_t*)(w + o_maskH);
        int32_t *cF = (int32_t*)(w + o_head), *cH = (int32_t*)(w + o_head + align256(P * 4)), *wF = (int32_t*)(w + o_head + 2 * align256(P * 4)),
                *wH = (int32_t*)(w + o_head + 3 * align256(P * 4));
        enqueue_model<EpipolarModel>(st, a, d_corr, stride, d_counts, n_pairs, g.t_f, g, maskF, cF, o.F, wF);
        enqueue_model<HomographyModel>(st, a2, d_corr, stride, d_counts, n_pairs, g.t_h, g, maskH, cH, o.Hm, wH);
        hipLaunchKernelGGL(geometry_select_kernel, dim3(std::max(1, ceil_div(stride, 256)), n_pairs), dim3(256), 0, st, stride, (const int32_t*)cF,
                           (const int32_t*)cH, (const int32_t*)wF, (const int32_t*)wH, (const uint8_t*)maskF, (const uint8_t*)maskH, g.hf_ratio, o.kind,
                           o.mask, o.count, o.counts2, o.winners);
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

static int twoview_enqueue(sfmhip_ctx* ctx, int models, const double* d_corr, int stride, const int32_t* d_counts, int n_pairs, const GeomParams& g,
                           const GeomOut& o)
{
    for (int q0 = 0; q0 < n_pairs; q0 += TWOVIEW_PAIRS_PER_LAUNCH) {
        const int rc = twoview_enqueue_slice(ctx, models, d_corr + geom_ncol(models) * (size_t)stride * q0, stride, d_counts + q0, std::min(TWOVIEW_PAIRS_PER_LAUNCH, n_pairs - q0),
                                             g, geom_out_at(o, models, (size_t)q0, (size_t)stride));
        if (rc != SFMHIP_OK) return rc;
    }
    return SFMHIP_OK;
}

static inline bool thr_ok(double t) { return std::isfinite(t) && t >= 0.0; }
static inline bool twoview_args_ok(const sfmhip_ctx* ctx, int models, int stride, int n_pairs, const GeomParams& g)
{
    return ctx && stride >= 0 && n_pairs >= 0 && (!(models & (GEOM_F | GEOM_P)) || thr_ok(g.t_f)) && (!(models & GEOM_H) || thr_ok(g.t_h)) &&
           g.H >= 1 && g.H <= TWOVIEW_H_MAX && g.rounds >= 1 && g.rounds <= TWOVIEW_ROUNDS_MAX &&
           g.min_inliers >= (models == GEOM_H ? 4 : models == GEOM_P ? 6 : 8) &&
           (models != GEOM_BOTH || (std::isfinite(g.hf_ratio) && g.hf_ratio > 0.0));
}

// the device form of all four calls
static int geometry_dev(sfmhip_ctx* ctx, int models, const double* d_corr, int stride, const int32_t* d_counts, int n_pairs, const GeomParams& g,
                        const GeomOut& o)
{
    SFM_ARG_CHECK(ctx, twoview_args_ok(ctx, models, stride, n_pairs, g));
    if (n_pairs == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, (d_corr || stride == 0) && d_counts && (o.mask || stride == 0) && o.count && (models != GEOM_BOTH || o.kind));
    return twoview_enqueue(ctx, models, d_corr, stride, d_counts, n_pairs, g, o);
}

// the host form of all four calls: blocks and counts up, the outputs the caller wants back.  o holds HOST pointers.
static int geometry_host(sfmhip_ctx* ctx, int models, const double* corr, int stride, const int32_t* counts, int n_pairs, const GeomParams& g, const GeomOut& o)
{
    SFM_ARG_CHECK(ctx, twoview_args_ok(ctx, models, stride, n_pairs, g));
    if (n_pairs == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, (corr || stride == 0) && counts && (o.mask || stride == 0) && o.count && (models != GEOM_BOTH || o.kind));
    const size_t P = (size_t)n_pairs, S = (size_t)stride, ncol = geom_ncol(models), npar = geom_npar(models);
    SfmPoolHold hold(ctx);
    double* d_corr = nullptr; int32_t* d_counts = nullptr; uint8_t* d_mask = nullptr; char* d_head = nullptr;
    // count, then winner F, winner H, kind, counts2, winners, F, Hm
    const size_t i4 = align256(P * 4), i8 = align256(P * 8), d9 = align256(P * npar * sizeof(double));
    const size_t o_wf = i4, o_wh = o_wf + i4, o_kind = o_wh + i4, o_c2 = o_kind + i4, o_w2 = o_c2 + i8, o_F = o_w2 + i8, o_Hm = o_F + d9, head_bytes = o_Hm + d9;
    int rc = hold.get(&d_corr, P * S * ncol);
    if (rc == SFMHIP_OK && S) rc = sfm_upload(ctx, d_corr, corr, P * S * ncol * sizeof(double));
    if (rc == SFMHIP_OK) rc = sfm_upload_async(ctx, hold, counts, P, d_counts);
    if (rc == SFMHIP_OK) rc = hold.get(&d_mask, P * S);
    if (rc == SFMHIP_OK) rc = hold.get(head_bytes, (void**)&d_head);
    GeomOut d = { d_mask, (int32_t*)d_head, o.F ? (double*)(d_head + o_F) : nullptr, o.winF ? (int32_t*)(d_head + o_wf) : nullptr,
                  o.Hm ? (double*)(d_head + o_Hm) : nullptr, o.winH ? (int32_t*)(d_head + o_wh) : nullptr, o.kind ? (int32_t*)(d_head + o_kind) : nullptr,
                  o.counts2 ? (int32_t*)(d_head + o_c2) : nullptr, o.winners ? (int32_t*)(d_head + o_w2) : nullptr };
    if (rc == SFMHIP_OK) rc = twoview_enqueue(ctx, models, d_corr, stride, d_counts, n_pairs, g, d);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    auto back = [&](void* dst, const void* src, size_t bytes) { if (e == hipSuccess && dst && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); };
    back(o.mask, d.mask, P * S);
    back(o.count, d.count, P * 4);
    back(o.F, d.F, P * npar * sizeof(double));
    back(o.winF, d.winF, P * 4);
    back(o.Hm, d.Hm, P * 9 * sizeof(double));
    back(o.winH, d.winH, P * 4);
    back(o.kind, d.kind, P * 4);
    back(o.counts2, d.counts2, P * 8);
    back(o.winners, d.winners, P * 8);
    return sfm_finish(ctx, e);
}

// the match-list form: gather through K4, the model(s), the ordered compaction of the resulting mask
static int geometry_matches_dev(sfmhip_ctx* ctx, int models, const sfm_keypoint* const* d_kp, int n_sets, const int32_t* pairs, int n_pairs, const double K4[4],
                                const sfm_dmatch* d_matches, int max_per_pair, const int32_t* d_counts, const GeomParams& g, sfm_dmatch* d_matches_out,
                                GeomOut o)
{
    SFM_ARG_CHECK(ctx, twoview_args_ok(ctx, models, max_per_pair, n_pairs, g) && n_sets >= 0);
    if (n_pairs == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, d_kp && pairs && K4 && (d_matches || max_per_pair == 0) && d_counts && (d_matches_out || max_per_pair == 0) && o.count &&
                           (models != GEOM_BOTH || o.kind));
    SFM_ARG_CHECK(ctx, std::isfinite(K4[0]) && std::isfinite(K4[1]) && std::isfinite(K4[2]) && std::isfinite(K4[3]) && K4[0] != 0.0 && K4[1] != 0.0);
    std::vector<TwoViewKp> tbl((size_t)n_pairs);
    for (int q = 0; q < n_pairs; ++q) {
        const int a = pairs[2 * q], b = pairs[2 * q + 1];
        SFM_ARG_CHECK(ctx, a >= 0 && a < n_sets && b >= 0 && b < n_sets);
        tbl[(size_t)q] = { d_kp[a], d_kp[b] };
    }
    const size_t P = (size_t)n_pairs, S = (size_t)max_per_pair;
    SfmPoolHold hold(ctx);
    TwoViewKp* d_tbl = nullptr; double* d_corr = nullptr; uint8_t* d_mask = nullptr;
    int rc = sfm_upload_async(ctx, hold, tbl.data(), P, d_tbl);           // pageable source: consumed when the call returns
    if (rc == SFMHIP_OK) rc = hold.get(&d_corr, P * S * 4);
    if (rc == SFMHIP_OK) rc = hold.get(&d_mask, P * S);
    if (rc != SFMHIP_OK) return rc;
    hipStream_t st = ctx->stream;
    for (int q0 = 0; q0 < n_pairs; q0 += TWOVIEW_PAIRS_PER_LAUNCH)
        hipLaunchKernelGGL(twoview_gather_kernel, dim3(std::max(1, ceil_div(max_per_pair, 256)), std::min(TWOVIEW_PAIRS_PER_LAUNCH, n_pairs - q0)), dim3(256), 0, st,
                           (const TwoViewKp*)d_tbl + q0, d_matches + S * q0, max_per_pair, d_counts + q0, K4[0], K4[1], K4[2], K4[3], d_corr + 4 * S * q0);
    o.mask = d_mask;
    rc = twoview_enqueue(ctx, models, d_corr, max_per_pair, d_counts, n_pairs, g, o);
    if (rc != SFMHIP_OK) return rc;
    hipLaunchKernelGGL(twoview_compact_kernel, dim3(n_pairs), dim3(256), 0, st, d_matches, max_per_pair, d_counts, (const uint8_t*)d_mask, d_matches_out);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

extern "C" {

int sfmhip_verify_pairs_dev(sfmhip_ctx* ctx, const double* d_corr, int stride, const int32_t* d_counts, int n_pairs, double t, int H, int rounds,
                            uint64_t seed, int min_inliers, uint8_t* d_mask, int32_t* d_count_out, double* d_F, int32_t* d_winner)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_verify_pairs_dev");
    return geometry_dev(ctx, GEOM_F, d_corr, stride, d_counts, n_pairs, GeomParams{ t, 0.0, H, rounds, (pu64)seed, min_inliers, 0.0 },
                        GeomOut{ d_mask, d_count_out, d_F, d_winner, nullptr, nullptr, nullptr, nullptr, nullptr });
}

int sfmhip_verify_pairs(sfmhip_ctx* ctx, const double* corr, int stride, const int32_t* counts, int n_pairs, double t, int H, int rounds, uint64_t seed,
                        int min_inliers, uint8_t* mask, int32_t* count_out, double* F, int32_t* winner)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_verify_pairs");
    return geometry_host(ctx, GEOM_F, corr, stride, counts, n_pairs, GeomParams{ t, 0.0, H, rounds, (pu64)seed, min_inliers, 0.0 },
                         GeomOut{ mask, count_out, F, winner, nullptr, nullptr, nullptr, nullptr, nullptr });
}

int sfmhip_verify_matches_dev(sfmhip_ctx* ctx, const sfm_keypoint* const* d_kp, int n_sets, const int32_t* pairs, int n_pairs, const double K4[4],
                              const sfm_dmatch* d_matches, int max_per_pair, const int32_t* d_counts, double t, int H, int rounds, uint64_t seed,
                              int min_inliers, sfm_dmatch* d_matches_out, int32_t* d_counts_out, double* d_F, int32_t* d_winner)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_verify_matches_dev");
    return geometry_matches_dev(ctx, GEOM_F, d_kp, n_sets, pairs, n_pairs, K4, d_matches, max_per_pair, d_counts,
                                GeomParams{ t, 0.0, H, rounds, (pu64)seed, min_inliers, 0.0 }, d_matches_out,
                                GeomOut{ nullptr, d_counts_out, d_F, d_winner, nullptr, nullptr, nullptr, nullptr, nullptr });
}

int sfmhip_verify_pairs_h_dev(sfmhip_ctx* ctx, const double* d_corr, int stride, const int32_t* d_counts, int n_pairs, double t, int H, int rounds,
                              uint64_t seed, int min_inliers, uint8_t* d_mask, int32_t* d_count_out, double* d_Hm, int32_t* d_winner)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_verify_pairs_h_dev");
    return geometry_dev(ctx, GEOM_H, d_corr, stride, d_counts, n_pairs, GeomParams{ 0.0, t, H, rounds, (pu64)seed, min_inliers, 0.0 },
                        GeomOut{ d_mask, d_count_out, nullptr, nullptr, d_Hm, d_winner, nullptr, nullptr, nullptr });
}

int sfmhip_verify_pairs_h(sfmhip_ctx* ctx, const double* corr, int stride, const int32_t* counts, int n_pairs, double t, int H, int rounds, uint64_t seed,
                          int min_inliers, uint8_t* mask, int32_t* count_out, double* Hm, int32_t* winner)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_verify_pairs_h");
    return geometry_host(ctx, GEOM_H, corr, stride, counts, n_pairs, GeomParams{ 0.0, t, H, rounds, (pu64)seed, min_inliers, 0.0 },
                         GeomOut{ mask, count_out, nullptr, nullptr, Hm, winner, nullptr, nullptr, nullptr });
}

int sfmhip_two_view_geometry_dev(sfmhip_ctx* ctx, const double* d_corr, int stride, const int32_t* d_counts, int n_pairs, double t_f, double t_h, int H,
                                 int rounds, uint64_t seed, int min_inliers, double hf_ratio, int32_t* d_kind, uint8_t* d_mask, int32_t* d_count_out,
                                 int32_t* d_counts2, double* d_F, double* d_Hm, int32_t* d_winners)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_two_view_geometry_dev");
    return geometry_dev(ctx, GEOM_BOTH, d_corr, stride, d_counts, n_pairs, GeomParams{ t_f, t_h, H, rounds, (pu64)seed, min_inliers, hf_ratio },
                        GeomOut{ d_mask, d_count_out, d_F, nullptr, d_Hm, nullptr, d_kind, d_counts2, d_winners });
}

int sfmhip_two_view_geometry(sfmhip_ctx* ctx, const double* corr, int stride, const int32_t* counts, int n_pairs, double t_f, double t_h, int H, int rounds,
                             uint64_t seed, int min_inliers, double hf_ratio, int32_t* kind, uint8_t* mask, int32_t* count_out, int32_t* counts2, double* F,
                             double* Hm, int32_t* winners)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_two_view_geometry");
    return geometry_host(ctx, GEOM_BOTH, corr, stride, counts, n_pairs, GeomParams{ t_f, t_h, H, rounds, (pu64)seed, min_inliers, hf_ratio },
                         GeomOut{ mask, count_out, F, nullptr, Hm, nullptr, kind, counts2, winners });
}

int sfmhip_two_view_geometry_matches_dev(sfmhip_ctx* ctx, const sfm_keypoint* const* d_kp, int n_sets, const int32_t* pairs, int n_pairs, const double K4[4],
                                         const sfm_dmatch* d_matches, int max_per_pair, const int32_t* d_counts, double t_f, double t_h, int H, int rounds,
                                         uint64_t seed, int min_inliers, double hf_ratio, int32_t* d_kind, sfm_dmatch* d_matches_out, int32_t* d_counts_out,
                                         int32_t* d_counts2, double* d_F, double* d_Hm, int32_t* d_winners)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_two_view_geometry_matches_dev");
    return geometry_matches_dev(ctx, GEOM_BOTH, d_kp, n_sets, pairs, n_pairs, K4, d_matches, max_per_pair, d_counts,
                                GeomParams{ t_f, t_h, H, rounds, (pu64)seed, min_inliers, hf_ratio }, d_matches_out,
                                GeomOut{ nullptr, d_counts_out, d_F, nullptr, d_Hm, nullptr, d_kind, d_counts2, d_winners });
}

int sfmhip_register_views_dev(sfmhip_ctx* ctx, const double* d_corr, int stride, const int32_t* d_counts, int n_views, double t, int H, int rounds,
                              uint64_t seed, int min_inliers, uint8_t* d_mask, int32_t* d_count_out, double* d_P, int32_t* d_winner)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_register_views_dev");
    return geometry_dev(ctx, GEOM_P, d_corr, stride, d_counts, n_views, GeomParams{ t, 0.0, H, rounds, (pu64)seed, min_inliers, 0.0 },
                        GeomOut{ d_mask, d_count_out, d_P, d_winner, nullptr, nullptr, nullptr, nullptr, nullptr });
}

int sfmhip_register_views(sfmhip_ctx* ctx, const double* corr, int stride, const int32_t* counts, int n_views, double t, int H, int rounds, uint64_t seed,
                          int min_inliers, uint8_t* mask, int32_t* count_out, double* P, int32_t* winner)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_register_views");
    return geometry_host(ctx, GEOM_P, corr, stride, counts, n_views, GeomParams{ t, 0.0, H, rounds, (pu64)seed, min_inliers, 0.0 },
                         GeomOut{ mask, count_out, P, winner, nullptr, nullptr, nullptr, nullptr, nullptr });
}

// Pure host code: the SVD of the left 3 x 3 block by the one-sided Jacobi rotations of svd3.hpp (Hestenes), which find the small singular
// value of a planar DLT to its own precision where an eigen-solver on M^T M would square the ratio away.
int sfmhip_pose_from_projection(const double P[12], double R[9], double t[3], double* sv_ratio)
{
    if (!P || !R || !t || !sv_ratio) return SFMHIP_E_ARG;
    for (int j = 0; j < 12; ++j)
        if (!std::isfinite(P[j])) return SFMHIP_E_NUMERIC;
    double M[3][3], u[3][3], v[3][3], S[3];                             // columns in descending order of the singular values
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = P[4 * i + j];
    svd3::jacobi(M, u, v, S);
    const double s0 = S[0], s1 = S[1], s2 = S[2];
    if (!(s0 > 0.0) || !(s1 > 0.0) || !std::isfinite(s0)) return SFMHIP_E_NUMERIC;                     // rank below two: no rotation to speak of
    double Rm[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rm[3 * i + j] = (u[i][0] * v[j][0] + u[i][1] * v[j][1]) + u[i][2] * v[j][2];
    const double det = Rm[0] * (Rm[4] * Rm[8] - Rm[5] * Rm[7]) - Rm[1] * (Rm[3] * Rm[8] - Rm[5] * Rm[6]) + Rm[2] * (Rm[3] * Rm[7] - Rm[4] * Rm[6]);
    *sv_ratio = s0 / s2;                                                // inf for an exactly planar DLT
    if (!(det > 0.0)) return SFMHIP_E_NUMERIC;                          // a reflection: P is not a camera looking at its points
    const double mean = (s0 + s1 + s2) / 3.0;
    for (int j = 0; j < 9; ++j) R[j] = Rm[j];
    for (int i = 0; i < 3; ++i) t[i] = P[4 * i + 3] / mean;
    return SFMHIP_OK;
}

}
