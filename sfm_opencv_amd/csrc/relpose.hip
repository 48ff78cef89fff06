// relpose.hip -- the relative pose of many image pairs in one call: the winning F of sfmhip_verify_pairs / sfmhip_two_view_geometry on
// K-normalised rows goes in, a refined (R, t) with its re-taken inlier set, its cheirality and parallax counts and the quality of the
// decomposition comes out (what the reference does for its first pair on the host: recoverPose behind findEssentialMat, NView:1048).  The
// definition is in sfmhip.h at sfmhip_relative_pose and is followed to the letter: the decomposition, the vote and the per-row tests are
// prescribed fp64 operation by operation, the refinement's sums are reduced in a fixed order.
//
// ONE kernel, one launch for the whole batch, one workgroup of 256 threads per pair (relpose_kernel):
//   prep      a row loop: which rows are in L_0 and in U, as one flag byte per row in a scratch area; |U|
//   decompose lane 0: the Jacobi SVD of svd3.hpp on F, the sign rule, Ra, Rb, t into LDS
//   vote      a row loop: the rows of U in front under each of the four candidates; lane 0 picks the winner
//   refine    rounds x iters Levenberg-Marquardt steps.  A step is one row loop for the 21 sums (15 of J^T J, 5 of J^T r, the cost), the
//             5 x 5 Cholesky solve and the candidate pose on lane 0, and one row loop for the candidate's cost per damping trial; a round
//             p >= 1 starts with a row loop that re-takes the set with THE Sampson test of twoview_rows.hpp
//   final     a row loop: the mask bits and the three counts under the final pose
// The rows stay in global memory and are read as rows of four doubles straight from the caller's block in every loop: a block is read
// some tens of times by the one workgroup that owns it, 64 KB for 2000 rows, and stays in that XCD's L2 (4 MB) after the first; staging
// it in LDS would bound the stride at 5000 rows and buy nothing while the kernel waits on its barriers and lane 0, not on loads.
// Thread x owns the rows x, x + 256, ..: it alone writes and reads their flag bytes, so the flags need no barrier.
// A sum is added up per thread in ascending row order, then inside a wave by a butterfly of five lane exchanges, then over the four
// waves in wave order: no atomics, the same bits in every run and every batch.  Whatever steers the loop (the solve failed, accept,
// stop, the set fell below 8) is decided on lane 0 and read back by all threads from LDS behind a barrier.
#include "common.hpp"
#pragma clang fp contract(off)
#include "svd3.hpp"
#include "twoview_rows.hpp"

#define RELPOSE_THREADS 256
#define RELPOSE_ROUNDS_MAX 8
#define RELPOSE_ITERS_MAX 50
#define RELPOSE_PAIRS_PER_LAUNCH 32768        // a longer batch goes in slices, as in twoview.hip (the pairs are independent)
#define RELPOSE_NSUM 21                       // 15 + 5 + 1

struct RelposeParams { double t2, max_depth, cos2; int rounds, iters; };

// what a workgroup keeps in LDS: the pose as it stands with its E and the five derivatives of E, the tangent basis they were taken in,
// the pose a step proposes, the two rotations and the baseline of the decomposition, and the areas of the reductions and decisions
struct RelposeShared {
    double R[9], t[3], E[9];
    double G[5][9];
    double b1[3], b2[3];
    double Rn[9], tn[3], En[9];
    double Rc[2][9], tc[3];
    double red[4][RELPOSE_NSUM];
    int ired[4][4];
    int ctrl;
};

// out = [w]x R
__device__ __forceinline__ void skew_mul(const double (&w)[3], const double (&R)[9], double (&out)[9])
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out[j] = w[1] * R[6 + j] - w[2] * R[3 + j];
        out[3 + j] = w[2] * R[j] - w[0] * R[6 + j];
        out[6 + j] = w[0] * R[3 + j] - w[1] * R[j];
    }
}

// the per-row test of the definition under (R, t): in front of both cameras (and nearer than max_depth baselines), and seen under at
// least the angle whose squared cosine is cos2.  Nothing is divided.
__device__ __forceinline__ void relpose_row_test(const double (&R)[9], const double (&t)[3], const double4& r, double max_depth, double cos2, bool& front,
                                                 bool& angle)
{
    const double p0 = (R[0] * r.x + R[1] * r.y) + R[2];
    const double p1 = (R[3] * r.x + R[4] * r.y) + R[5];
    const double p2 = (R[6] * r.x + R[7] * r.y) + R[8];
    const double aa = (p0 * p0 + p1 * p1) + p2 * p2;
    const double bb = (r.z * r.z + r.w * r.w) + 1.0;
    const double ab = (p0 * r.z + p1 * r.w) + p2;
    const double at = (p0 * t[0] + p1 * t[1]) + p2 * t[2];
    const double bt = (r.z * t[0] + r.w * t[1]) + t[2];
    const double D = aa * bb - ab * ab;
    const double n1 = ab * bt - at * bb;
    const double n2 = aa * bt - ab * at;
    front = D > 0.0 && n1 > 0.0 && n2 > 0.0;
    if (max_depth > 0.0) front = front && n1 < max_depth * D && n2 < max_depth * D;
    angle = front && (ab <= 0.0 || ab * ab <= cos2 * (aa * bb));
}

// the Sampson residual e / sqrt(d) of a row under E, and what its derivatives need
struct RelposeResidual { double l0, l1, m0, m1, s, r; };
__device__ __forceinline__ RelposeResidual relpose_residual(const double (&E)[9], const double4& q)
{
    RelposeResidual o;
    o.l0 = (E[0] * q.x + E[1] * q.y) + E[2];
    o.l1 = (E[3] * q.x + E[4] * q.y) + E[5];
    const double l2 = (E[6] * q.x + E[7] * q.y) + E[8];
    o.m0 = (E[0] * q.z + E[3] * q.w) + E[6];
    o.m1 = (E[1] * q.z + E[4] * q.w) + E[7];
    const double e = (q.z * o.l0 + q.w * o.l1) + l2;
    const double d = (((o.l0 * o.l0 + o.l1 * o.l1) + o.m0 * o.m0) + o.m1 * o.m1) + 1e-300;
    o.s = 1.0 / sqrt(d);
    o.r = e * o.s;
    return o;
}

__device__ __forceinline__ double4 relpose_load(const double* p) { return make_double4(p[0], p[1], p[2], p[3]); }
__device__ __forceinline__ bool relpose_finite(const double4& r) { return isfinite(r.x) && isfinite(r.y) && isfinite(r.z) && isfinite(r.w); }

// the sum of v over the workgroup, in every thread: the lanes of a wave by a butterfly, the four waves in wave order.  Every thread of
// the workgroup calls it.
template <int N, int W, typename T>
__device__ __forceinline__ void relpose_block_sum(T (&v)[N], T (&area)[4][W])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                                     // the previous call's readers are done with the area
#pragma unroll
    for (int k = 0; k < N; ++k) {
        T x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x = x + __shfl_xor(x, off);
        if (lane == 0) area[wave][k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((area[0][k] + area[1][k]) + area[2][k]) + area[3][k];
}

// a decision of lane 0, in every thread.  Every thread of the workgroup calls it.
__device__ __forceinline__ int relpose_decide(RelposeShared& sh, int v)
{
    __syncthreads();                                                     // what lane 0 wrote before deciding is visible with the decision
    if (threadIdx.x == 0) sh.ctrl = v;
    __syncthreads();
    const int c = sh.ctrl;
    __syncthreads();                                                     // everybody has read it before the next decision
    return c;
}

// lane 0: the tangent basis of refine_motion at t
__device__ __forceinline__ void relpose_tangent(const double (&t)[3], double (&b1)[3], double (&b2)[3])
{
    const double f0 = fabs(t[0]), f1 = fabs(t[1]), f2 = fabs(t[2]);
    const int k = f0 < f1 ? (f0 < f2 ? 0 : 2) : (f1 < f2 ? 1 : 2);
    const double e[3] = { k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0 };
    b1[0] = t[1] * e[2] - t[2] * e[1]; b1[1] = t[2] * e[0] - t[0] * e[2]; b1[2] = t[0] * e[1] - t[1] * e[0];
    const double n1 = sqrt((b1[0] * b1[0] + b1[1] * b1[1]) + b1[2] * b1[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) b1[a] = b1[a] / n1;
    b2[0] = t[1] * b1[2] - t[2] * b1[1]; b2[1] = t[2] * b1[0] - t[0] * b1[2]; b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// lane 0: the five derivatives of E = [t]x R at the pose in LDS, dE/dw_k = [t]x [e_k]x R and dE/d(alpha, beta) = [b1]x R, [b2]x R
__device__ __forceinline__ void relpose_make_G(RelposeShared& sh)
{
    double R[9], t[3], b1[3], b2[3], Q[9], G[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = sh.R[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = sh.t[j];
    relpose_tangent(t, b1, b2);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double e[3] = { k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0 };
        skew_mul(e, R, Q);
        skew_mul(t, Q, G);
#pragma unroll
        for (int j = 0; j < 9; ++j) sh.G[k][j] = G[j];
    }
    skew_mul(b1, R, G);
#pragma unroll
    for (int j = 0; j < 9; ++j) sh.G[3][j] = G[j];
    skew_mul(b2, R, G);
#pragma unroll
    for (int j = 0; j < 9; ++j) sh.G[4][j] = G[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) { sh.b1[j] = b1[j]; sh.b2[j] = b2[j]; }
}

// lane 0: the damped 5 x 5 system of a step (A: the upper triangle by rows, g) solved by Cholesky, as la::solve_spd; false where the
// matrix is not positive definite
__device__ __forceinline__ bool relpose_solve(const double (&S)[RELPOSE_NSUM], double lambda, double (&x)[5])
{
    double M[5][5];
    int at = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = a; b < 5; ++b) { M[a][b] = S[at]; M[b][a] = S[at]; ++at; }
#pragma unroll
    for (int a = 0; a < 5; ++a) { M[a][a] = M[a][a] + lambda * (M[a][a] + 1e-12); x[a] = -S[15 + a]; }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        double d = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - M[j][k] * M[j][k];
        ok = ok && d > 0.0;
        d = sqrt(d); M[j][j] = d;
#pragma unroll
        for (int i = j + 1; i < 5; ++i) {
            double s = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - M[i][k] * M[j][k];
            M[i][j] = s / d;
        }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - M[i][k] * x[k];
        x[i] = s / M[i][i];
    }
#pragma unroll
    for (int i = 4; i >= 0; --i) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < 5; ++k) s = s - M[k][i] * x[k];
        x[i] = s / M[i][i];
    }
    return ok;
}

// lane 0: the pose a step d proposes, R <- exp([d0..2]x) R and t <- normalise(t + d3 b1 + d4 b2), with its E, into Rn, tn, En
__device__ __forceinline__ void relpose_apply(RelposeShared& sh, const double (&d)[5])
{
    const double th = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const double a = th < 1e-9 ? 1.0 - th * th / 6.0 : sin(th) / th, b = th < 1e-9 ? 0.5 - th * th / 24.0 : (1.0 - cos(th)) / (th * th);
    const double K[9] = { 0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0 };
    double dR[9], Rn[9], tn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
            dR[3 * i + j] = ((i == j ? 1.0 : 0.0) + a * K[3 * i + j]) + b * k2;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (dR[3 * i] * sh.R[j] + dR[3 * i + 1] * sh.R[3 + j]) + dR[3 * i + 2] * sh.R[6 + j];
#pragma unroll
    for (int c = 0; c < 3; ++c) tn[c] = (sh.t[c] + d[3] * sh.b1[c]) + d[4] * sh.b2[c];
    const double nn = sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) tn[c] = tn[c] / nn;
    double En[9];
    skew_mul(tn, Rn, En);
#pragma unroll
    for (int j = 0; j < 9; ++j) { sh.Rn[j] = Rn[j]; sh.En[j] = En[j]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) sh.tn[c] = tn[c];
}

// the cost of the current set (the rows whose flag has bit 1) under the E at `E`, in every thread
__device__ __forceinline__ double relpose_cost(const double* __restrict__ rows, const uint8_t* __restrict__ flag, int cnt, const double* E_lds, RelposeShared& sh)
{
    double E[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) E[j] = E_lds[j];
    double c[1] = { 0.0 };
    for (int i = threadIdx.x; i < cnt; i += RELPOSE_THREADS) {
        if (!(flag[i] & 2)) continue;
        const RelposeResidual o = relpose_residual(E, relpose_load(rows + 4 * (size_t)i));
        c[0] = c[0] + o.r * o.r;
    }
    relpose_block_sum(c, sh.red);
    return c[0];
}

__global__ __launch_bounds__(RELPOSE_THREADS) void relpose_kernel(const double* __restrict__ corr, int stride, const int32_t* __restrict__ counts,
                                                                  const uint8_t* __restrict__ mask_in, const double* __restrict__ Fin, RelposeParams P,
                                                                  uint8_t* __restrict__ flags, double* __restrict__ pose, int32_t* __restrict__ info,
                                                                  double* __restrict__ quality, uint8_t* __restrict__ mask_out)
{
    __shared__ RelposeShared sh;
    const size_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const int cnt = clamp_count(counts[q], stride);
    const double* rows = corr + 4 * (size_t)stride * q;
    uint8_t* flag = flags + (size_t)stride * q;
    const uint8_t* min = mask_in ? mask_in + (size_t)stride * q : nullptr;
    uint8_t* mout = mask_out ? mask_out + (size_t)stride * q : nullptr;

    // prep: flag bit 0 = the row is in L_0, bit 1 = it is in the current set, which starts as U
    int iv[4] = { 0, 0, 0, 0 };
    for (int i = tid; i < cnt; i += RELPOSE_THREADS) {
        const bool fin = relpose_finite(relpose_load(rows + 4 * (size_t)i));
        const bool in = fin && (!min || min[i] != 0);
        flag[i] = fin ? (in ? 3 : 1) : 0;
        iv[0] += in ? 1 : 0;
    }
    relpose_block_sum(iv, sh.ired);
    const int n_used = iv[0];

    // decompose, on lane 0
    double sv[3] = { NAN, NAN, NAN };
    int ok = 0;
    if (tid == 0) {
        double M[3][3], u[3][3], v[3][3];
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { M[i][j] = Fin[9 * q + 3 * i + j]; fin = fin && isfinite(M[i][j]); }
        if (fin && n_used >= 8) {
            svd3::jacobi(M, u, v, sv);
            if (sv[1] > 0.0 && isfinite(sv[0])) {
                ok = 1;
                const double su = svd3::det(u) < 0 ? -1.0 : 1.0, sw = svd3::det(v) < 0 ? -1.0 : 1.0;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) { u[i][j] = su < 0 ? -u[i][j] : u[i][j]; v[i][j] = sw < 0 ? -v[i][j] : v[i][j]; }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        sh.Rc[0][3 * i + j] = (u[i][0] * v[j][1] - u[i][1] * v[j][0]) + u[i][2] * v[j][2];
                        sh.Rc[1][3 * i + j] = (u[i][1] * v[j][0] - u[i][0] * v[j][1]) + u[i][2] * v[j][2];
                    }
                    sh.tc[i] = u[i][2];
                }
            }
        }
    }
    ok = relpose_decide(sh, ok);

    // vote: the rows of U in front under each candidate
    int cand = -1;
    int n4[4] = { 0, 0, 0, 0 };
    if (ok) {
        double Ra[9], Rb[9], tp[3], tm[3];
#pragma unroll
        for (int j = 0; j < 9; ++j) { Ra[j] = sh.Rc[0][j]; Rb[j] = sh.Rc[1][j]; }
#pragma unroll
        for (int j = 0; j < 3; ++j) { tp[j] = sh.tc[j]; tm[j] = -tp[j]; }
        for (int i = tid; i < cnt; i += RELPOSE_THREADS) {
            if (!(flag[i] & 2)) continue;
            const double4 r = relpose_load(rows + 4 * (size_t)i);
            bool f, a;
            relpose_row_test(Ra, tp, r, P.max_depth, P.cos2, f, a); n4[0] += f ? 1 : 0;
            relpose_row_test(Rb, tp, r, P.max_depth, P.cos2, f, a); n4[1] += f ? 1 : 0;
            relpose_row_test(Ra, tm, r, P.max_depth, P.cos2, f, a); n4[2] += f ? 1 : 0;
            relpose_row_test(Rb, tm, r, P.max_depth, P.cos2, f, a); n4[3] += f ? 1 : 0;
        }
        relpose_block_sum(n4, sh.ired);
        int c = -1;
        if (tid == 0) {
            int best = n4[0];
            c = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (n4[k] > best) { best = n4[k]; c = k; }              // the largest count, the smallest k among equals
            if (best == 0) c = -1;
            else {
#pragma unroll
                for (int j = 0; j < 9; ++j) sh.R[j] = (c & 1) ? Rb[j] : Ra[j];
#pragma unroll
                for (int j = 0; j < 3; ++j) sh.t[j] = (c & 2) ? tm[j] : tp[j];
                double R[9], t[3], E[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) R[j] = sh.R[j];
#pragma unroll
                for (int j = 0; j < 3; ++j) t[j] = sh.t[j];
                skew_mul(t, R, E);
#pragma unroll
                for (int j = 0; j < 9; ++j) sh.E[j] = E[j];
            }
        }
        cand = relpose_decide(sh, c);
    }

    if (cand < 0) {                                                      // no pose
        for (int i = tid; mout && i < stride; i += RELPOSE_THREADS) mout[i] = 0;
        if (tid < 12) pose[12 * q + tid] = NAN;
        if (tid < 10) info[10 * q + tid] = tid == 1 ? -1 : tid == 6 ? n_used : 0;
        if (tid < 5 && quality) quality[5 * q + tid] = NAN;
        return;
    }

    // refine
    double cost0 = relpose_cost(rows, flag, cnt, sh.E, sh), cost1 = cost0;        // no round: the cost of U under the voted candidate, twice
    const int rounds = P.iters > 0 ? P.rounds : 0;
    for (int p = 0; p < rounds; ++p) {
        if (p >= 1) {                                                    // re-take the set under the current E
            double E[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) E[j] = sh.E[j];
            int m[4] = { 0, 0, 0, 0 };
            for (int i = tid; i < cnt; i += RELPOSE_THREADS) {
                const uint8_t f = flag[i];
                if (!(f & 1)) continue;
                const double4 r = relpose_load(rows + 4 * (size_t)i);
                const bool in = twoview_inlier(E, r.x, r.y, r.z, r.w, P.t2);
                flag[i] = in ? 3 : 1;
                m[0] += in ? 1 : 0;
            }
            relpose_block_sum(m, sh.ired);
            if (relpose_decide(sh, m[0] < 8)) break;
        }
        double cost = 0.0, lambda = 1e-3;                                // lane 0's; the others carry copies nobody reads
        for (int it = 0; it < P.iters; ++it) {
            if (tid == 0) relpose_make_G(sh);
            __syncthreads();
            double S[RELPOSE_NSUM];
            {
                double E[9], G[5][9];
#pragma unroll
                for (int j = 0; j < 9; ++j) E[j] = sh.E[j];
#pragma unroll
                for (int k = 0; k < 5; ++k)
#pragma unroll
                    for (int j = 0; j < 9; ++j) G[k][j] = sh.G[k][j];
#pragma unroll
                for (int k = 0; k < RELPOSE_NSUM; ++k) S[k] = 0.0;
                for (int i = tid; i < cnt; i += RELPOSE_THREADS) {
                    if (!(flag[i] & 2)) continue;
                    const double4 r = relpose_load(rows + 4 * (size_t)i);
                    const RelposeResidual o = relpose_residual(E, r);
                    double J[5];
#pragma unroll
                    for (int k = 0; k < 5; ++k) {
                        const double (&g)[9] = G[k];
                        const double dl0 = (g[0] * r.x + g[1] * r.y) + g[2];
                        const double dl1 = (g[3] * r.x + g[4] * r.y) + g[5];
                        const double dl2 = (g[6] * r.x + g[7] * r.y) + g[8];
                        const double dm0 = (g[0] * r.z + g[3] * r.w) + g[6];
                        const double dm1 = (g[1] * r.z + g[4] * r.w) + g[7];
                        const double de = (r.z * dl0 + r.w * dl1) + dl2;
                        const double dd = 2.0 * (((o.l0 * dl0 + o.l1 * dl1) + o.m0 * dm0) + o.m1 * dm1);
                        J[k] = o.s * de - ((0.5 * o.r) * dd) * (o.s * o.s);
                    }
                    int at = 0;
#pragma unroll
                    for (int a = 0; a < 5; ++a)
#pragma unroll
                        for (int b = a; b < 5; ++b) { S[at] = S[at] + J[a] * J[b]; ++at; }
#pragma unroll
                    for (int a = 0; a < 5; ++a) S[15 + a] = S[15 + a] + J[a] * o.r;
                    S[20] = S[20] + o.r * o.r;
                }
            }
            relpose_block_sum(S, sh.red);
            if (it == 0) { cost = S[20]; cost0 = cost; cost1 = cost; }
            int verdict = 0;                                             // 0: no trial improved; 1: accepted; 2: accepted, and the gain was tiny
            for (int tries = 0; tries < 8; ++tries) {
                int solved = 0;
                if (tid == 0) {
                    double d[5];
                    solved = relpose_solve(S, lambda, d) ? 1 : 0;
                    if (solved) relpose_apply(sh, d); else lambda = lambda * 10.0;
                }
                if (!relpose_decide(sh, solved)) continue;
                const double c1 = relpose_cost(rows, flag, cnt, sh.En, sh);
                int v = 0;
                if (tid == 0) {
                    if (c1 < cost) {
                        v = cost - c1 <= 1e-12 * cost ? 2 : 1;
#pragma unroll
                        for (int j = 0; j < 9; ++j) { sh.R[j] = sh.Rn[j]; sh.E[j] = sh.En[j]; }
#pragma unroll
                        for (int j = 0; j < 3; ++j) sh.t[j] = sh.tn[j];
                        cost = c1;
                        lambda = fmax(lambda * 0.3, 1e-9);
                    } else lambda = lambda * 10.0;
                }
                v = relpose_decide(sh, v);
                if (v) { verdict = v; cost1 = c1; break; }
            }
            if (verdict != 1) break;
        }
    }

    // final: the mask bits and the counts under the pose as it stands
    {
        __syncthreads();
        double R[9], t[3], E[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) { R[j] = sh.R[j]; E[j] = sh.E[j]; }
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = sh.t[j];
        int n[4] = { 0, 0, 0, 0 };
        for (int i = tid; i < stride; i += RELPOSE_THREADS) {
            uint8_t b = 0;
            if (i < cnt && (flag[i] & 1)) {
                const double4 r = relpose_load(rows + 4 * (size_t)i);
                if (twoview_inlier(E, r.x, r.y, r.z, r.w, P.t2)) {
                    bool f, a;
                    relpose_row_test(R, t, r, P.max_depth, P.cos2, f, a);
                    b = a ? 7 : f ? 3 : 1;
                    n[0] += 1; n[1] += f ? 1 : 0; n[2] += a ? 1 : 0;
                }
            }
            if (mout) mout[i] = b;
        }
        relpose_block_sum(n, sh.ired);
        if (tid < 9) pose[12 * q + tid] = R[tid];
        else if (tid < 12) pose[12 * q + tid] = t[tid - 9];
        if (tid == 0) {
            int32_t* o = info + 10 * q;
            o[0] = 1; o[1] = cand; o[2] = n4[0]; o[3] = n4[1]; o[4] = n4[2]; o[5] = n4[3]; o[6] = n_used; o[7] = n[0]; o[8] = n[1]; o[9] = n[2];
            if (quality) { double* w = quality + 5 * q; w[0] = sv[0]; w[1] = sv[1]; w[2] = sv[2]; w[3] = cost0; w[4] = cost1; }
        }
    }
}

static inline bool relpose_nonneg(double x) { return std::isfinite(x) && x >= 0.0; }
static inline bool relpose_args_ok(const sfmhip_ctx* ctx, int stride, int n_pairs, double t, int rounds, int iters, double max_depth, double min_angle)
{
    return ctx && stride >= 0 && n_pairs >= 0 && relpose_nonneg(t) && relpose_nonneg(max_depth) && relpose_nonneg(min_angle) &&
           min_angle <= 1.57079632679489661923 && rounds >= 0 && rounds <= RELPOSE_ROUNDS_MAX && iters >= 0 && iters <= RELPOSE_ITERS_MAX;
}
static inline RelposeParams relpose_params(double t, int rounds, int iters, double max_depth, double min_angle)
{
    const double c = std::cos(min_angle);
    return RelposeParams{ t * t, max_depth, c * c, rounds, iters };
}

// the whole batch on the context's stream, in slices of RELPOSE_PAIRS_PER_LAUNCH pairs as twoview_enqueue; the flag bytes come from the block
// cache, one area that the slices, which run one after the other on the stream, use in turn
static int relpose_enqueue(sfmhip_ctx* ctx, const double* d_corr, int stride, const int32_t* d_counts, int n_pairs, const uint8_t* d_mask_in, const double* d_F,
                           const RelposeParams& P, double* d_pose, int32_t* d_info, double* d_quality, uint8_t* d_mask_out)
{
    const size_t S = (size_t)stride;
    SfmPoolHold hold(ctx);
    uint8_t* d_flags = nullptr;
    const int rc = hold.get(&d_flags, (size_t)std::min(n_pairs, RELPOSE_PAIRS_PER_LAUNCH) * S);
    if (rc != SFMHIP_OK) return rc;
    for (int q0 = 0; q0 < n_pairs; q0 += RELPOSE_PAIRS_PER_LAUNCH) {
        const size_t Q = (size_t)q0;
        hipLaunchKernelGGL(relpose_kernel, dim3(std::min(RELPOSE_PAIRS_PER_LAUNCH, n_pairs - q0)), dim3(RELPOSE_THREADS), 0, ctx->stream, d_corr + 4 * S * Q, stride,
                           d_counts + Q, d_mask_in ? d_mask_in + S * Q : nullptr, d_F + 9 * Q, P, d_flags, d_pose + 12 * Q, d_info + 10 * Q,
                           d_quality ? d_quality + 5 * Q : nullptr, d_mask_out ? d_mask_out + S * Q : nullptr);
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

extern "C" {

int sfmhip_relative_pose_dev(sfmhip_ctx* ctx, const double* d_corr, int stride, const int32_t* d_counts, int n_pairs, const uint8_t* d_mask_in, const double* d_F,
                             double t, int rounds, int iters, double max_depth, double min_angle, double* d_pose, int32_t* d_info, double* d_quality,
                             uint8_t* d_mask_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_relative_pose_dev");
    SFM_ARG_CHECK(ctx, relpose_args_ok(ctx, stride, n_pairs, t, rounds, iters, max_depth, min_angle));
    if (n_pairs == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, (d_corr || stride == 0) && d_counts && d_F && d_pose && d_info);
    return relpose_enqueue(ctx, d_corr, stride, d_counts, n_pairs, d_mask_in, d_F, relpose_params(t, rounds, iters, max_depth, min_angle), d_pose, d_info,
                           d_quality, d_mask_out);
}

int sfmhip_relative_pose(sfmhip_ctx* ctx, const double* corr, int stride, const int32_t* counts, int n_pairs, const uint8_t* mask_in, const double* F, double t,
                         int rounds, int iters, double max_depth, double min_angle, double* pose, int32_t* info, double* quality, uint8_t* mask_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_relative_pose");
    SFM_ARG_CHECK(ctx, relpose_args_ok(ctx, stride, n_pairs, t, rounds, iters, max_depth, min_angle));
    if (n_pairs == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, (corr || stride == 0) && counts && F && pose && info);
    const size_t P = (size_t)n_pairs, S = (size_t)stride;
    SfmPoolHold hold(ctx);
    double* d_corr = nullptr; int32_t* d_counts = nullptr; uint8_t* d_mask_in = nullptr; double* d_F = nullptr; uint8_t* d_mask_out = nullptr; char* d_head = nullptr;
    SfmCarve carve;
    const size_t o_pose = carve(P * 12 * sizeof(double)), o_info = carve(P * 10 * 4), o_quality = carve(P * 5 * sizeof(double));
    int rc = hold.get(&d_corr, P * S * 4);
    if (rc == SFMHIP_OK && S) rc = sfm_upload(ctx, d_corr, corr, P * S * 4 * sizeof(double));
    if (rc == SFMHIP_OK) rc = sfm_upload_async(ctx, hold, counts, P, d_counts);
    if (rc == SFMHIP_OK) rc = sfm_upload_async(ctx, hold, F, P * 9, d_F);
    if (rc == SFMHIP_OK && mask_in && S) { rc = hold.get(&d_mask_in, P * S); if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d_mask_in, mask_in, P * S); }
    if (rc == SFMHIP_OK && mask_out) rc = hold.get(&d_mask_out, P * S);
    if (rc == SFMHIP_OK) rc = hold.get(carve.bytes, (void**)&d_head);
    if (rc == SFMHIP_OK)
        rc = relpose_enqueue(ctx, d_corr, stride, d_counts, n_pairs, d_mask_in, d_F, relpose_params(t, rounds, iters, max_depth, min_angle), (double*)(d_head + o_pose),
                             (int32_t*)(d_head + o_info), quality ? (double*)(d_head + o_quality) : nullptr, d_mask_out);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    auto back = [&](void* dst, const void* src, size_t bytes) { if (e == hipSuccess && dst && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); };
    back(pose, d_head + o_pose, P * 12 * sizeof(double));
    back(info, d_head + o_info, P * 10 * 4);
    back(quality, d_head + o_quality, P * 5 * sizeof(double));
    back(mask_out, d_mask_out, P * S);
    return sfm_finish(ctx, e);
}

}
