// points.hip -- neighbour search over a 3-D point cloud: the K nearest OTHER points of every point, exact, and what is built on
// it (statistical outlier removal; normals.hip fits its planes on the same table); the fixed-radius neighbour COUNT on the same grid
// (radius outlier removal) and voxel-grid down-sampling on the same sort (second half of the file).
//
// Semantics, the same for every method (they are what normals_kernel has always done):
//   d(i, j) = sqrt((dx*dx + dy*dy) + dz*dz) in fp64 without contraction; neighbours ordered by (d, j) ascending; i itself excluded by
//   index (a duplicate at distance 0 is a neighbour); a slot without a neighbour is idx -1 / dist +inf; a point with a non-finite
//   coordinate is nobody's neighbour and has none.
//
// SFMHIP_POINTS_BRUTE: one thread per query streams the whole cloud through LDS tiles (the sweep of normals_kernel).
// SFMHIP_POINTS_GRID : the cloud is binned into cubic cells on the device (64-bit key, 21 bits per axis, stable radix sort of
//   sortscan.hpp), a query visits the cells within Chebyshev ring r = 0, 1, .. RMAX of its own and stops as soon as its K-th distance
//   is CERTIFIED final (see points_knn_grid_kernel); a query not certified by RMAX goes on a list that the brute-force sweep finishes.
//   Nothing here needs the host: cell size, origin, list length all stay on the device.
#include "common.hpp"
#include "sortscan.hpp"
#include "unionfind.hpp"
#pragma clang fp contract(off)

#define KMAX 16
#define NTILE 256
#define CELL_BITS 21
#define CELL_MAX ((1 << CELL_BITS) - 1)
#define RMAX 2
#define NSAMPLE 1024

typedef unsigned long long pu64;
typedef unsigned int pu32;

// ------------------------------------------------------------------------------------------------
// the sorted top-16 of a query, in registers.  (d, j) < (bd[k], bi[k]) lexicographically; an empty slot is (+inf, -1) and never beats
// anything.  dk / ik: the K-th entry (the only one a candidate has to beat), kept beside the list so that no register is indexed by K.
// ------------------------------------------------------------------------------------------------
struct TopK {
    double bd[KMAX]; int bi[KMAX];
    double dk; int ik;        // bd[K - 1], bi[K - 1]
    double gate2;             // no candidate with d2 > gate2 can have sqrt(d2) <= dk (see normals_kernel)
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) { bd[k] = INFINITY; bi[k] = -1; }
        dk = INFINITY; ik = -1; gate2 = INFINITY;
    }
    // candidate j at squared distance d2 (cells are not visited in index order: the tie rule is explicit)
    __device__ __forceinline__ void offer(double d2, int j, int K)
    {
        if (!(d2 <= gate2)) return;
        const double d = sqrt(d2);
        if (!(d < dk || (d == dk && j < ik))) return;
        bd[KMAX - 1] = d; bi[KMAX - 1] = j;           // replaces the 16th: never one of the first K
#pragma unroll
        for (int k = KMAX - 1; k > 0; --k) {
            if (bd[k] < bd[k - 1] || (bd[k] == bd[k - 1] && bi[k] < bi[k - 1])) {
                const double td = bd[k]; bd[k] = bd[k - 1]; bd[k - 1] = td;
                const int ti = bi[k]; bi[k] = bi[k - 1]; bi[k - 1] = ti;
            }
        }
#pragma unroll
        for (int k = 0; k < KMAX; ++k) if (k == K - 1) { dk = bd[k]; ik = bi[k]; }
        gate2 = dk * dk * (1.0 + 0x1p-50);            // inf while the list is not full
    }
    __device__ __forceinline__ void store(int K, size_t row, int32_t* __restrict__ idx, double* __restrict__ dist) const
    {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                if (idx) idx[row * K + k] = bi[k];
                if (dist) dist[row * K + k] = bd[k];
            }
    }
};

// ------------------------------------------------------------------------------------------------
// the all-pairs sweep, the first of the file's two traversals: the query (px, py, pz) of every thread of the workgroup against the
// points [0, jend), LDS tiles of NTILE points, j ascending.  Every thread of the workgroup has to come here (the barriers), with or
// without a query.  stage(j0) runs between the barriers beside the staging of point j0 (a fourth LDS column of the caller's);
// visit(j, s, d2) gets point j = base + s of the tile and the squared distance defined at the top of the file.
// ------------------------------------------------------------------------------------------------
template <class Stage, class Visit>
__device__ __forceinline__ void tile_sweep(const double* __restrict__ pts, int jend, double px, double py, double pz, double* tx, double* ty, double* tz,
                                           Stage stage, Visit visit)
{
    for (int base = 0; base < jend; base += NTILE) {
        const int j0 = base + threadIdx.x;
        __syncthreads();
        if (j0 < jend) { tx[threadIdx.x] = pts[3 * (size_t)j0]; ty[threadIdx.x] = pts[3 * (size_t)j0 + 1]; tz[threadIdx.x] = pts[3 * (size_t)j0 + 2]; stage(j0); }
        __syncthreads();
        const int cnt = jend - base < NTILE ? jend - base : NTILE;
        for (int s = 0; s < cnt; ++s) {
            const double dx = px - tx[s], dy = py - ty[s], dz = pz - tz[s];
            const double d2 = dx * dx + dy * dy + dz * dz;
            visit(base + s, s, d2);
        }
    }
}
// the staging functor of a sweep with three columns
struct NoStage { __device__ __forceinline__ void operator()(int) const {} };

// ------------------------------------------------------------------------------------------------
// brute force: query t of the list (or point t where there is no list) against every point.  Scanning j ascending with a strict
// (d, j) test is the order of normals_kernel.  The grid's fallback pass is this kernel on its list: the launch covers n queries and
// the workgroups beyond the list's length (read from the device) leave at once.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTILE) void points_knn_brute_kernel(const double* __restrict__ pts, int n, int K, const pu32* __restrict__ list,
                                                                 const pu32* __restrict__ list_len, int32_t* __restrict__ idx, double* __restrict__ dist)
{
    __shared__ double tx[NTILE], ty[NTILE], tz[NTILE];
    const int m = list ? (int)min(*list_len, (pu32)n) : n;
    if (blockIdx.x * NTILE >= m) return;                           // uniform over the workgroup
    const int t = blockIdx.x * NTILE + threadIdx.x;
    const bool active = t < m;
    const int i = active ? (list ? (int)list[t] : t) : -1;
    const double px = active ? pts[3 * (size_t)i] : 0.0, py = active ? pts[3 * (size_t)i + 1] : 0.0, pz = active ? pts[3 * (size_t)i + 2] : 0.0;
    TopK top; top.init();
    tile_sweep(pts, n, px, py, pz, tx, ty, tz, NoStage(), [&](int j, int, double d2) { if (j != i) top.offer(d2, j, K); });
    if (active) top.store(K, (size_t)i, idx, dist);
}

// ------------------------------------------------------------------------------------------------
// cell size and origin from robust statistics of a strided sample (one workgroup).  A bounding box is useless for SfM clouds: one point
// at 4e4 beside a cloud of unit size would put everything else into one cell.  Instead: the per-axis MEDIAN of the sample is the centre
// of the 2^21-cell range, and the cell size comes from neighbour distances inside the sample: with the sample a 1-in-f thinning of the
// cloud, the distance r_m to a sample point's m-th nearest sample point holds about m f points of the cloud, and between m = 2 and
// m = 8 the growth of r_m tells the local dimension D of the cloud (a surface: 2, a volume: 3), so the radius that holds T = 2K points
// is r_8 (T / (8 f))^(1/D).  Medians over the sample points throughout.  The cell size only steers speed: whatever comes out, the
// certificate and the fallback keep the result exact.  rmin > 0 (the fixed-radius search): h is at least rmin (1 + 2^-20), whatever the
// sample says.  params: [0..2] origin, [3] 1/h, [4] h_lo (a lower bound of h, see the certificate)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void lds_bitonic_sort(double* a, int len)       // len: power of two, NTILE threads
{
    for (int k = 2; k <= len; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < len; t += NTILE) {
                const int u = t ^ j;
                if (u > t) {
                    const double x = a[t], y = a[u];
                    const bool up = (t & k) == 0;
                    if ((x > y) == up) { a[t] = y; a[u] = x; }
                }
            }
        }
    __syncthreads();
}

__global__ __launch_bounds__(NTILE) void points_cell_stats_kernel(const double* __restrict__ pts, int n, int K, double rmin, double* __restrict__ params)
{
    __shared__ double sx[NSAMPLE], sy[NSAMPLE], sz[NSAMPLE], srt[NSAMPLE];
    __shared__ double med[3];
    __shared__ int s_valid;
    const int ns = n < NSAMPLE ? n : NSAMPLE;
    if (threadIdx.x == 0) s_valid = 0;
    __syncthreads();
    int mine = 0;
    for (int s = threadIdx.x; s < NSAMPLE; s += NTILE) {
        double x = INFINITY, y = INFINITY, z = INFINITY;
        if (s < ns) {
            const size_t i = (size_t)((pu64)s * (pu64)n / (pu64)ns);
            const double a = pts[3 * i], b = pts[3 * i + 1], c = pts[3 * i + 2];
            if (isfinite(a) && isfinite(b) && isfinite(c)) { x = a; y = b; z = c; ++mine; }
        }
        sx[s] = x; sy[s] = y; sz[s] = z;
    }
    if (mine) atomicAdd(&s_valid, mine);
    __syncthreads();
    const int nv = s_valid;
    // per-axis medians (the invalid entries are +inf and sort last)
    for (int a = 0; a < 3; ++a) {
        const double* src = a == 0 ? sx : a == 1 ? sy : sz;
        for (int s = threadIdx.x; s < NSAMPLE; s += NTILE) srt[s] = src[s];
        lds_bitonic_sort(srt, NSAMPLE);
        if (threadIdx.x == 0) med[a] = nv > 0 ? srt[nv / 2] : 0.0;
        __syncthreads();
    }
    // thread t: sample point 4 t against the sample; its 2nd and 8th smallest squared distances
    double best[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) best[k] = INFINITY;
    const int q = 4 * threadIdx.x;
    const double qx = sx[q], qy = sy[q], qz = sz[q];
    const bool qok = qx < INFINITY;
    for (int s = 0; s < NSAMPLE; ++s) {
        const double dx = qx - sx[s], dy = qy - sy[s], dz = qz - sz[s];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (s != q && d2 < best[7]) {
            best[7] = d2;
#pragma unroll
            for (int k = 7; k > 0; --k) if (best[k] < best[k - 1]) { const double t = best[k]; best[k] = best[k - 1]; best[k - 1] = t; }
        }
    }
    __syncthreads();
    const bool ok = qok && best[7] < INFINITY;
    srt[threadIdx.x] = ok ? best[1] : INFINITY;
    srt[NTILE + threadIdx.x] = ok ? best[7] : INFINITY;
    __syncthreads();
    lds_bitonic_sort(srt, NTILE);
    lds_bitonic_sort(srt + NTILE, NTILE);
    if (threadIdx.x == 0) {
        int nq = 0;
        for (int t = 0; t < NTILE; ++t) nq += srt[NTILE + t] < INFINITY ? 1 : 0;
        double h = 1.0;
        if (nq > 0) {
            const double r2 = sqrt(srt[nq / 2]), r8 = sqrt(srt[NTILE + nq / 2]);
            double D = 2.0;
            if (r2 > 0.0 && r8 > r2) D = log(4.0) / log(r8 / r2);
            D = D < 1.0 ? 1.0 : D > 3.0 ? 3.0 : D;
            const double f = (double)n / (double)ns, T = 2.0 * (double)K;
            if (r8 > 0.0) h = r8 * pow(T / (8.0 * f), 1.0 / D);
        }
        if (!(h >= 1e-100 && h <= 1e100)) h = 1.0;
        if (rmin > 0.0) { const double hr = rmin * (1.0 + 0x1p-20); h = h < hr ? hr : h; }      // rmin <= 1e100 (the caller's business)
        const double inv_h = 1.0 / h;
        params[0] = med[0] - 0x1p20 * h; params[1] = med[1] - 0x1p20 * h; params[2] = med[2] - 0x1p20 * h;
        params[3] = inv_h;
        params[4] = (1.0 / inv_h) * (1.0 - 0x1p-40);
    }
}

// position of a coordinate in cell units, and the cell it is binned into.  The ONE definition used by the binning and by the
// certificate: what matters is not where a point "really" lies but what this function says.
__device__ __forceinline__ double cell_pos(double x, double origin, double inv_h) { return (x - origin) * inv_h; }
__device__ __forceinline__ int cell_of(double t) { return t < 1.0 ? 0 : !(t < (double)CELL_MAX) ? CELL_MAX : (int)t; }
__device__ __forceinline__ pu64 cell_key(int cx, int cy, int cz) { return ((pu64)cx << (2 * CELL_BITS)) | ((pu64)cy << CELL_BITS) | (pu64)cz; }

// key of every point; a point with a non-finite coordinate gets the all-ones key: it sorts behind every cell and no search looks there
__global__ __launch_bounds__(256) void points_cell_key_kernel(const double* __restrict__ pts, int n, const double* __restrict__ params, pu64* __restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    pu64 key = ~0ull;
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
        const double inv_h = params[3];
        key = cell_key(cell_of(cell_pos(x, params[0], inv_h)), cell_of(cell_pos(y, params[1], inv_h)), cell_of(cell_pos(z, params[2], inv_h)));
    }
    keys[i] = key;
}

// the cloud in cell order (a query's candidates are then runs of neighbouring records)
__global__ __launch_bounds__(256) void points_gather_kernel(const double* __restrict__ pts, const pu32* __restrict__ order, int n, double* __restrict__ spts)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const size_t i = order[p];
    spts[3 * (size_t)p] = pts[3 * i]; spts[3 * (size_t)p + 1] = pts[3 * i + 1]; spts[3 * (size_t)p + 2] = pts[3 * i + 2];
}

// first position of the sorted keys with keys[pos] >= key, in [lo, n): at most 32 halvings
__device__ __forceinline__ int keys_lower_bound(const pu64* __restrict__ keys, int lo, int n, pu64 key)
{
    int hi = n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------
// the cell-run visit, the second traversal: cells with the same (x, y) and consecutive z are consecutive keys, so the column
// (X, Y, z0 .. z1), 0 <= z0 <= z1 <= CELL_MAX, is ONE run of the sorted keys, found by two binary searches.  visit(s, d2) gets every
// record s of the run (a position in cell order, the query's own included) and its squared distance from (qx, qy, qz).
// ------------------------------------------------------------------------------------------------
template <class Visit>
__device__ __forceinline__ void cell_run_visit(const pu64* __restrict__ keys, const double* __restrict__ spts, int n, int X, int Y, int z0, int z1,
                                               double qx, double qy, double qz, Visit visit)
{
    const pu64 k0 = cell_key(X, Y, z0), k1 = cell_key(X, Y, z1);
    const int a = keys_lower_bound(keys, 0, n, k0);
    if (a >= n || keys[a] > k1) return;                                // an empty run
    const int b = keys_lower_bound(keys, a, n, k1 + 1ull);
    for (int s = a; s < b; ++s) {
        const double ex = qx - spts[3 * (size_t)s], ey = qy - spts[3 * (size_t)s + 1], ez = qz - spts[3 * (size_t)s + 2];
        const double d2 = ex * ex + ey * ey + ez * ez;
        visit(s, d2);
    }
}

// ------------------------------------------------------------------------------------------------
// grid search.  Thread p handles the p-th point in cell order (a wave walks the same cells) and writes to the row of its point.
//
// Ring r visits the cells of the cube [c - r, c + r]^3 (clipped to [0, CELL_MAX]) that ring r - 1 has not visited, column by column
// (cell_run_visit).
//
// The certificate.  Let t_q = cell_pos(q_a) on axis a, c = cell_of(t_q) with 0 < c < CELL_MAX on every axis (a query in a border cell is
// not searched at all: border cells are unbounded outward and hold whatever was clamped into them).  A point p that the cube has NOT
// visited has, on some axis, cell_of(t_p) >= m with m = c + r + 1 <= CELL_MAX, or cell_of(t_p) <= m' - 1 with m' = c - r >= 1.  By the
// definition of cell_of that means t_p >= m, resp. t_p < m', also where p was clamped (clamping from above only yields CELL_MAX, from
// below only 0), while c <= t_q < c + 1.  cell_pos rounds twice: t = (x - o)(1 + e1) inv_h (1 + e2), |e| <= 2^-53, so x - o = t / (inv_h
// (1 + e)) with |e| < 2^-51 (a subnormal product is off by less than 1e-323, far inside the slack below), and therefore
//     p_a - q_a >= (m - t_q - (m + |t_q|) 2^-51) / inv_h        resp.        q_a - p_a >= (t_q - m' - (m' + |t_q|) 2^-51) / inv_h.
// The code evaluates these gaps with 2^-48 in place of 2^-51, which covers the roundings of the evaluation itself, takes the smallest
// gap over the faces that exist (a face beyond the clamped range has nothing behind it) and multiplies by h_lo = fl(1 / inv_h) (1 - 2^-40):
// `bound` is then below the true distance from q to any unvisited point by a relative 2^-41, while the distance the kernels COMPUTE for
// a pair is below the true one by at most a relative 2^-50 (h >= 1e-100 keeps the squares of such gaps from underflowing).  Hence every unvisited p has
// computed d(q, p) >= bound, and with dk < bound -- STRICTLY: at d == dk a lower index would still enter -- no unvisited point can be
// among the first K by (d, j).  A non-finite gap (t_q overflowed) compares false and certifies nothing.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTILE) void points_knn_grid_kernel(const pu64* __restrict__ keys, const pu32* __restrict__ order, const double* __restrict__ spts,
                                                                int n, int K, const double* __restrict__ params, int32_t* __restrict__ idx,
                                                                double* __restrict__ dist, pu32* __restrict__ fb_list, pu32* __restrict__ fb_len)
{
    const int p = blockIdx.x * NTILE + threadIdx.x;
    if (p >= n) return;
    const pu64 key = keys[p];
    const int i = (int)order[p];
    TopK top; top.init();
    if (key >> 63) { top.store(K, (size_t)i, idx, dist); return; }        // non-finite: no neighbours
    const int cx = (int)(key >> (2 * CELL_BITS)), cy = (int)(key >> CELL_BITS) & CELL_MAX, cz = (int)key & CELL_MAX;
    const double qx = spts[3 * (size_t)p], qy = spts[3 * (size_t)p + 1], qz = spts[3 * (size_t)p + 2];
    const double inv_h = params[3], h_lo = params[4];
    const double tq[3] = { cell_pos(qx, params[0], inv_h), cell_pos(qy, params[1], inv_h), cell_pos(qz, params[2], inv_h) };
    const int c[3] = { cx, cy, cz };
    bool certified = false;
    const bool border = cx == 0 || cx == CELL_MAX || cy == 0 || cy == CELL_MAX || cz == 0 || cz == CELL_MAX;
    if (!border) {
        for (int r = 0; r <= RMAX; ++r) {
            for (int dx = -r; dx <= r; ++dx) {
                const int X = cx + dx;
                if (X < 0 || X > CELL_MAX) continue;
                for (int dy = -r; dy <= r; ++dy) {
                    const int Y = cy + dy;
                    if (Y < 0 || Y > CELL_MAX) continue;
                    const bool shell = dx == -r || dx == r || dy == -r || dy == r;
                    // a column of the shell: z in [cz - r, cz + r]; an inner column: its two ends only (the same cell where r = 0: shell)
                    const int nrun = shell ? 1 : 2;
                    for (int run = 0; run < nrun; ++run) {
                        int z0 = shell ? cz - r : run == 0 ? cz - r : cz + r;
                        int z1 = shell ? cz + r : z0;
                        if (z1 < 0 || z0 > CELL_MAX) continue;
                        z0 = z0 < 0 ? 0 : z0; z1 = z1 > CELL_MAX ? CELL_MAX : z1;
                        cell_run_visit(keys, spts, n, X, Y, z0, z1, qx, qy, qz, [&](int s, double d2) { if (s != p) top.offer(d2, (int)order[s], K); });
                    }
                }
            }
            double gmin = INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int m_hi = c[a] + r + 1, m_lo = c[a] - r;
                if (m_hi <= CELL_MAX) { const double g = ((double)m_hi - tq[a]) - ((double)m_hi + fabs(tq[a])) * 0x1p-48; gmin = g < gmin || !(g == g) ? g : gmin; }
                if (m_lo >= 1)        { const double g = (tq[a] - (double)m_lo) - ((double)m_lo + fabs(tq[a])) * 0x1p-48; gmin = g < gmin || !(g == g) ? g : gmin; }
            }
            const double bound = gmin * h_lo;
            if (top.dk < bound) { certified = true; break; }
        }
    }
    if (!certified) { fb_list[atomicAdd(fb_len, 1u)] = (pu32)i; return; }
    top.store(K, (size_t)i, idx, dist);
}

// SFMHIP_POINTS_AUTO.  Measured (profiles/r09_time_points.log: normals, K = 10, noisy sphere / that sphere with 1 % far outliers / a
// volume cloud): 300,000 is the smallest size from which the grid is faster by at least 10 % on all three; below it the brute-force
// pass over the fallback list (one sweep of the cloud at one-workgroup speed, 13 ms at 100k) can cost more than the whole all-pairs sweep.
#define POINTS_AUTO_GRID_FROM 300000
int sfm_points_auto_method(int n) { return n >= POINTS_AUTO_GRID_FROM ? SFMHIP_POINTS_GRID : SFMHIP_POINTS_BRUTE; }

// the binning shared by the two grid searches: cell statistics, keys, stable sort, the cloud gathered into cell order, an empty fallback
// list.  Everything lives in one block of the cache that `hold` gives back.
struct PointsGrid { const double* params; const pu64* keys; const pu32* order; const double* spts; pu32* list; };
static int points_grid_enqueue(sfmhip_ctx* ctx, SfmPoolHold& hold, const double* d_pts, int n, int K, double rmin, PointsGrid* G)
{
    hipStream_t st = ctx->stream;
    if (!ctx->d_points_fallback) {
        void* q = nullptr;
        const int rc = sfm_pool_get(ctx, 256, &q);            // kept for the life of the context
        if (rc != SFMHIP_OK) return rc;
        ctx->d_points_fallback = (unsigned*)q;
    }
    // one block of the cache, carved up
    const size_t N = (size_t)n;
    SfmCarve carve;
    const size_t o_par = carve(8 * sizeof(double)), o_spts = carve(N * 24), o_list = carve(N * 4);
    SfmSort S(carve, N);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    S.bind(w);
    double* params = (double*)(w + o_par);
    double* spts = (double*)(w + o_spts);
    SFM_HIP_TRY(ctx, hipMemsetAsync(ctx->d_points_fallback, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(points_cell_stats_kernel, dim3(1), dim3(NTILE), 0, st, d_pts, n, K, rmin, params);
    hipLaunchKernelGGL(points_cell_key_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, d_pts, n, (const double*)params, S.k[0]);
    const int cur = S.sort(st, N, 0, 64, true);
    hipLaunchKernelGGL(points_gather_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, d_pts, (const pu32*)S.v[cur], n, spts);
    G->params = params; G->keys = S.k[cur]; G->order = S.v[cur]; G->spts = spts; G->list = (pu32*)(w + o_list);
    return SFMHIP_OK;
}

int sfm_points_knn_enqueue(sfmhip_ctx* ctx, const double* d_pts, int n, int K, int method, int32_t* d_idx, double* d_dist)
{
    if (method == SFMHIP_POINTS_AUTO) method = sfm_points_auto_method(n);
    hipStream_t st = ctx->stream;
    const int nb = ceil_div(n, NTILE);
    if (method == SFMHIP_POINTS_BRUTE) {
        hipLaunchKernelGGL(points_knn_brute_kernel, dim3(nb), dim3(NTILE), 0, st, d_pts, n, K, (const pu32*)nullptr, (const pu32*)nullptr, d_idx, d_dist);
        SFM_HIP_TRY(ctx, hipGetLastError());
        return SFMHIP_OK;
    }
    SfmPoolHold hold(ctx);
    PointsGrid G;
    const int rc = points_grid_enqueue(ctx, hold, d_pts, n, K, 0.0, &G);
    if (rc != SFMHIP_OK) return rc;
    hipLaunchKernelGGL(points_knn_grid_kernel, dim3(nb), dim3(NTILE), 0, st, G.keys, G.order, G.spts, n, K, G.params, d_idx, d_dist, G.list, ctx->d_points_fallback);
    hipLaunchKernelGGL(points_knn_brute_kernel, dim3(nb), dim3(NTILE), 0, st, d_pts, n, K, (const pu32*)G.list, (const pu32*)ctx->d_points_fallback, d_idx, d_dist);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// statistical outlier removal (PCL StatisticalOutlierRemoval / Open3D remove_statistical_outlier): mean distance to the K nearest
// neighbours, then keep what lies within mu + std_ratio * sigma of the finite means.  The sums are fixed-order trees (a tile per
// workgroup, then one workgroup over the tiles), so a rerun gives the same bits.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void points_mean_dist_kernel(const int32_t* __restrict__ idx, const double* __restrict__ dist, int n, int K, double* __restrict__ mean_dist)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    bool full = true;
    for (int k = 0; k < K; ++k) { s += dist[(size_t)i * K + k]; full = full && idx[(size_t)i * K + k] >= 0; }
    mean_dist[i] = full ? s / (double)K : INFINITY;
}

#define RED_TILE 4096
// 256 threads: tree sum of (v, c) over the workgroup, valid in thread 0
__device__ __forceinline__ void block_tree_sum(double& v, double& c, double* sv, double* sc)
{
    sv[threadIdx.x] = v; sc[threadIdx.x] = c;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { sv[threadIdx.x] += sv[threadIdx.x + off]; sc[threadIdx.x] += sc[threadIdx.x + off]; }
        __syncthreads();
    }
    v = sv[0]; c = sc[0];
}
// pass 0: partial[b] = (sum, count) of the finite m of tile b;  pass 1: (sum of (m - mu)^2, count), mu = stats[0]
__global__ __launch_bounds__(256) void points_stat_tile_kernel(const double* __restrict__ m, int n, int pass, const double* __restrict__ stats, double* __restrict__ partial)
{
    __shared__ double sv[256], sc[256];
    const double mu = pass ? stats[0] : 0.0;
    double v = 0.0, c = 0.0;
    for (int r = 0; r < RED_TILE / 256; ++r) {
        const size_t i = (size_t)blockIdx.x * RED_TILE + (size_t)r * 256 + threadIdx.x;
        if (i < (size_t)n) {
            const double x = m[i];
            if (isfinite(x)) { const double e = x - mu; v += pass ? e * e : x; c += 1.0; }
        }
    }
    block_tree_sum(v, c, sv, sc);
    if (threadIdx.x == 0) { partial[2 * (size_t)blockIdx.x] = v; partial[2 * (size_t)blockIdx.x + 1] = c; }
}
// one workgroup over the tiles.  pass 0: stats[0] = mu;  pass 1: stats[1] = sigma, stats[2] = thr = mu + ratio * sigma
__global__ __launch_bounds__(256) void points_stat_top_kernel(const double* __restrict__ partial, int nt, int pass, double ratio, double* __restrict__ stats)
{
    __shared__ double sv[256], sc[256];
    double v = 0.0, c = 0.0;
    for (int t = threadIdx.x; t < nt; t += 256) { v += partial[2 * (size_t)t]; c += partial[2 * (size_t)t + 1]; }
    block_tree_sum(v, c, sv, sc);
    if (threadIdx.x == 0) {
        if (pass == 0) stats[0] = v / c;                          // no finite value: 0 / 0 = NaN
        else { const double sigma = sqrt(v / c); stats[1] = sigma; stats[2] = stats[0] + ratio * sigma; }
    }
}
__global__ __launch_bounds__(256) void points_keep_kernel(const double* __restrict__ m, int n, const double* __restrict__ stats, uint8_t* __restrict__ keep)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keep[i] = m[i] <= stats[2] ? 1 : 0;               // false for an infinite mean and for a NaN threshold
}

// ------------------------------------------------------------------------------------------------
// fixed radius: count[i] = #{ j != i : d(i, j) <= r }, d the distance above, the comparison on the computed d, inclusive.
//
// The gate.  The decision `sqrt(d2) <= r` is made without the square root on both sides of a thin band: with q = fl(r * r) normal and
// finite, lo2 = q (1 - 2^-50) <= r^2 <= q (1 + 2^-50) = hi2 whatever the three roundings did (each is off by a relative 2^-53).
// d2 <= lo2: the real root is <= r, and rounding is monotone, so the computed d is <= r.  d2 > hi2: the real root exceeds
// r sqrt(1 + 3/4 2^-50) > r (1 + 2^-52), which is at least the double after r, so the computed d is > r.  In between the root is
// taken.  r = 0: lo2 = -1, hi2 = 0 (d2 = 0 takes the root: 0 <= 0).  q subnormal, zero or infinite: lo2 = -1, hi2 = inf, every
// candidate takes the root.  A NaN d2 (a non-finite coordinate on either side) fails `d2 <= hi2`; an infinite one has an infinite root.
// ------------------------------------------------------------------------------------------------
struct RadiusGate { double r, lo2, hi2; };
static inline RadiusGate radius_gate(double r)
{
    RadiusGate g = { r, -1.0, INFINITY };
    const double q = r * r;
    if (r == 0.0) g.hi2 = 0.0;
    else if (q >= 0x1p-960 && q <= 0x1p960) { g.lo2 = q * (1.0 - 0x1p-50); g.hi2 = q * (1.0 + 0x1p-50); }
    return g;
}
__device__ __forceinline__ int radius_hit(double d2, const RadiusGate& g) { return d2 <= g.hi2 && (d2 <= g.lo2 || sqrt(d2) <= g.r) ? 1 : 0; }

// all pairs
__global__ __launch_bounds__(NTILE) void points_radius_brute_kernel(const double* __restrict__ pts, int n, RadiusGate g, int32_t* __restrict__ count)
{
    __shared__ double tx[NTILE], ty[NTILE], tz[NTILE];
    const int i = blockIdx.x * NTILE + threadIdx.x;
    const bool active = i < n;
    const double px = active ? pts[3 * (size_t)i] : 0.0, py = active ? pts[3 * (size_t)i + 1] : 0.0, pz = active ? pts[3 * (size_t)i + 2] : 0.0;
    int c = 0;
    tile_sweep(pts, n, px, py, pz, tx, ty, tz, NoStage(), [&](int j, int, double d2) { c += j != i ? radius_hit(d2, g) : 0; });
    if (active) count[i] = c;
}

// ------------------------------------------------------------------------------------------------
// the 27-cell visit of every fixed-radius sweep on the grid.  The p-th point in cell order, with key `key` (finite: bit 63 clear),
// visits the 3 x 3 columns (x, y) of its cell's neighbourhood, each with z in [cz - 1, cz + 1] as ONE run of the sorted keys
// (cell_run_visit, whose visit(s, d2) this passes on), everything clipped to [0, CELL_MAX].  No rings, no test at run time, no fallback
// list: the cell size is chosen so that the 27 cells suffice, h >= r (1 + 2^-20) (points_cell_stats_kernel, rmin = r).
//
// Why they suffice.  For a finite x let delta = x - o (real) and t = cell_pos(x) = fl(fl(delta) inv_h) = delta inv_h (1 + e), |e| < 2^-51,
// wherever fl(delta) is finite; cell_pos is monotone in x.  For 1 <= m <= 2^21 therefore
//     t >= m  =>  delta >= m (1 - 2^-51) / inv_h,            t < m  =>  delta < m (1 + 2^-51) / inv_h
// (m / inv_h >= 1e-100 is far from subnormal; an overflowed fl(delta) or t only lies farther out on its side).  Let c = cell_of(t_q) on
// some axis.  By the definition of cell_of, t_q < c + 1 unless c = CELL_MAX, and t_q >= c unless c = 0: clamping from above only yields
// CELL_MAX, from below only 0.  A finite point p outside the 27 cells has, on some axis, cell_of(t_p) >= c + 2 -- then c < CELL_MAX,
// t_p >= c + 2 and t_q < c + 1 -- or cell_of(t_p) <= c - 2 -- then c > 0, t_p < c - 1 and t_q >= c.  Either way, with 2c + 3 < 2^23,
//     |p_a - q_a| = |delta_p - delta_q| > (1 - 2^-28) / inv_h.
// The cell size IS 1 / inv_h, and inv_h = fl(1 / h) with h >= fl(r (1 + 2^-20)), so 1 / inv_h >= r (1 + 2^-20) (1 - 2^-52): the true
// distance from q to p exceeds r (1 + 2^-21).  The distance the kernels COMPUTE is below the true one by at most a relative 2^-50 (the
// slack the certificate above names), so it exceeds r: no point outside the 27 cells can be counted.  What IS visited is decided by
// the computed distance itself, so a cell size larger than needed (a small r against the point spacing; r = 0) changes the work, never
// the result.
//
// Border cells.  The argument is EXTENDED to them rather than handing their queries to a brute-force pass: nothing above needs t_q to be
// bounded outward.  A query in or next to a clamped border cell visits that cell whole, with whatever was clamped into it, and the
// unvisited side only needs the definition of cell_of.  (Far outliers are what lands in border cells -- 16,000 of the 20,000 far points
// of the 2M-point outlier cloud at a radius of 0.02 -- and an all-pairs pass for them would cost 60 times the search itself.)
// ------------------------------------------------------------------------------------------------
template <class Visit>
__device__ __forceinline__ void cells27_visit(const pu64* __restrict__ keys, const double* __restrict__ spts, int n, int p, pu64 key, Visit visit)
{
    const int cx = (int)(key >> (2 * CELL_BITS)), cy = (int)(key >> CELL_BITS) & CELL_MAX, cz = (int)key & CELL_MAX;
    const double qx = spts[3 * (size_t)p], qy = spts[3 * (size_t)p + 1], qz = spts[3 * (size_t)p + 2];
    const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz < CELL_MAX ? cz + 1 : CELL_MAX;
    for (int dx = -1; dx <= 1; ++dx) {
        const int X = cx + dx;
        if (X < 0 || X > CELL_MAX) continue;
        for (int dy = -1; dy <= 1; ++dy) {
            const int Y = cy + dy;
            if (Y < 0 || Y > CELL_MAX) continue;
            cell_run_visit(keys, spts, n, X, Y, z0, z1, qx, qy, qz, visit);
        }
    }
}

// grid count: thread p is the p-th point in cell order
__global__ __launch_bounds__(NTILE) void points_radius_grid_kernel(const pu64* __restrict__ keys, const pu32* __restrict__ order, const double* __restrict__ spts,
                                                                   int n, RadiusGate g, int32_t* __restrict__ count)
{
    const int p = blockIdx.x * NTILE + threadIdx.x;
    if (p >= n) return;
    const pu64 key = keys[p];
    const int i = (int)order[p];
    if (key >> 63) { count[i] = 0; return; }                               // non-finite: counts nobody
    int c = 0;
    cells27_visit(keys, spts, n, p, key, [&](int s, double d2) { c += s != p ? radius_hit(d2, g) : 0; });
    count[i] = c;
}

// SFMHIP_POINTS_AUTO of the radius count.  Measured (profiles/r10_time_radius.log: median count 10 and 100, noisy sphere / that sphere
// with 1 % far outliers / a volume cloud, 20k .. 2M points): the grid is faster by at least 10 % on all three clouds at every measured
// size, three times at 20,000 points, the smallest one measured, so that is the crossover.
#define RADIUS_AUTO_GRID_FROM 20000
// beyond this radius the binning has nothing to offer (and h = r would leave the range the cell statistics are written for)
#define RADIUS_GRID_MAX 1e100
// the cell size where r is small against the point spacing: what the kNN grid derives from its sample for this K
#define RADIUS_GRID_K 4

// the method a fixed-radius sweep runs with: AUTO by the caller's measured crossover, brute force beyond RADIUS_GRID_MAX
static inline int radius_method(int method, int n, double r, int auto_grid_from)
{
    if (method == SFMHIP_POINTS_AUTO) method = n >= auto_grid_from ? SFMHIP_POINTS_GRID : SFMHIP_POINTS_BRUTE;
    return r > RADIUS_GRID_MAX ? SFMHIP_POINTS_BRUTE : method;
}
// the binning of a fixed-radius sweep at radius r (leaves the context's fallback count at 0: these sweeps have no list)
static inline int radius_grid_enqueue(sfmhip_ctx* ctx, SfmPoolHold& hold, const double* d_pts, int n, double r, PointsGrid* G)
{
    return points_grid_enqueue(ctx, hold, d_pts, n, RADIUS_GRID_K, r, G);
}
// count[i] by all pairs, or (G given) on a binning of radius_grid_enqueue at g.r that the caller holds
static void radius_count_launch(hipStream_t st, const double* d_pts, const PointsGrid* G, int n, const RadiusGate& g, int32_t* d_count)
{
    const int nb = ceil_div(n, NTILE);
    if (!G) hipLaunchKernelGGL(points_radius_brute_kernel, dim3(nb), dim3(NTILE), 0, st, d_pts, n, g, d_count);
    else hipLaunchKernelGGL(points_radius_grid_kernel, dim3(nb), dim3(NTILE), 0, st, G->keys, G->order, G->spts, n, g, d_count);
}

// count[i] of a device cloud, on the context's stream; method: SFMHIP_POINTS_*
static int points_radius_count_enqueue(sfmhip_ctx* ctx, const double* d_pts, int n, double r, int method, int32_t* d_count)
{
    method = radius_method(method, n, r, RADIUS_AUTO_GRID_FROM);
    SfmPoolHold hold(ctx);
    PointsGrid G;
    if (method != SFMHIP_POINTS_BRUTE) {
        const int rc = radius_grid_enqueue(ctx, hold, d_pts, n, r, &G);
        if (rc != SFMHIP_OK) return rc;
    }
    radius_count_launch(ctx->stream, d_pts, method == SFMHIP_POINTS_BRUTE ? nullptr : &G, n, radius_gate(r), d_count);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

__global__ __launch_bounds__(256) void points_count_keep_kernel(const int32_t* __restrict__ count, int n, int min_neighbors, uint8_t* __restrict__ keep)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keep[i] = count[i] >= min_neighbors ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// voxel-grid down-sampling.  origin_a = (min over the finite points of x_a) - voxel * 0.5, c_a = floor((x_a - origin_a) / voxel) -- a
// subtraction, a true division, a floor --, a voxel is a distinct (c_x, c_y, c_z), voxels are numbered in ascending (c_x, c_y, c_z), and a
// centroid is ((x_j0 + x_j1) + x_j2 ...) / count over the voxel's points in ascending original index: the order in which the STABLE sort
// of the packed key (identity values) delivers them.  The minimum is exact, so its reduction order does not matter; a rerun gives the
// same bits.  c_a >= 0 always (origin <= min <= x, and rounding is monotone); c_a > CELL_MAX raises the overflow flag.
// One thread sums a whole voxel: a voxel that holds the entire cloud is one sequential chain (accepted: the point of the operation is
// many small voxels).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void block_min3(double (&v)[3], double* sm)          // 256 threads, result in every thread
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        sm[threadIdx.x] = v[a];
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) { const double y = sm[threadIdx.x + off]; if (y < sm[threadIdx.x]) sm[threadIdx.x] = y; }
            __syncthreads();
        }
        v[a] = sm[0];
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void voxel_min_tile_kernel(const double* __restrict__ pts, int n, double* __restrict__ partial)
{
    __shared__ double sm[256];
    double v[3] = { INFINITY, INFINITY, INFINITY };
    for (int r = 0; r < RED_TILE / 256; ++r) {
        const size_t i = (size_t)blockIdx.x * RED_TILE + (size_t)r * 256 + threadIdx.x;
        if (i < (size_t)n) {
            const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
            if (isfinite(x) && isfinite(y) && isfinite(z)) { v[0] = x < v[0] ? x : v[0]; v[1] = y < v[1] ? y : v[1]; v[2] = z < v[2] ? z : v[2]; }
        }
    }
    block_min3(v, sm);
    if (threadIdx.x < 3) partial[3 * (size_t)blockIdx.x + threadIdx.x] = v[threadIdx.x];
}
// one workgroup over the tiles: origin[a] (+inf where the cloud has no finite point); the overflow flag starts at 0
__global__ __launch_bounds__(256) void voxel_min_top_kernel(const double* __restrict__ partial, int nt, double voxel, double* __restrict__ origin, pu32* __restrict__ overflow)
{
    __shared__ double sm[256];
    double v[3] = { INFINITY, INFINITY, INFINITY };
    for (int t = threadIdx.x; t < nt; t += 256)
#pragma unroll
        for (int a = 0; a < 3; ++a) { const double y = partial[3 * (size_t)t + a]; v[a] = y < v[a] ? y : v[a]; }
    block_min3(v, sm);
    if (threadIdx.x < 3) origin[threadIdx.x] = v[threadIdx.x] - voxel * 0.5;
    if (threadIdx.x == 0) *overflow = 0u;
}
__global__ __launch_bounds__(256) void voxel_key_kernel(const double* __restrict__ pts, int n, double voxel, const double* __restrict__ origin,
                                                        pu64* __restrict__ keys, pu32* __restrict__ overflow)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    pu64 key = ~0ull;
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
        const double cx = floor((x - origin[0]) / voxel), cy = floor((y - origin[1]) / voxel), cz = floor((z - origin[2]) / voxel);
        const double cmax = (double)CELL_MAX;
        if (cx >= 0.0 && cx <= cmax && cy >= 0.0 && cy <= cmax && cz >= 0.0 && cz <= cmax) key = cell_key((int)cx, (int)cy, (int)cz);
        else *overflow = 1u;                                               // every writer writes the same value
    }
    keys[i] = key;
}
// thread t: the t-th point in key order writes its voxel number; the head of a run also sums the run
__global__ __launch_bounds__(256) void voxel_centroid_kernel(const pu64* __restrict__ keys, const pu32* __restrict__ order, const double* __restrict__ pts, int n,
                                                             const pu32* __restrict__ excl, const pu32* __restrict__ overflow, double* __restrict__ centroids,
                                                             int32_t* __restrict__ counts, int32_t* __restrict__ voxel_of, int32_t* __restrict__ n_voxels)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0) *n_voxels = *overflow ? -1 : (int32_t)excl[n];
    if (t >= n) return;
    const pu64 key = keys[t];
    const size_t i = order[t];
    if (key >> 63) { if (voxel_of) voxel_of[i] = -1; return; }
    const bool head = t == 0 || keys[t - 1] != key;
    const int v = (int)excl[t] + (head ? 1 : 0) - 1;                       // heads at or before t, minus one
    if (voxel_of) voxel_of[i] = v;
    if (!head) return;
    double sx = pts[3 * i], sy = pts[3 * i + 1], sz = pts[3 * i + 2];
    int c = 1;
    for (int s = t + 1; s < n && keys[s] == key; ++s, ++c) {
        const size_t j = order[s];
        sx += pts[3 * j]; sy += pts[3 * j + 1]; sz += pts[3 * j + 2];
    }
    centroids[3 * (size_t)v] = sx / (double)c; centroids[3 * (size_t)v + 1] = sy / (double)c; centroids[3 * (size_t)v + 2] = sz / (double)c;
    if (counts) counts[v] = c;
}

// everything on the context's stream; d_counts / d_voxel_of / d_origin may be null
static int voxel_downsample_enqueue(sfmhip_ctx* ctx, const double* d_pts, int n, double voxel, double* d_centroids, int32_t* d_counts,
                                    int32_t* d_voxel_of, int32_t* d_n_voxels, double* d_origin)
{
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)n;
    const int nt = ceil_div(n, RED_TILE), nb = ceil_div(n, 256);
    SfmCarve carve;
    const size_t o_org = carve(4 * sizeof(double)), o_ovf = carve(sizeof(pu32)), o_part = carve((size_t)3 * nt * sizeof(double));
    SfmSort S(carve, N); SfmScan F(carve, N + 1);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    S.bind(w); F.bind(w);
    double* origin = (double*)(w + o_org);
    pu32* overflow = (pu32*)(w + o_ovf);
    hipLaunchKernelGGL(voxel_min_tile_kernel, dim3(nt), dim3(256), 0, st, d_pts, n, (double*)(w + o_part));
    hipLaunchKernelGGL(voxel_min_top_kernel, dim3(1), dim3(256), 0, st, (const double*)(w + o_part), nt, voxel, origin, overflow);
    hipLaunchKernelGGL(voxel_key_kernel, dim3(nb), dim3(256), 0, st, d_pts, n, voxel, (const double*)origin, S.k[0], overflow);
    const int cur = S.sort(st, N, 0, 64, true);
    sfm_enqueue_run_heads(st, S.k[cur], N, 1ull << 63, F.data);           // a point outside every voxel has the top bit set: no run of its own
    F.scan(st, N + 1);                                                     // the number of voxels in F.data[n]
    hipLaunchKernelGGL(voxel_centroid_kernel, dim3(nb), dim3(256), 0, st, (const pu64*)S.k[cur], (const pu32*)S.v[cur], d_pts, n, (const pu32*)F.data,
                       (const pu32*)overflow, d_centroids, d_counts, d_voxel_of, d_n_voxels);
    SFM_HIP_TRY(ctx, hipGetLastError());
    if (d_origin) SFM_HIP_TRY(ctx, hipMemcpyAsync(d_origin, origin, 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    return SFMHIP_OK;
}
// the door for mesh.hip (vertex clustering), declared in common.hpp
int sfm_voxel_downsample_enqueue(sfmhip_ctx* ctx, const double* d_pts, int n, double voxel, double* d_centroids, int32_t* d_counts, int32_t* d_voxel_of,
                                 int32_t* d_n_voxels)
{
    return voxel_downsample_enqueue(ctx, d_pts, n, voxel, d_centroids, d_counts, d_voxel_of, d_n_voxels, nullptr);
}

// ------------------------------------------------------------------------------------------------
// DBSCAN / Euclidean clustering (PCL EuclideanClusterExtraction, Open3D cluster_dbscan; the definition is in sfmhip.h).  count[] is
// the radius count above; core[i] = finite and count[i] + 1 >= min_points; two core points within r (radius_hit) are linked; a cluster
// is a connected component of the core points, numbered by its smallest core index; a non-core point takes the smallest number among
// its core neighbours (border), else -1.  Everything is integer work on decisions radius_hit makes, so the labels do not depend on the
// method, the launch geometry or the order in which the atomics land.
//
// The components: a union-find over ORIGINAL indices, parent[x] <= x for every core x at all times (parent[x] == x: a root; a non-core
// entry is never read).  A union hooks the LARGER root under the smaller with atomicCAS(parent + hi, hi, lo), so a root is hooked once
// and the root of a finished component is its smallest member: the numbering needs nothing more than the roots in index order.
// Every access to parent[] while unions run (cluster_link_*, cluster_flatten_kernel) is an agent-scope atomic -- a plain load may be
// served from a line another XCD's L2 has since changed; the kernels after them read it with plain loads behind the kernel boundary.
//
// Termination of cluster_find / cluster_unite, and the retry cap: unionfind.hpp, which mesh.hip shares.
// ------------------------------------------------------------------------------------------------
// core flags, and every core point a root
__global__ __launch_bounds__(256) void cluster_init_kernel(const double* __restrict__ pts, const int32_t* __restrict__ count, int n, int min_points,
                                                           uint8_t* __restrict__ core, pu32* __restrict__ parent)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    core[i] = isfinite(x) && isfinite(y) && isfinite(z) && count[i] >= min_points - 1 ? 1 : 0;
    parent[i] = (pu32)i;
}

// link sweep, all pairs: core point i unites itself with every core j < i within r (each pair from its larger index only, so a
// workgroup needs the tiles below its own last point and no others).
__global__ __launch_bounds__(NTILE) void cluster_link_brute_kernel(const double* __restrict__ pts, int n, RadiusGate g, const uint8_t* __restrict__ core,
                                                                   pu32* parent, pu32* err)
{
    __shared__ double tx[NTILE], ty[NTILE], tz[NTILE];
    __shared__ int tc[NTILE];
    const int i = blockIdx.x * NTILE + threadIdx.x;
    const bool mine = i < n && core[i];
    if (!__syncthreads_or(mine ? 1 : 0)) return;                           // uniform: no core point in this workgroup
    const double px = mine ? pts[3 * (size_t)i] : 0.0, py = mine ? pts[3 * (size_t)i + 1] : 0.0, pz = mine ? pts[3 * (size_t)i + 2] : 0.0;
    const int jend = n < (blockIdx.x + 1) * NTILE ? n : (blockIdx.x + 1) * NTILE;
    pu32 me = (pu32)i;
    tile_sweep(pts, jend, px, py, pz, tx, ty, tz, [&](int j0) { tc[threadIdx.x] = core[j0]; }, [&](int j, int s, double d2) {
        if (mine && j < i && tc[s] && radius_hit(d2, g)) me = cluster_unite(parent, me, (pu32)j, err);
    });
}

// link sweep on the grid
__global__ __launch_bounds__(NTILE) void cluster_link_grid_kernel(const pu64* __restrict__ keys, const pu32* __restrict__ order, const double* __restrict__ spts,
                                                                  int n, RadiusGate g, const uint8_t* __restrict__ core, pu32* parent, pu32* err)
{
    const int p = blockIdx.x * NTILE + threadIdx.x;
    if (p >= n) return;
    const pu64 key = keys[p];
    const pu32 i = order[p];
    if ((key >> 63) || !core[i]) return;
    pu32 me = i;
    cells27_visit(keys, spts, n, p, key, [&](int s, double d2) {
        if (!radius_hit(d2, g)) return;
        const pu32 j = order[s];
        if (j < i && core[j]) me = cluster_unite(parent, me, j, err);
    });
}

// after the sweep: every core point is pointed at its root; flag[i] = 1 where i is a root, n + 1 entries for the exclusive scan.  A root
// stays one from here on (nothing hooks any more), so the flags can be written in the same pass.
__global__ __launch_bounds__(256) void cluster_flatten_kernel(const uint8_t* __restrict__ core, int n, pu32* parent, pu32* __restrict__ flag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    pu32 f = 0u;
    if (i < n && core[i]) {
        const pu32 r = cluster_find(parent, (pu32)i);
        if (r == (pu32)i) f = 1u; else atomicMin(parent + i, r);
    }
    flag[i] = f;
}

// excl[x] = roots below x = the number of the cluster whose root is x (roots are the smallest core members: ascending order of them)
__global__ __launch_bounds__(256) void cluster_label_kernel(const uint8_t* __restrict__ core, const pu32* __restrict__ parent, const pu32* __restrict__ excl,
                                                            const pu32* __restrict__ err, int n, int32_t* __restrict__ labels, int32_t* __restrict__ n_clusters)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *n_clusters = *err ? -1 : (int32_t)excl[n];
    if (i < n) labels[i] = core[i] ? (int32_t)excl[parent[i]] : -1;
}

// border sweep, all pairs: a non-core point takes the smallest label among the core points within r.  labels[] is read at core points
// and written at non-core points only.
__global__ __launch_bounds__(NTILE) void cluster_border_brute_kernel(const double* __restrict__ pts, int n, RadiusGate g, const uint8_t* __restrict__ core,
                                                                     int32_t* labels)
{
    __shared__ double tx[NTILE], ty[NTILE], tz[NTILE];
    __shared__ int tl[NTILE];
    const int i = blockIdx.x * NTILE + threadIdx.x;
    const bool mine = i < n && !core[i];
    if (!__syncthreads_or(mine ? 1 : 0)) return;                           // uniform: core points only
    const double px = mine ? pts[3 * (size_t)i] : 0.0, py = mine ? pts[3 * (size_t)i + 1] : 0.0, pz = mine ? pts[3 * (size_t)i + 2] : 0.0;
    int lab = INT32_MAX;
    tile_sweep(pts, n, px, py, pz, tx, ty, tz, [&](int j0) { tl[threadIdx.x] = core[j0] ? labels[j0] : -1; }, [&](int, int s, double d2) {
        if (tl[s] >= 0 && tl[s] < lab && radius_hit(d2, g)) lab = tl[s];          // a non-finite point of either side: d2 fails the gate
    });
    if (mine) labels[i] = lab == INT32_MAX ? -1 : lab;
}

__global__ __launch_bounds__(NTILE) void cluster_border_grid_kernel(const pu64* __restrict__ keys, const pu32* __restrict__ order, const double* __restrict__ spts,
                                                                    int n, RadiusGate g, const uint8_t* __restrict__ core, int32_t* labels)
{
    const int p = blockIdx.x * NTILE + threadIdx.x;
    if (p >= n) return;
    const pu64 key = keys[p];
    const pu32 i = order[p];
    if ((key >> 63) || core[i]) return;                                    // non-finite: -1 already
    int lab = INT32_MAX;
    cells27_visit(keys, spts, n, p, key, [&](int s, double d2) {
        if (!radius_hit(d2, g)) return;
        const pu32 j = order[s];
        if (core[j]) { const int l = labels[j]; lab = l < lab ? l : lab; }
    });
    labels[i] = lab == INT32_MAX ? -1 : lab;
}

// sizes[c] += 1 per point labelled c (sizes zeroed by the caller).  A wave first settles up to four of its labels with one add each
// -- the lanes that share the first open lane's label count themselves by ballot --, which is the whole wave wherever a cluster fills
// it; lanes still open after that add for themselves.
__global__ __launch_bounds__(256) void cluster_sizes_kernel(const int32_t* __restrict__ labels, int n, int32_t* __restrict__ sizes)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lab = i < n ? labels[i] : -1;
    const int lane = threadIdx.x & 63;
    bool open = lab >= 0;
    for (int round = 0; round < 4; ++round) {
        const pu64 m = __ballot(open);
        if (!m) break;                                                     // uniform over the wave
        const int leader = __ffsll((long long)m) - 1;
        const int lab0 = __shfl(lab, leader);
        const bool same = open && lab == lab0;
        const pu64 ms = __ballot(same);
        if (same) { if (lane == leader) atomicAdd(sizes + lab0, (int32_t)__popcll(ms)); open = false; }
    }
    if (open) atomicAdd(sizes + lab, 1);
}

// one workgroup: best[0] = the cluster with the most points (the smallest number among equals), -1 without a cluster; best[1] = its size
__global__ __launch_bounds__(256) void cluster_largest_kernel(const int32_t* __restrict__ sizes, const int32_t* __restrict__ n_clusters, int32_t* __restrict__ best)
{
    __shared__ pu64 sb[256];
    const int C = *n_clusters;
    pu64 b = 0ull;
    for (int c = threadIdx.x; c < C; c += 256) {
        const pu64 v = ((pu64)(pu32)sizes[c] << 32) | (pu64)(0xffffffffu - (pu32)c);       // a cluster has at least one point: v > 0
        b = v > b ? v : b;
    }
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off && sb[threadIdx.x + off] > sb[threadIdx.x]) sb[threadIdx.x] = sb[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) { best[0] = sb[0] ? (int32_t)(0xffffffffu - (pu32)sb[0]) : -1; best[1] = (int32_t)(sb[0] >> 32); }
}
__global__ __launch_bounds__(256) void cluster_keep_kernel(const int32_t* __restrict__ labels, int n, const int32_t* __restrict__ best, uint8_t* __restrict__ keep)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keep[i] = best[0] >= 0 && labels[i] == best[0] ? 1 : 0;
}

// SFMHIP_POINTS_AUTO of the clustering.  Measured (profiles/r11_time_cluster.log: radius for a median count of 10, min_points 1 and 10,
// noisy sphere / that sphere with 1 % far outliers / a volume cloud, 20k .. 2M points): the grid is faster by at least 10 % on all
// three clouds at every measured size, five to seven times at 20,000 points, the smallest one measured, so that is the crossover.
#define CLUSTER_AUTO_GRID_FROM 20000

// labels / n_clusters / sizes (n entries, may be null) / count (may be null) of a device cloud, on the context's stream.  One binning
// serves the three neighbourhood sweeps (count, link, border) of SFMHIP_POINTS_GRID.
static int cluster_dbscan_enqueue(sfmhip_ctx* ctx, const double* d_pts, int n, double r, int min_points, int method, int32_t* d_labels,
                                  int32_t* d_n_clusters, int32_t* d_sizes, int32_t* d_count)
{
    method = radius_method(method, n, r, CLUSTER_AUTO_GRID_FROM);
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)n;
    const int nb = ceil_div(n, NTILE), nb256 = ceil_div(n, 256);
    SfmCarve carve;
    const size_t o_err = carve(sizeof(pu32)), o_core = carve(N), o_par = carve(N * 4), o_cnt = carve(d_count ? 0 : N * 4);
    SfmScan F(carve, N + 1);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    F.bind(w);
    pu32* err = (pu32*)(w + o_err);
    uint8_t* core = (uint8_t*)(w + o_core);
    pu32* parent = (pu32*)(w + o_par);
    pu32* flag = F.data;
    int32_t* count = d_count ? d_count : (int32_t*)(w + o_cnt);
    const RadiusGate g = radius_gate(r);
    PointsGrid G;
    const bool grid = method != SFMHIP_POINTS_BRUTE;
    if (grid) {
        rc = radius_grid_enqueue(ctx, hold, d_pts, n, r, &G);
        if (rc != SFMHIP_OK) return rc;
    }
    SFM_HIP_TRY(ctx, hipMemsetAsync(err, 0, sizeof(pu32), st));
    radius_count_launch(st, d_pts, grid ? &G : nullptr, n, g, count);
    hipLaunchKernelGGL(cluster_init_kernel, dim3(nb256), dim3(256), 0, st, d_pts, (const int32_t*)count, n, min_points, core, parent);
    if (grid) hipLaunchKernelGGL(cluster_link_grid_kernel, dim3(nb), dim3(NTILE), 0, st, G.keys, G.order, G.spts, n, g, (const uint8_t*)core, parent, err);
    else hipLaunchKernelGGL(cluster_link_brute_kernel, dim3(nb), dim3(NTILE), 0, st, d_pts, n, g, (const uint8_t*)core, parent, err);
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3(ceil_div(n + 1, 256)), dim3(256), 0, st, (const uint8_t*)core, n, parent, flag);
    F.scan(st, N + 1);
    hipLaunchKernelGGL(cluster_label_kernel, dim3(nb256), dim3(256), 0, st, (const uint8_t*)core, (const pu32*)parent, (const pu32*)flag, (const pu32*)err, n,
                       d_labels, d_n_clusters);
    if (min_points > 1) {                                                  // min_points = 1: every finite point is core, nothing to adopt
        if (grid) hipLaunchKernelGGL(cluster_border_grid_kernel, dim3(nb), dim3(NTILE), 0, st, G.keys, G.order, G.spts, n, g, (const uint8_t*)core, d_labels);
        else hipLaunchKernelGGL(cluster_border_brute_kernel, dim3(nb), dim3(NTILE), 0, st, d_pts, n, g, (const uint8_t*)core, d_labels);
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    if (d_sizes) {
        SFM_HIP_TRY(ctx, hipMemsetAsync(d_sizes, 0, N * sizeof(int32_t), st));
        hipLaunchKernelGGL(cluster_sizes_kernel, dim3(nb256), dim3(256), 0, st, (const int32_t*)d_labels, n, d_sizes);
        SFM_HIP_TRY(ctx, hipGetLastError());
    }
    return SFMHIP_OK;
}

// the argument conditions shared by the entry points: of a kNN query, of a fixed-radius query
static inline bool knn_args_ok(const sfmhip_ctx* ctx, int n, int K, int method) { return ctx && n >= 0 && K >= 1 && K <= KMAX && points_method_ok(method); }
static inline bool radius_args_ok(const sfmhip_ctx* ctx, int n, double r, int method) { return ctx && n >= 0 && std::isfinite(r) && r >= 0.0 && points_method_ok(method); }

extern "C" {

int sfmhip_knn_points_dev(sfmhip_ctx* ctx, const double* d_pts, int n, int K, int method, int32_t* d_idx, double* d_dist)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_knn_points_dev");
    SFM_ARG_CHECK(ctx, knn_args_ok(ctx, n, K, method));
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, d_pts);
    if (!d_idx && !d_dist) return SFMHIP_OK;
    return sfm_points_knn_enqueue(ctx, d_pts, n, K, method, d_idx, d_dist);
}

int sfmhip_knn_points(sfmhip_ctx* ctx, const double* pts, int n, int K, int method, int32_t* idx, double* dist)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_knn_points");
    SFM_ARG_CHECK(ctx, knn_args_ok(ctx, n, K, method));
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, pts);
    if (!idx && !dist) return SFMHIP_OK;
    SfmPoolHold hold(ctx);
    double *d_p = nullptr, *d_d = nullptr; int32_t* d_i = nullptr;
    int rc = sfm_upload_async(ctx, hold, pts, 3 * (size_t)n, d_p);
    if (rc == SFMHIP_OK && idx) rc = hold.get((size_t)n * K * sizeof(int32_t), (void**)&d_i);
    if (rc == SFMHIP_OK && dist) rc = hold.get((size_t)n * K * sizeof(double), (void**)&d_d);
    if (rc == SFMHIP_OK) rc = sfm_points_knn_enqueue(ctx, d_p, n, K, method, d_i, d_d);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipError_t e = hipSuccess;
    if (idx) e = hipMemcpyAsync(idx, d_i, (size_t)n * K * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && dist) e = hipMemcpyAsync(dist, d_d, (size_t)n * K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    return sfm_finish(ctx, e);
}

int sfmhip_statistical_outliers(sfmhip_ctx* ctx, const double* pts, int n, int K, double std_ratio, int method, uint8_t* keep, double* mean_dist, double stats[3])
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_statistical_outliers");
    SFM_ARG_CHECK(ctx, knn_args_ok(ctx, n, K, method));
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, pts && keep);
    const int nt = ceil_div(n, RED_TILE);
    SfmPoolHold hold(ctx);
    double *d_p = nullptr, *d_d = nullptr, *d_m = nullptr, *d_part = nullptr; int32_t* d_i = nullptr; uint8_t* d_keep = nullptr;
    int rc = sfm_upload_async(ctx, hold, pts, 3 * (size_t)n, d_p);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * K * sizeof(int32_t), (void**)&d_i);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * K * sizeof(double), (void**)&d_d);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * sizeof(double), (void**)&d_m);
    if (rc == SFMHIP_OK) rc = hold.get(((size_t)2 * nt + 4) * sizeof(double), (void**)&d_part);       // tile sums, then stats[3]
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n, (void**)&d_keep);
    if (rc == SFMHIP_OK) rc = sfm_points_knn_enqueue(ctx, d_p, n, K, method, d_i, d_d);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    double* d_stats = d_part + 2 * (size_t)nt;
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(points_mean_dist_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const int32_t*)d_i, (const double*)d_d, n, K, d_m);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(points_stat_tile_kernel, dim3(nt), dim3(256), 0, st, (const double*)d_m, n, pass, (const double*)d_stats, d_part);
        hipLaunchKernelGGL(points_stat_top_kernel, dim3(1), dim3(256), 0, st, (const double*)d_part, nt, pass, std_ratio, d_stats);
    }
    hipLaunchKernelGGL(points_keep_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const double*)d_m, n, (const double*)d_stats, d_keep);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && mean_dist) e = hipMemcpyAsync(mean_dist, d_m, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && stats) e = hipMemcpyAsync(stats, d_stats, 3 * sizeof(double), hipMemcpyDeviceToHost, st);
    return sfm_finish(ctx, e);
}

int sfmhip_radius_count_dev(sfmhip_ctx* ctx, const double* d_pts, int n, double r, int method, int32_t* d_count)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_radius_count_dev");
    SFM_ARG_CHECK(ctx, radius_args_ok(ctx, n, r, method));
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, d_pts && d_count);
    return points_radius_count_enqueue(ctx, d_pts, n, r, method, d_count);
}

// count (and keep, where min_neighbors >= 1) of a host cloud: the body of the two host entry points
static int radius_count_host(sfmhip_ctx* ctx, const double* pts, int n, double r, int min_neighbors, int method, uint8_t* keep, int32_t* count)
{
    SfmPoolHold hold(ctx);
    double* d_p = nullptr; int32_t* d_c = nullptr; uint8_t* d_keep = nullptr;
    int rc = sfm_upload_async(ctx, hold, pts, 3 * (size_t)n, d_p);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * sizeof(int32_t), (void**)&d_c);
    if (rc == SFMHIP_OK && keep) rc = hold.get((size_t)n, (void**)&d_keep);
    if (rc == SFMHIP_OK) rc = points_radius_count_enqueue(ctx, d_p, n, r, method, d_c);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    if (keep) {
        hipLaunchKernelGGL(points_count_keep_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const int32_t*)d_c, n, min_neighbors, d_keep);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess && count) e = hipMemcpyAsync(count, d_c, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    return sfm_finish(ctx, e);
}

int sfmhip_radius_count(sfmhip_ctx* ctx, const double* pts, int n, double r, int method, int32_t* count)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_radius_count");
    SFM_ARG_CHECK(ctx, radius_args_ok(ctx, n, r, method));
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, pts && count);
    return radius_count_host(ctx, pts, n, r, 0, method, nullptr, count);
}

int sfmhip_radius_outliers(sfmhip_ctx* ctx, const double* pts, int n, double r, int min_neighbors, int method, uint8_t* keep, int32_t* count)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_radius_outliers");
    SFM_ARG_CHECK(ctx, radius_args_ok(ctx, n, r, method) && min_neighbors >= 1);
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, pts && keep);
    return radius_count_host(ctx, pts, n, r, min_neighbors, method, keep, count);
}

int sfmhip_voxel_downsample_dev(sfmhip_ctx* ctx, const double* d_pts, int n, double voxel, double* d_centroids, int32_t* d_counts, int32_t* d_voxel_of,
                                int32_t* d_n_voxels, double* d_origin)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_voxel_downsample_dev");
    SFM_ARG_CHECK(ctx, ctx && n >= 0 && std::isfinite(voxel) && voxel > 0.0);
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, d_pts && d_centroids && d_n_voxels);
    return voxel_downsample_enqueue(ctx, d_pts, n, voxel, d_centroids, d_counts, d_voxel_of, d_n_voxels, d_origin);
}

int sfmhip_voxel_downsample(sfmhip_ctx* ctx, const double* pts, int n, double voxel, double* centroids, int32_t* counts, int32_t* voxel_of, int* n_voxels,
                            double origin[3])
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_voxel_downsample");
    SFM_ARG_CHECK(ctx, ctx && n >= 0 && std::isfinite(voxel) && voxel > 0.0);
    if (n == 0) { if (n_voxels) *n_voxels = 0; return SFMHIP_OK; }
    SFM_ARG_CHECK(ctx, pts && centroids && n_voxels);
    *n_voxels = 0;
    SfmPoolHold hold(ctx);
    double *d_p = nullptr, *d_c = nullptr, *d_org = nullptr; int32_t *d_cnt = nullptr, *d_vof = nullptr, *d_nv = nullptr;
    int rc = sfm_upload_async(ctx, hold, pts, 3 * (size_t)n, d_p);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * 24, (void**)&d_c);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * sizeof(int32_t), (void**)&d_cnt);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * sizeof(int32_t), (void**)&d_vof);
    if (rc == SFMHIP_OK) rc = hold.get(256, (void**)&d_org);               // origin[3], then n_voxels
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    d_nv = (int32_t*)(d_org + 4);
    rc = voxel_downsample_enqueue(ctx, d_p, n, voxel, d_c, d_cnt, d_vof, d_nv, d_org);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipStream_t st = ctx->stream;
    int32_t nv = 0;
    rc = sfm_finish(ctx, hipMemcpyAsync(&nv, d_nv, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (rc != SFMHIP_OK) return rc;
    if (nv < 0) {
        ctx->last_error = "bad argument: the voxel is too small for the cloud's extent (more than 2^21 voxels along an axis; filter far outliers first)";
        return SFMHIP_E_ARG;
    }
    hipError_t e = hipSuccess;
    if (nv > 0) e = hipMemcpyAsync(centroids, d_c, (size_t)nv * 24, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && counts && nv > 0) e = hipMemcpyAsync(counts, d_cnt, (size_t)nv * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && voxel_of) e = hipMemcpyAsync(voxel_of, d_vof, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && origin) e = hipMemcpyAsync(origin, d_org, 3 * sizeof(double), hipMemcpyDeviceToHost, st);
    rc = sfm_finish(ctx, e);
    if (rc == SFMHIP_OK) *n_voxels = nv;
    return rc;
}

int sfmhip_cluster_dbscan_dev(sfmhip_ctx* ctx, const double* d_pts, int n, double r, int min_points, int method, int32_t* d_labels, int32_t* d_n_clusters,
                              int32_t* d_sizes, int32_t* d_count)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_cluster_dbscan_dev");
    SFM_ARG_CHECK(ctx, radius_args_ok(ctx, n, r, method) && min_points >= 1);
    if (n == 0) return SFMHIP_OK;
    SFM_ARG_CHECK(ctx, d_pts && d_labels && d_n_clusters);
    return cluster_dbscan_enqueue(ctx, d_pts, n, r, min_points, method, d_labels, d_n_clusters, d_sizes, d_count);
}

// the clustering of a host cloud and, where keep is given, its largest cluster: the body of the two host entry points
static int cluster_host(sfmhip_ctx* ctx, const double* pts, int n, double r, int min_points, int method, int32_t* labels, int* n_clusters, int32_t* sizes,
                        int32_t* count, uint8_t* keep, int* largest_size)
{
    SfmPoolHold hold(ctx);
    double* d_p = nullptr; int32_t *d_lab = nullptr, *d_sz = nullptr, *d_cnt = nullptr, *d_head = nullptr; uint8_t* d_keep = nullptr;
    int rc = sfm_upload_async(ctx, hold, pts, 3 * (size_t)n, d_p);
    if (rc == SFMHIP_OK) rc = hold.get((size_t)n * sizeof(int32_t), (void**)&d_lab);
    if (rc == SFMHIP_OK && (sizes || keep)) rc = hold.get((size_t)n * sizeof(int32_t), (void**)&d_sz);
    if (rc == SFMHIP_OK && count) rc = hold.get((size_t)n * sizeof(int32_t), (void**)&d_cnt);
    if (rc == SFMHIP_OK && keep) rc = hold.get((size_t)n, (void**)&d_keep);
    if (rc == SFMHIP_OK) rc = hold.get(256, (void**)&d_head);              // n_clusters, then the largest cluster's number and size
    if (rc == SFMHIP_OK) rc = cluster_dbscan_enqueue(ctx, d_p, n, r, min_points, method, d_lab, d_head, d_sz, d_cnt);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipStream_t st = ctx->stream;
    if (keep) {
        hipLaunchKernelGGL(cluster_largest_kernel, dim3(1), dim3(256), 0, st, (const int32_t*)d_sz, (const int32_t*)d_head, d_head + 1);
        hipLaunchKernelGGL(cluster_keep_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const int32_t*)d_lab, n, (const int32_t*)(d_head + 1), d_keep);
    }
    int32_t head[3] = { 0, -1, 0 };
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(head, d_head, (keep ? 3 : 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    rc = sfm_finish(ctx, e);
    if (rc != SFMHIP_OK) return rc;
    if (head[0] < 0) {
        ctx->last_error = "clustering: a union exceeded its retry cap (the parent array broke its invariant); no result";
        return SFMHIP_E_NUMERIC;
    }
    e = hipSuccess;
    if (labels) e = hipMemcpyAsync(labels, d_lab, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && sizes && head[0] > 0) e = hipMemcpyAsync(sizes, d_sz, (size_t)head[0] * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && count) e = hipMemcpyAsync(count, d_cnt, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && keep) e = hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, st);
    rc = sfm_finish(ctx, e);
    if (rc != SFMHIP_OK) return rc;
    if (n_clusters) *n_clusters = head[0];
    if (largest_size) *largest_size = head[2];
    return SFMHIP_OK;
}

int sfmhip_cluster_dbscan(sfmhip_ctx* ctx, const double* pts, int n, double r, int min_points, int method, int32_t* labels, int* n_clusters, int32_t* sizes,
                          int32_t* count)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_cluster_dbscan");
    SFM_ARG_CHECK(ctx, radius_args_ok(ctx, n, r, method) && min_points >= 1);
    if (n == 0) { if (n_clusters) *n_clusters = 0; return SFMHIP_OK; }
    SFM_ARG_CHECK(ctx, pts && labels && n_clusters);
    return cluster_host(ctx, pts, n, r, min_points, method, labels, n_clusters, sizes, count, nullptr, nullptr);
}

int sfmhip_largest_cluster(sfmhip_ctx* ctx, const double* pts, int n, double r, int min_points, int method, uint8_t* keep, int32_t* labels, int* n_clusters,
                           int* largest_size)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_largest_cluster");
    SFM_ARG_CHECK(ctx, radius_args_ok(ctx, n, r, method) && min_points >= 1);
    if (n == 0) { if (n_clusters) *n_clusters = 0; if (largest_size) *largest_size = 0; return SFMHIP_OK; }
    SFM_ARG_CHECK(ctx, pts && keep);
    return cluster_host(ctx, pts, n, r, min_points, method, labels, n_clusters, nullptr, nullptr, keep, largest_size);
}

int sfmhip_points_fallback_count(sfmhip_ctx* ctx, int* count)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_ARG_CHECK(ctx, ctx && count);
    *count = 0;
    if (!ctx->d_points_fallback) return SFMHIP_OK;
    unsigned c = 0;
    SFM_HIP_TRY(ctx, hipMemcpyAsync(&c, ctx->d_points_fallback, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    SFM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *count = (int)c;
    return SFMHIP_OK;
}

}  // extern "C"
