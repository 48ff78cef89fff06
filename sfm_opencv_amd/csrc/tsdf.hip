// tsdf.hip -- the dense mesh: truncated signed distance fusion of the depth maps into a voxel volume (sfmhip_tsdf_integrate) and marching
// tetrahedra on the Kuhn split of its cells (sfmhip_tsdf_mesh).  The definition is in sfmhip.h at sfmhip_tsdf_integrate and is followed to
// the letter: the projections are doubles in the written order, the volume is integer sums, the crossing of an edge is a quotient of two
// 64-bit integers.  A voxel is owned by one thread and a mesh edge by one voxel, so nothing here needs an atomic and no result depends on
// the launch geometry.
//
// Kernels (all one thread per voxel, lanes along x, a grid sized by the CUs that walks the volume with its stride)
//   tsdf_integrate_kernel   every view of the call in one pass over the volume: the views' 16 doubles and 3 pointers are kernel
//                           arguments (wave-uniform), the sums of a voxel are kept in registers and the volume is read and written once,
//                           and only where a view counted
//   tsdf_cell_kernel        the voxel as the lowest corner of a cell: the inside bits of the 8 corners, whether the cell is processed,
//                           and the number of its triangles
//   tsdf_edge_kernel        the voxel as the owner of its 7 edges: the mask of those that carry a vertex (a sign change, and a
//                           processed cell among the 1, 2 or 4 around the edge), and their number
//                           -- the exclusive scans of sortscan.hpp then number the vertices and place the triangles
//   tsdf_vertex_kernel      the vertices of a voxel's edges: position and colour
//   tsdf_triangle_kernel    the triangles of a cell; a vertex number is base[owner] + popcount(mask[owner] & below(bit))
#include "common.hpp"
#include "sortscan.hpp"
#include <cmath>
#pragma clang fp contract(off)

#define TSDF_VIEWS_MAX 8
#define TSDF_VOXELS_MAX ((size_t)1 << 28)
#define TSDF_DIM_MAX 16384
#define TSDF_PROCESSED 0x100u                 // bit 8 of a voxel's code: the cell above it is processed; bits 0 .. 7: corner c is inside

struct TsdfGrid { double o[3], voxel; unsigned nx, ny, nz, nvox; };
struct TsdfViews {
    const float* depth[TSDF_VIEWS_MAX];
    const uint8_t* keep[TSDF_VIEWS_MAX];
    const uint8_t* img[TSDF_VIEWS_MAX];
    double R[TSDF_VIEWS_MAX][9], t[TSDF_VIEWS_MAX][3];
    double fx, fy, cx, cy, trunc;
    size_t ld;
    int n_views, rows, cols, channels;
};

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(TsdfGrid G, TsdfViews V, int32_t* __restrict__ dsum, int32_t* __restrict__ wsum, uint32_t* __restrict__ csum)
{
    for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < G.nvox; v += gridDim.x * 256u) {
        const unsigned i = v % G.nx, jk = v / G.nx, j = jk % G.ny, k = jk / G.ny;
        const double X0 = G.o[0] + ((double)i + 0.5) * G.voxel, X1 = G.o[1] + ((double)j + 0.5) * G.voxel, X2 = G.o[2] + ((double)k + 0.5) * G.voxel;
        int dq = 0, w = 0;
        uint32_t cb = 0, cg = 0, cr = 0;
        for (int s = 0; s < V.n_views; ++s) {
            const double* R = V.R[s];
            const double Y0 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + V.t[s][0];
            const double Y1 = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + V.t[s][1];
            const double Y2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + V.t[s][2];
            if (!(Y2 > 0.0)) continue;
            const double pu = floor(((V.fx * Y0) / Y2 + V.cx) + 0.5), pv = floor(((V.fy * Y1) / Y2 + V.cy) + 0.5);
            if (!(pu >= 0.0 && pu < (double)V.cols && pv >= 0.0 && pv < (double)V.rows)) continue;
            const size_t px = (size_t)pv * (size_t)V.cols + (size_t)pu;
            const float df = V.depth[s][px];
            if (!isfinite(df)) continue;
            if (V.keep[s] && V.keep[s][px] == 0) continue;
            const double sd = (double)df - Y2;
            if (!(sd >= -V.trunc)) continue;
            dq += (int)floor(((sd > V.trunc ? V.trunc : sd) / V.trunc) * 32767.0 + 0.5);
            ++w;
            if (csum) {
                const uint8_t* p = V.img[s] + (size_t)pv * V.ld + (size_t)pu * (size_t)V.channels;
                cb += p[0]; cg += V.channels == 1 ? p[0] : p[1]; cr += V.channels == 1 ? p[0] : p[2];
            }
        }
        if (w == 0) continue;
        dsum[v] += dq; wsum[v] += w;
        if (csum) { csum[3 * (size_t)v] += cb; csum[3 * (size_t)v + 1] += cg; csum[3 * (size_t)v + 2] += cr; }
    }
}

// ---- marching tetrahedra.  The tetrahedra of a cell as corner codes, 3 bits per position (position 0 lowest), and their parities.
__device__ __forceinline__ constexpr unsigned tsdf_tet(int t)
{
    return t == 0 ? (0u | 1u << 3 | 3u << 6 | 7u << 9) : t == 1 ? (0u | 1u << 3 | 5u << 6 | 7u << 9) : t == 2 ? (0u | 2u << 3 | 3u << 6 | 7u << 9)
         : t == 3 ? (0u | 2u << 3 | 6u << 6 | 7u << 9) : t == 4 ? (0u | 4u << 3 | 5u << 6 | 7u << 9) : (0u | 4u << 3 | 6u << 6 | 7u << 9);
}
__device__ __forceinline__ constexpr bool tsdf_sigma_positive(int t) { return t == 0 || t == 3 || t == 4; }
// the inside bits of the 4 corners of tetrahedron t (bit p: the corner at position p) from the inside bits of the cell's 8 corners
__device__ __forceinline__ unsigned tsdf_tet_bits(unsigned ins, int t)
{
    const unsigned pack = tsdf_tet(t);
    return (ins >> (pack & 7u) & 1u) | (ins >> (pack >> 3 & 7u) & 1u) << 1 | (ins >> (pack >> 6 & 7u) & 1u) << 2 | (ins >> (pack >> 9 & 7u) & 1u) << 3;
}
__device__ __forceinline__ unsigned tsdf_offset(const TsdfGrid& G, unsigned c) { return (c & 1u) + (c >> 1 & 1u) * G.nx + (c >> 2 & 1u) * G.nx * G.ny; }

__global__ __launch_bounds__(256) void tsdf_cell_kernel(TsdfGrid G, const int32_t* __restrict__ dsum, const int32_t* __restrict__ wsum, int min_weight,
                                                        uint32_t* __restrict__ code, unsigned* __restrict__ tcount)
{
    for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < G.nvox; v += gridDim.x * 256u) {
        const unsigned i = v % G.nx, jk = v / G.nx, j = jk % G.ny, k = jk / G.ny;
        unsigned ins = 0, val = 0;
#pragma unroll
        for (unsigned c = 0; c < 8; ++c) {
            if (i + (c & 1u) >= G.nx || j + (c >> 1 & 1u) >= G.ny || k + (c >> 2) >= G.nz) continue;
            const unsigned at = v + tsdf_offset(G, c);
            if (wsum[at] >= min_weight) val |= 1u << c;
            if (dsum[at] < 0) ins |= 1u << c;
        }
        const bool processed = val == 0xFFu;                             // eight corners in the volume, all valid
        unsigned nt = 0;
        if (processed && ins != 0 && ins != 0xFFu) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int n = __popc(tsdf_tet_bits(ins, t));
                nt += n == 2 ? 2u : (n == 1 || n == 3) ? 1u : 0u;
            }
        }
        code[v] = ins | (processed ? TSDF_PROCESSED : 0u);
        tcount[v] = nt;
        if (v == 0) tcount[G.nvox] = 0;                                  // becomes the total under the exclusive scan
    }
}

__global__ __launch_bounds__(256) void tsdf_edge_kernel(TsdfGrid G, const uint32_t* __restrict__ code, uint8_t* __restrict__ mask, unsigned* __restrict__ vcount)
{
    for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < G.nvox; v += gridDim.x * 256u) {
        const unsigned i = v % G.nx, jk = v / G.nx, j = jk % G.ny, k = jk / G.ny;
        const unsigned c0 = code[v], in0 = c0 & 1u;
        unsigned m = 0;
#pragma unroll
        for (unsigned d = 1; d < 8; ++d) {
            if (i + (d & 1u) >= G.nx || j + (d >> 1 & 1u) >= G.ny || k + (d >> 2) >= G.nz) continue;
            if ((c0 >> d & 1u) == in0) continue;
            // the cells around the edge: their lowest corner is v - e, e in {0,1}^3 with e_a = 0 where d_a = 1
            unsigned any = 0;
#pragma unroll
            for (unsigned e = 0; e < 8; ++e) {
                if (e & d) continue;
                if (i < (e & 1u) || j < (e >> 1 & 1u) || k < (e >> 2)) continue;
                any |= code[v - tsdf_offset(G, e)] & TSDF_PROCESSED;
            }
            if (any) m |= 1u << (d - 1);
        }
        mask[v] = (uint8_t)m;
        vcount[v] = (unsigned)__popc(m);
        if (v == 0) vcount[G.nvox] = 0;
    }
}

__global__ __launch_bounds__(256) void tsdf_vertex_kernel(TsdfGrid G, const int32_t* __restrict__ dsum, const int32_t* __restrict__ wsum, const uint32_t* __restrict__ csum,
                                                          const uint8_t* __restrict__ mask, const unsigned* __restrict__ vbase, double* __restrict__ xyz,
                                                          uint8_t* __restrict__ bgr, unsigned cap, int32_t* __restrict__ n_vertices)
{
    for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < G.nvox; v += gridDim.x * 256u) {
        if (v == 0) *n_vertices = (int32_t)vbase[G.nvox];
        const unsigned m = mask[v];
        if (m == 0) continue;
        unsigned at = vbase[v];
        if (at >= cap) continue;
        const unsigned i = v % G.nx, jk = v / G.nx, j = jk % G.ny, k = jk / G.ny;
        const int64_t da = dsum[v], wa = wsum[v];
        const double Xa[3] = { G.o[0] + ((double)i + 0.5) * G.voxel, G.o[1] + ((double)j + 0.5) * G.voxel, G.o[2] + ((double)k + 0.5) * G.voxel };
#pragma unroll
        for (unsigned d = 1; d < 8; ++d) {
            if (!(m >> (d - 1) & 1u)) continue;
            if (at >= cap) break;
            const unsigned b = v + tsdf_offset(G, d);
            const int64_t db = dsum[b], wb = wsum[b];
            const int64_t num = da * wb, den = num - db * wa;
            const double s = (double)num / (double)den;
            if (xyz) {
                const double Xb[3] = { G.o[0] + ((double)(i + (d & 1u)) + 0.5) * G.voxel, G.o[1] + ((double)(j + (d >> 1 & 1u)) + 0.5) * G.voxel,
                                       G.o[2] + ((double)(k + (d >> 2)) + 0.5) * G.voxel };
#pragma unroll
                for (int c = 0; c < 3; ++c) xyz[3 * (size_t)at + c] = Xa[c] + s * (Xb[c] - Xa[c]);
            }
            if (bgr) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int64_t ma = (2 * (int64_t)csum[3 * (size_t)v + c] + wa) / (2 * wa), mb = (2 * (int64_t)csum[3 * (size_t)b + c] + wb) / (2 * wb);
                    bgr[3 * (size_t)at + c] = (uint8_t)floor(((double)ma + s * ((double)mb - (double)ma)) + 0.5);
                }
            }
            ++at;
        }
    }
}

// the number of the vertex on the edge between the corners cx and cy (codes, cx below cy in every axis) of the cell above voxel v
__device__ __forceinline__ int32_t tsdf_vertex_of(const TsdfGrid& G, unsigned v, unsigned cx, unsigned cy, const uint8_t* __restrict__ mask,
                                                  const unsigned* __restrict__ vbase)
{
    const unsigned owner = v + tsdf_offset(G, cx), bit = (cy ^ cx) - 1u;
    return (int32_t)(vbase[owner] + (unsigned)__popc(mask[owner] & ((1u << bit) - 1u)));
}

__global__ __launch_bounds__(256) void tsdf_triangle_kernel(TsdfGrid G, const uint32_t* __restrict__ code, const uint8_t* __restrict__ mask,
                                                            const unsigned* __restrict__ vbase, const unsigned* __restrict__ tbase, int32_t* __restrict__ tri, unsigned cap,
                                                            int32_t* __restrict__ n_triangles)
{
    for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < G.nvox; v += gridDim.x * 256u) {
        if (v == 0) *n_triangles = (int32_t)tbase[G.nvox];
        const unsigned c = code[v], ins = c & 0xFFu;
        if (!(c & TSDF_PROCESSED) || ins == 0 || ins == 0xFFu || !tri) continue;
        unsigned at = tbase[v];
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const unsigned pack = tsdf_tet(t), b = tsdf_tet_bits(ins, t);
            const int n = __popc(b);
            if (n == 0 || n == 4) continue;
            if (at >= cap) break;
            // E(x, y) for two positions of this tetrahedron: the corner at the lower position is below the other in every axis
            auto E = [&](unsigned x, unsigned y) {
                const unsigned lo = min(x, y), hi = max(x, y);
                return tsdf_vertex_of(G, v, pack >> (3u * lo) & 7u, pack >> (3u * hi) & 7u, mask, vbase);
            };
            if (n == 2) {
                const unsigned out = ~b & 15u;
                const unsigned k = __ffs(b) - 1, l = __ffs(b & (b - 1u)) - 1, m = __ffs(out) - 1, nn = __ffs(out & (out - 1u)) - 1;
                const unsigned inv = (k > m) + (k > nn) + (l > m) + (l > nn);
                const bool pos = ((inv & 1u) == 0) == tsdf_sigma_positive(t);
                const int32_t q0 = E(k, m), q1 = E(k, nn), q2 = E(l, nn), q3 = E(l, m);
                int32_t* o = tri + 3 * (size_t)at;
                o[0] = q0; o[1] = pos ? q1 : q2; o[2] = pos ? q2 : q1;
                if (at + 1 < cap) { o[3] = q0; o[4] = pos ? q2 : q3; o[5] = pos ? q3 : q2; }
                at += 2;
            } else {
                const unsigned odd = n == 1 ? b : ~b & 15u;
                const unsigned k = __ffs(odd) - 1;
                unsigned rest = 15u ^ (1u << k);
                const unsigned l = __ffs(rest) - 1; rest &= rest - 1u;
                const unsigned m = __ffs(rest) - 1; rest &= rest - 1u;
                const unsigned nn = __ffs(rest) - 1;
                bool pos = ((k & 1u) == 0) == tsdf_sigma_positive(t);       // the permutation (k, l, m, n) has k inversions
                if (n == 3) pos = !pos;
                const int32_t e1 = E(k, l), e2 = E(k, m), e3 = E(k, nn);
                int32_t* o = tri + 3 * (size_t)at;
                o[0] = e1; o[1] = pos ? e2 : e3; o[2] = pos ? e3 : e2;
                at += 1;
            }
        }
    }
}

// ---- host side
static inline bool tsdf_pos_finite(double x) { return std::isfinite(x) && x > 0.0; }
static inline bool tsdf_grid_ok(const int* dims, const double* origin, double voxel)
{
    if (!dims || !origin || !tsdf_pos_finite(voxel)) return false;
    size_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1 || (size_t)dims[a] > TSDF_VOXELS_MAX || !std::isfinite(origin[a])) return false;
        n *= (size_t)dims[a];
        if (n > TSDF_VOXELS_MAX) return false;
    }
    return true;
}
static inline TsdfGrid tsdf_grid(const int* dims, const double* origin, double voxel)
{
    TsdfGrid G;
    for (int a = 0; a < 3; ++a) G.o[a] = origin[a];
    G.voxel = voxel; G.nx = (unsigned)dims[0]; G.ny = (unsigned)dims[1]; G.nz = (unsigned)dims[2]; G.nvox = G.nx * G.ny * G.nz;
    return G;
}
static inline dim3 tsdf_launch_grid(const sfmhip_ctx* ctx, size_t nvox) { return dim3((unsigned)std::max<size_t>(1, std::min((nvox + 255) / 256, (size_t)ctx->num_cus * 8))); }

static inline bool integrate_args_ok(const sfmhip_ctx* ctx, const int* dims, const double* origin, double voxel, double trunc, const void* const* depth,
                                     const void* const* img, int n_views, int rows, int cols, int channels, size_t ld, const double* K4, const double* R, const double* t,
                                     const void* dsum, const void* wsum, const void* csum)
{
    if (!ctx || !tsdf_grid_ok(dims, origin, voxel) || !tsdf_pos_finite(trunc) || !depth || n_views < 1 || n_views > TSDF_VIEWS_MAX || rows < 1 || rows > TSDF_DIM_MAX ||
        cols < 1 || cols > TSDF_DIM_MAX || !K4 || !R || !t || !dsum || !wsum || (img != nullptr) != (csum != nullptr))
        return false;
    for (int s = 0; s < n_views; ++s)
        if (!depth[s] || (img && !img[s])) return false;
    return !img || ((channels == 1 || channels == 3) && ld >= (size_t)cols * (size_t)channels);
}

static int integrate_enqueue(sfmhip_ctx* ctx, const int* dims, const double* origin, double voxel, double trunc, const float* const* d_depth, const uint8_t* const* d_keep,
                             const uint8_t* const* d_img, int n_views, int rows, int cols, int channels, size_t ld, const double* K4, const double* R, const double* t,
                             int32_t* d_dsum, int32_t* d_wsum, uint32_t* d_csum)
{
    const TsdfGrid G = tsdf_grid(dims, origin, voxel);
    TsdfViews V = {};
    for (int s = 0; s < n_views; ++s) {
        V.depth[s] = d_depth[s]; V.keep[s] = d_keep ? d_keep[s] : nullptr; V.img[s] = d_img ? d_img[s] : nullptr;
        std::memcpy(V.R[s], R + 9 * s, 9 * sizeof(double));
        std::memcpy(V.t[s], t + 3 * s, 3 * sizeof(double));
    }
    V.fx = K4[0]; V.fy = K4[1]; V.cx = K4[2]; V.cy = K4[3]; V.trunc = trunc;
    V.ld = ld; V.n_views = n_views; V.rows = rows; V.cols = cols; V.channels = channels;
    hipLaunchKernelGGL(tsdf_integrate_kernel, tsdf_launch_grid(ctx, G.nvox), dim3(256), 0, ctx->stream, G, V, d_dsum, d_wsum, d_csum);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

static inline bool mesh_args_ok(const sfmhip_ctx* ctx, const int* dims, const double* origin, double voxel, const void* dsum, const void* wsum, const void* csum,
                                int min_weight, const void* bgr, int vertex_cap, int triangle_cap, const void* n_vertices, const void* n_triangles)
{
    return ctx && tsdf_grid_ok(dims, origin, voxel) && dsum && wsum && min_weight >= 1 && vertex_cap >= 0 && triangle_cap >= 0 && n_vertices && n_triangles && (csum || !bgr);
}

// the four passes and the two scans; the per-voxel arrays come from the block cache
static int mesh_enqueue(sfmhip_ctx* ctx, const int* dims, const double* origin, double voxel, const int32_t* d_dsum, const int32_t* d_wsum, const uint32_t* d_csum,
                        int min_weight, double* d_xyz, uint8_t* d_bgr, int vertex_cap, int32_t* d_tri, int triangle_cap, int32_t* d_nv, int32_t* d_nt)
{
    const TsdfGrid G = tsdf_grid(dims, origin, voxel);
    const size_t nvox = G.nvox;
    SfmCarve carve;
    const size_t o_code = carve(nvox * 4), o_mask = carve(nvox);
    SfmScan VB(carve, nvox + 1), TB(carve, nvox + 1);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    VB.bind(w); TB.bind(w);
    uint32_t* code = (uint32_t*)(w + o_code);
    uint8_t* mask = (uint8_t*)(w + o_mask);
    unsigned *vb = VB.data, *tb = TB.data;
    const dim3 grid = tsdf_launch_grid(ctx, nvox), block(256);
    hipLaunchKernelGGL(tsdf_cell_kernel, grid, block, 0, ctx->stream, G, d_dsum, d_wsum, min_weight, code, tb);
    hipLaunchKernelGGL(tsdf_edge_kernel, grid, block, 0, ctx->stream, G, (const uint32_t*)code, mask, vb);
    VB.scan(ctx->stream, nvox + 1);
    TB.scan(ctx->stream, nvox + 1);
    hipLaunchKernelGGL(tsdf_vertex_kernel, grid, block, 0, ctx->stream, G, d_dsum, d_wsum, d_csum, (const uint8_t*)mask, (const unsigned*)vb, d_xyz, d_bgr,
                       (unsigned)vertex_cap, d_nv);
    hipLaunchKernelGGL(tsdf_triangle_kernel, grid, block, 0, ctx->stream, G, (const uint32_t*)code, (const uint8_t*)mask, (const unsigned*)vb, (const unsigned*)tb, d_tri,
                       (unsigned)triangle_cap, d_nt);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

extern "C" {

int sfmhip_tsdf_integrate_dev(sfmhip_ctx* ctx, const int dims[3], const double origin[3], double voxel, double trunc, const float* const* d_depth,
                              const uint8_t* const* d_keep, const uint8_t* const* d_img, int n_views, int rows, int cols, int channels, size_t ld, const double K4[4],
                              const double* R, const double* t, int32_t* d_dsum, int32_t* d_wsum, uint32_t* d_csum)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_tsdf_integrate_dev");
    SFM_ARG_CHECK(ctx, integrate_args_ok(ctx, dims, origin, voxel, trunc, (const void* const*)d_depth, (const void* const*)d_img, n_views, rows, cols, channels, ld, K4, R, t,
                                         d_dsum, d_wsum, d_csum));
    return integrate_enqueue(ctx, dims, origin, voxel, trunc, d_depth, d_keep, d_img, n_views, rows, cols, channels, ld, K4, R, t, d_dsum, d_wsum, d_csum);
}

int sfmhip_tsdf_integrate(sfmhip_ctx* ctx, const int dims[3], const double origin[3], double voxel, double trunc, const float* const* depth, const uint8_t* const* keep,
                          const uint8_t* const* img, int n_views, int rows, int cols, int channels, size_t ld, const double K4[4], const double* R, const double* t,
                          int32_t* dsum, int32_t* wsum, uint32_t* csum)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_tsdf_integrate");
    SFM_ARG_CHECK(ctx, integrate_args_ok(ctx, dims, origin, voxel, trunc, (const void* const*)depth, (const void* const*)img, n_views, rows, cols, channels, ld, K4, R, t, dsum,
                                         wsum, csum));
    const size_t npx = (size_t)rows * cols, nvox = (size_t)dims[0] * dims[1] * dims[2];
    const size_t img_bytes = img ? (size_t)(rows - 1) * ld + (size_t)cols * (size_t)channels : 0;
    SfmCarve carve;
    size_t o_depth[TSDF_VIEWS_MAX], o_keep[TSDF_VIEWS_MAX], o_img[TSDF_VIEWS_MAX];
    for (int s = 0; s < n_views; ++s) { o_depth[s] = carve(npx * 4); o_keep[s] = carve(keep && keep[s] ? npx : 0); o_img[s] = carve(img_bytes); }
    const size_t o_d = carve(nvox * 4), o_w = carve(nvox * 4), o_c = carve(csum ? nvox * 12 : 0);
    SfmPoolHold hold(ctx);
    char* d = nullptr;
    int rc = hold.get(carve.bytes, (void**)&d);
    const float* d_depth[TSDF_VIEWS_MAX] = {};
    const uint8_t *d_keep[TSDF_VIEWS_MAX] = {}, *d_img[TSDF_VIEWS_MAX] = {};
    for (int s = 0; s < n_views && rc == SFMHIP_OK; ++s) {
        d_depth[s] = (const float*)(d + o_depth[s]);
        rc = sfm_upload(ctx, d + o_depth[s], depth[s], npx * 4);
        if (rc == SFMHIP_OK && keep && keep[s]) { d_keep[s] = (const uint8_t*)(d + o_keep[s]); rc = sfm_upload(ctx, d + o_keep[s], keep[s], npx); }
        if (rc == SFMHIP_OK && img) { d_img[s] = (const uint8_t*)(d + o_img[s]); rc = sfm_upload(ctx, d + o_img[s], img[s], img_bytes); }
    }
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d + o_d, dsum, nvox * 4);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d + o_w, wsum, nvox * 4);
    if (rc == SFMHIP_OK && csum) rc = sfm_upload(ctx, d + o_c, csum, nvox * 12);
    if (rc == SFMHIP_OK)
        rc = integrate_enqueue(ctx, dims, origin, voxel, trunc, d_depth, d_keep, img ? d_img : nullptr, n_views, rows, cols, channels, ld, K4, R, t, (int32_t*)(d + o_d),
                               (int32_t*)(d + o_w), csum ? (uint32_t*)(d + o_c) : nullptr);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipError_t e = hipMemcpyAsync(dsum, d + o_d, nvox * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(wsum, d + o_w, nvox * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && csum) e = hipMemcpyAsync(csum, d + o_c, nvox * 12, hipMemcpyDeviceToHost, ctx->stream);
    return sfm_finish(ctx, e);
}

int sfmhip_tsdf_mesh_dev(sfmhip_ctx* ctx, const int dims[3], const double origin[3], double voxel, const int32_t* d_dsum, const int32_t* d_wsum, const uint32_t* d_csum,
                         int min_weight, double* d_xyz, uint8_t* d_bgr, int vertex_cap, int32_t* d_tri, int triangle_cap, int32_t* d_n_vertices, int32_t* d_n_triangles)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_tsdf_mesh_dev");
    SFM_ARG_CHECK(ctx, mesh_args_ok(ctx, dims, origin, voxel, d_dsum, d_wsum, d_csum, min_weight, d_bgr, vertex_cap, triangle_cap, d_n_vertices, d_n_triangles));
    return mesh_enqueue(ctx, dims, origin, voxel, d_dsum, d_wsum, d_csum, min_weight, d_xyz, d_bgr, vertex_cap, d_tri, triangle_cap, d_n_vertices, d_n_triangles);
}

int sfmhip_tsdf_mesh(sfmhip_ctx* ctx, const int dims[3], const double origin[3], double voxel, const int32_t* dsum, const int32_t* wsum, const uint32_t* csum, int min_weight,
                     double* xyz, uint8_t* bgr, int vertex_cap, int32_t* tri, int triangle_cap, int32_t* n_vertices, int32_t* n_triangles)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_tsdf_mesh");
    SFM_ARG_CHECK(ctx, mesh_args_ok(ctx, dims, origin, voxel, dsum, wsum, csum, min_weight, bgr, vertex_cap, triangle_cap, n_vertices, n_triangles));
    const size_t nvox = (size_t)dims[0] * dims[1] * dims[2], VC = (size_t)vertex_cap, TC = (size_t)triangle_cap;
    SfmCarve carve;
    const size_t o_d = carve(nvox * 4), o_w = carve(nvox * 4), o_c = carve(csum && bgr ? nvox * 12 : 0), o_xyz = carve(xyz ? VC * 24 : 0), o_bgr = carve(bgr ? VC * 3 : 0),
                 o_tri = carve(tri ? TC * 12 : 0), o_n = carve(8);
    SfmPoolHold hold(ctx);
    char* d = nullptr;
    int rc = hold.get(carve.bytes, (void**)&d);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d + o_d, dsum, nvox * 4);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d + o_w, wsum, nvox * 4);
    if (rc == SFMHIP_OK && csum && bgr) rc = sfm_upload(ctx, d + o_c, csum, nvox * 12);
    if (rc == SFMHIP_OK)
        rc = mesh_enqueue(ctx, dims, origin, voxel, (const int32_t*)(d + o_d), (const int32_t*)(d + o_w), csum && bgr ? (const uint32_t*)(d + o_c) : nullptr, min_weight,
                          xyz ? (double*)(d + o_xyz) : nullptr, bgr ? (uint8_t*)(d + o_bgr) : nullptr, vertex_cap, tri ? (int32_t*)(d + o_tri) : nullptr, triangle_cap,
                          (int32_t*)(d + o_n), (int32_t*)(d + o_n) + 1);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    int32_t n[2] = { 0, 0 };
    hipError_t e = hipMemcpyAsync(n, d + o_n, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    const size_t mv = std::min((size_t)std::max(n[0], 0), VC), mt = std::min((size_t)std::max(n[1], 0), TC);
    if (e == hipSuccess && xyz && mv) e = hipMemcpyAsync(xyz, d + o_xyz, mv * 24, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && bgr && mv) e = hipMemcpyAsync(bgr, d + o_bgr, mv * 3, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && tri && mt) e = hipMemcpyAsync(tri, d + o_tri, mt * 12, hipMemcpyDeviceToHost, ctx->stream);
    const int rc2 = sfm_finish(ctx, e);
    if (rc2 == SFMHIP_OK) { *n_vertices = n[0]; *n_triangles = n[1]; }
    return rc2;
}

}
