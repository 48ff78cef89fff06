// mesh.hip -- clean-up of an indexed triangle mesh on the device: connected components and their filter, vertex clustering, area-weighted
// vertex normals, Laplacian / Taubin smoothing.  The definitions are in sfmhip.h at sfmhip_mesh_components and are followed to the letter.
// Every kernel is one thread per triangle, vertex or record.  Nothing adds floating-point numbers with atomics: a sum over the corners or
// the neighbours of a vertex is made by ONE thread that walks a run of a stably sorted record list, so its order is the one the header
// words and no result depends on the launch geometry.  Integer atomics appear in the union-find (unionfind.hpp, shared with points.hip)
// and in the size counters only; both are order-free.
//
// Kernels
//   components   mesh_cc_init_kernel, mesh_cc_link_kernel (a triangle unites v0 with v1 and with v2), mesh_cc_flatten_kernel (every
//                referenced vertex pointed at its root, the roots flagged) -- scan -- mesh_cc_label_kernel, mesh_cc_sizes_kernel (a
//                workgroup settles its labels in LDS first: one huge component is the normal case, and costs one global add per workgroup)
//   filter       mesh_largest_kernel (one workgroup), mesh_keep_kernel (flags of the kept triangles and their vertices) -- two scans --
//                mesh_filter_emit_kernel
//   simplify     mesh_ref_kernel, mesh_mask_kernel (NaN rows for the unreferenced vertices), the voxel grid of points.hip,
//                mesh_map_tri_kernel (the rotated triple of cluster numbers and its sort key) -- radix sort, one pass set or two --
//                mesh_tri_head_kernel (the distinct triples and the clusters they name) -- two scans -- mesh_colour_key_kernel -- sort --
//                mesh_colour_kernel, mesh_simplify_emit_kernel
//   normals      mesh_tri_normal_kernel (N_t and the three corner records) -- sort by vertex -- mesh_run_start_kernel,
//                mesh_vertex_normal_kernel (a gather of 24-byte rows N_t in ascending (t, corner))
//   smooth       mesh_pair_key_kernel (six directed pairs per triangle) -- sort -- run heads -- scan -- mesh_csr_kernel,
//                then per step mesh_smooth_step_kernel (a gather of 24-byte rows x_w in ascending w)
// The two gather kernels read rows at random; the vertex numbering of sfmhip_tsdf_mesh (by edge id, x fastest) keeps a vertex's
// neighbours within a few volume rows of it, which is what makes those reads hit in L2.  Nothing here re-orders vertices.
#include "common.hpp"
#include "sortscan.hpp"
#include "unionfind.hpp"
#include <cmath>
#pragma clang fp contract(off)

#define MESH_NV_MAX (1 << 30)
#define MESH_NT_MAX (1 << 28)
#define MESH_ITER_MAX 1000
#define MESH_NONE 0xffffffffu

// b with 2^b - 1 >= nv: every vertex or cluster number fits b bits, and the all-ones value of b bits names none of them
static inline int mesh_bits(int nv) { int b = 1; while (((1ll << b) - 1) < (long long)nv) ++b; return b; }
static inline dim3 mesh_grid(size_t n) { return dim3((unsigned)std::max<size_t>(1, (n + 255) / 256)); }

__device__ __forceinline__ bool mesh_valid(int a, int b, int c, int nv) { return (pu32)a < (pu32)nv && (pu32)b < (pu32)nv && (pu32)c < (pu32)nv; }

// ------------------------------------------------------------------------------------------------ components
__global__ __launch_bounds__(256) void mesh_cc_init_kernel(int nv, pu32* __restrict__ parent, uint8_t* __restrict__ ref, pu32* __restrict__ err)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *err = 0u;
    if (i < (size_t)nv) { parent[i] = (pu32)i; ref[i] = 0; }
}

__global__ __launch_bounds__(256) void mesh_cc_link_kernel(const int32_t* __restrict__ tri, int nt, int nv, pu32* parent, uint8_t* ref, pu32* err)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nt) return;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (!mesh_valid(a, b, c, nv)) return;
    ref[a] = 1; ref[b] = 1; ref[c] = 1;                                    // every writer writes the same value
    const pu32 me = cluster_unite(parent, (pu32)a, (pu32)b, err);
    cluster_unite(parent, me, (pu32)c, err);
}

// every referenced vertex is pointed at its root; flag[i] = 1 where i is a referenced root, nv + 1 entries for the exclusive scan
__global__ __launch_bounds__(256) void mesh_cc_flatten_kernel(const uint8_t* __restrict__ ref, int nv, pu32* parent, pu32* __restrict__ flag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i > (size_t)nv) return;
    pu32 f = 0u;
    if (i < (size_t)nv && ref[i]) {
        const pu32 r = cluster_find(parent, (pu32)i);
        if (r == (pu32)i) f = 1u; else atomicMin(parent + i, r);
    }
    flag[i] = f;
}

// excl[x] = referenced roots below x = the number of the component whose root (its smallest vertex) is x
__global__ __launch_bounds__(256) void mesh_cc_label_kernel(const int32_t* __restrict__ tri, int nt, int nv, const uint8_t* __restrict__ ref,
                                                            const pu32* __restrict__ parent, const pu32* __restrict__ excl, const pu32* __restrict__ err,
                                                            int32_t* __restrict__ tri_label, int32_t* __restrict__ vertex_label, int32_t* __restrict__ n_components)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *n_components = *err ? -1 : (int32_t)excl[nv];
    if (i < (size_t)nv && vertex_label) vertex_label[i] = ref[i] ? (int32_t)excl[parent[i]] : -1;
    if (i < (size_t)nt) {
        const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
        tri_label[i] = mesh_valid(a, b, c, nv) ? (int32_t)excl[parent[a]] : -1;
    }
}

// sizes[c] += 1 per triangle labelled c (sizes zeroed by the caller).  A wave settles up to four of its labels by ballot, as
// cluster_sizes_kernel of points.hip does, but leaves them in LDS; the workgroup then adds each distinct label among those 16 entries
// once.  Where one component fills the workgroup that is one global add for 256 triangles.  Lanes still open add for themselves.
__global__ __launch_bounds__(256) void mesh_cc_sizes_kernel(const int32_t* __restrict__ labels, int nt, int32_t* __restrict__ sizes)
{
    __shared__ int32_t sl[16], sc[16];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lab = i < (size_t)nt ? labels[i] : -1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 16) { sl[threadIdx.x] = -1; sc[threadIdx.x] = 0; }
    __syncthreads();
    bool open = lab >= 0;
    for (int round = 0; round < 4; ++round) {
        const pu64 m = __ballot(open);
        if (!m) break;                                                     // uniform over the wave
        const int leader = __ffsll((long long)m) - 1;
        const int lab0 = __shfl(lab, leader);
        const bool same = open && lab == lab0;
        const pu64 ms = __ballot(same);
        if (same) { if (lane == leader) { sl[wave * 4 + round] = lab0; sc[wave * 4 + round] = (int32_t)__popcll(ms); } open = false; }
    }
    if (open) atomicAdd(sizes + lab, 1);
    __syncthreads();
    if (threadIdx.x < 16 && sl[threadIdx.x] >= 0) {
        const int l = sl[threadIdx.x];
        int total = 0; bool first = true;
        for (int j = 0; j < 16; ++j)
            if (sl[j] == l) { if (j < (int)threadIdx.x) first = false; total += sc[j]; }
        if (first) atomicAdd(sizes + l, total);
    }
}

// tri_label / vertex_label (may be null) / n_components / sizes (nt entries, may be null) of a device mesh, on the context's stream
static int components_enqueue(sfmhip_ctx* ctx, int nv, const int32_t* d_tri, int nt, int32_t* d_tri_label, int32_t* d_vertex_label, int32_t* d_ncomp, int32_t* d_sizes)
{
    hipStream_t st = ctx->stream;
    const size_t NV = (size_t)nv, NT = (size_t)nt;
    SfmCarve carve;
    const size_t o_err = carve(sizeof(pu32)), o_ref = carve(NV), o_par = carve(NV * 4);
    SfmScan F(carve, NV + 1);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    F.bind(w);
    pu32 *err = (pu32*)(w + o_err), *parent = (pu32*)(w + o_par), *flag = F.data;
    uint8_t* ref = (uint8_t*)(w + o_ref);
    hipLaunchKernelGGL(mesh_cc_init_kernel, mesh_grid(NV), dim3(256), 0, st, nv, parent, ref, err);
    hipLaunchKernelGGL(mesh_cc_link_kernel, mesh_grid(NT), dim3(256), 0, st, d_tri, nt, nv, parent, ref, err);
    hipLaunchKernelGGL(mesh_cc_flatten_kernel, mesh_grid(NV + 1), dim3(256), 0, st, (const uint8_t*)ref, nv, parent, flag);
    F.scan(st, NV + 1);
    hipLaunchKernelGGL(mesh_cc_label_kernel, mesh_grid(std::max(NV, NT)), dim3(256), 0, st, d_tri, nt, nv, (const uint8_t*)ref, (const pu32*)parent, (const pu32*)flag,
                       (const pu32*)err, d_tri_label, d_vertex_label, d_ncomp);
    SFM_HIP_TRY(ctx, hipGetLastError());
    if (d_sizes && nt > 0) {
        SFM_HIP_TRY(ctx, hipMemsetAsync(d_sizes, 0, NT * sizeof(int32_t), st));
        hipLaunchKernelGGL(mesh_cc_sizes_kernel, mesh_grid(NT), dim3(256), 0, st, (const int32_t*)d_tri_label, nt, d_sizes);
        SFM_HIP_TRY(ctx, hipGetLastError());
    }
    return SFMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ the component filter
// one workgroup: best[0] = the component with the most triangles (the smallest number among equals), -1 without a component
__global__ __launch_bounds__(256) void mesh_largest_kernel(const int32_t* __restrict__ sizes, const int32_t* __restrict__ n_components, int32_t* __restrict__ best)
{
    __shared__ pu64 sb[256];
    const int C = *n_components;
    pu64 b = 0ull;
    for (int c = threadIdx.x; c < C; c += 256) {
        const pu64 v = ((pu64)(pu32)sizes[c] << 32) | (pu64)(0xffffffffu - (pu32)c);       // a component has at least one triangle: v > 0
        b = v > b ? v : b;
    }
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off && sb[threadIdx.x + off] > sb[threadIdx.x]) sb[threadIdx.x] = sb[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) best[0] = sb[0] ? (int32_t)(0xffffffffu - (pu32)sb[0]) : -1;
}

// tflag[t] = 1 for a kept triangle (nt + 1 entries), vflag[v] = 1 for a vertex of one (nv + 1 entries, zeroed by the caller)
__global__ __launch_bounds__(256) void mesh_keep_kernel(const int32_t* __restrict__ tri, int nt, const int32_t* __restrict__ tri_label, const int32_t* __restrict__ sizes,
                                                        const int32_t* __restrict__ best, int min_triangles, int keep_largest, pu32* __restrict__ tflag, pu32* vflag)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t > (size_t)nt) return;
    pu32 f = 0u;
    if (t < (size_t)nt) {
        const int lab = tri_label[t];
        if (lab >= 0 && sizes[lab] >= min_triangles && (!keep_largest || lab == best[0])) {
            f = 1u;
            vflag[tri[3 * t]] = 1u; vflag[tri[3 * t + 1]] = 1u; vflag[tri[3 * t + 2]] = 1u;       // a labelled triangle is valid
        }
    }
    tflag[t] = f;
}

// vex / tex: the exclusive scans of the flags.  Row i is kept iff the scan steps at i, and goes to the row the scan names.
__global__ __launch_bounds__(256) void mesh_filter_emit_kernel(const double* __restrict__ xyz, const uint8_t* __restrict__ bgr, int nv, const int32_t* __restrict__ tri, int nt,
                                                               const pu32* __restrict__ vex, const pu32* __restrict__ tex, const int32_t* __restrict__ n_components,
                                                               double* __restrict__ xyz_out, uint8_t* __restrict__ bgr_out, int32_t* __restrict__ tri_out,
                                                               int32_t* __restrict__ vertex_map, int32_t* __restrict__ nv_out, int32_t* __restrict__ nt_out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { const bool bad = *n_components < 0; *nv_out = bad ? -1 : (int32_t)vex[nv]; *nt_out = bad ? -1 : (int32_t)tex[nt]; }
    if (i < (size_t)nv) {
        const size_t at = vex[i];
        const bool kept = vex[i + 1] != at;
        if (kept) {
#pragma unroll
            for (int c = 0; c < 3; ++c) xyz_out[3 * at + c] = xyz[3 * i + c];
            if (bgr)
#pragma unroll
                for (int c = 0; c < 3; ++c) bgr_out[3 * at + c] = bgr[3 * i + c];
        }
        if (vertex_map) vertex_map[i] = kept ? (int32_t)at : -1;
    }
    if (i < (size_t)nt) {
        const size_t at = tex[i];
        if (tex[i + 1] != at)
#pragma unroll
            for (int c = 0; c < 3; ++c) tri_out[3 * at + c] = (int32_t)vex[tri[3 * i + c]];
    }
}

static int filter_enqueue(sfmhip_ctx* ctx, const double* d_xyz, const uint8_t* d_bgr, int nv, const int32_t* d_tri, int nt, int min_triangles, int keep_largest,
                          double* d_xyz_out, uint8_t* d_bgr_out, int32_t* d_tri_out, int32_t* d_vertex_map, int32_t* d_nv_out, int32_t* d_nt_out)
{
    hipStream_t st = ctx->stream;
    const size_t NV = (size_t)nv, NT = (size_t)nt, big = std::max(NV, NT);
    SfmCarve carve;
    const size_t o_head = carve(2 * sizeof(int32_t)), o_lab = carve(NT * 4), o_size = carve(NT * 4);
    SfmScan TF(carve, NT + 1), VF(carve, NV + 1);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    TF.bind(w); VF.bind(w);
    int32_t *head = (int32_t*)(w + o_head), *lab = (int32_t*)(w + o_lab), *sizes = (int32_t*)(w + o_size);
    pu32 *tf = TF.data, *vf = VF.data;
    rc = components_enqueue(ctx, nv, d_tri, nt, lab, nullptr, head, sizes);
    if (rc != SFMHIP_OK) return rc;
    if (keep_largest) hipLaunchKernelGGL(mesh_largest_kernel, dim3(1), dim3(256), 0, st, (const int32_t*)sizes, (const int32_t*)head, head + 1);
    SFM_HIP_TRY(ctx, hipMemsetAsync(vf, 0, (NV + 1) * 4, st));
    hipLaunchKernelGGL(mesh_keep_kernel, mesh_grid(NT + 1), dim3(256), 0, st, d_tri, nt, (const int32_t*)lab, (const int32_t*)sizes, (const int32_t*)(head + 1), min_triangles,
                       keep_largest, tf, vf);
    TF.scan(st, NT + 1);
    VF.scan(st, NV + 1);
    hipLaunchKernelGGL(mesh_filter_emit_kernel, mesh_grid(big), dim3(256), 0, st, d_xyz, d_bgr, nv, d_tri, nt, (const pu32*)vf, (const pu32*)tf, (const int32_t*)head, d_xyz_out,
                       d_bgr_out, d_tri_out, d_vertex_map, d_nv_out, d_nt_out);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ vertex clustering
__global__ __launch_bounds__(256) void mesh_ref_kernel(const int32_t* __restrict__ tri, int nt, int nv, uint8_t* ref)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nt) return;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (mesh_valid(a, b, c, nv)) { ref[a] = 1; ref[b] = 1; ref[c] = 1; }
}

__global__ __launch_bounds__(256) void mesh_mask_kernel(const double* __restrict__ xyz, const uint8_t* __restrict__ ref, int nv, double* __restrict__ masked)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nv) return;
    const bool r = ref[i] != 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) masked[3 * i + c] = r ? xyz[3 * i + c] : (double)NAN;
}

// rec[t] = the triangle's cluster numbers, rotated so that the smallest comes first, or (none, none, none), none = 2^bits - 1, for a
// triangle that is dropped; key[t] = the whole triple in 3 * bits bits (two_pass == 0) or its last member (two_pass == 1)
__global__ __launch_bounds__(256) void mesh_map_tri_kernel(const int32_t* __restrict__ tri, int nt, int nv, const int32_t* __restrict__ cluster_of, int bits, int two_pass,
                                                           pu32* __restrict__ rec, pu64* __restrict__ key)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nt) return;
    const pu32 none = (pu32)((1ull << bits) - 1ull);
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    pu32 r0 = none, r1 = none, r2 = none;
    if (mesh_valid(a, b, c, nv)) {
        const int ca = cluster_of[a], cb = cluster_of[b], cc = cluster_of[c];
        if (ca >= 0 && cb >= 0 && cc >= 0 && ca != cb && cb != cc && ca != cc) {
            if (ca < cb && ca < cc) { r0 = (pu32)ca; r1 = (pu32)cb; r2 = (pu32)cc; }
            else if (cb < cc) { r0 = (pu32)cb; r1 = (pu32)cc; r2 = (pu32)ca; }
            else { r0 = (pu32)cc; r1 = (pu32)ca; r2 = (pu32)cb; }
        }
    }
    rec[3 * t] = r0; rec[3 * t + 1] = r1; rec[3 * t + 2] = r2;
    key[t] = two_pass ? (pu64)r2 : ((((pu64)r0 << bits) | (pu64)r1) << bits) | (pu64)r2;
}

// the key of the second sort: the first two members of the triple that stands at place i after the first
__global__ __launch_bounds__(256) void mesh_key2_kernel(const pu32* __restrict__ rec, const pu32* __restrict__ order, int nt, int bits, pu64* __restrict__ key)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nt) return;
    const size_t t = order[i];
    key[i] = ((pu64)rec[3 * t] << bits) | (pu64)rec[3 * t + 1];
}

// the triples in sorted order: tflag[i] = 1 where a new triple begins (nt + 1 entries), cflag[c] = 1 for every cluster such a triple
// names (nv + 1 entries, zeroed by the caller)
__global__ __launch_bounds__(256) void mesh_tri_head_kernel(const pu32* __restrict__ rec, const pu32* __restrict__ order, int nt, pu32* __restrict__ tflag, pu32* cflag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i > (size_t)nt) return;
    pu32 f = 0u;
    if (i < (size_t)nt) {
        const size_t t = order[i];
        const pu32 r0 = rec[3 * t], r1 = rec[3 * t + 1], r2 = rec[3 * t + 2];
        if (r0 != r1) {                                                    // a kept triple has three different members
            f = 1u;
            if (i > 0) { const size_t p = order[i - 1]; if (rec[3 * p] == r0 && rec[3 * p + 1] == r1 && rec[3 * p + 2] == r2) f = 0u; }
            if (f) { cflag[r0] = 1u; cflag[r1] = 1u; cflag[r2] = 1u; }
        }
    }
    tflag[i] = f;
}

__global__ __launch_bounds__(256) void mesh_colour_key_kernel(const int32_t* __restrict__ cluster_of, int nv, int bits, pu64* __restrict__ key)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nv) return;
    const int c = cluster_of[i];
    key[i] = c >= 0 ? (pu64)c : (1ull << bits) - 1ull;
}

// thread i: the head of a cluster's run in the sorted vertex list sums the run's colours (integers: any order gives the same sums)
__global__ __launch_bounds__(256) void mesh_colour_kernel(const pu64* __restrict__ key, const pu32* __restrict__ order, const uint8_t* __restrict__ bgr, int nv, int bits,
                                                          const pu32* __restrict__ cex, uint8_t* __restrict__ bgr_out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nv) return;
    const pu64 k = key[i];
    if (k == (1ull << bits) - 1ull || (i > 0 && key[i - 1] == k)) return;
    const size_t at = cex[k];
    if (cex[k + 1] == at) return;                                          // a cluster no triangle names
    pu64 s0 = 0, s1 = 0, s2 = 0, n = 0;
    for (size_t j = i; j < (size_t)nv && key[j] == k; ++j, ++n) {
        const size_t v = order[j];
        s0 += bgr[3 * v]; s1 += bgr[3 * v + 1]; s2 += bgr[3 * v + 2];
    }
    bgr_out[3 * at] = (uint8_t)((2 * s0 + n) / (2 * n)); bgr_out[3 * at + 1] = (uint8_t)((2 * s1 + n) / (2 * n)); bgr_out[3 * at + 2] = (uint8_t)((2 * s2 + n) / (2 * n));
}

__global__ __launch_bounds__(256) void mesh_simplify_emit_kernel(const double* __restrict__ centroid, const int32_t* __restrict__ cluster_of, int nv,
                                                                 const pu32* __restrict__ rec, const pu32* __restrict__ order, int nt, const pu32* __restrict__ cex,
                                                                 const pu32* __restrict__ tex, const int32_t* __restrict__ n_clusters, double* __restrict__ xyz_out,
                                                                 int32_t* __restrict__ tri_out, int32_t* __restrict__ vertex_map, int32_t* __restrict__ nv_out,
                                                                 int32_t* __restrict__ nt_out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { const bool bad = *n_clusters < 0; *nv_out = bad ? -1 : (int32_t)cex[nv]; *nt_out = bad ? 0 : (int32_t)tex[nt]; }
    if (i < (size_t)nv) {
        const size_t at = cex[i];                                          // i as a cluster number
        if (cex[i + 1] != at)
#pragma unroll
            for (int c = 0; c < 3; ++c) xyz_out[3 * at + c] = centroid[3 * i + c];
        if (vertex_map) {                                                  // i as a vertex
            const int c = cluster_of[i];
            vertex_map[i] = c >= 0 && cex[c + 1] != cex[c] ? (int32_t)cex[c] : -1;
        }
    }
    if (i < (size_t)nt) {
        const size_t at = tex[i];
        if (tex[i + 1] != at) {
            const size_t t = order[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) tri_out[3 * at + c] = (int32_t)cex[rec[3 * t + c]];
        }
    }
}

static int simplify_enqueue(sfmhip_ctx* ctx, const double* d_xyz, const uint8_t* d_bgr, int nv, const int32_t* d_tri, int nt, double voxel, double* d_xyz_out,
                            uint8_t* d_bgr_out, int32_t* d_tri_out, int32_t* d_vertex_map, int32_t* d_nv_out, int32_t* d_nt_out)
{
    hipStream_t st = ctx->stream;
    if (nv == 0) {                                                         // nothing to cluster: an empty mesh
        SFM_HIP_TRY(ctx, hipMemsetAsync(d_nv_out, 0, sizeof(int32_t), st));
        SFM_HIP_TRY(ctx, hipMemsetAsync(d_nt_out, 0, sizeof(int32_t), st));
        return SFMHIP_OK;
    }
    const size_t NV = (size_t)nv, NT = (size_t)nt, big = std::max(NV, NT);
    const int bits = mesh_bits(nv), two_pass = 3 * bits > 64 ? 1 : 0;
    SfmCarve carve;
    const size_t o_nc = carve(sizeof(int32_t)), o_ref = carve(NV), o_mask = carve(NV * 24), o_cen = carve(NV * 24), o_cof = carve(NV * 4), o_rec = carve(NT * 12);
    SfmScan TF(carve, NT + 1), CF(carve, NV + 1);
    SfmSort S(carve, big);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    TF.bind(w); CF.bind(w); S.bind(w);
    int32_t *nc = (int32_t*)(w + o_nc), *cof = (int32_t*)(w + o_cof);
    uint8_t* ref = (uint8_t*)(w + o_ref);
    double *masked = (double*)(w + o_mask), *cen = (double*)(w + o_cen);
    pu32 *rec = (pu32*)(w + o_rec), *tf = TF.data, *cf = CF.data;
    SFM_HIP_TRY(ctx, hipMemsetAsync(ref, 0, NV, st));
    hipLaunchKernelGGL(mesh_ref_kernel, mesh_grid(NT), dim3(256), 0, st, d_tri, nt, nv, ref);
    hipLaunchKernelGGL(mesh_mask_kernel, mesh_grid(NV), dim3(256), 0, st, d_xyz, (const uint8_t*)ref, nv, masked);
    SFM_HIP_TRY(ctx, hipGetLastError());
    rc = sfm_voxel_downsample_enqueue(ctx, masked, nv, voxel, cen, nullptr, cof, nc);
    if (rc != SFMHIP_OK) return rc;
    hipLaunchKernelGGL(mesh_map_tri_kernel, mesh_grid(NT), dim3(256), 0, st, d_tri, nt, nv, (const int32_t*)cof, bits, two_pass, rec, S.k[0]);
    int cur = S.sort(st, NT, 0, two_pass ? bits : 3 * bits, true);
    if (two_pass && nt > 0) {
        hipLaunchKernelGGL(mesh_key2_kernel, mesh_grid(NT), dim3(256), 0, st, (const pu32*)rec, (const pu32*)S.v[cur], nt, bits, S.k[cur]);
        cur = S.sort(st, NT, cur, 2 * bits, false);
    }
    SFM_HIP_TRY(ctx, hipMemsetAsync(cf, 0, (NV + 1) * 4, st));
    hipLaunchKernelGGL(mesh_tri_head_kernel, mesh_grid(NT + 1), dim3(256), 0, st, (const pu32*)rec, (const pu32*)S.v[cur], nt, tf, cf);
    TF.scan(st, NT + 1);
    CF.scan(st, NV + 1);
    hipLaunchKernelGGL(mesh_simplify_emit_kernel, mesh_grid(big), dim3(256), 0, st, (const double*)cen, (const int32_t*)cof, nv, (const pu32*)rec, (const pu32*)S.v[cur], nt,
                       (const pu32*)cf, (const pu32*)tf, (const int32_t*)nc, d_xyz_out, d_tri_out, d_vertex_map, d_nv_out, d_nt_out);
    SFM_HIP_TRY(ctx, hipGetLastError());
    if (d_bgr) {                                                           // the triangle sort is done with: its buffers serve the vertices
        hipLaunchKernelGGL(mesh_colour_key_kernel, mesh_grid(NV), dim3(256), 0, st, (const int32_t*)cof, nv, bits, S.k[0]);
        const int cc = S.sort(st, NV, 0, bits, true);
        hipLaunchKernelGGL(mesh_colour_kernel, mesh_grid(NV), dim3(256), 0, st, (const pu64*)S.k[cc], (const pu32*)S.v[cc], d_bgr, nv, bits, (const pu32*)cf, d_bgr_out);
        SFM_HIP_TRY(ctx, hipGetLastError());
    }
    return SFMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ vertex normals
// N_t of a valid triangle and its three corner records (key: the vertex; the record number 3 t + corner is the sort's value)
__global__ __launch_bounds__(256) void mesh_tri_normal_kernel(const double* __restrict__ xyz, const int32_t* __restrict__ tri, int nt, int nv, int bits,
                                                              double* __restrict__ tn, pu64* __restrict__ key)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nt) return;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (!mesh_valid(a, b, c, nv)) {
        const pu64 none = (1ull << bits) - 1ull;
        key[3 * t] = none; key[3 * t + 1] = none; key[3 * t + 2] = none;
        return;
    }
    const double* p0 = xyz + 3 * (size_t)a; const double* p1 = xyz + 3 * (size_t)b; const double* p2 = xyz + 3 * (size_t)c;
    const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2], e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    tn[3 * t] = e1y * e2z - e1z * e2y; tn[3 * t + 1] = e1z * e2x - e1x * e2z; tn[3 * t + 2] = e1x * e2y - e1y * e2x;
    key[3 * t] = (pu64)a; key[3 * t + 1] = (pu64)b; key[3 * t + 2] = (pu64)c;
}

// start[v] = the place of vertex v's first record in the sorted list (start holds MESH_NONE everywhere before)
__global__ __launch_bounds__(256) void mesh_run_start_kernel(const pu64* __restrict__ key, size_t n, int bits, pu32* __restrict__ start)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const pu64 k = key[i];
    if (k != (1ull << bits) - 1ull && (i == 0 || key[i - 1] != k)) start[k] = (pu32)i;
}

__global__ __launch_bounds__(256) void mesh_vertex_normal_kernel(const pu64* __restrict__ key, const pu32* __restrict__ order, const double* __restrict__ tn, size_t n, int nv,
                                                                 const pu32* __restrict__ start, double* __restrict__ normals)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= (size_t)nv) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    const pu32 s = start[v];
    if (s != MESH_NONE)
        for (size_t j = s; j < n && key[j] == (pu64)v; ++j) {
            const size_t t = order[j] / 3u;
            sx += tn[3 * t]; sy += tn[3 * t + 1]; sz += tn[3 * t + 2];
        }
    const double l = sqrt((sx * sx + sy * sy) + sz * sz);
    const bool ok = l > 0.0 && isfinite(l);
    normals[3 * v] = ok ? sx / l : 0.0; normals[3 * v + 1] = ok ? sy / l : 0.0; normals[3 * v + 2] = ok ? sz / l : 0.0;
}

static int normals_enqueue(sfmhip_ctx* ctx, const double* d_xyz, int nv, const int32_t* d_tri, int nt, double* d_normals)
{
    hipStream_t st = ctx->stream;
    if (nv == 0) return SFMHIP_OK;
    const size_t NV = (size_t)nv, NT = (size_t)nt, n3 = 3 * NT;
    const int bits = mesh_bits(nv);
    SfmCarve carve;
    const size_t o_tn = carve(NT * 24), o_start = carve(NV * 4);
    SfmSort S(carve, n3);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    S.bind(w);
    double* tn = (double*)(w + o_tn);
    pu32* start = (pu32*)(w + o_start);
    hipLaunchKernelGGL(mesh_tri_normal_kernel, mesh_grid(NT), dim3(256), 0, st, d_xyz, d_tri, nt, nv, bits, tn, S.k[0]);
    const int cur = S.sort(st, n3, 0, bits, true);
    SFM_HIP_TRY(ctx, hipMemsetAsync(start, 0xff, NV * 4, st));
    hipLaunchKernelGGL(mesh_run_start_kernel, mesh_grid(n3), dim3(256), 0, st, (const pu64*)S.k[cur], n3, bits, start);
    hipLaunchKernelGGL(mesh_vertex_normal_kernel, mesh_grid(NV), dim3(256), 0, st, (const pu64*)S.k[cur], (const pu32*)S.v[cur], (const double*)tn, n3, nv, (const pu32*)start,
                       d_normals);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ smoothing
// the six directed pairs (v, w) of a valid triangle as v * 2^bits + w; all ones in 2 * bits bits for v == w and for an invalid triangle
__global__ __launch_bounds__(256) void mesh_pair_key_kernel(const int32_t* __restrict__ tri, int nt, int nv, int bits, pu64* __restrict__ key)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nt) return;
    const pu64 none = (1ull << (2 * bits)) - 1ull;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    const bool ok = mesh_valid(a, b, c, nv);
    const pu64 A = (pu64)(pu32)a, B = (pu64)(pu32)b, C = (pu64)(pu32)c;
    pu64* k = key + 6 * t;
    k[0] = ok && a != b ? (A << bits) | B : none; k[1] = ok && a != c ? (A << bits) | C : none;
    k[2] = ok && a != b ? (B << bits) | A : none; k[3] = ok && b != c ? (B << bits) | C : none;
    k[4] = ok && a != c ? (C << bits) | A : none; k[5] = ok && b != c ? (C << bits) | B : none;
}

// the distinct pairs in order: pair[excl[i]] = the pair, row[v] = the place of v's first pair (row holds MESH_NONE everywhere before)
__global__ __launch_bounds__(256) void mesh_csr_kernel(const pu64* __restrict__ key, size_t n, int bits, const pu32* __restrict__ excl, pu64* __restrict__ pair,
                                                       pu32* __restrict__ row)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const pu32 at = excl[i];
    if (excl[i + 1] == at) return;
    const pu64 k = key[i];
    pair[at] = k;
    if (i == 0 || (key[i - 1] >> bits) != (k >> bits)) row[k >> bits] = at;
}

// one step: out = p + f * (mean of the neighbours - p), the neighbours summed from +0.0 in ascending index; no neighbour: out = p
__global__ __launch_bounds__(256) void mesh_smooth_step_kernel(const double* __restrict__ in, double* __restrict__ out, int nv, const pu32* __restrict__ row,
                                                               const pu64* __restrict__ pair, const pu32* __restrict__ n_pairs, int bits, double f)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= (size_t)nv) return;
    const double px = in[3 * v], py = in[3 * v + 1], pz = in[3 * v + 2];
    double ox = px, oy = py, oz = pz;
    const pu32 s = row[v];
    if (s != MESH_NONE) {
        const size_t E = *n_pairs;
        const pu64 low = (1ull << bits) - 1ull;
        double mx = 0.0, my = 0.0, mz = 0.0;
        int deg = 0;
        for (size_t j = s; j < E; ++j, ++deg) {
            const pu64 k = pair[j];
            if ((k >> bits) != (pu64)v) break;
            const size_t u = (size_t)(k & low);
            mx += in[3 * u]; my += in[3 * u + 1]; mz += in[3 * u + 2];
        }
        const double d = (double)deg;
        mx = mx / d; my = my / d; mz = mz / d;
        ox = px + f * (mx - px); oy = py + f * (my - py); oz = pz + f * (mz - pz);
    }
    out[3 * v] = ox; out[3 * v + 1] = oy; out[3 * v + 2] = oz;
}

static int smooth_enqueue(sfmhip_ctx* ctx, const double* d_xyz, int nv, const int32_t* d_tri, int nt, int iterations, double lambda, double mu, double* d_xyz_out)
{
    hipStream_t st = ctx->stream;
    if (nv == 0) return SFMHIP_OK;
    const size_t NV = (size_t)nv, NT = (size_t)nt, n6 = 6 * NT;
    const int steps = mu == 0.0 ? iterations : 2 * iterations;
    if (steps == 0) {
        SFM_HIP_TRY(ctx, hipMemcpyAsync(d_xyz_out, d_xyz, NV * 24, hipMemcpyDeviceToDevice, st));
        return SFMHIP_OK;
    }
    const int bits = mesh_bits(nv);
    SfmCarve carve;
    const size_t o_row = carve(NV * 4), o_tmp = carve(steps > 1 ? NV * 24 : 0);
    SfmScan F(carve, n6 + 1);
    SfmSort S(carve, n6);
    SfmPoolHold hold(ctx);
    char* w = nullptr;
    const int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    F.bind(w); S.bind(w);
    pu32 *row = (pu32*)(w + o_row), *flag = F.data;
    double* tmp = (double*)(w + o_tmp);
    hipLaunchKernelGGL(mesh_pair_key_kernel, mesh_grid(NT), dim3(256), 0, st, d_tri, nt, nv, bits, S.k[0]);
    const int cur = S.sort(st, n6, 0, 2 * bits, true);
    sfm_enqueue_run_heads(st, S.k[cur], n6, (1ull << (2 * bits)) - 1ull, flag);      // mesh_pair_key_kernel's "none": no pair begins there
    F.scan(st, n6 + 1);
    SFM_HIP_TRY(ctx, hipMemsetAsync(row, 0xff, NV * 4, st));
    pu64* pair = S.k[cur ^ 1];                                             // the sort's other key buffer is free now
    hipLaunchKernelGGL(mesh_csr_kernel, mesh_grid(n6), dim3(256), 0, st, (const pu64*)S.k[cur], n6, bits, (const pu32*)flag, pair, row);
    // two buffers, the last step writes the output
    const double* src = d_xyz;
    for (int s = 0; s < steps; ++s) {
        double* dst = (steps - 1 - s) % 2 == 0 ? d_xyz_out : tmp;
        const double f = mu == 0.0 || s % 2 == 0 ? lambda : mu;
        hipLaunchKernelGGL(mesh_smooth_step_kernel, mesh_grid(NV), dim3(256), 0, st, src, dst, nv, (const pu32*)row, (const pu64*)pair, (const pu32*)(flag + n6), bits, f);
        src = dst;
    }
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool mesh_shape_ok(const sfmhip_ctx* ctx, int nv, int nt) { return ctx && nv >= 0 && nv <= MESH_NV_MAX && nt >= 0 && nt <= MESH_NT_MAX; }
// an output that is also an input
static inline bool mesh_alias(std::initializer_list<const void*> in, std::initializer_list<const void*> out)
{
    for (const void* o : out)
        for (const void* i : in)
            if (o && o == i) return true;
    return false;
}
static inline bool mesh_io_ok(const void* xyz, const void* bgr, int nv, const void* tri, int nt, const void* xyz_out, const void* bgr_out, const void* tri_out,
                              const void* vertex_map, const void* nv_out, const void* nt_out)
{
    return (nv == 0 || (xyz && xyz_out && (!bgr || bgr_out))) && (nt == 0 || (tri && tri_out)) && nv_out && nt_out &&
           !mesh_alias({ xyz, bgr, tri }, { xyz_out, bgr_out, tri_out, vertex_map, nv_out, nt_out });
}

// the device image of a host mesh and of the outputs of a filter or a simplification
struct MeshIo {
    double *xyz = nullptr, *xyz_out = nullptr; uint8_t *bgr = nullptr, *bgr_out = nullptr; int32_t *tri = nullptr, *tri_out = nullptr, *map = nullptr, *n = nullptr;
};
static int mesh_io_upload(sfmhip_ctx* ctx, SfmPoolHold& hold, const double* xyz, const uint8_t* bgr, int nv, const int32_t* tri, int nt, bool want_map, MeshIo& d)
{
    const size_t NV = (size_t)nv, NT = (size_t)nt;
    SfmCarve carve;
    const size_t o_xyz = carve(NV * 24), o_xo = carve(NV * 24), o_bgr = carve(bgr ? NV * 3 : 0), o_bo = carve(bgr ? NV * 3 : 0), o_tri = carve(NT * 12), o_to = carve(NT * 12),
                 o_map = carve(want_map ? NV * 4 : 0), o_n = carve(2 * sizeof(int32_t));
    char* w = nullptr;
    int rc = hold.get(carve.bytes, (void**)&w);
    if (rc != SFMHIP_OK) return rc;
    d.xyz = (double*)(w + o_xyz); d.xyz_out = (double*)(w + o_xo); d.bgr = bgr ? (uint8_t*)(w + o_bgr) : nullptr; d.bgr_out = bgr ? (uint8_t*)(w + o_bo) : nullptr;
    d.tri = (int32_t*)(w + o_tri); d.tri_out = (int32_t*)(w + o_to); d.map = want_map ? (int32_t*)(w + o_map) : nullptr; d.n = (int32_t*)(w + o_n);
    if (nv > 0) rc = sfm_upload(ctx, d.xyz, xyz, NV * 24);
    if (rc == SFMHIP_OK && nv > 0 && bgr) rc = sfm_upload(ctx, d.bgr, bgr, NV * 3);
    if (rc == SFMHIP_OK && nt > 0) rc = sfm_upload(ctx, d.tri, tri, NT * 12);
    return rc;
}
// the counts, then the rows they name; the caller's counts are written last, and only when everything arrived
static int mesh_io_download(sfmhip_ctx* ctx, const MeshIo& d, int nv, double* xyz_out, uint8_t* bgr_out, int32_t* tri_out, int32_t* vertex_map, int* nv_out, int* nt_out,
                            const char* what_minus_one, int rc_minus_one)
{
    hipStream_t st = ctx->stream;
    int32_t n[2] = { 0, 0 };
    int rc = sfm_finish(ctx, hipMemcpyAsync(n, d.n, sizeof n, hipMemcpyDeviceToHost, st));
    if (rc != SFMHIP_OK) return rc;
    if (n[0] < 0) { ctx->last_error = what_minus_one; return rc_minus_one; }
    hipError_t e = hipSuccess;
    if (n[0] > 0) e = hipMemcpyAsync(xyz_out, d.xyz_out, (size_t)n[0] * 24, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && n[0] > 0 && d.bgr_out) e = hipMemcpyAsync(bgr_out, d.bgr_out, (size_t)n[0] * 3, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && n[1] > 0) e = hipMemcpyAsync(tri_out, d.tri_out, (size_t)n[1] * 12, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && vertex_map && nv > 0) e = hipMemcpyAsync(vertex_map, d.map, (size_t)nv * 4, hipMemcpyDeviceToHost, st);
    rc = sfm_finish(ctx, e);
    if (rc == SFMHIP_OK) { *nv_out = n[0]; *nt_out = n[1]; }
    return rc;
}

static const char* const MESH_ERR_CAP = "mesh components: a union exceeded its retry cap (the parent array broke its invariant); no result";
static const char* const MESH_ERR_EXTENT =
    "bad argument: the cluster cell is too small for the mesh's extent (more than 2^21 cells along an axis; filter far fragments first)";

// the shape of the two host calls that turn a mesh into one nv x 3 array of doubles
template <class Enqueue>
static int mesh_rows_host(sfmhip_ctx* ctx, const double* xyz, int nv, const int32_t* tri, int nt, double* out, Enqueue enqueue)
{
    if (nv == 0) return SFMHIP_OK;
    const size_t NV = (size_t)nv, NT = (size_t)nt;
    SfmCarve carve;
    const size_t o_xyz = carve(NV * 24), o_tri = carve(NT * 12), o_out = carve(NV * 24);
    SfmPoolHold hold(ctx);
    char* d = nullptr;
    int rc = hold.get(carve.bytes, (void**)&d);
    if (rc == SFMHIP_OK) rc = sfm_upload(ctx, d + o_xyz, xyz, NV * 24);
    if (rc == SFMHIP_OK && nt > 0) rc = sfm_upload(ctx, d + o_tri, tri, NT * 12);
    if (rc == SFMHIP_OK) rc = enqueue((const double*)(d + o_xyz), (const int32_t*)(d + o_tri), (double*)(d + o_out));
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    return sfm_finish(ctx, hipMemcpyAsync(out, d + o_out, NV * 24, hipMemcpyDeviceToHost, ctx->stream));
}

static inline bool smooth_args_ok(const sfmhip_ctx* ctx, const void* xyz, int nv, const void* tri, int nt, int iterations, double lambda, double mu, const void* out)
{
    return mesh_shape_ok(ctx, nv, nt) && iterations >= 0 && iterations <= MESH_ITER_MAX && std::isfinite(lambda) && std::isfinite(mu) && (nv == 0 || (xyz && out)) &&
           (nt == 0 || tri) && !mesh_alias({ xyz, tri }, { out });
}

extern "C" {

int sfmhip_mesh_components_dev(sfmhip_ctx* ctx, int nv, const int32_t* d_tri, int nt, int32_t* d_tri_label, int32_t* d_vertex_label, int32_t* d_n_components,
                               int32_t* d_sizes)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_components_dev");
    SFM_ARG_CHECK(ctx, mesh_shape_ok(ctx, nv, nt) && d_n_components && (nt == 0 || (d_tri && d_tri_label)) &&
                           !mesh_alias({ d_tri }, { d_tri_label, d_vertex_label, d_n_components, d_sizes }));
    return components_enqueue(ctx, nv, d_tri, nt, d_tri_label, d_vertex_label, d_n_components, d_sizes);
}

int sfmhip_mesh_components(sfmhip_ctx* ctx, int nv, const int32_t* tri, int nt, int32_t* tri_label, int32_t* vertex_label, int* n_components, int32_t* sizes)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_components");
    SFM_ARG_CHECK(ctx, mesh_shape_ok(ctx, nv, nt) && n_components && (nt == 0 || (tri && tri_label)) && !mesh_alias({ tri }, { tri_label, vertex_label, n_components, sizes }));
    const size_t NV = (size_t)nv, NT = (size_t)nt;
    SfmCarve carve;
    const size_t o_tri = carve(NT * 12), o_tl = carve(NT * 4), o_vl = carve(vertex_label ? NV * 4 : 0), o_sz = carve(sizes ? NT * 4 : 0), o_n = carve(sizeof(int32_t));
    SfmPoolHold hold(ctx);
    char* d = nullptr;
    int rc = hold.get(carve.bytes, (void**)&d);
    if (rc == SFMHIP_OK && nt > 0) rc = sfm_upload(ctx, d + o_tri, tri, NT * 12);
    if (rc == SFMHIP_OK)
        rc = components_enqueue(ctx, nv, (const int32_t*)(d + o_tri), nt, (int32_t*)(d + o_tl), vertex_label ? (int32_t*)(d + o_vl) : nullptr, (int32_t*)(d + o_n),
                                sizes ? (int32_t*)(d + o_sz) : nullptr);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    hipStream_t st = ctx->stream;
    int32_t C = 0;
    rc = sfm_finish(ctx, hipMemcpyAsync(&C, d + o_n, sizeof C, hipMemcpyDeviceToHost, st));
    if (rc != SFMHIP_OK) return rc;
    if (C < 0) { ctx->last_error = MESH_ERR_CAP; return SFMHIP_E_NUMERIC; }
    hipError_t e = hipSuccess;
    if (nt > 0) e = hipMemcpyAsync(tri_label, d + o_tl, NT * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && vertex_label && nv > 0) e = hipMemcpyAsync(vertex_label, d + o_vl, NV * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && sizes && C > 0) e = hipMemcpyAsync(sizes, d + o_sz, (size_t)C * 4, hipMemcpyDeviceToHost, st);
    rc = sfm_finish(ctx, e);
    if (rc == SFMHIP_OK) *n_components = C;
    return rc;
}

int sfmhip_mesh_filter_components_dev(sfmhip_ctx* ctx, const double* d_xyz, const uint8_t* d_bgr, int nv, const int32_t* d_tri, int nt, int min_triangles, int keep_largest,
                                      double* d_xyz_out, uint8_t* d_bgr_out, int32_t* d_tri_out, int32_t* d_vertex_map, int32_t* d_nv_out, int32_t* d_nt_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_filter_components_dev");
    SFM_ARG_CHECK(ctx, mesh_shape_ok(ctx, nv, nt) && min_triangles >= 1 && (keep_largest == 0 || keep_largest == 1) &&
                           mesh_io_ok(d_xyz, d_bgr, nv, d_tri, nt, d_xyz_out, d_bgr_out, d_tri_out, d_vertex_map, d_nv_out, d_nt_out));
    return filter_enqueue(ctx, d_xyz, d_bgr, nv, d_tri, nt, min_triangles, keep_largest, d_xyz_out, d_bgr_out, d_tri_out, d_vertex_map, d_nv_out, d_nt_out);
}

int sfmhip_mesh_filter_components(sfmhip_ctx* ctx, const double* xyz, const uint8_t* bgr, int nv, const int32_t* tri, int nt, int min_triangles, int keep_largest,
                                  double* xyz_out, uint8_t* bgr_out, int32_t* tri_out, int32_t* vertex_map, int* nv_out, int* nt_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_filter_components");
    SFM_ARG_CHECK(ctx, mesh_shape_ok(ctx, nv, nt) && min_triangles >= 1 && (keep_largest == 0 || keep_largest == 1) &&
                           mesh_io_ok(xyz, bgr, nv, tri, nt, xyz_out, bgr_out, tri_out, vertex_map, nv_out, nt_out));
    SfmPoolHold hold(ctx);
    MeshIo d;
    int rc = mesh_io_upload(ctx, hold, xyz, bgr, nv, tri, nt, vertex_map != nullptr, d);
    if (rc == SFMHIP_OK) rc = filter_enqueue(ctx, d.xyz, d.bgr, nv, d.tri, nt, min_triangles, keep_largest, d.xyz_out, d.bgr_out, d.tri_out, d.map, d.n, d.n + 1);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    return mesh_io_download(ctx, d, nv, xyz_out, bgr_out, tri_out, vertex_map, nv_out, nt_out, MESH_ERR_CAP, SFMHIP_E_NUMERIC);
}

int sfmhip_mesh_simplify_dev(sfmhip_ctx* ctx, const double* d_xyz, const uint8_t* d_bgr, int nv, const int32_t* d_tri, int nt, double voxel, double* d_xyz_out,
                             uint8_t* d_bgr_out, int32_t* d_tri_out, int32_t* d_vertex_map, int32_t* d_nv_out, int32_t* d_nt_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_simplify_dev");
    SFM_ARG_CHECK(ctx, mesh_shape_ok(ctx, nv, nt) && std::isfinite(voxel) && voxel > 0.0 &&
                           mesh_io_ok(d_xyz, d_bgr, nv, d_tri, nt, d_xyz_out, d_bgr_out, d_tri_out, d_vertex_map, d_nv_out, d_nt_out));
    return simplify_enqueue(ctx, d_xyz, d_bgr, nv, d_tri, nt, voxel, d_xyz_out, d_bgr_out, d_tri_out, d_vertex_map, d_nv_out, d_nt_out);
}

int sfmhip_mesh_simplify(sfmhip_ctx* ctx, const double* xyz, const uint8_t* bgr, int nv, const int32_t* tri, int nt, double voxel, double* xyz_out, uint8_t* bgr_out,
                         int32_t* tri_out, int32_t* vertex_map, int* nv_out, int* nt_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_simplify");
    SFM_ARG_CHECK(ctx, mesh_shape_ok(ctx, nv, nt) && std::isfinite(voxel) && voxel > 0.0 &&
                           mesh_io_ok(xyz, bgr, nv, tri, nt, xyz_out, bgr_out, tri_out, vertex_map, nv_out, nt_out));
    SfmPoolHold hold(ctx);
    MeshIo d;
    int rc = mesh_io_upload(ctx, hold, xyz, bgr, nv, tri, nt, vertex_map != nullptr, d);
    if (rc == SFMHIP_OK) rc = simplify_enqueue(ctx, d.xyz, d.bgr, nv, d.tri, nt, voxel, d.xyz_out, d.bgr_out, d.tri_out, d.map, d.n, d.n + 1);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    return mesh_io_download(ctx, d, nv, xyz_out, bgr_out, tri_out, vertex_map, nv_out, nt_out, MESH_ERR_EXTENT, SFMHIP_E_ARG);
}

int sfmhip_mesh_vertex_normals_dev(sfmhip_ctx* ctx, const double* d_xyz, int nv, const int32_t* d_tri, int nt, double* d_normals)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_vertex_normals_dev");
    SFM_ARG_CHECK(ctx, mesh_shape_ok(ctx, nv, nt) && (nv == 0 || (d_xyz && d_normals)) && (nt == 0 || d_tri) && !mesh_alias({ d_xyz, d_tri }, { d_normals }));
    return normals_enqueue(ctx, d_xyz, nv, d_tri, nt, d_normals);
}

int sfmhip_mesh_vertex_normals(sfmhip_ctx* ctx, const double* xyz, int nv, const int32_t* tri, int nt, double* normals)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_vertex_normals");
    SFM_ARG_CHECK(ctx, mesh_shape_ok(ctx, nv, nt) && (nv == 0 || (xyz && normals)) && (nt == 0 || tri) && !mesh_alias({ xyz, tri }, { normals }));
    return mesh_rows_host(ctx, xyz, nv, tri, nt, normals, [&](const double* dx, const int32_t* dt, double* dout) { return normals_enqueue(ctx, dx, nv, dt, nt, dout); });
}

int sfmhip_mesh_smooth_dev(sfmhip_ctx* ctx, const double* d_xyz, int nv, const int32_t* d_tri, int nt, int iterations, double lambda, double mu, double* d_xyz_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_smooth_dev");
    SFM_ARG_CHECK(ctx, smooth_args_ok(ctx, d_xyz, nv, d_tri, nt, iterations, lambda, mu, d_xyz_out));
    return smooth_enqueue(ctx, d_xyz, nv, d_tri, nt, iterations, lambda, mu, d_xyz_out);
}

int sfmhip_mesh_smooth(sfmhip_ctx* ctx, const double* xyz, int nv, const int32_t* tri, int nt, int iterations, double lambda, double mu, double* xyz_out)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_mesh_smooth");
    SFM_ARG_CHECK(ctx, smooth_args_ok(ctx, xyz, nv, tri, nt, iterations, lambda, mu, xyz_out));
    return mesh_rows_host(ctx, xyz, nv, tri, nt, xyz_out,
                          [&](const double* dx, const int32_t* dt, double* dout) { return smooth_enqueue(ctx, dx, nv, dt, nt, iterations, lambda, mu, dout); });
}

}  // extern "C"
