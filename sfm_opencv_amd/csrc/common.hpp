// common.hpp -- internal definitions shared by the translation units of libsfmhip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/sfmhip.h"

struct sfmhip_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;       // the stream every launch goes to (own_stream or an external one)
    std::string last_error;
    // grow-only pinned host staging (results the kernels write straight into host memory: sfmhip_match_pairs)
    void*  pinned = nullptr;
    size_t pinned_bytes = 0;
    // pinned staging ring for large uploads from the caller's pageable memory (sfm_upload, context.hip)
    static constexpr size_t STAGE_BYTES = (size_t)16 << 20;
    void*  stage[2] = { nullptr, nullptr };
    hipEvent_t stage_ev[2] = { nullptr, nullptr };
    bool   stage_busy[2] = { false, false };
    int    stage_next = 0;
    struct CopyPool* copy_pool = nullptr;      // 4 to 16 threads, the caller among them, that fill the staging buffers (copy_pool.hpp)
    // Cache of device blocks (sfm_pool_get / sfm_pool_put), the one source of device memory of this library: the arrays of
    // descriptor sets and bundle-adjustment problems, and every temporary of every call (through an SfmPoolHold, below).
    //  * Who may take blocks: code that works on ctx->stream, and only on it (a BA problem also runs on a second stream:
    //    sfmhip_ba_destroy drains both before its blocks can be handed out again).
    //  * Reuse is stream-ordered: a block that is put back may be handed out at once, while work that reads or writes it is
    //    still queued.  Its next user is enqueued behind that work on the same stream, so it sees the block only afterwards;
    //    nobody waits on the host.  A block comes back with whatever its last user left in it.
    //  * An enqueue-only (_dev) call may therefore hold its temporaries in an SfmPoolHold of its own scope and return with its
    //    launches still queued.  It may not assume anything about a block's contents, nor keep a pointer to one past its return.
    //    A call whose HOST buffers are sources or targets of queued copies drains the stream before it returns (sfm_finish /
    //    sfm_drain); sfmhip_set_stream drains the old stream before work moves to another.
    // Giving gigabytes back to the driver costs ~0.1 s that surfaces in whatever HIP call comes next (measured: the second
    // sfmhip_ba_create at C5 took 127 ms against 13 ms for the first), so freed blocks are kept and handed out again;
    // sfmhip_trim / sfmhip_destroy release them.
    struct PoolBlock { void* p; size_t bytes; bool used; };
    std::vector<PoolBlock> pool;
    size_t pool_idle_bytes = 0;
    static constexpr size_t POOL_IDLE_CAP = (size_t)48 << 30;      // idle bytes kept at most (of 288 GB)
    // "every value an integer in [0, 255]" flags of the descriptor sets, one slot each in ONE device array: the preparation
    // kernels raise them, and a batch of sets is resolved with a single copy + sync when a launch first needs to know
    static constexpr int FLAG_SLOTS = 1 << 16;
    int*   d_flagpool = nullptr;
    int    flag_next = 0;
    std::vector<int> flag_free;
    // second stream of the bundle-adjustment problems (created on first use and kept: a hipStreamCreate costs milliseconds)
    hipStream_t aux_stream = nullptr;
    int    num_cus = 256;
    // grow-only host block for the shards' arrays of sfmhip_ba_solve_multi (fresh allocations of that size cost a page fault per 4 KB: 60 ms at C5)
    void*  host_scratch = nullptr; size_t host_scratch_bytes = 0;
    unsigned* d_points_fallback = nullptr;      // points.hip: length of the last grid search's fallback list (a pool block taken on first use and kept)
    int    inject_alloc_failures = 0;      // sfmhip_debug_fail_allocations: the next N sfm_pool_get calls fail (tests of the error paths)
    // optional per-kernel timing of the matching path (sfmhip_set_kernel_timing): event triples
    // [before kNN kernel, after it, after merge / re-score] for up to TIMING_SLOTS calls since the last query
    static constexpr int TIMING_SLOTS = 64;
    bool   timing = false;
    int    timing_used = 0;
    hipEvent_t tev[TIMING_SLOTS][3] = {};
};

// Every C-ABI entry point binds the calling thread to its context's device for the duration of the call (and restores the
// caller's current device): allocations, event creation and launches then land on ctx->device whatever the caller did
// with hipSetDevice in between, and two contexts on different GPUs can live in one process.
struct SfmDeviceGuard {
    int prev = -1; bool switched = false;
    explicit SfmDeviceGuard(const sfmhip_ctx* c)
    {
        if (c && hipGetDevice(&prev) == hipSuccess && prev != c->device) switched = hipSetDevice(c->device) == hipSuccess;
    }
    ~SfmDeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    SfmDeviceGuard(const SfmDeviceGuard&) = delete;
    SfmDeviceGuard& operator=(const SfmDeviceGuard&) = delete;
};
#define SFM_DEVICE_GUARD(ctx) SfmDeviceGuard _sfm_device_guard(ctx)

// roctx ranges around the C-ABI calls (tracing): visible in `rocprofv3 --marker-trace`.  The marker library is
// looked up at run time (librocprofiler-sdk-roctx, else libroctx64); without it the ranges are no-ops, so libsfmhip.so keeps
// its single dependency on the HIP runtime.
struct SfmRoctx {
    int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
    SfmRoctx();
    static const SfmRoctx& get() { static const SfmRoctx r; return r; }
};
struct SfmRange {
    bool on;
    explicit SfmRange(const char* name) : on(SfmRoctx::get().push != nullptr) { if (on) (void)SfmRoctx::get().push(name); }
    ~SfmRange() { if (on) (void)SfmRoctx::get().pop(); }
    SfmRange(const SfmRange&) = delete;
    SfmRange& operator=(const SfmRange&) = delete;
};
#define SFM_RANGE(name) SfmRange _sfm_range(name)

#define SFM_HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);               \
            return SFMHIP_E_HIP;                                                                 \
        }                                                                                        \
    } while (0)

#define SFM_ARG_CHECK(ctx, cond)                                                                 \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            if (ctx) (ctx)->last_error = std::string("bad argument: ") + #cond;                  \
            return SFMHIP_E_ARG;                                                                 \
        }                                                                                        \
    } while (0)

static inline int sfm_pinned(sfmhip_ctx* ctx, size_t bytes, void** out)
{
    if (bytes > ctx->pinned_bytes) {
        SFM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->pinned) SFM_HIP_TRY(ctx, hipHostFree(ctx->pinned));
        ctx->pinned = nullptr; ctx->pinned_bytes = 0;
        size_t want = bytes + bytes / 4 + 4096;
        SFM_HIP_TRY(ctx, hipHostMalloc(&ctx->pinned, want, hipHostMallocDefault));
        ctx->pinned_bytes = want;
    }
    *out = ctx->pinned;
    return SFMHIP_OK;
}

// Host -> HBM copy of a caller's (pageable) array, ordered on the context's stream.  hipMemcpyAsync from pageable memory runs at
// 9-13 GB/s on the MI355X boxes (one runtime thread staging); this goes through two pinned 16 MB buffers filled by four host
// threads instead (43 GB/s, experiments/h2d_bench.hip).  The source has been consumed when the call returns.
int sfm_upload(sfmhip_ctx* ctx, void* dst, const void* src, size_t bytes);
// the same, but every pinned piece is PRODUCED on the copy threads on its way into the staging ring (a conversion, a gather of strided
// rows).  The contract of the ring, in one place (the arithmetic is in copy_pool.hpp):
//  * Pieces.  The transfer is cut, in order, into pieces [off, off + n) of stage_piece_bytes(STAGE_BYTES, granule) bytes, the last one
//    shorter: every off is a multiple of `granule`, every n but the last is, no n exceeds STAGE_BYTES.  granule 0 promises nothing
//    (pieces of STAGE_BYTES); a granule above STAGE_BYTES is refused with SFMHIP_E_ARG before anything is enqueued, whatever `bytes`.
//  * fill(piece, off, n, t, nt) writes thread t's share of the transfer's bytes [off, off + n) to piece[0 .. n).  A piece of at least
//    STAGE_PARALLEL_BYTES is filled by one call for every t of [0, nt) at once, on nt = 4 .. 16 threads (the machine decides), a
//    shorter one by the single call (t, nt) = (0, 1) on the caller's thread; the shares of a piece must cover it for every nt.  fill
//    runs only inside this call, a piece's calls have all returned before the next piece's begin, and no (off, t) comes twice.
//  * The source.  Everything fill reads has been consumed when the call returns; the copies to `dst` are then queued on ctx->stream,
//    not finished.
//  * Reuse.  The two buffers alternate, across calls too.  A buffer is refilled only after hipEventSynchronize on the event recorded
//    behind its last copy, so never before that copy has run; when the context moves to another stream, sfmhip_set_stream has drained
//    the old one first, and the events of the old stream are complete.
int sfm_upload_produced(sfmhip_ctx* ctx, void* dst, size_t bytes, size_t granule, const std::function<void(char*, size_t, size_t, int, int)>& fill);
// f(t, nt) on every copy thread of the context, the caller included
void sfm_parallel(sfmhip_ctx* ctx, const std::function<void(int, int)>& f);

// device block of at least `bytes` from the context's cache (an idle block of up to 4x the size, else a new hipMalloc); the rule of
// use is stated at sfmhip_ctx::pool
int  sfm_pool_get(sfmhip_ctx* ctx, size_t bytes, void** out);
void sfm_pool_put(sfmhip_ctx* ctx, void* p);
void sfm_pool_trim(sfmhip_ctx* ctx);
// rccl.hip: communicators cached for sets of contexts go when one of their contexts does
void sfm_rccl_forget_ctx(sfmhip_ctx* ctx);

// points.hip: K nearest other points of every point of a device cloud (n x 3 double) into d_idx (n x K int32) / d_dist (n x K double),
// either may be null; method: SFMHIP_POINTS_*.  Enqueues on the context's stream, never synchronises.  The grid leaves the number of
// queries it handed to its brute-force pass in ctx->d_points_fallback.
int sfm_points_knn_enqueue(sfmhip_ctx* ctx, const double* d_pts, int n, int K, int method, int32_t* d_idx, double* d_dist);
// points.hip: the voxel-grid down-sampling of sfmhip_voxel_downsample_dev on a device cloud of n >= 1 points (mesh.hip clusters the
// vertices of a mesh with it); d_counts / d_voxel_of may be null.  Enqueues on the context's stream, never synchronises.
int sfm_voxel_downsample_enqueue(sfmhip_ctx* ctx, const double* d_pts, int n, double voxel, double* d_centroids, int32_t* d_counts, int32_t* d_voxel_of,
                                 int32_t* d_n_voxels);
// normals.hip: plane fit on the K neighbours listed in d_idx (n x K, -1 = none), the fit of normals_kernel
int sfm_normals_from_knn_enqueue(sfmhip_ctx* ctx, const double* d_pts, const int32_t* d_idx, int n, int K, double* d_normals);
// the method SFMHIP_POINTS_AUTO stands for at n points
int sfm_points_auto_method(int n);

// device blocks of the context's cache that go back to it when the holder leaves scope (the first few are kept in the holder
// itself: a call that takes a block or two per pass allocates nothing on the heap for it)
struct SfmPoolHold {
    sfmhip_ctx* ctx; void* few[4]; int n_few = 0; std::vector<void*> more;
    explicit SfmPoolHold(sfmhip_ctx* c) : ctx(c) {}
    ~SfmPoolHold() { for (int i = 0; i < n_few; ++i) sfm_pool_put(ctx, few[i]); for (void* p : more) sfm_pool_put(ctx, p); }
    int get(size_t bytes, void** out)
    {
        const int rc = sfm_pool_get(ctx, bytes, out);
        if (rc == SFMHIP_OK) { if (n_few < 4) few[n_few++] = *out; else more.push_back(*out); }
        return rc;
    }
    template <typename T> int get(T** out, size_t count) { return get((count > 0 ? count : 1) * sizeof(T), (void**)out); }
    SfmPoolHold(const SfmPoolHold&) = delete;
    SfmPoolHold& operator=(const SfmPoolHold&) = delete;
};

// the call shape of the host entry points of points.hip, normals.hip and triangulate.hip: hold, upload, enqueue, download, finish
static inline bool points_method_ok(int method) { return method == SFMHIP_POINTS_AUTO || method == SFMHIP_POINTS_BRUTE || method == SFMHIP_POINTS_GRID; }
// a device block of `count` elements from `hold`, filled from the caller's array on the context's stream
template <typename T>
static inline int sfm_upload_async(sfmhip_ctx* ctx, SfmPoolHold& hold, const T* src, size_t count, T*& d)
{
    const int rc = hold.get(&d, count);
    if (rc != SFMHIP_OK) return rc;
    SFM_HIP_TRY(ctx, hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return SFMHIP_OK;
}
// a step failed with rc while work may be in flight: drain the stream (the blocks go back to the cache behind this call), return rc
static inline int sfm_drain(sfmhip_ctx* ctx, int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
// the end of a call, also after an error with work possibly in flight: drain the stream (the caller's host buffers may be sources or
// targets of copies), keep the first error
static inline int sfm_finish(sfmhip_ctx* ctx, hipError_t e)
{
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return SFMHIP_E_HIP; }
    return SFMHIP_OK;
}

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
static inline int ceil_div(int x, int m) { return (x + m - 1) / m; }
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// do the host ranges [a, a + na) and [b, b + nb) share a byte (a null pointer shares none): the test hooks refuse such arguments
static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    return a && b && (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}

// one pool block carved into areas that start at multiples of 256 bytes: carve(n) is the offset of the next area of n bytes, and
// carve.bytes the size of the block that holds the areas handed out so far
struct SfmCarve {
    size_t bytes = 0;
    size_t operator()(size_t n) { const size_t at = bytes; bytes += align256(n); return at; }
};

// descriptor set (one image), see match.hip
struct sfmhip_descset {
    sfmhip_ctx* ctx = nullptr;
    int kind = 0;
    int rows = 0, rows_pad = 0;      // rows_pad: multiple of 128
    int dim = 0;                      // L2: elements; Hamming: bytes
    // L2
    const float* d_f32 = nullptr; size_t ld = 0; bool owns_f32 = false;
    int dim_pad = 0;                  // multiple of 32 (int8 copy row length in bytes)
    int8_t* d_i8 = nullptr;           // rows_pad x dim_pad, value - 128; pad rows zero
    int32_t* d_norm = nullptr;        // 2 x rows_pad: [sum b^2 | sum b^2 + 2 sum b], b = value - 128; pad rows = PAD_NORM
    int exact_u8 = 0;                 // every value an integer in [0,255] and dim <= 128 (valid once !exact_pending)
    bool exact_pending = false;       // the preparation kernel's verdict is still in d_flag (descsets_resolve reads it)
    int flag_slot = -1;               // d_flag = ctx->d_flagpool + flag_slot; -1: a block of its own
    // Hamming2
    uint32_t* d_u32 = nullptr;        // rows_pad x 16 words (64 B rows, zero padded)
    uint32_t* d_f4 = nullptr;         // rows_pad x 96 words: 768 FP4 values per row (prep_hamming_fp4_kernel), nbytes <= 61 only
    int* d_flag = nullptr;
};
