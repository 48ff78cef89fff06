// copy_pool.hpp -- the host side of the pinned staging ring (sfm_upload / sfm_upload_produced of context.hip, stage_host_images of
// match.hip) that needs no HIP: the copy threads, the plan of a transfer's pieces and a thread's share of a piece's rows.
// tests/host/copy_pool_test.cpp compiles this header by itself.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include <sched.h>

// Helper threads of sfm_upload / sfm_upload_produced: they sleep on a condition variable and each runs its share of the current job.
// As many as the cores this process may use, between 4 and 16 (the caller is one of them): a memcpy into the staging ring reaches
// 43 GB/s with four, and a float -> byte conversion on the way in is bound by the DRAM read rate of as many as there are.
// (The thread count is an argument only for the host test, which has to see 4 and 16 on whatever machine it runs.)
struct CopyPool {
    int NT;
    std::vector<std::thread> th;
    std::mutex mu; std::condition_variable cv_go, cv_done;
    unsigned long long gen = 0; int pending = 0; bool quit = false;
    const std::function<void(int, int)>* job = nullptr;
    static int pick_threads()
    {
        int cores = (int)std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) cores = CPU_COUNT(&set);
        return std::min(16, std::max(4, cores));
    }
    explicit CopyPool(int nt = pick_threads()) : NT(nt)
    {
        for (int t = 1; t < NT; ++t)
            th.emplace_back([this, t] {
                unsigned long long seen = 0;
                for (;;) {
                    std::unique_lock<std::mutex> lk(mu);
                    cv_go.wait(lk, [&] { return quit || gen != seen; });
                    if (quit) return;
                    seen = gen;
                    const std::function<void(int, int)>* f = job;
                    lk.unlock();
                    (*f)(t, NT);
                    lk.lock();
                    if (--pending == 0) cv_done.notify_one();
                }
            });
    }
    ~CopyPool()
    {
        { std::lock_guard<std::mutex> lk(mu); quit = true; }
        cv_go.notify_all();
        for (auto& t : th) t.join();
    }
    void run(const std::function<void(int, int)>& f)
    {
        { std::lock_guard<std::mutex> lk(mu); job = &f; pending = NT - 1; ++gen; }
        cv_go.notify_all();
        f(0, NT);
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
    }
};

// a piece at least this long is filled by all copy threads, a shorter one by the caller alone
static constexpr size_t STAGE_PARALLEL_BYTES = (size_t)256 << 10;

// bytes of every piece but the last of a transfer through staging buffers of stage_bytes whose pieces are multiples of `granule`
// (0: no such promise; a granule above stage_bytes cannot be kept, sfm_upload_produced refuses it)
static inline size_t stage_piece_bytes(size_t stage_bytes, size_t granule)
{
    return granule > 0 && granule <= stage_bytes ? stage_bytes / granule * granule : stage_bytes;
}

// the pieces of a transfer of `bytes` in order: piece(off, n) for [off, off + n), until one returns non-zero (which is returned)
template <class Piece>
static inline int stage_for_each_piece(size_t bytes, size_t stage_bytes, size_t granule, const Piece& piece)
{
    const size_t CH = stage_piece_bytes(stage_bytes, granule);
    for (size_t off = 0; off < bytes; off += CH) {
        const size_t n = std::min(CH, bytes - off);
        const int rc = piece(off, n);
        if (rc) return rc;
    }
    return 0;
}

// Thread t of nt's share of the piece [off, off + nb) of a transfer of rows of w bytes, the rows of image i being first[i] ..
// first[i + 1] - 1 of the transfer (first: one entry more than images, ascending; an image may have no rows): rows
// [cnt * t / nt, cnt * (t + 1) / nt) of the piece's cnt = nb / w, as runs inside one image each.
// visit(image, first row of the run within the image, rows in the run, byte offset of the run in the piece).
template <class Visit>
static inline void stage_share_runs(const std::vector<long long>& first, size_t w, size_t off, size_t nb, int t, int nt, const Visit& visit)
{
    const long long g0 = (long long)(off / w), cnt = (long long)(nb / w);
    long long r = g0 + cnt * t / nt;
    const long long re = g0 + cnt * (t + 1) / nt;
    int img = (int)(std::upper_bound(first.begin(), first.end(), r) - first.begin()) - 1;
    while (r < re) {
        while (r >= first[img + 1]) ++img;
        const long long run = std::min(re, first[img + 1]) - r;          // rows of this image in the share
        visit(img, r - first[img], run, (size_t)(r - g0) * w);
        r += run;
    }
}
