// sortscan.hpp -- the library's two device primitives, sortscan.hip: a stable LSD radix sort of (64-bit key, 32-bit value) pairs and an
// in-place exclusive prefix sum of 32-bit counters, with the workspaces they need.  Everything here enqueues on the stream it is given
// and never synchronises; a workspace is either carved from one block of the cache (constructor or carve, then bind to the block) or,
// for the sort, made of areas the caller already owns (of); the scan of such areas is sfm_enqueue_scan itself.
//
// What the code does, which is not always what a caller would assume:
//   * the sort moves 8 bits per pass and always makes at least one pass, so it orders by the low 8 * max(1, ceil(bits / 8)) bits of the
//     keys, not by the low `bits` bits: key bits between `bits` and the next multiple of 8 take part.  Bits above that are carried along
//     untouched.  Equal keys keep their order.  bits > 64 is not allowed.
//   * the prefix sums are modulo 2^32.
//   * *total64 is exact only while every tile of 4096 counters, and every group of 256 consecutive tile totals, sums below 2^32:
//     sfm_scan_top_kernel adds 32-bit partial sums before its 64-bit carry.  A caller whose counters may go beyond that counts for itself
//     (ba.hip: setup_pair_count_kernel).
#pragma once
#include "common.hpp"

// exclusive prefix sum, in place, of the n counters at data (bsum: SfmScan::bsum_words(n) counters of scratch); *total64 (device, may be
// null) = their sum, 0 at n == 0
void sfm_enqueue_scan(hipStream_t st, unsigned* data, size_t n, unsigned* bsum, unsigned long long* total64 = nullptr);

// n counters and the tile sums of their scan.  Scanning a list's n flags or counts as n + 1 counters, the last one zero, leaves the total
// behind the prefixes: that is how every list of the library is numbered and compacted.
struct SfmScan {
    unsigned *data = nullptr, *bsum = nullptr;
    size_t o_data = 0, o_bsum = 0;
    static size_t bsum_words(size_t n);
    SfmScan() {}
    SfmScan(SfmCarve& c, size_t n) { carve(c, n); }
    void carve(SfmCarve& c, size_t n) { o_data = c(n * 4); o_bsum = c(bsum_words(n) * 4); }
    void bind(char* w) { data = (unsigned*)(w + o_data); bsum = (unsigned*)(w + o_bsum); }
    void scan(hipStream_t st, size_t n, unsigned long long* total64 = nullptr) const { sfm_enqueue_scan(st, data, n, bsum, total64); }
};

// the six areas of a sort of n pairs: keys and values on two sides, the digit counters of every tile and the tile sums of their scan
struct SfmSort {
    unsigned long long* k[2] = { nullptr, nullptr };
    unsigned* v[2] = { nullptr, nullptr };
    unsigned *hist = nullptr, *bsum = nullptr;
    size_t o_k[2] = { 0, 0 }, o_v[2] = { 0, 0 }, o_hist = 0, o_bsum = 0;      // offsets in the block: of use between carve and bind only
    static size_t hist_words(size_t n);
    static size_t bsum_words(size_t n);
    SfmSort() {}
    SfmSort(SfmCarve& c, size_t n) { carve(c, n); }
    void carve(SfmCarve& c, size_t n)
    {
        for (int i = 0; i < 2; ++i) { o_k[i] = c(n * 8); o_v[i] = c(n * 4); }
        o_hist = c(hist_words(n) * 4); o_bsum = c(bsum_words(n) * 4);
    }
    void bind(char* w)
    {
        for (int i = 0; i < 2; ++i) { k[i] = (unsigned long long*)(w + o_k[i]); v[i] = (unsigned*)(w + o_v[i]); }
        hist = (unsigned*)(w + o_hist); bsum = (unsigned*)(w + o_bsum);
    }
    static SfmSort of(unsigned long long* k0, unsigned long long* k1, unsigned* v0, unsigned* v1, unsigned* hist, unsigned* bsum)
    {
        SfmSort S; S.k[0] = k0; S.k[1] = k1; S.v[0] = v0; S.v[1] = v1; S.hist = hist; S.bsum = bsum; return S;
    }
    // The keys are in k[cur], the values in v[cur] (or they are the element index, where identity_vals).  Returns the side that holds
    // the sorted keys and their values; the other side is scratch afterwards.  n == 0: nothing is enqueued, the side is cur.
    int sort(hipStream_t st, size_t n, int cur, int bits, bool identity_vals) const;
};

// run heads of sorted keys, n + 1 entries: flag[i] = i < n && keys[i] < limit && (i == 0 || keys[i - 1] != keys[i]).  `limit` is the
// caller's "none" (~0ull: every key counts but all-ones); the scan of the n + 1 flags numbers the runs and leaves their count in flag[n].
void sfm_enqueue_run_heads(hipStream_t st, const unsigned long long* keys, size_t n, unsigned long long limit, unsigned* flag);
