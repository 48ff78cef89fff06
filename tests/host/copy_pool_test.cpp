// copy_pool_test.cpp -- csrc/copy_pool.hpp by itself on the CPU: the plan of a transfer's pieces, a copy thread's share of a piece's
// rows, and the thread pool.  Every expectation comes from a plain loop written here, never from the header.
// Built twice (Makefile): plain, and with -fsanitize=thread, where the pool part also has the workers and the caller exchange
// ordinary (non-atomic) memory, so that a missing happens-before edge of CopyPool::run is a ThreadSanitizer report.
//
//   usage: copy_pool_test [plan | shares | pool | count BYTES GRANULE]      no argument: all three; exit code 1 on a mismatch
#include "../../sfm_opencv_amd/csrc/copy_pool.hpp"

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

static const size_t Ki = 1024, Mi = 1024 * 1024, STAGE = 16 * Mi;
static int failures = 0;

#define EXPECT(cond, ...)                                                                        \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            if (++failures <= 20) { printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                        \
    } while (0)

// ------------------------------------------------------------------------------------------------
// piece plan
// ------------------------------------------------------------------------------------------------
struct Piece { size_t off, n; };

static std::vector<Piece> plan_of(size_t bytes, size_t granule)
{
    std::vector<Piece> p;
    const int rc = stage_for_each_piece(bytes, STAGE, granule, [&](size_t off, size_t n) { p.push_back({ off, n }); return 0; });
    EXPECT(rc == 0, "rc %d", rc);
    return p;
}

static void test_plan()
{
    const size_t sizes[] = { 0, 1, 63, 64, 65, 256 * Ki - 1, 256 * Ki, 256 * Ki + 1, 16 * Mi - 1, 16 * Mi, 16 * Mi + 1, 32 * Mi, 32 * Mi + 1, 48 * Mi + 5 };
    const size_t granules[] = { 1, 61, 64, 128, 512, 16 * Mi };
    int combos = 0;
    for (size_t bytes : sizes)
        for (size_t g : granules) {
            const std::vector<Piece> p = plan_of(bytes, g);
            size_t at = 0;
            for (size_t i = 0; i < p.size(); ++i) {
                const bool last = i + 1 == p.size();
                EXPECT(p[i].off == at, "bytes %zu granule %zu piece %zu: off %zu, expected %zu (contiguous)", bytes, g, i, p[i].off, at);
                EXPECT(p[i].n > 0 && p[i].n <= STAGE, "bytes %zu granule %zu piece %zu: n %zu", bytes, g, i, p[i].n);
                EXPECT(p[i].off % g == 0, "bytes %zu granule %zu piece %zu: off %zu is no multiple", bytes, g, i, p[i].off);
                if (!last) EXPECT(p[i].n % g == 0, "bytes %zu granule %zu piece %zu: n %zu is no multiple", bytes, g, i, p[i].n);
                // a piece that is not the last is as long as the buffer allows: one granule more would not fit
                if (!last) EXPECT(p[i].n + g > STAGE, "bytes %zu granule %zu piece %zu: n %zu is shorter than it could be", bytes, g, i, p[i].n);
                at += p[i].n;
            }
            EXPECT(at == bytes, "bytes %zu granule %zu: the pieces cover %zu", bytes, g, at);
            EXPECT((bytes == 0) == p.empty(), "bytes %zu granule %zu: %zu pieces", bytes, g, p.size());
            ++combos;
        }
    // an early non-zero result of the piece callback ends the loop and is returned
    int calls = 0;
    const int rc = stage_for_each_piece(48 * Mi, STAGE, 64, [&](size_t, size_t) { return ++calls == 2 ? -7 : 0; });
    EXPECT(rc == -7 && calls == 2, "rc %d after %d calls", rc, calls);
    // granule 0 promises nothing: pieces of the whole buffer
    const std::vector<Piece> p0 = plan_of(32 * Mi + 1, 0);
    EXPECT(p0.size() == 3 && p0[0].n == STAGE && p0[1].off == STAGE && p0[2].off == 2 * STAGE && p0[2].n == 1, "granule 0: %zu pieces", p0.size());
    printf("plan: %d combinations\n", combos);
}

// ------------------------------------------------------------------------------------------------
// row shares
// ------------------------------------------------------------------------------------------------
struct Expect { int img; long long k; };

// rows per image: random, with images of no rows at the start, in the middle, at the end and several in a row
static std::vector<long long> random_first(std::mt19937_64& rng, int n_img, long long want_rows, int zero_pattern)
{
    std::vector<long long> rows((size_t)n_img, 0);
    std::vector<int> live;
    for (int i = 0; i < n_img; ++i) {
        bool zero = false;
        if (zero_pattern & 1) zero |= i == 0;                                   // at the start
        if (zero_pattern & 2) zero |= i == n_img - 1;                           // at the end
        if (zero_pattern & 4) zero |= i >= n_img / 2 && i < n_img / 2 + 3;      // several in a row in the middle
        if (zero_pattern & 8) zero |= rng() % 4 == 0;                           // scattered
        if (!zero) live.push_back(i);
    }
    if (live.empty()) live.push_back(n_img / 2);
    // every live image gets one row (images of one row matter), the rest lands at random, so some images are long and most short
    for (int i : live) rows[i] = 1;
    long long left = want_rows - (long long)live.size();
    while (left > 0) {
        const long long chunk = std::min<long long>(left, 1 + (long long)(rng() % (size_t)(1 + want_rows / 3)));
        rows[live[rng() % live.size()]] += chunk; left -= chunk;
    }
    std::vector<long long> first((size_t)n_img + 1, 0);
    for (int i = 0; i < n_img; ++i) first[i + 1] = first[i] + rows[i];
    return first;
}

static void test_shares_one(std::mt19937_64& rng, const std::vector<long long>& first, size_t w, long long g0, long long cnt, bool with_ld, long long* checked)
{
    const int n_img = (int)first.size() - 1;
    const long long total = first[n_img];
    // the sources: image i with row stride ld[i] >= w, every byte of a row a function of (image, row, column), the gaps 0xA5
    std::vector<size_t> ld((size_t)n_img);
    std::vector<std::vector<uint8_t>> src((size_t)n_img);
    auto value = [](int img, long long k, size_t c) { return (uint8_t)(1 + (img * 131 + k * 31 + (long long)c * 7) % 199); };      // (0xA5 is mapped away below)
    for (int i = 0; i < n_img; ++i) {
        ld[i] = with_ld ? w + (size_t)(rng() % 9) : w;
        const long long r = first[i + 1] - first[i];
        src[i].assign((size_t)std::max<long long>(r, 1) * ld[i], 0xA5);
        for (long long k = 0; k < r; ++k)
            for (size_t c = 0; c < w; ++c) { uint8_t v = value(i, k, c); if (v == 0xA5) v = 0xA6; src[i][(size_t)k * ld[i] + c] = v; }
    }
    // the reference: a plain double loop over images and their rows
    std::vector<Expect> expect((size_t)total);
    const size_t GUARD = 256;
    std::vector<uint8_t> want(GUARD + (size_t)cnt * w + GUARD, 0x5C);
    for (int i = 0; i < n_img; ++i)
        for (long long k = 0; k < first[i + 1] - first[i]; ++k) {
            const long long r = first[i] + k;
            expect[(size_t)r] = { i, k };
            if (r >= g0 && r < g0 + cnt) memcpy(&want[GUARD + (size_t)(r - g0) * w], &src[i][(size_t)k * ld[i]], w);
        }
    const size_t off = (size_t)g0 * w, nb = (size_t)cnt * w;
    for (int nt = 1; nt <= 16; ++nt) {
        std::vector<int> visits((size_t)total, 0);
        std::vector<uint8_t> got(want.size(), 0x5C);
        uint8_t* piece = got.data() + GUARD;
        for (int t = 0; t < nt; ++t)
            stage_share_runs(first, w, off, nb, t, nt, [&](int img, long long row, long long run, size_t at) {
                EXPECT(run > 0, "w %zu nt %d t %d: a run of %lld rows", w, nt, t, run);
                EXPECT(img >= 0 && img < n_img, "w %zu nt %d t %d: image %d of %d", w, nt, t, img, n_img);
                EXPECT(at % w == 0 && at + (size_t)run * w <= nb, "w %zu nt %d t %d: bytes [%zu, %zu) of a piece of %zu", w, nt, t, at, at + (size_t)run * w, nb);
                if (img < 0 || img >= n_img || run <= 0 || at % w || at + (size_t)run * w > nb) return;
                for (long long j = 0; j < run; ++j) {
                    const long long r = g0 + (long long)(at / w) + j;          // the row of the transfer these destination bytes belong to
                    ++visits[(size_t)r];
                    EXPECT(expect[(size_t)r].img == img, "w %zu nt %d t %d row %lld: under image %d, expected %d", w, nt, t, r, img, expect[(size_t)r].img);
                    EXPECT(expect[(size_t)r].k == row + j, "w %zu nt %d t %d row %lld: source row %lld, expected %lld", w, nt, t, r, row + j, expect[(size_t)r].k);
                    if (row + j < 0 || row + j >= first[img + 1] - first[img]) continue;          // (reported above: keep the copy in bounds)
                    memcpy(piece + at + (size_t)j * w, &src[img][(size_t)(row + j) * ld[img]], w);      // what the visitors of match.hip do
                }
                // thread t's share is [cnt * t / nt, cnt * (t + 1) / nt) of the piece's rows
                const long long a = (long long)(at / w), lo = cnt * t / nt, hi = cnt * (t + 1) / nt;
                EXPECT(a >= lo && a + run <= hi, "w %zu nt %d t %d: rows [%lld, %lld) outside the share [%lld, %lld)", w, nt, t, a, a + run, lo, hi);
            });
        for (long long r = 0; r < total; ++r) {
            const int e = r >= g0 && r < g0 + cnt ? 1 : 0;
            EXPECT(visits[(size_t)r] == e, "w %zu nt %d piece [%lld, %lld) row %lld: visited %d times", w, nt, g0, g0 + cnt, r, visits[(size_t)r]);
        }
        EXPECT(got == want, "w %zu nt %d piece [%lld, %lld) ld %d: the bytes differ (or a guard byte changed)", w, nt, g0, g0 + cnt, (int)with_ld);
        ++*checked;
    }
}

static void test_shares()
{
    std::mt19937_64 rng(20240607);
    const size_t widths[] = { 1, 32, 61, 64, 128 };
    const long long piece_rows[] = { 1, 2, 15, 16, 17, 3001, 4096 };
    long long checked = 0;
    for (size_t w : widths)
        for (long long cnt : piece_rows)
            for (int table = 0; table < 8; ++table) {
                const int n_img = table == 0 ? 1 : table == 1 ? 40 : 1 + (int)(rng() % 40);
                const int zeros = table < 2 ? table * 15 : (int)(rng() % 16);
                // the piece lies somewhere inside the transfer: rows before it and behind it that must stay untouched
                const long long before = table % 3 == 0 ? 0 : (long long)(rng() % 50), behind = table % 3 == 1 ? 0 : (long long)(rng() % 50);
                const std::vector<long long> first = random_first(rng, n_img, before + cnt + behind, zeros);
                const long long total = first.back();
                const long long g0 = std::min(before, total - cnt);
                test_shares_one(rng, first, w, g0, cnt, false, &checked);
                test_shares_one(rng, first, w, g0, cnt, true, &checked);
            }
    // the edges by hand: a piece that starts exactly at an image boundary behind images of no rows, and one that ends at one
    {
        const std::vector<long long> first = { 0, 0, 0, 5, 5, 5, 9, 9 };
        test_shares_one(rng, first, 61, 5, 4, true, &checked);
        test_shares_one(rng, first, 61, 0, 5, true, &checked);
        test_shares_one(rng, first, 61, 0, 9, false, &checked);
        test_shares_one(rng, first, 61, 4, 2, true, &checked);
    }
    printf("shares: %lld (table, piece, nt) cases\n", checked);
}

// ------------------------------------------------------------------------------------------------
// CopyPool
// ------------------------------------------------------------------------------------------------
static void spin(unsigned n)
{
    volatile unsigned x = 0;
    for (unsigned i = 0; i < n; ++i) x = x + i;
}

static void test_pool_jobs(int NT, int jobs)
{
    CopyPool pool(NT);
    EXPECT(pool.NT == NT, "NT %d", pool.NT);
    std::vector<std::atomic<int>> seen((size_t)NT);
    std::atomic<int> finished_prev{NT}, finished_now{0}, bad_t{0}, early{0};
    // ordinary memory both ways: the caller writes `token` before run, every worker reads it and writes its slot, the caller reads the
    // slots after run -- data races unless run() orders them
    std::vector<unsigned long long> slot((size_t)NT, 0);
    unsigned long long token = 0;
    for (int j = 0; j < jobs; ++j) {
        for (auto& s : seen) s.store(0);
        finished_now.store(0);
        token = 0x9e3779b97f4a7c15ull * (unsigned long long)(j + 1);
        const std::function<void(int, int)> f = [&](int t, int nt) {
            if (finished_prev.load() != NT) early.fetch_add(1);          // the job before has not ended on every thread
            if (nt != NT || t < 0 || t >= NT) { bad_t.fetch_add(1); return; }
            seen[(size_t)t].fetch_add(1);
            spin((unsigned)((token >> (t % 16)) % 4000) * (t % 3 == 0 ? 3 : 1));          // uneven, and different from job to job
            slot[(size_t)t] = token + (unsigned long long)t;
            finished_now.fetch_add(1);
        };
        pool.run(f);
        EXPECT(finished_now.load() == NT, "NT %d job %d: run returned with %d of %d shares done", NT, j, finished_now.load(), NT);
        for (int t = 0; t < NT; ++t) {
            EXPECT(seen[(size_t)t].load() == 1, "NT %d job %d: t = %d ran %d times", NT, j, t, seen[(size_t)t].load());
            EXPECT(slot[(size_t)t] == token + (unsigned long long)t, "NT %d job %d: slot %d holds another job's value", NT, j, t);
        }
        finished_prev.store(finished_now.load());
    }
    EXPECT(bad_t.load() == 0, "NT %d: %d calls with t outside [0, NT) or another nt", NT, bad_t.load());
    EXPECT(early.load() == 0, "NT %d: %d shares began before the job in front had ended", NT, early.load());
}

static void test_pool()
{
    const int picked = CopyPool::pick_threads();
    EXPECT(picked >= 4 && picked <= 16, "pick_threads() = %d", picked);
    test_pool_jobs(4, 3000);
    test_pool_jobs(16, 3000);
    // construct and destroy: with no job, with one, with a few; the default thread count among them
    for (int i = 0; i < 100; ++i) {
        if (i % 10 == 9) { CopyPool pool; EXPECT(pool.NT == picked, "default NT %d", pool.NT); continue; }
        const int NT = i % 2 ? 16 : 4;
        CopyPool pool(NT);
        std::atomic<int> calls{0};
        const std::function<void(int, int)> f = [&](int, int) { calls.fetch_add(1); };
        for (int j = 0; j < i % 3; ++j) pool.run(f);
        EXPECT(calls.load() == NT * (i % 3), "NT %d: %d calls in %d jobs", NT, calls.load(), i % 3);
    }
    printf("pool: 2 x 3000 jobs, 100 lifetimes\n");
}

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "all";
    if (what == "count" && argc == 4) {          // the number of pieces of one transfer, for whoever wants to compare
        int n = 0;
        stage_for_each_piece((size_t)strtoull(argv[2], nullptr, 10), STAGE, (size_t)strtoull(argv[3], nullptr, 10), [&](size_t, size_t) { ++n; return 0; });
        printf("%d\n", n);
        return 0;
    }
    if (what != "all" && what != "plan" && what != "shares" && what != "pool") { fprintf(stderr, "usage: copy_pool_test [plan | shares | pool | count BYTES GRANULE]\n"); return 2; }
    if (what == "all" || what == "plan") test_plan();
    if (what == "all" || what == "shares") test_shares();
    if (what == "all" || what == "pool") test_pool();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("copy_pool_test: all checks passed\n");
    return 0;
}
