// Stand-alone check of csrc/lds_limit.h (no HIP, no GPU): the memo behind edgl_lds_limit with a counting fake in place of
// hipFuncSetAttribute.  Built and run by tests/test_cpu_lds_limit.py under ThreadSanitizer and under Address/UB-Sanitizer.
// Exit status 0 and "ok" on stdout, or the failed checks on stderr and exit status 1.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "lds_limit.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                          \
        }                                                                        \
    } while (0)

constexpr size_t THR = 1000;      // the test's own threshold, not the library's 48 KB
char g_kern[4];                   // four "kernels": only their addresses matter

struct FakeSetter {
    int calls = 0;
    const void* last_kern = nullptr;
    size_t last_bytes = 0;
    int fail_next = 0;
    int operator()(const void* k, size_t b) {
        ++calls;
        last_kern = k;
        last_bytes = b;
        if (fail_next > 0) { --fail_next; return 7; }
        return 0;
    }
};

void single_thread_cases() {
    LdsLimitMemo memo(THR);
    FakeSetter set;
    const void* k0 = &g_kern[0];
    const void* k1 = &g_kern[1];
    // at or below the threshold: never set
    CHECK(memo.ensure(k0, 0, 0, set) == 0);
    CHECK(memo.ensure(k0, 0, THR - 1, set) == 0);
    CHECK(memo.ensure(k0, 0, THR, set) == 0);
    CHECK(memo.ensure(k0, -1, THR, set) == 0);
    CHECK(set.calls == 0);
    // first request above it: one call
    CHECK(memo.ensure(k0, 0, 5000, set) == 0);
    CHECK(set.calls == 1 && set.last_kern == k0 && set.last_bytes == 5000);
    // the same or a smaller request: no call
    CHECK(memo.ensure(k0, 0, 5000, set) == 0);
    CHECK(memo.ensure(k0, 0, 2000, set) == 0);
    CHECK(memo.ensure(k0, 0, THR, set) == 0);
    CHECK(set.calls == 1);
    // a larger one: one more call with the larger value
    CHECK(memo.ensure(k0, 0, 9000, set) == 0);
    CHECK(set.calls == 2 && set.last_bytes == 9000);
    CHECK(memo.ensure(k0, 0, 5000, set) == 0);
    CHECK(set.calls == 2);
    // the same kernel on a second ordinal: its own call; another kernel on the first ordinal too
    CHECK(memo.ensure(k0, 1, 5000, set) == 0);
    CHECK(set.calls == 3 && set.last_kern == k0 && set.last_bytes == 5000);
    CHECK(memo.ensure(k0, 1, 5000, set) == 0);
    CHECK(set.calls == 3);
    CHECK(memo.ensure(k1, 0, 5000, set) == 0);
    CHECK(set.calls == 4 && set.last_kern == k1);
    // ordinal 70: remembered like any other
    CHECK(memo.ensure(k0, 70, 5000, set) == 0);
    CHECK(memo.ensure(k0, 70, 5000, set) == 0);
    CHECK(memo.ensure(k0, 70, 4000, set) == 0);
    CHECK(set.calls == 5);
    CHECK(memo.ensure(k0, 0, 9000, set) == 0);      // (... and it did not alias ordinal 0)
    CHECK(set.calls == 5);
    // unknown ordinal: a call every time, nothing remembered
    CHECK(memo.ensure(k0, -1, 5000, set) == 0);
    CHECK(memo.ensure(k0, -1, 5000, set) == 0);
    CHECK(memo.ensure(k0, -1, 3000, set) == 0);
    CHECK(set.calls == 8 && set.last_bytes == 3000);
    // a failing setter: the error comes back, nothing is recorded, the next request calls again and succeeds
    set.fail_next = 1;
    CHECK(memo.ensure(k1, 2, 6000, set) == 7);
    CHECK(set.calls == 9);
    CHECK(memo.ensure(k1, 2, 6000, set) == 0);
    CHECK(set.calls == 10);
    CHECK(memo.ensure(k1, 2, 6000, set) == 0);
    CHECK(set.calls == 10);
    set.fail_next = 1;                               // a failed raise keeps what was granted before
    CHECK(memo.ensure(k1, 2, 8000, set) == 7);
    CHECK(memo.ensure(k1, 2, 6000, set) == 0);
    CHECK(set.calls == 11);
    CHECK(memo.ensure(k1, 2, 8000, set) == 0);
    CHECK(set.calls == 12 && set.last_bytes == 8000);
    set.fail_next = 1;
    CHECK(memo.ensure(k0, -1, 5000, set) == 7);
    // the library's threshold is the default
    LdsLimitMemo dflt;
    FakeSetter set2;
    CHECK(EDGL_LDS_DEFAULT_LIMIT == 48 * 1024);
    CHECK(dflt.ensure(k0, 0, 48 * 1024, set2) == 0 && set2.calls == 0);
    CHECK(dflt.ensure(k0, 0, 48 * 1024 + 1, set2) == 0 && set2.calls == 1);
}

// 8 threads x 10 000 requests over 4 kernels x 3 devices, sizes growing along each thread's sequence: every thread asks every
// (kernel, device) for the same values THR + 64 * (1 .. NVAL) in increasing order.
void threaded_case() {
    constexpr int NTHREAD = 8, NREQ = 10000, NK = 4, ND = 3, NPAIR = NK * ND;
    constexpr int NVAL = (NREQ + NPAIR - 1) / NPAIR;      // distinct values a pair can be asked for
    LdsLimitMemo memo(THR);
    std::atomic<long> calls[NPAIR];
    std::atomic<size_t> granted[NPAIR];
    std::atomic<int> not_increasing{0}, errors{0};
    for (int i = 0; i < NPAIR; ++i) { calls[i] = 0; granted[i] = 0; }
    auto worker = [&] {
        for (int j = 0; j < NREQ; ++j) {
            const int pair = j % NPAIR, k = pair % NK, d = pair / NK;
            const size_t bytes = THR + 64 * (size_t)(j / NPAIR + 1);
            const int rc = memo.ensure(&g_kern[k], d, bytes, [&, pair](const void* kern, size_t b) {
                if (kern != &g_kern[pair % NK]) ++errors;
                ++calls[pair];
                if (granted[pair].exchange(b) >= b) ++not_increasing;      // a call must raise the limit
                return 0;
            });
            if (rc != 0) ++errors;
        }
    };
    std::vector<std::thread> threads;
    for (int t = 0; t < NTHREAD; ++t) threads.emplace_back(worker);
    for (auto& t : threads) t.join();
    CHECK(errors == 0);
    CHECK(not_increasing == 0);
    long total = 0, bound = 0;
    FakeSetter set;
    for (int pair = 0; pair < NPAIR; ++pair) {
        const int nval = (NREQ - pair + NPAIR - 1) / NPAIR;      // requests j = pair, pair + NPAIR, ... < NREQ
        const size_t top = THR + 64 * (size_t)nval;
        CHECK(nval <= NVAL);
        CHECK(granted[pair] == top);                              // every pair ends at its maximum ...
        CHECK(calls[pair] >= 1 && calls[pair] <= nval);
        total += calls[pair];
        bound += nval;
        CHECK(memo.ensure(&g_kern[pair % NK], pair / NK, top, set) == 0);      // ... and the memo knows it
    }
    CHECK(set.calls == 0);
    CHECK(total <= bound);
    CHECK(memo.ensure(&g_kern[0], 0, THR + 64 * (size_t)(NVAL + 1), set) == 0);
    CHECK(set.calls == 1);
}

}  // namespace

int main() {
    single_thread_cases();
    threaded_case();
    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::puts("ok");
    return 0;
}
