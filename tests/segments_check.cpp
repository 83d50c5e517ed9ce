// segments_check.cpp -- csrc/segments.h compiled for the host (tests/test_ordering.py): segment_of against a linear scan, in its
// pointer and its callable form, with 32- and 64-bit indices (signed and unsigned), over sets with one segment, with empty
// segments at the start, at the end and three in a row; every element is searched, so the elements equal to an offset and the
// last element are among them.  The two forwards are held to the same scan: frame_of_point (scan_points.h) in both offset
// dialects, and tg_owner (track_graph_device.h), whose n is the LAST index, not the count.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../global-lvba_amd/csrc/segments.h"
#include "../global-lvba_amd/csrc/scan_points.h"
#include "../global-lvba_amd/csrc/track_graph_device.h"

using namespace lvba;

static int fails = 0;
#define CHECK(cond, ...)                                                                                                    \
    do {                                                                                                                    \
        if (!(cond)) {                                                                                                      \
            if (++fails <= 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                                   \
    } while (0)

struct Job { int64_t pad, first; };

// the segment that holds element i, by walking all of them; -1: none
static int linear(const std::vector<int64_t> &off, int64_t i)
{
    int want = -1;
    for (int s = 0; s + 1 < (int)off.size(); ++s)
        if (off[s] <= i && i < off[s + 1]) want = s;
    return want;
}

static void check_set(const std::vector<int> &count, int64_t first)
{
    const int n = (int)count.size();
    std::vector<int64_t> off(n + 1), rel(n + 1);
    std::vector<uint32_t> off32(n + 1);
    std::vector<Job> jobs(n);
    off[0] = first;
    for (int s = 0; s < n; ++s) off[s + 1] = off[s] + count[s];
    for (int s = 0; s <= n; ++s) { rel[s] = off[s] - first; off32[s] = (uint32_t)rel[s]; }
    for (int s = 0; s < n; ++s) jobs[s] = Job{-1, rel[s]};
    const Job *jp = jobs.data();
    const int64_t *op = off.data();
    int seen = 0;
    for (int64_t i = 0; i < rel[n]; ++i) {
        const int want = linear(rel, i);
        CHECK(want >= 0 && count[want] > 0, "n=%d i=%lld: the linear scan finds no segment", n, (long long)i);
        seen += (i == rel[want]) + (i == rel[n] - 1);
        const int p32 = segment_of(rel.data(), n, i);
        const int64_t p64 = segment_of(rel.data(), (int64_t)n, i);
        const uint32_t pu = segment_of(off32.data(), (uint32_t)n, (uint32_t)i);
        const int c32 = segment_of([=](int s) { return jp[s].first; }, n, i);
        const int64_t c64 = segment_of([=](int64_t s) { return op[s] - first; }, (int64_t)n, i);
        CHECK(p32 == want && p64 == want && (int)pu == want && c32 == want && c64 == want,
              "n=%d first=%lld i=%lld: pointer %d / %lld / %u, callable %d / %lld, linear scan %d", n, (long long)first, (long long)i, p32,
              (long long)p64, pu, c32, (long long)c64, want);
        const int f = frame_of_point(off.data(), n, i);                    // a slice: off[0] = first
        CHECK(f == want, "frames=%d first=%lld i=%lld: frame %d, linear scan %d", n, (long long)first, (long long)i, f, want);
        if (first == 0) {
            const int64_t t = tg_owner(off.data(), n - 1, i);
            CHECK(t == want, "n=%d i=%lld: tg_owner %lld, linear scan %d", n, (long long)i, (long long)t, want);
        }
    }
    CHECK(rel[n] == 0 || seen >= 2, "n=%d: no element equal to an offset or no last element was searched", n);
}

int main()
{
    for (const int64_t first : {(int64_t)0, (int64_t)1000}) {
        check_set({0, 1, 0, 0, 65, 3, 0}, first);   // empty at both ends and two in a row
        check_set({0, 1, 0, 0, 65, 40, 0}, first);
        check_set({5}, first);                      // n = 1
        check_set({1}, first);
        check_set({0, 0, 4}, first);
        check_set({4, 0, 0}, first);
        check_set({0, 0, 0, 2}, first);             // three in a row at the start,
        check_set({3, 0, 0, 0, 2}, first);          // in the middle
        check_set({2, 0, 0, 0}, first);             // and at the end
        check_set({1, 1, 1, 1, 1, 1, 1, 1, 1}, first);
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("segments ok\n");
    return 0;
}
