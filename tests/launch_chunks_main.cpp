// Host-only check of launch_chunks (csrc/srg_internal.h), the walk behind every chunked kernel launch of
// the library: a recording callable stands in for the launch, so no GPU call is made.  Built and run by
// tests/test_launch_chunks_cpu.py; prints one line per case and exits non-zero when any fact fails.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "srg_internal.h"

namespace {

struct Chunk {
    int64_t b0;
    unsigned nb;
};

constexpr int64_t kPerLaunch = 4;
constexpr int kStatus = 7;   // any non-zero status

// the chunks tile [0, blocks) in ascending order, none empty, none larger than kPerLaunch
bool tiles(int64_t blocks)
{
    std::vector<Chunk> seen;
    const int rc = launch_chunks(blocks, kPerLaunch, [&](int64_t b0, unsigned nb) {
        seen.push_back({b0, nb});
        return 0;
    });
    bool ok = rc == 0 && (int64_t)seen.size() == (blocks + kPerLaunch - 1) / kPerLaunch;
    int64_t next = 0;
    for (const Chunk& c : seen) {
        ok = ok && c.b0 == next && c.nb >= 1 && c.nb <= kPerLaunch;
        next += c.nb;
    }
    return ok && next == blocks;
}

// a status at the second chunk ends the walk there and is what the walk returns
bool stops(int64_t blocks)
{
    const int64_t chunks = (blocks + kPerLaunch - 1) / kPerLaunch;
    int64_t calls = 0;
    const int rc = launch_chunks(blocks, kPerLaunch, [&](int64_t, unsigned) { return ++calls == 2 ? kStatus : 0; });
    return chunks >= 2 ? (rc == kStatus && calls == 2) : (rc == 0 && calls == chunks);
}

}  // namespace

int main()
{
    int failed = 0;
    for (int64_t blocks : {0, 1, 3, 4, 5, 8, 9}) {
        const bool t = tiles(blocks), s = stops(blocks);
        std::printf("blocks=%lld tiles=%s stops=%s\n", (long long)blocks, t ? "ok" : "FAIL", s ? "ok" : "FAIL");
        failed += !t + !s;
    }
    return failed ? 1 : 0;
}
