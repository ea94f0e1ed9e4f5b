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

// one walk of launch_chunks_capped at the site default kPerLaunch: its chunks and what the counter rose by
struct Walk {
    int rc;
    std::vector<Chunk> seen;
    int64_t counted;
};

Walk capped_walk(int64_t blocks, int fail_at = 0)
{
    Walk w{0, {}, g_chunk_launches.load()};
    w.rc = launch_chunks_capped(blocks, kPerLaunch, [&](int64_t b0, unsigned nb) {
        w.seen.push_back({b0, nb});
        return (int)w.seen.size() == fail_at ? kStatus : 0;
    });
    w.counted = g_chunk_launches.load() - w.counted;
    return w;
}

bool same(const Walk& w, std::initializer_list<Chunk> want, int rc = 0)
{
    bool ok = w.rc == rc && w.seen.size() == want.size() && w.counted == (int64_t)want.size();
    size_t i = 0;
    for (const Chunk& c : want) {
        ok = ok && i < w.seen.size() && w.seen[i].b0 == c.b0 && w.seen[i].nb == c.nb;
        ++i;
    }
    return ok;
}

// the override of the capped walk (what srg_debug_launch_cap sets): g_launch_cap_override
int capped_facts()
{
    int failed = 0;
    auto fact = [&](const char* name, bool ok) {
        std::printf("capped %s=%s\n", name, ok ? "ok" : "FAIL");
        failed += !ok;
    };
    g_launch_cap_override.store(0);
    fact("default", launch_cap(kPerLaunch) == kPerLaunch && same(capped_walk(8), {{0, 4}, {4, 4}}));
    g_launch_cap_override.store(3);
    fact("override3", launch_cap(kPerLaunch) == 3 && same(capped_walk(8), {{0, 3}, {3, 3}, {6, 2}}));
    fact("stops", same(capped_walk(8, 2), {{0, 3}, {3, 3}}, kStatus));
    g_launch_cap_override.store(100);   // larger than the site's default: the default holds
    fact("no_raise", launch_cap(kPerLaunch) == kPerLaunch && same(capped_walk(8), {{0, 4}, {4, 4}}));
    g_launch_cap_override.store(0);
    fact("restored", launch_cap(kPerLaunch) == kPerLaunch && launch_cap(kMaxLaunchBlocks) == kMaxLaunchBlocks &&
                         same(capped_walk(9), {{0, 4}, {4, 4}, {8, 1}}));
    return failed;
}

}  // namespace

int main()
{
    int failed = capped_facts();
    for (int64_t blocks : {0, 1, 3, 4, 5, 8, 9}) {
        const bool t = tiles(blocks), s = stops(blocks);
        std::printf("blocks=%lld tiles=%s stops=%s\n", (long long)blocks, t ? "ok" : "FAIL", s ? "ok" : "FAIL");
        failed += !t + !s;
    }
    return failed ? 1 : 0;
}
