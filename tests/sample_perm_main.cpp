// Prints the draws of the samplers' shared bijection (FeistelWalk, csrc/srg_device.h) as the host compiles
// it: one line "seed v m k" per case on standard input, one line of the k draws walk(0) .. walk(k - 1) over
// [0, m) under key = sample_key(seed, v) per case on standard output ("failed" for a walk that hit its bound).
// tests/test_neighbor_cpu.py compares the lines with the Python restatement (tests/neighbor_ref.py).  No GPU call.
#include <cinttypes>
#include <cstdio>

#include "srg_device.h"

int main()
{
    uint64_t seed, v, m, k;
    while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &seed, &v, &m, &k) == 4) {
        const FeistelWalk fw(sample_key(seed, v), m);
        for (uint64_t t = 0; t < k; ++t) {
            const uint64_t x = fw.walk(t);
            if (x == kWalkFailed)
                std::printf("failed%s", t + 1 < k ? " " : "");
            else
                std::printf("%" PRIu64 "%s", x, t + 1 < k ? " " : "");
        }
        std::printf("\n");
    }
    return 0;
}
