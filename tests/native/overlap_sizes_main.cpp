// Host-side check of csrc/overlap.hpp's sizing: overlap_blocks, the launch group and the scratch a call allocates, over every
// register size, number of kept states and group limit a handle can meet.  Built with -fsanitize=address,undefined by
// tests/test_overlap_host.py and run as a program of its own; it walks the partial-tile indices the two kernels use against a
// buffer of exactly the allocated size for the small cases, and checks the arithmetic for all.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "overlap.hpp"

using namespace qsv;

static int failures = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (++failures < 20) std::printf("line %d: %s failed (n=%d K=%zu g=%zu op=%d)\n", __LINE__, #cond, n, K, g, int(op)); \
        }                                                                                \
    } while (0)

int main() {
    long cases = 0;
    for (int n = 1; n <= 28; ++n)
        for (size_t K = 1; K <= kOvlMaxStates; ++K)
            for (size_t g = 1; g <= 256; ++g)
                for (int o = 0; o < 2; ++o) {
                    const bool op = o != 0;
                    ++cases;
                    const uint32_t blocks = overlap_blocks(n);
                    const uint64_t chunks = (((uint64_t(1) << n) + 63) / 64);
                    CHECK(blocks >= 1 && blocks <= kOvlMaxBlocks && blocks <= chunks);
                    CHECK(blocks == overlap_blocks(n));  // (the register alone)
                    const size_t G = overlap_group(n, K, op, g);
                    CHECK(G >= 1 && G <= g);
                    CHECK(G == g || G % kOvlBlock == 0);
                    const size_t bytes = overlap_partial_bytes(n, K, op, G);
                    CHECK(bytes <= kOvlScratchBytes);
                    CHECK(bytes == size_t(overlap_state_blocks(G)) * overlap_state_blocks(K) * blocks * overlap_partial(op) * sizeof(double));
                    // a smaller last group never needs more
                    CHECK(overlap_partial_bytes(n, K, op, (G + 1) / 2) <= bytes);
                    // the last double the panels kernel's last workgroup writes, and the combine kernel's last thread reads
                    const size_t eb = overlap_state_blocks(G) - 1, rb = overlap_state_blocks(K) - 1, w = blocks - 1;
                    const size_t last = ((eb * overlap_state_blocks(K) + rb) * blocks + w) * overlap_partial(op) + overlap_partial(op) - 1;
                    CHECK((last + 1) * sizeof(double) == bytes);
                    if (n <= 8 && g <= 40 && K % 7 == 1) {  // touch every index once in a buffer of exactly that size
                        std::vector<double> buf(bytes / sizeof(double), 0.0);
                        for (size_t e = 0; e <= eb; ++e)
                            for (size_t r = 0; r <= rb; ++r)
                                for (size_t b = 0; b < blocks; ++b) {
                                    double* out = buf.data() + ((e * (rb + 1) + r) * blocks + b) * overlap_partial(op);
                                    for (uint32_t lane = 0; lane < 64; ++lane)
                                        for (uint32_t reg = 0; reg < 4; ++reg)
                                            for (uint32_t part = 0; part < overlap_partial(op) / 256; ++part)
                                                out[part * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] += 1.0;
                                }
                        for (double v : buf) CHECK(v == 1.0);
                    }
                }
    std::printf("%ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
