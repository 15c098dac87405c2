// Host-side check of csrc/reduced_density.hpp: the subset table the kernels read, the workgroups per (evaluation, subset) and the
// scratch a launch needs.  Built with -fsanitize=address,undefined by tests/test_rdm_host.py and run as a program of its own.  It
// walks a register as rdm_panels_kernel does -- blocks, runs, lanes -- with the table's numbers: every amplitude read lies inside
// the state, every amplitude of the register is read exactly once (n <= 12), it goes to panel row a = the subset's bits and to a
// column below 64, and no two amplitudes of a block share a panel cell.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "reduced_density.hpp"

using namespace qsv;

static int failures = 0;
#define CHECK(cond)                                                                                                     \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            if (++failures < 20) std::printf("line %d: %s failed (n=%d k=%u subset %d %d %d %d)\n", __LINE__, #cond, n, k, q[0], q[1], q[2], q[3]); \
        }                                                                                                               \
    } while (0)

static long walk(int n, const int32_t* q, uint32_t k) {
    RdmSubset sub;
    rdm_subset(n, q, k, 7, sub);
    const uint64_t dim = uint64_t(1) << n;
    const uint32_t size = uint32_t(n) < 6 + k ? uint32_t(n) : 6 + k;
    CHECK(sub.k == k && sub.out_at == 7);
    CHECK(sub.runs >= 1 && sub.runs <= kRdmMaxRuns && sub.n_high <= kRdmMaxQubits && sub.runs == 1u << sub.n_high);
    CHECK(uint64_t(sub.blocks) * sub.runs * 64 == (dim < 64 ? 64 : dim));
    CHECK(sub.blocks >= rdm_blocks(n));  // (no workgroup of the grid is without a block)
    CHECK(uint64_t(sub.blocks) << size == dim);
    const bool full = n <= 12;
    std::vector<unsigned char> seen(full ? dim : 0, 0);
    const uint32_t step = full ? 1 : (sub.blocks > 64 ? sub.blocks / 61 : 1);  // (large registers: a sample of the blocks, the last included)
    for (uint32_t block = 0; block < sub.blocks; block = (block + step < sub.blocks || block == sub.blocks - 1) ? block + step : sub.blocks - 1) {
        uint32_t first = block << 6;
        for (uint32_t j = 0; j < sub.n_high; ++j) {
            const uint32_t p = sub.high[j];
            CHECK(p >= 6 && p < uint32_t(n) && (j == 0 || p > sub.high[j - 1]));
            first = ((first >> p) << (p + 1)) | (first & ((1u << p) - 1u));
        }
        std::vector<unsigned char> cell((kRdmSide + 1) * kRdmRow, 0);
        for (uint32_t t = 0; t < sub.runs; ++t)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const bool live = lane < dim;
                const uint32_t mine = live ? lane : 0u;
                uint32_t to = 0;
                for (uint32_t p = 0; p < 6; ++p) to += (lane >> p & 1u) * sub.lane_to[p];
                if (!live) to = kRdmSide * kRdmRow + lane;
                const uint64_t index = uint64_t(first) + sub.run_at[t] + mine;
                const uint32_t w = to + sub.run_to[t];
                CHECK(index < dim);
                CHECK(w < (kRdmSide + 1) * kRdmRow);
                if (index >= dim || w >= (kRdmSide + 1) * kRdmRow) continue;
                if (!live) {
                    CHECK(w >= kRdmSide * kRdmRow);
                    continue;
                }
                uint32_t a = 0;
                for (uint32_t j = 0; j < k; ++j) a |= uint32_t(index >> q[j] & 1u) << j;
                CHECK(w / kRdmRow == a && w % kRdmRow < 64);
                CHECK(size >= 6 + k || w % kRdmRow < (1u << (size - k)));
                CHECK(cell[w] == 0);
                cell[w] = 1;
                if (full) {
                    CHECK(seen[index] == 0);
                    seen[index] = 1;
                }
            }
    }
    if (full)
        for (uint64_t i = 0; i < dim; ++i) CHECK(seen[i] == 1);
    return 1;
}

int main() {
    long cases = 0;
    int n = 0;
    uint32_t k = 0;
    int32_t q[4] = {-1, -1, -1, -1};
    // every ordered subset of up to four qubits for n <= 7; for larger registers subsets drawn over the low, middle and top qubits
    for (n = 1; n <= 28; ++n) {
        std::vector<int> pool;
        if (n <= 7)
            for (int i = 0; i < n; ++i) pool.push_back(i);
        else
            for (int i : {0, 5, 6, 7, n / 2, n - 1}) pool.push_back(i);
        const int m = int(pool.size());
        for (k = 1; k <= kRdmMaxQubits && int(k) <= n; ++k) {
            std::vector<int> at(k, 0);
            while (true) {
                bool distinct = true;
                for (uint32_t i = 0; i < k; ++i)
                    for (uint32_t j = 0; j < i; ++j) distinct = distinct && pool[at[i]] != pool[at[j]];
                if (distinct) {
                    for (uint32_t i = 0; i < 4; ++i) q[i] = i < k ? pool[at[i]] : -1;
                    cases += walk(n, q, k);
                }
                uint32_t d = 0;
                while (d < k && ++at[d] == m) at[d++] = 0;
                if (d == k) break;
            }
        }
        // the scratch: a launch of `group` evaluations and its run of subsets stays inside kRdmScratchBytes, whatever the limit
        k = 0;
        for (size_t limit = 1; limit <= 300; ++limit) {
            const size_t group = rdm_group(n, limit), run = rdm_subset_run(n, group);
            CHECK(group >= 1 && group <= limit && run >= 1);
            CHECK(group * run * rdm_blocks(n) * kRdmPartial * sizeof(double) <= kRdmScratchBytes);
            CHECK(rdm_subset_run(n, (group + 1) / 2) >= run);  // (a smaller last group takes no fewer subsets: sized by the first)
        }
        CHECK(rdm_blocks(n) >= 1 && rdm_blocks(n) <= kRdmMaxBlocks && rdm_pairs(n) >= 256);
        CHECK(n > 10 || rdm_blocks(n) == 1);
        CHECK(n <= 10 || rdm_blocks(n) == (n - 10 >= 6 ? 64u : 1u << (n - 10)));
    }
    std::printf("%ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
