// Reduced density matrices of qubit subsets of a launch group's states: sizes, the subset table and kernel
// launch wrappers.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kernels.hpp"

namespace qsv {

constexpr uint32_t kRdmMaxQubits = QSV_RDM_MAX_QUBITS;          // qubits of a subset: 2^4 rows, one side of a v_mfma_f64_16x16x4_f64 tile
constexpr uint32_t kRdmMaxSubsets = QSV_RDM_MAX_SUBSETS;        // subsets per call
constexpr uint32_t kRdmSide = 1u << kRdmMaxQubits;              // rows and columns of a tile
constexpr uint32_t kRdmMaxRuns = kRdmSide;                      // runs of 64 consecutive amplitudes per block
constexpr uint32_t kRdmPartial = 2 * kRdmSide * kRdmSide;       // doubles a workgroup leaves: 256 of Re rho, then 256 of X
constexpr uint32_t kRdmMaxBlocks = 64;                          // workgroups (one wave each) per (evaluation, subset)
constexpr size_t kRdmScratchBytes = size_t(64) << 20;           // most a launch's partial tiles may take

// What the kernels need of one subset A = (q_0 .. q_{k-1}), all of it read at wave-uniform addresses.  The block B is A and the
// six lowest qubits outside A (the whole register where n - k < 6); it always holds qubits 0 .. 5, so it is `runs` = 2^(|B| - 6)
// runs of 64 consecutive amplitudes (one run, of 2^n, below six qubits).  An amplitude's place in the LDS panel is row a (bit j
// of a: qubit q_j) and column b (bit r of b: the r-th lowest qubit of B outside A), in doubles: a * row stride + b.
struct RdmSubset {
    uint32_t k;                     // qubits of the subset
    uint32_t runs;                  // runs of a block
    uint32_t blocks;                // blocks of the register: 2^(n - |B|)
    uint32_t n_high;                // qubits of B above qubit 5 ...
    uint32_t high[kRdmMaxQubits];   // ... ascending: a block's number gets a zero bit there
    uint32_t out_at;                // doubles before this subset in an evaluation's row of the output: sum of 2 * 4^k
    uint32_t lane_to[6];            // panel offset that bit p of the lane adds (qubit p)
    uint32_t run_at[kRdmMaxRuns];   // run t: its amplitudes' index within the block (t's bits at `high`) ...
    uint32_t run_to[kRdmMaxRuns];   // ... and the panel offset they add
    uint32_t pad_[1];
};
static_assert(sizeof(RdmSubset) == 48 * sizeof(uint32_t), "RdmSubset is a table row of 192 bytes");

constexpr uint32_t kRdmRow = 66;  // doubles per panel row (overlap.hip: the operand reads take every bank once)

// fills `out` for the subset `qubits` (k distinct qubits below n_qubits, 1 <= k <= 4) whose block of the output starts at out_at
inline void rdm_subset(int n_qubits, const int32_t* qubits, uint32_t k, uint32_t out_at, RdmSubset& out) {
    out = RdmSubset{};
    out.k = k;
    out.out_at = out_at;
    uint32_t in_a = 0;
    for (uint32_t j = 0; j < k; ++j) in_a |= 1u << qubits[j];
    // B's qubits ascending: where each goes in the panel
    uint32_t to[6 + kRdmMaxQubits], members[6 + kRdmMaxQubits], size = 0, outside = 0;
    for (int q = 0; q < n_qubits && size < 6 + k; ++q) {
        if (in_a >> q & 1u) {
            uint32_t j = 0;
            while (uint32_t(qubits[j]) != uint32_t(q)) ++j;
            to[size] = (1u << j) * kRdmRow;
        } else {
            if (outside == 6) continue;
            to[size] = 1u << outside++;
        }
        members[size++] = uint32_t(q);
    }
    // (qubits 0 .. 5 are B's six lowest; below six qubits the lanes past 2^n are dead and their bits add nothing)
    for (uint32_t p = 0; p < 6 && p < size; ++p) out.lane_to[p] = to[p];
    out.n_high = size > 6 ? size - 6 : 0;
    for (uint32_t j = 0; j < out.n_high; ++j) out.high[j] = members[6 + j];
    out.runs = 1u << out.n_high;
    out.blocks = 1u << (uint32_t(n_qubits) - size);
    for (uint32_t t = 0; t < out.runs; ++t)
        for (uint32_t j = 0; j < out.n_high; ++j)
            if (t >> j & 1u) {
                out.run_at[t] |= 1u << out.high[j];
                out.run_to[t] += to[6 + j];
            }
}

// Workgroups per (evaluation, subset): a function of the register alone -- the blocks of a four-qubit subset, at most 64 --
// so a result depends neither on the batch nor on what else the call names.  No subset has fewer blocks.
inline uint32_t rdm_blocks(int n_qubits) {
    const uint64_t blocks = n_qubits > 6 + int(kRdmMaxQubits) ? uint64_t(1) << (n_qubits - 6 - int(kRdmMaxQubits)) : 1;
    return uint32_t(blocks < kRdmMaxBlocks ? blocks : kRdmMaxBlocks);
}
// (evaluation, subset) pairs whose partial tiles one launch may leave: at least 256 (64 workgroups x 4 KiB each)
inline size_t rdm_pairs(int n_qubits) { return kRdmScratchBytes / (size_t(rdm_blocks(n_qubits)) * kRdmPartial * sizeof(double)); }
// the launch group: `limit` evaluations (at least one), fewer where one subset's partial tiles would pass kRdmScratchBytes
inline size_t rdm_group(int n_qubits, size_t limit) { return std::max<size_t>(1, std::min(limit, rdm_pairs(n_qubits))); }
// the subsets one launch takes behind a launch group of `group` evaluations
inline size_t rdm_subset_run(int n_qubits, size_t group) { return std::max<size_t>(1, rdm_pairs(n_qubits) / std::max<size_t>(1, group)); }

// partials[((e * n_subsets + s) * blocks + w) * kRdmPartial + ..]: workgroup w's share, for the evaluations e < n_evals in the
// state slots of `states` and the subsets table[s], s < n_subsets, of Re rho at [a * 16 + a'] and of X = sum_b Im psi(a, b)
// Re psi(a', b) at [256 + a * 16 + a'].  Rows and columns past 2^k are zero.  Nothing state-sized is written.
hipError_t launch_rdm_panels(int dtype, const void* states, int n_qubits, int n_evals, const RdmSubset* table, uint32_t n_subsets,
                             double* partials, hipStream_t stream);

// out[position * row + table[s].out_at + 2 * (a * 2^k + a') + {0, 1}] = rho_s[a][a'] of the evaluation at `position`: the sums
// of the partial tiles in ascending workgroup order, Im rho = X - X^T, the live 2^k x 2^k entries only.
hipError_t launch_rdm_combine(const double* partials, int n_qubits, int n_evals, const RdmSubset* table, uint32_t n_subsets, size_t row,
                              double* out, hipStream_t stream);

}  // namespace qsv
