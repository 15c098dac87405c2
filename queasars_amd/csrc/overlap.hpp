// Overlaps and operator matrix elements of a launch group's states against kept states: sizes and kernel launch
// wrappers.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kernels.hpp"

namespace qsv {

constexpr uint32_t kOvlBlock = 16;                              // states per block: one side of a v_mfma_f64_16x16x4_f64 tile
constexpr uint32_t kOvlMaxStates = QSV_OVERLAP_MAX_STATES;      // kept states per call
constexpr uint32_t kOvlTile = 2 * kOvlBlock * kOvlBlock;        // doubles of one complex tile: 256 real parts, then 256 imaginary parts
constexpr uint32_t kOvlMaxBlocks = 512;                         // workgroups (one wave each) per pair of blocks
constexpr size_t kOvlScratchBytes = size_t(64) << 20;           // most a launch group's partial tiles may take

// the kept states' slots of the kept-state buffer, in the caller's order (a kernel argument: read at wave-uniform addresses)
struct OverlapRefs {
    uint32_t slot[kOvlMaxStates];
};

inline uint32_t overlap_state_blocks(size_t n_states) { return uint32_t((n_states + kOvlBlock - 1) / kOvlBlock); }
// Workgroups per pair of blocks: a function of the register alone, so neither an evaluation's row nor a kept state's column
// depends on the batch or on how many kept states the call names.
inline uint32_t overlap_blocks(int n_qubits) {
    const uint64_t chunks = n_qubits > 6 ? uint64_t(1) << (n_qubits - 6) : 1;
    return uint32_t(chunks < kOvlMaxBlocks ? chunks : kOvlMaxBlocks);
}
// doubles a workgroup leaves: the tile of S, then (with the operator) the tile of T
inline uint32_t overlap_partial(bool with_operator) { return with_operator ? 2 * kOvlTile : kOvlTile; }
// bytes of the partial tiles of a launch group of `group` evaluations
inline size_t overlap_partial_bytes(int n_qubits, size_t n_refs, bool with_operator, size_t group) {
    return size_t(overlap_state_blocks(group)) * overlap_state_blocks(n_refs) * overlap_blocks(n_qubits) * overlap_partial(with_operator) *
           sizeof(double);
}
// The launch group: `limit` evaluations (at least one), fewer -- whole blocks of 16 -- where the partial tiles would pass
// kOvlScratchBytes.  One block of evaluations always fits: 4 blocks of kept states x 512 workgroups x 8 KiB = 16 MiB.
inline size_t overlap_group(int n_qubits, size_t n_refs, bool with_operator, size_t limit) {
    const size_t per_block = overlap_partial_bytes(n_qubits, n_refs, with_operator, kOvlBlock);
    const size_t most = std::max<size_t>(1, kOvlScratchBytes / per_block) * kOvlBlock;
    return std::max<size_t>(1, std::min(limit, most));
}

// partials[((eb * ref_blocks + rb) * blocks + w) * overlap_partial(..) + ..]: workgroup w's share, for the evaluations
// 16 eb + c in the state slots of `states` and the kept states refs.slot[16 rb + r] of `kept`, of <phi_r|psi_c> at [r * 16 + c]
// (real part) and [256 + r * 16 + c] (imaginary part) and, where op.n_groups >= 0, of <phi_r|H_h psi_c> at 512 + the same: the
// diagonal table (may be null) and the x-mask groups as operator_row reads them.  op.n_groups < 0 (kNoOperator): no operator,
// nothing of it is read.  Rows and columns past n_refs / n_evals are zero.  Nothing state-sized is written.
constexpr OperatorView kNoOperator{nullptr, -1, nullptr, nullptr, nullptr, nullptr};
hipError_t launch_overlap_panels(int dtype, const void* states, const void* kept, const OverlapRefs& refs, uint32_t n_refs, int n_qubits,
                                 int n_evals, const OperatorView& op, double* partials, hipStream_t stream);

// out_s[((position * n_refs) + k) * 2 + {0, 1}] = <phi_k|psi_position>, the sums of the partial tiles in ascending workgroup
// order; out_t the same for <phi_k|H_h psi> (null: the partials hold no such tile).
hipError_t launch_overlap_combine(const double* partials, int n_qubits, int n_evals, uint32_t n_refs, double* out_s, double* out_t,
                                  hipStream_t stream);

}  // namespace qsv
