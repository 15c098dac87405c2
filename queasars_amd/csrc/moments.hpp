// The operator's first two moments on a launch group's states: kernel launch wrappers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace qsv {

constexpr int kMomentsThreads = 256;
constexpr uint32_t kMomentsMaxBlocks = 256;  // workgroups per evaluation of operator_moments_kernel

// Workgroups per evaluation: a function of the register alone, so an evaluation's partials do not depend on its batch.
inline uint32_t moments_blocks(int n_qubits) {
    const uint64_t want = (uint64_t(1) << n_qubits) / uint64_t(kMomentsThreads);
    return uint32_t(want < 1 ? 1 : want > kMomentsMaxBlocks ? kMomentsMaxBlocks : want);
}

// partials[(position * moments_blocks(n) + b) * 2 + {0, 1}]: workgroup b's share of Re<psi|H_h psi> and of |H_h psi|^2 for the
// state in slot `position` (slot s at s * 2^n amplitudes of `states`): the diagonal table (may be null) for the x = 0 group, the
// x-mask groups with pauli_groups_kernel's conventions.  One read of the state per group; nothing state-sized is written.
hipError_t launch_operator_moments(int dtype, const void* states, int n_qubits, int n_evals, const OperatorView& op, double* partials,
                                   hipStream_t stream);

// out[position * 2] = m1, out[position * 2 + 1] = m2 - m1 * m1 (not clamped), m1 / m2 the sums of the position's `blocks`
// partials in a fixed order.
hipError_t launch_moments_combine(const double* partials, uint32_t blocks, int n_evals, double* out, hipStream_t stream);

}  // namespace qsv
