// Exact CVaR gradients: the adjoint sweep's seed under CVaR_alpha of a diagonal operator.  With the basis states
// sorted ascending by (value, index), b the boundary state the exact CVaR stops at and t = v_b, the gradient is that of the
// expectation value of the clipped operator diag(w), w_i = -max(t - v_i, 0) / alpha, t held fixed: the threshold search from the
// amplitudes of the state slots, the seed lambda = diag(w) psi with the workgroups' shares of Re<psi|lambda>, and the kernel that
// turns the combined share into the CVaR.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adjoint.hpp"

namespace qsv {

// Doubles of scratch for a launch group of n_evals: [n_evals][2] (t, s) | [n_evals][cvar_exact_chunks(2^n)] chunk masses.
inline size_t cvar_gradient_scratch_doubles(int n_qubits, size_t n_evals) {
    return n_evals * (2 + size_t(cvar_exact_chunks(uint64_t(1) << n_qubits)));
}

// launch_cvar_exact's search with p_i = |psi_i|^2 read from the group's state slots (slot e at e * 2^n amplitudes of `states`),
// gathered through order[]: the mass of every chunk of kCvarChunk ranks in a fixed order, then one workgroup per evaluation that
// finds the chunk and the rank.  target = alpha - (1e-8 + 1e-5 |alpha|); b = the first rank with cumulative mass cum_b >= target,
// the last rank where none has.  scratch[position * 2 + {0, 1}] = t = sorted_values[b] and s = max(alpha - cum_b, 0), the mass
// the stopping rule leaves out; the chunk masses lie behind the group's pairs (cvar_gradient_scratch_doubles).
hipError_t launch_cvar_gradient_threshold(int dtype, const void* states, int n_qubits, int n_evals, const uint32_t* order,
                                          const double* sorted_values, double alpha, double* scratch, hipStream_t stream);

// lambda_i = -(max(t - diag[i], 0) / alpha) psi_i in fp64, rounded to the states' type (lambda null: not stored -- a group that
// sweeps no gate), and e_partials[position * adjoint_op_blocks(n) + b] = workgroup b's share of Re<psi|lambda>:
// launch_adjoint_apply_operator's layout, for launch_adjoint_combine.  t is scratch[position * 2].
hipError_t launch_cvar_gradient_seed(int dtype, const void* states, void* lambda, int n_qubits, int n_evals, const double* diag,
                                     const double* scratch, double alpha, bool streaming, double* e_partials, hipStream_t stream);

// Per evaluation of the group, by its row evals[position].row: values[row] = t (1 - s / alpha) + values[row] (may be null; on entry
// the combined Re<psi|lambda>) and thresholds[row] = t (may be null).  scratch null (alpha within numpy.isclose of 1: the plain
// expectation value): the values stay and thresholds[row] = *largest_value.
hipError_t launch_cvar_gradient_finish(const AdjEval* evals, int n_evals, const double* scratch, double alpha, const double* largest_value,
                                       double* values, double* thresholds, hipStream_t stream);

}  // namespace qsv
