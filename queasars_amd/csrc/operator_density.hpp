// Operator-weighted reduced density matrices W_A = Tr_rest(H_h |psi><psi|) of qubit subsets of a launch group's states
// (DESIGN.md 4.19): sizes and kernel launch wrappers.  The subset table, the workgroup count and the launch sizes are
// reduced_density.hpp's (RdmSubset, rdm_blocks, rdm_group, rdm_subset_run): a partial tile here is as large as one there.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "reduced_density.hpp"

namespace qsv {

constexpr uint32_t kOpdmPartial = kRdmPartial;  // doubles a workgroup leaves: 256 of Re W, then 256 of Im W

// partials[((e * n_subsets + s) * blocks + w) * kOpdmPartial + ..]: workgroup w's share, for the evaluations e < n_evals in the
// state slots of `states`, lambda = H_h psi at the same slots of `lambda`, and the subsets table[s], s < n_subsets, of
// Re W[a][a'] = sum_b Re(lambda(a, b) conj psi(a', b)) at [a * 16 + a'] and of Im W at [256 + a * 16 + a'].  Rows and columns past
// 2^k are zero.  Nothing state-sized is written.
hipError_t launch_opdm_panels(int dtype, const void* states, const void* lambda, int n_qubits, int n_evals, const RdmSubset* table,
                              uint32_t n_subsets, double* partials, hipStream_t stream);

// out[position * row + table[s].out_at + 2 * (a * 2^k + a') + {0, 1}] = W_s[a][a'] of the evaluation at `position`: the sums of
// the partial tiles in ascending workgroup order, the live 2^k x 2^k entries only.  W is not Hermitian: nothing is mirrored.
hipError_t launch_opdm_combine(const double* partials, int n_qubits, int n_evals, const RdmSubset* table, uint32_t n_subsets, size_t row,
                               double* out, hipStream_t stream);

// values[position] = the sum of e_partials[position * op_blocks ..] (launch_adjoint_apply_operator's shares of Re<psi|H_h|psi>),
// lane by lane and then across the wave's butterfly: the order of launch_adjoint_combine's value.
hipError_t launch_opdm_values(const double* e_partials, uint32_t op_blocks, int n_evals, double* values, hipStream_t stream);

}  // namespace qsv
