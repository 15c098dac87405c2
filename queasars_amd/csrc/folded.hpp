// Folded-spectrum and variance costs: the adjoint sweep's seed under <psi|(H_h - c)^2|psi>.  With the centre c
// of an evaluation -- the call's target, or the evaluation's own E = Re<psi|H_h psi> --, r = H_h psi - c psi the residual, the
// cost is |r|^2 (the centred form, never negative) and the gradient is the sweep's from lambda_G = (H_h - c) r, c held fixed:
// d/dc <(H_h - c)^2> = -2 (E - c) vanishes at c = E.  The seed that is stored is lambda_G - (E - c)^2 psi: a real multiple of psi
// adds 2 alpha Re<psi|d psi> = alpha d<psi|psi> = 0 to every entry, and with a target far from E it is most of lambda_G's norm --
// swept along, it gives nothing but its rounding (DESIGN.md 4.21 has the figures).  With c = E the two are the same.  The
// kernels run behind launch_adjoint_apply_operator, which leaves lambda_1 = H_h psi and the shares of E.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adjoint.hpp"

namespace qsv {

// Workgroups per evaluation of the residual, seed and fused passes: launch_adjoint_apply_operator's.
inline uint32_t folded_blocks(int n_qubits) { return adjoint_op_blocks(n_qubits); }

// Doubles of scratch for a launch group of n_evals: [n_evals][2] (E, c) | [n_evals][folded_blocks(n)] shares of |r|^2.
inline size_t folded_scratch_doubles(int n_qubits, size_t n_evals) { return n_evals * (2 + size_t(folded_blocks(n_qubits))); }

// One wave per evaluation: E = the sum of e_partials[position * op_blocks + b] as launch_adjoint_combine adds it (a lane its
// shares b = lane, lane + 64, ... in ascending order, then the butterfly), scratch[position * 2 + {0, 1}] = E and the centre
// (own_mean: E; else `target`).
hipError_t launch_folded_centre(const double* e_partials, uint32_t op_blocks, int n_evals, bool own_mean, double target, double* scratch,
                                hipStream_t stream);

// r_i = lambda_1,i - c psi_i in fp64, rounded to the states' type into `residual` (null: not stored -- a group that sweeps no
// gate), and workgroup b's share of |r|^2, taken before the rounding, behind the group's pairs of `scratch`
// (folded_scratch_doubles).  One access per amplitude of psi, lambda_1 and r.
hipError_t launch_folded_residual(int dtype, const void* states, const void* lambda1, void* residual, int n_qubits, int n_evals,
                                  double* scratch, bool streaming, hipStream_t stream);

// lambda_i = (H_h r)_i - c r_i - (E - c)^2 psi_i: operator_row.hpp's row over the residual, in fp64, rounded to the states' type.
// `residual` and `lambda` are different buffers (the row gathers r at i ^ x).
hipError_t launch_folded_seed(int dtype, const void* states, const void* residual, void* lambda, int n_qubits, int n_evals,
                              const OperatorView& op, const double* scratch, bool streaming, hipStream_t stream);

// An operator without x-mask groups, both passes in one: r_i = (diag[i] - c) psi_i, its shares of |r|^2 as launch_folded_residual
// leaves them, and lambda_i = (diag[i] - c) r_i - (E - c)^2 psi_i (lambda null: not stored).
hipError_t launch_folded_diagonal(int dtype, const void* states, void* lambda, int n_qubits, int n_evals, const double* diag,
                                  double* scratch, bool streaming, hipStream_t stream);

// One thread per evaluation of the group, by its row evals[position].row: values[row] (may be null) = |r|^2, the shares added in
// ascending workgroup order, and energies[row] (may be null) = E.
hipError_t launch_folded_finish(const AdjEval* evals, int n_evals, int n_qubits, const double* scratch, double* values, double* energies,
                                hipStream_t stream);

}  // namespace qsv
