// Deflated (VQD) costs against kept states: the rank-K update of a launch group's lambda that turns the adjoint
// sweep's seed H_h psi_e into H_h psi_e + sum_k beta_k c_ek phi_k, and the kernel that adds the penalties to the values.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adjoint.hpp"
#include "overlap.hpp"

namespace qsv {

constexpr int kDeflateThreads = 256;         // four waves, each with a 16 x 64 tile (evaluations x amplitudes) of its own
constexpr uint32_t kDeflateMaxBlocks = 1024;  // workgroups per block of 16 evaluations

// Workgroups per block of evaluations: every wave has a tile of 64 amplitudes where there are that many.
inline uint32_t deflate_blocks(int n_qubits) {
    const uint64_t chunks = n_qubits > 6 ? uint64_t(1) << (n_qubits - 6) : 1;
    const uint64_t want = (chunks + kDeflateThreads / 64 - 1) / (kDeflateThreads / 64);
    return uint32_t(want > kDeflateMaxBlocks ? kDeflateMaxBlocks : want);
}

// lambda_e[i] += sum_k (betas[k] * c_ek) phi_k[i] for the group's evaluations e (slot e at e * 2^n amplitudes of `lambda`), the
// kept states refs.slot[k] of `kept` and c_ek = overlaps[(e * n_refs + k) * 2 + {0, 1}] as launch_overlap_combine leaves them
// (device memory, by position).  The sum over k is fp64, ascending, whatever the states' type.
hipError_t launch_deflate(int dtype, void* lambda, const void* kept, const OverlapRefs& refs, uint32_t n_refs, int n_qubits, int n_evals,
                          const double* betas, const double* overlaps, bool streaming, hipStream_t stream);

// Per evaluation of the group, by its row evals[position].row of the call: out_overlaps[row][k] = overlaps[position][k] (may be
// null), and out_values[row] = energies[row] + sum_k betas[k] |c_k|^2, ascending k (may be null; `energies` may be `out_values`).
hipError_t launch_deflation_finish(const AdjEval* evals, int n_evals, uint32_t n_refs, const double* betas, const double* overlaps,
                                   const double* energies, double* out_values, double* out_overlaps, hipStream_t stream);

}  // namespace qsv
