// Second moments of an observable set on a launch group's states: kernel launch wrappers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace qsv {

constexpr uint32_t kCovBlock = 16;          // observables per block: one side of a v_mfma_f64_16x16x4_f64 tile
constexpr uint32_t kCovMaxObservables = QSV_COVARIANCE_MAX_OBSERVABLES;
constexpr uint32_t kCovPartial = kCovBlock * kCovBlock + kCovBlock;  // doubles a workgroup leaves: the tile, then the block's E_m
constexpr uint32_t kCovMaxBlocks = 1024;    // workgroups (one wave each) per evaluation, over all its block pairs

// A term of an observable as covariance_panels_kernel reads it: the z mask, with bit 63 set where the string has an odd number of
// Y factors (its coefficient then counts towards the imaginary part of the group's weight, else towards the real part), and the
// real coefficient with (-1)^floor(ny / 2) folded in.
struct CovTerm {
    uint64_t z;
    double c;
};
constexpr uint64_t kCovOddY = uint64_t(1) << 63;

inline uint32_t covariance_obs_blocks(uint32_t n_obs) { return (n_obs + kCovBlock - 1) / kCovBlock; }
// block pairs (a <= b), in the order a = 0: b = 0 .., a = 1: b = 1 ..
inline uint32_t covariance_pairs(uint32_t n_obs) {
    const uint32_t nb = covariance_obs_blocks(n_obs);
    return nb * (nb + 1) / 2;
}
// Workgroups per evaluation and block pair: a function of the register and the set's size alone, so an evaluation's partials do
// not depend on its batch.
inline uint32_t covariance_blocks(int n_qubits, uint32_t n_obs) {
    const uint64_t chunks = n_qubits > 6 ? uint64_t(1) << (n_qubits - 6) : 1;
    const uint64_t cap = kCovMaxBlocks / covariance_pairs(n_obs);
    return uint32_t(chunks < cap ? chunks : cap);
}

// partials[((position * pairs + p) * blocks + w) * kCovPartial + ..]: workgroup w's share, for the state in slot `position` and
// the block pair p = (a, b), of Re<lambda_(16a + r)|lambda_(16b + c)> at [r * 16 + c] and, where a == b, of
// Re<psi|lambda_(16a + r)> at [256 + r]; lambda_m = O_m psi from the set's tables: obs_first[m] .. obs_first[m + 1] are observable
// m's x-mask groups (x = 0 among them), each a run of `terms`.  Nothing state-sized is written.
hipError_t launch_covariance_panels(int dtype, const void* states, int n_qubits, int n_evals, uint32_t n_obs, const uint32_t* obs_first,
                                    const PauliGroup* groups, const CovTerm* terms, double* partials, hipStream_t stream);

// values[position * M + m] = E_m and cov[(position * M + a) * M + b] = Re<lambda_a|lambda_b> - E_a E_b (not clamped), the sums of
// the position's partials in ascending workgroup order; the upper triangle is computed and mirrored.
hipError_t launch_covariance_combine(const double* partials, int n_qubits, int n_evals, uint32_t n_obs, double* values, double* cov,
                                     hipStream_t stream);

}  // namespace qsv
