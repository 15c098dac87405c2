// Adjoint gradients: device tables and kernel launch wrappers of the reverse sweep.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adjoint_plan.hpp"
#include "kernels.hpp"

namespace qsv {

// (The gate and run tables, AdjGate and AdjRunDesc, are adjoint_plan.hpp's.)
// One evaluation of a launch group, by its position in the group.
struct AdjEval {
    uint32_t gate_base;  // the circuit's gates in the gate table
    uint32_t run_base;   // ... and its runs in the run table
    uint32_t n_runs;     // runs THIS evaluation sweeps (a wrt that stops early: fewer than the circuit has)
    uint32_t n_gates;    // gates it sweeps (its last run ends there)
    uint32_t row;        // the evaluation's number in the call: its row of the points and of the output
    uint32_t pad;
};
// One requested entry of an evaluation's gradient: the angle slots (3 * gate + slot, ascending) that read its parameter are
// slots[first .. first + count)
struct AdjEntry {
    uint32_t first, count;
};

constexpr int kAdjointThreads = 256;
constexpr uint32_t kAdjointMaxBlocks = 512;  // workgroups per evaluation of the run kernel
constexpr uint32_t kAdjointOpBlocks = 256;   // ... of apply_operator_kernel
constexpr int kAdjointMatDoubles = 32;       // per (evaluation, gate): U^dagger and dU/dtheta, dU/dphi, dU/dlambda, 8 doubles each

// Workgroups per evaluation of the run kernel: every workgroup loops over at least two tiles where there are two.
inline uint32_t adjoint_blocks(int n_qubits) {
    const int outer = n_qubits > kAdjointTileBits ? n_qubits - kAdjointTileBits : 0;
    const uint64_t tiles = uint64_t(1) << outer;
    const uint64_t want = tiles / 2;
    return uint32_t(want < 1 ? 1 : want > kAdjointMaxBlocks ? kAdjointMaxBlocks : want);
}
inline uint32_t adjoint_op_blocks(int n_qubits) {
    const uint64_t want = (uint64_t(1) << n_qubits) / (uint64_t(kAdjointThreads) * 8);
    return uint32_t(want < 1 ? 1 : want > kAdjointOpBlocks ? kAdjointOpBlocks : want);
}

// mats[(position * max_gates + g) * kAdjointMatDoubles ..] for every swept gate g of every evaluation of the group; the angles
// are literals or come from row evals[position].row of `values` (rows of `width` doubles, device memory).
hipError_t launch_adjoint_prepare(const AdjEval* evals, int n_evals, const AdjGate* gates, uint32_t max_gates, const double* values,
                                  int64_t width, double* mats, hipStream_t stream);

// lambda = H_h psi for the group's states (slot s at s * 2^n amplitudes of `states` / `lambda`): the diagonal table (may be null)
// for the x = 0 group, the x-mask groups with pauli_groups_kernel's conventions.  e_partials[position * adjoint_op_blocks(n) + b]:
// workgroup b's share of Re<psi|lambda>.
hipError_t launch_adjoint_apply_operator(int dtype, const void* states, void* lambda, int n_qubits, int n_evals, const OperatorView& op,
                                         bool streaming, double* e_partials, hipStream_t stream);

// Run `run` of every evaluation of the group that has one.  partials[(position * 3 * max_gates + 3 * g + slot) *
// adjoint_blocks(n) + b]: workgroup b's sum of Re<lambda_g| dU_g/d(slot) |psi_(g-1)> over its tiles, for the gates g of the run.
hipError_t launch_adjoint_run(int dtype, void* states, void* lambda, int n_qubits, int n_evals, uint32_t run, const AdjEval* evals,
                              const AdjRunDesc* runs, const AdjGate* gates, const double* mats, uint32_t max_gates, bool streaming,
                              double* partials, hipStream_t stream);

// out[row * out_width + j] = 2 * (sum over the slots of entry j, ascending, and over workgroups, in a fixed order) for j below the
// row's number of entries, 0 behind them; out_values[row] (may be null) = the sum of the row's e_partials.
hipError_t launch_adjoint_combine(const AdjEval* evals, int n_evals, const int64_t* entry_offsets, const AdjEntry* entries,
                                  const uint32_t* slots, const double* partials, uint32_t max_gates, uint32_t blocks,
                                  const double* e_partials, uint32_t op_blocks, int out_width, double* out, double* out_values,
                                  hipStream_t stream);

}  // namespace qsv
