// The Fubini-Study metric of a circuit's parameters: device tables, sizes and kernel launch wrappers of the
// sweep that carries derivative states and of the real Gram matrix behind it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "adjoint.hpp"

namespace qsv {

// One evaluation of a launch group, by its position in the group.  Its gates, runs and matrices are the adjoint sweep's
// (AdjGate, AdjRunDesc, launch_adjoint_prepare) of the WHOLE circuit's plan.
struct MetEval {
    uint32_t gate_base;   // the circuit's gates in the gate table
    uint32_t run_base;    // ... and its runs in the run table
    uint32_t n_runs;      // runs it sweeps: the circuit's, or 0 where it has no column
    uint32_t n_gates;     // gates it sweeps (its last run ends there)
    uint32_t row;         // the evaluation's number in the call: its row of the points and its matrix of the output
    uint32_t col_base;    // its columns in the column table, in birth order: the sweep's order of gates, slots 0 .. 2 within a gate
    uint32_t n_cols;
    uint32_t entry_base;  // its requested parameters in the entry table
    uint32_t n_entries;
    uint32_t pad;
};
// A column xi: the angle slot that gives birth to it, as 3 * (swept gate) + slot.
struct MetCol {
    uint32_t slot;
};
// One requested parameter: the columns of the slots that read it are entry_cols[first .. first + count), in ascending (gate, slot)
// order of the circuit -- descending column number.
struct MetEntry {
    uint32_t first, count;
};

constexpr int kMetricThreads = 256;
constexpr uint32_t kMetricMaxBlocks = 1024;    // workgroups per state of the run kernel
constexpr uint32_t kMetBlock = 16;             // vectors per block: one side of a v_mfma_f64_16x16x4_f64 tile
constexpr uint32_t kMetTile = kMetBlock * kMetBlock;
constexpr uint32_t kMetricGramMaxBlocks = 256;  // workgroups (one wave each) per pair of blocks of the Gram kernel

// Workgroups per state of the run kernel: one per tile up to kMetricMaxBlocks, which then loop.
inline uint32_t metric_blocks(int n_qubits) {
    const int outer = n_qubits > kAdjointTileBits ? n_qubits - kAdjointTileBits : 0;
    const uint64_t tiles = uint64_t(1) << outer;
    return uint32_t(tiles > kMetricMaxBlocks ? kMetricMaxBlocks : tiles);
}
// Workgroups per pair of blocks of the Gram kernel: a function of the register alone, so no entry depends on the batch, on the
// evaluation's position or on how many columns it has.
inline uint32_t metric_gram_blocks(int n_qubits) {
    const uint64_t chunks = n_qubits > 6 ? uint64_t(1) << (n_qubits - 6) : 1;
    return uint32_t(chunks < kMetricGramMaxBlocks ? chunks : kMetricGramMaxBlocks);
}
// The Gram matrix of an evaluation is over its columns and, last, i psi: blocks of 16 vectors, pairs (rb <= cb) of the upper
// triangle numbered cb * (cb + 1) / 2 + rb.
inline uint32_t metric_vec_blocks(size_t n_cols) { return uint32_t((n_cols + 1 + kMetBlock - 1) / kMetBlock); }
inline uint32_t metric_pairs(size_t n_cols) {
    const uint32_t nb = metric_vec_blocks(n_cols);
    return nb * (nb + 1) / 2;
}

// An evaluation's scratch is `stride` states (of 2^n amplitudes): psi's two buffers, then its columns.  Run r reads psi from the
// group's state slot (r == 0) or from buffer (r - 1) & 1, and writes buffer r & 1 -- the last run as i psi = (-Im psi, Re psi),
// which the Gram kernel takes as the vector behind the columns.
constexpr uint32_t kMetricPsiBuffers = 2;

// Run `run` of every evaluation of the group that has one.  Grid (metric_blocks(n), 1 + max_cols, evaluations): state 0 is psi,
// state 1 + c column c.  A column born in this run starts from psi's tile as the run found it.  Nothing is summed.
hipError_t launch_metric_run(int dtype, const void* states, void* scratch, uint64_t stride, int n_qubits, int n_evals, uint32_t max_cols,
                             uint32_t run, const MetEval* evals, const AdjRunDesc* runs, const AdjGate* gates, const MetCol* cols,
                             const double* mats, uint32_t max_gates, bool streaming, hipStream_t stream);

// partials[((position * max_pairs + pair) * metric_gram_blocks(n) + w) * kMetTile + r * 16 + c]: workgroup w's share of
// Re<v_(16 rb + r)|v_(16 cb + c)> over the evaluation's vectors v = (its columns, i psi) -- so row and column n_cols hold
// b = Im<psi|xi>.  Pairs past an evaluation's own are left unwritten and never read.
hipError_t launch_metric_gram(int dtype, const void* scratch, uint64_t stride, int n_qubits, int n_evals, uint32_t max_cols,
                              const MetEval* evals, double* partials, hipStream_t stream);

// out[(row * out_width + i) * out_width + j] = sum over the columns a of entry i and b of entry j, in the entries' order, of
// T_ab - b_a b_b, with T and b the sums of the partial tiles in ascending workgroup order; the lower triangle is the upper one's
// copy; zeros behind the evaluation's entries.
hipError_t launch_metric_combine(const MetEval* evals, int n_evals, const MetEntry* entries, const uint32_t* entry_cols,
                                 const double* partials, uint32_t max_pairs, uint32_t blocks, int out_width, double* out,
                                 hipStream_t stream);

}  // namespace qsv
