// Register splitting: evaluate a weakly entangled circuit as two small circuits and a combination of their final states.
//
// EVQE individuals are shallow (a few layers of one gate per qubit), so their controlled rotations often leave the
// register in two halves A and B that interact through very few cu3 gates.  Every such CROSS gate (control c on one
// side, target on the other) is  P0(c) (x) I  +  P1(c) (x) U : applied to a sum of product terms it doubles the number
// of terms, unless the terms already have a definite value of c (the same control was used before and not rotated
// since: one KEY = one control qubit between two gates that target it).  With K keys cut by the partition
//
//     psi[i] = sum over kappa in {0,1}^K of  a_kappa[i restricted to A] * b_kappa[i restricted to B]
//
// where a_kappa / b_kappa are the final states of two VIRTUAL circuits on |A| + K and |B| + K qubits: the side's own
// gates, plus one extra qubit per key that starts as (1, 1) and is never targeted.  On the target side the cross gate
// becomes cu3(key -> target); on the control side the key's first use becomes the projector P_kappa(c), written as
// [X(c) if key] P0(c) [X(c) if key].  Both virtual circuits are small (at most a few qubits more than a tile), so the
// ordinary pass kernel runs each in one to sixteen workgroups.  What is left is the expectation value of
// psi = sum_kappa a_kappa (x) b_kappa:
//   * under a diagonal operator whose terms have at most two Z factors (Ising / QUBO), from weighted Gram matrices of the
//     two small states alone (kernels.hpp: launch_factor) -- nothing of size 2^n is touched;
//   * under any other diagonal operator, one streaming kernel (contract_kernel) forms psi on the fly and reduces
//     <psi|D|psi> -- the only sweep over 2^n indices, with 4 * 2^K + 3 fp64 operations per amplitude instead of a pass of
//     gates;
//   * under a general Pauli operator, two small matrices per term (launch_factor_terms);
//   * and samples of |psi|^2 are drawn from the two states directly (launch_split_sample).
//
// This generalises the compact first pass (plan.hpp): there only pass 0 worked on a table of tiles, here every gate
// does.  A circuit that has no such partition (deeper, well entangled circuits) keeps the ordinary multi-pass plan.
#pragma once

#include <cstdint>
#include <vector>

#include "plan.hpp"

namespace qsv {

// Angle-table entries with p_theta below -1 are FIXED matrices (prepare_kernel): the virtual circuits need a projector,
// an unnormalised |0> + |1> and an exact X.  Public op lists cannot contain them (validate_ops).
constexpr int32_t kFixedProj0 = -2;  // [[1, 0], [0, 0]]
constexpr int32_t kFixedOnes = -3;   // [[1, 0], [1, 0]]: applied to |0> it gives (1, 1)
constexpr int32_t kFixedX = -4;      // [[0, 1], [1, 0]]

constexpr int kMaxSplitKeys = 5;  // (beyond three: 16 / 32 product terms, kernels.hpp launch_factor_big; quadratic operators only)

struct SplitCircuits {
    bool ok = false;
    int n_keys = 0;
    int n_side[2] = {0, 0};          // real qubits of side A / B (virtual circuits have n_side + n_keys qubits)
    uint64_t mask[2] = {0, 0};       // qubits of side A / B
    std::vector<GateIn> gates[2];    // the virtual circuits: side qubits renumbered 0.. in ascending order, then the keys
    std::vector<AngleSource> angles[2];
};

// max_side: most qubits a virtual circuit may have.  Deterministic.
SplitCircuits find_split(int n_qubits, const std::vector<GateIn>& gates, const std::vector<AngleSource>& op_angles,
                         int max_side, int max_keys = kMaxSplitKeys);
// Several size limits in order of preference (smaller virtual circuits first): the result of the first limit that has a
// partition, found in ONE enumeration of key sets.
SplitCircuits find_split(int n_qubits, const std::vector<GateIn>& gates, const std::vector<AngleSource>& op_angles,
                         const std::vector<int>& max_sides, int max_keys = kMaxSplitKeys);

// The REDUCED form of the same partition and keys.  A key's control c is FINAL when nothing targets c after the key's first
// gate (only the last epoch of a control can be).  P_kappa(c) then commutes with everything that follows on c's side, so
//
//     a_kappa(x) = a(x) [x_c = kappa_j]
//
// with a(x) the state of the side's circuit WITHOUT the key: no key qubit, no (1, 1) start, no CX / P0 / CX.  The rows for
// kappa_j = 0 / 1 are the two halves of the one state, Gram entries whose final-key bits differ are exactly zero and the others
// are sums over half of x.  The target's side of the key is as in the full form.
//
// Layout of a reduced side: its real qubits that are no final controls in ascending order, then its final controls in
// ascending order of their keys, then its simulated keys in ascending order -- so the restriction x_c = beta is a contiguous
// half and (simulated keys, final-control bits) index the rows the way the keys do in the full form.
struct ReducedSplit {
    bool any = false;                // at least one side got smaller
    uint32_t final_keys[2] = {0, 0};      // per side: the keys (bits of kappa) whose control is final on it
    uint32_t simulated_keys[2] = {0, 0};  // per side: the keys it still simulates (the others)
    int n_virtual[2] = {0, 0};            // n_side + popcount(simulated_keys)
    int key_bit[2][kMaxSplitKeys];        // per side and key: its bit in the side's index (a key qubit's, or the final control's)
    std::vector<int> qubit_of[2];         // per side: the full form's local qubit (0 .. n_side - 1) at each reduced real position
    std::vector<GateIn> gates[2];
    std::vector<AngleSource> angles[2];
};

// From the full form alone (the projector triples and (1, 1) starts are told by their fixed matrices).  Deterministic.
ReducedSplit reduce_final_controls(const SplitCircuits& full);

}  // namespace qsv
