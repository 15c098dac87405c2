// Host planner of the adjoint gradient sweep: which gates one reverse sweep of the state visits, cut into
// runs of consecutive gates whose qubits fit one workgroup tile.  Plain C++, no device.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/qsv.h"

namespace qsv {

// A workgroup tile of the sweep: 2^kAdjointTileBits amplitudes of psi and of lambda (fp64: 64 KiB of a CU's 160 KiB of LDS).
// A tile is addressed by that many tile qubits; the lowest kAdjointLowBits qubits are always among them, so a thread's
// global accesses are runs of 2^kAdjointLowBits amplitudes (256 bytes in fp64).
constexpr int kAdjointTileBits = 11;
constexpr int kAdjointLowBits = 4;
// Most gates of a run: the run kernel keeps one sum per (gate, angle slot, wave) in LDS behind the two tiles.
constexpr int kAdjointMaxRunGates = 64;

// One run, in the order the sweep takes them (run 0 holds the circuit's LAST gates).  Its swept gates are
// gates[first_gate .. first_gate + n_gates) of the plan, last gate first.
struct AdjointRun {
    uint64_t mask;       // the tile's qubits: min(kAdjointTileBits, n) bits, the low min(kAdjointLowBits, n) among them
    int32_t first_op;    // smallest and largest op index of its gates (circuit order)
    int32_t last_op;
    int32_t first_gate;
    int32_t n_gates;
};

struct AdjointPlan {
    std::vector<AdjointRun> runs;
    std::vector<int32_t> gates;  // op index of every swept gate (non-id), last first
    int32_t stop_op = 0;         // the earliest op the sweep visits (n_ops: it visits none)
};

// The plan of ops[0 .. n_ops) on n_qubits differentiated by wrt[0 .. n_wrt) (n_wrt < 0: by every parameter).  The runs are cut
// greedily from the last gate backwards, over the WHOLE circuit; the plan then ends at the earliest gate that reads a requested
// parameter -- the run that gate lies in keeps the mask it has in the whole circuit's plan, so the tiles (and with them every
// partial sum) of a gate do not depend on wrt.  Returns QSV_OK or QSV_E_ARG (an op kind, qubit, parameter or wrt index out of
// range; n_qubits outside 1 .. 63).
int adjoint_plan(int n_qubits, int n_ops, const qsv_op* ops, int n_params, int n_wrt, const int32_t* wrt, AdjointPlan* out);

}  // namespace qsv
