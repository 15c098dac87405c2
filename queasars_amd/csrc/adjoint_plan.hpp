// Host planner of the adjoint gradient sweep: which gates one reverse sweep of the state visits, cut into
// runs of consecutive gates whose qubits fit one workgroup tile, and the gate and run tables the sweep's kernels read of a
// call's circuits.  Plain C++, no device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
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

// ---- the sweep's tables, as the kernels of adjoint.hpp and metric.hpp read them ------------------------------------------------

// One swept gate of a circuit, in sweep order (the circuit's last gate first).
struct AdjGate {
    uint8_t kind;     // QSV_OP_U / QSV_OP_CU3
    uint8_t tpos;     // the target's bit inside the tile of the gate's run
    uint8_t cpos;     // the control's (cu3), QSV_NO_CONTROL otherwise
    uint8_t pad;
    int32_t p[3];     // theta, phi, lambda: parameter index, or -1 for the literal
    double lit[3];
};
struct AdjRunDesc {
    uint64_t mask;        // the tile's qubits
    uint32_t first_gate;  // its gates are [first_gate, first_gate + n_gates) of the circuit's swept gates
    uint32_t n_gates;
};

// A distinct circuit of a call in the tables below: the sweep by EVERY parameter (every other sweep of the circuit is a front
// part of it).
struct SweepCircuit {
    uint32_t gate_base, run_base;  // its gates and runs in SweepTables::gates / runs
    uint32_t n_runs, n_gates;
    std::vector<std::vector<uint32_t>> readers;  // per parameter: 3 * (swept gate) + slot, ascending -- the latest gate first
};
struct SweepTables {
    std::vector<AdjGate> gates;
    std::vector<AdjRunDesc> runs;
    std::unordered_map<const void*, SweepCircuit> circuits;  // by the caller's key (any pointer that tells circuits apart)
};
// The entry of the circuit `key` names, appended to the tables when the key is seen for the first time; nullptr where adjoint_plan
// refuses the circuit (the tables are then as they were).  The entry stays where it is while the tables live.
const SweepCircuit* sweep_tables_add(SweepTables& tables, const void* key, int n_qubits, int n_ops, const qsv_op* ops, int n_params);

// The tables of a call back to back, as one upload takes them: every part starts on 8 bytes (zeros fill the gaps).
struct TableBlob {
    std::vector<char> bytes;
    // the offset of the part
    size_t add(const void* src, size_t n) {
        const size_t off = bytes.size();
        bytes.resize(off + (n + 7) / 8 * 8, 0);
        if (n) std::memcpy(bytes.data() + off, src, n);
        return off;
    }
    template <class T>
    size_t add(const std::vector<T>& part) {
        return add(part.data(), part.size() * sizeof(T));
    }
    // the part at `off` of the blob's copy at `base`
    template <class T>
    static const T* at(const void* base, size_t off) {
        return reinterpret_cast<const T*>(static_cast<const char*>(base) + off);
    }
};

}  // namespace qsv
