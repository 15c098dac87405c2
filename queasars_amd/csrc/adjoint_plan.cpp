// Host planner of the adjoint gradient sweep (adjoint_plan.hpp).
#include "adjoint_plan.hpp"

#include <algorithm>

namespace qsv {

int adjoint_plan(int n_qubits, int n_ops, const qsv_op* ops, int n_params, int n_wrt, const int32_t* wrt, AdjointPlan* out) {
    if (!out || n_qubits < 1 || n_qubits > 63 || n_ops < 0 || n_params < 0 || (n_ops > 0 && !ops) || (n_wrt > 0 && !wrt)) return QSV_E_ARG;
    for (int i = 0; i < n_ops; ++i) {
        const qsv_op& o = ops[i];
        if (o.kind > QSV_OP_CU3) return QSV_E_ARG;
        if (o.kind == QSV_OP_ID) continue;
        if (o.target >= n_qubits) return QSV_E_ARG;
        if (o.kind == QSV_OP_CU3 && (o.control >= n_qubits || o.control == o.target)) return QSV_E_ARG;
        for (int32_t p : {o.p_theta, o.p_phi, o.p_lambda})
            if (p >= n_params || p < -1) return QSV_E_ARG;
    }
    std::vector<char> wanted(size_t(n_params), n_wrt < 0 ? 1 : 0);
    for (int j = 0; j < n_wrt; ++j) {
        if (wrt[j] < 0 || wrt[j] >= n_params) return QSV_E_ARG;
        wanted[size_t(wrt[j])] = 1;
    }
    out->runs.clear();
    out->gates.clear();
    out->stop_op = n_ops;
    for (int i = 0; i < n_ops && out->stop_op == n_ops; ++i) {
        if (ops[i].kind == QSV_OP_ID) continue;
        for (int32_t p : {ops[i].p_theta, ops[i].p_phi, ops[i].p_lambda})
            if (p >= 0 && wanted[size_t(p)]) out->stop_op = i;
    }

    const int tile_bits = std::min(kAdjointTileBits, n_qubits), low_bits = std::min(kAdjointLowBits, n_qubits);
    const uint64_t low_mask = (uint64_t(1) << low_bits) - 1;
    const int free_bits = tile_bits - low_bits;  // tile qubits a run chooses
    uint64_t high = 0;
    AdjointRun cur{};
    bool open = false;
    auto close = [&]() {
        // (a run that needs fewer qubits than a tile has takes the lowest ones it does not hold yet)
        uint64_t mask = low_mask | high;
        for (int q = 0; __builtin_popcountll(mask) < tile_bits; ++q) mask |= uint64_t(1) << q;
        cur.mask = mask;
        out->runs.push_back(cur);
        open = false;
    };
    for (int i = n_ops - 1; i >= 0; --i) {
        const qsv_op& o = ops[i];
        if (o.kind == QSV_OP_ID) continue;
        uint64_t need = uint64_t(1) << o.target;
        if (o.kind == QSV_OP_CU3) need |= uint64_t(1) << o.control;
        need &= ~low_mask;
        if (open && (__builtin_popcountll(high | need) > free_bits || cur.n_gates >= kAdjointMaxRunGates)) close();
        if (!open) {
            open = true;
            high = 0;
            cur = AdjointRun{0, i, i, int32_t(out->gates.size()), 0};
        }
        high |= need;
        cur.first_op = i;
        cur.n_gates += 1;
        out->gates.push_back(i);
    }
    if (open) close();

    // the sweep ends at stop_op: whole runs in front of it go, the run it lies in is shortened and keeps its mask
    while (!out->runs.empty() && out->runs.back().last_op < out->stop_op) out->runs.pop_back();
    if (out->runs.empty()) {
        out->gates.clear();
        return QSV_OK;
    }
    AdjointRun& last = out->runs.back();
    if (last.first_op < out->stop_op) {
        int32_t kept = 0;
        while (kept < last.n_gates && out->gates[size_t(last.first_gate + kept)] >= out->stop_op) ++kept;
        last.n_gates = kept;
        last.first_op = out->stop_op;
    }
    out->gates.resize(size_t(last.first_gate + last.n_gates));
    return QSV_OK;
}

const SweepCircuit* sweep_tables_add(SweepTables& tables, const void* key, int n_qubits, int n_ops, const qsv_op* ops, int n_params) {
    const auto found = tables.circuits.find(key);
    if (found != tables.circuits.end()) return &found->second;
    AdjointPlan plan;
    if (adjoint_plan(n_qubits, n_ops, ops, n_params, -1, nullptr, &plan)) return nullptr;
    SweepCircuit t{uint32_t(tables.gates.size()), uint32_t(tables.runs.size()), uint32_t(plan.runs.size()), uint32_t(plan.gates.size()), {}};
    t.readers.resize(size_t(n_params));
    for (const AdjointRun& r : plan.runs) {
        tables.runs.push_back(AdjRunDesc{r.mask, uint32_t(r.first_gate), uint32_t(r.n_gates)});
        for (int32_t g = r.first_gate; g < r.first_gate + r.n_gates; ++g) {
            const qsv_op& o = ops[size_t(plan.gates[size_t(g)])];
            auto tile_bit = [&](int q) { return uint8_t(__builtin_popcountll(r.mask & ((uint64_t(1) << q) - 1))); };
            AdjGate ag{};
            ag.kind = o.kind;
            ag.tpos = tile_bit(o.target);
            ag.cpos = o.kind == QSV_OP_CU3 ? tile_bit(o.control) : uint8_t(QSV_NO_CONTROL);
            const int32_t p[3] = {o.p_theta, o.p_phi, o.p_lambda};
            const double lit[3] = {o.theta, o.phi, o.lambda};
            for (int s = 0; s < 3; ++s) {
                ag.p[s] = p[s] >= 0 ? p[s] : -1;
                ag.lit[s] = lit[s];
                if (p[s] >= 0) t.readers[size_t(p[s])].push_back(uint32_t(3 * g + s));
            }
            tables.gates.push_back(ag);
        }
    }
    return &tables.circuits.emplace(key, std::move(t)).first->second;
}

}  // namespace qsv
