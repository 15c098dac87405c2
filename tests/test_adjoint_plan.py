"""Adjoint gradients without a device: the NumPy sweep of tests/adjoint_reference.py against the independent
dense derivative, and the host planner (qsv_adjoint_describe) on circuits of every shape."""

import json
from pathlib import Path

import numpy as np
import pytest

import adjoint_reference
import circuit_families as cf
import dense_gradient
import helpers
from queasars_amd import _lib
from queasars_amd.ir import OP_ID, CircuitIR, ParamRef

P = ParamRef
REFERENCE_TOL = 1e-12  # two fp64 evaluations of the same sums in another order: values of order 1 .. 10, a few hundred terms


def _fixture_population():
    from queasars_amd.evqe.serialization import population_from_dict

    data = json.loads((Path(__file__).resolve().parent / "golden" / "population_n6.json").read_text())
    population = population_from_dict(data["population"])
    circuits = [ind.get_parameterized_quantum_circuit() for ind in population.individuals]
    return circuits, [list(ind.parameter_values) for ind in population.individuals]


def _both_control_directions():
    c = CircuitIR(4)
    c.u(P(0), P(1), P(2), 0).u(P(3), P(4), P(5), 2)
    c.cu3(P(6), P(7), P(8), 0, 1).cu3(P(9), P(10), P(11), 3, 2)
    c.u(P(12), P(13), P(14), 1).cu3(P(15), P(16), P(17), 2, 0).cu3(P(18), P(19), P(20), 1, 3)
    rng = np.random.default_rng(11)
    return [c, c], [rng.uniform(-np.pi, np.pi, 21).tolist(), rng.uniform(-7.0, 7.0, 21).tolist()]


def _shared_and_literal():
    circuit, params = cf.generic(7, 40, share=0.3, literal=0.2)
    slots = circuit.packed()
    read = np.concatenate([slots[name][slots["kind"] != OP_ID] for name in ("p_theta", "p_phi", "p_lambda")])
    assert len(np.unique(read[read >= 0])) < (read >= 0).sum(), "the case is about shared parameters"
    assert (read < 0).any(), "... and literals"
    return [circuit], [params]


CASES = {"n6": _fixture_population, "cu3": _both_control_directions, "generic": _shared_and_literal}


# ---- part 1: the reference is the dense derivative ----------------------------------------------------------------------------


@pytest.mark.parametrize("population", list(CASES))
@pytest.mark.parametrize("operator", ["ising", "pauli50"])
def test_the_numpy_sweep_is_the_dense_derivative(population, operator):
    circuits, params = CASES[population]()
    n = circuits[0].n_qubits
    op = helpers.random_ising_operator(n, seed=3) if operator == "ising" else helpers.random_pauli_operator(n, 50, seed=4)
    h = dense_gradient.dense_operator(op)
    worst = worst_value = 0.0
    for circuit, values in zip(circuits, params):
        got, value = adjoint_reference.gradient_and_value(circuit, values, op)
        want = dense_gradient.gradient(circuit, values, h)
        assert got.shape == want.shape
        worst = max(worst, float(np.abs(got - want).max(initial=0.0)))
        worst_value = max(worst_value, abs(value - dense_gradient.expectation(circuit, values, h)))
    print(f"{population} / {operator}: largest deviation {worst:.3e}, of the value {worst_value:.3e}")
    assert worst < REFERENCE_TOL and worst_value < REFERENCE_TOL


# ---- part 2: the planner ----------------------------------------------------------------------------------------------------


def _genome():
    population, circuits, _ = helpers.population_circuits(13, 4, 3, seed=2)
    individual = population.individuals[0]
    start = individual.circuit_parameter_offsets[len(individual.layers) - 1]
    last_layer = list(range(start, start + individual.layers[-1].n_parameters))
    return circuits[0], last_layer


def _last_gates_parameters(circuit: CircuitIR, count: int = 5) -> list[int]:
    """The parameters the circuit's last `count` gates read: a family's "last layer"."""
    rows = [row for row in circuit.packed() if row["kind"] != OP_ID][-count:]
    return sorted({int(row[name]) for row in rows for name in ("p_theta", "p_phi", "p_lambda") if row[name] >= 0})


PLAN_CASES = {
    "ladder": lambda: cf.ladder(13)[0],
    "star": lambda: cf.star(13)[0],
    "all_pairs": lambda: cf.all_pairs(13)[0],
    "generic": lambda: cf.generic(13, 120, share=0.3, literal=0.2)[0],
    "two_blocks": lambda: cf.two_blocks(13, 3)[0],
    "genome": lambda: _genome()[0],
}


def _gate_qubits(row) -> int:
    mask = 1 << int(row["target"])
    if row["kind"] == 2:
        mask |= 1 << int(row["control"])
    return mask


def _check_cover(circuit: CircuitIR, plan: dict, stop: int):
    """The runs cover every non-id gate from op `stop` on exactly once, last to first, each inside its run's mask."""
    rows = circuit.packed()
    n = circuit.n_qubits
    tile, low = min(plan["tile_bits"], n), min(plan["low_bits"], n)
    swept = [i for i in range(len(rows)) if rows[i]["kind"] != OP_ID and i >= stop]
    assert plan["n_gates"] == len(swept)
    covered = []
    for mask, first, last in plan["runs"]:
        assert first <= last
        assert bin(mask).count("1") <= tile and mask & ((1 << low) - 1) == (1 << low) - 1 and mask < (1 << n)
        run_gates = [i for i in swept if first <= i <= last]
        assert run_gates and run_gates[0] == first and run_gates[-1] == last
        for i in run_gates:
            assert _gate_qubits(rows[i]) & ~mask == 0, f"op {i} leaves its run's tile"
        covered += reversed(run_gates)
    assert covered == list(reversed(swept))


@pytest.mark.parametrize("family", list(PLAN_CASES))
def test_runs_cover_the_swept_gates_once_inside_their_tiles(family):
    circuit = PLAN_CASES[family]()
    plan = adjoint_reference.describe(circuit)
    assert 10 <= plan["tile_bits"] <= 12 and plan["low_bits"] in (4, 5)
    assert circuit.n_qubits > plan["tile_bits"], "thirteen qubits do not fit one tile: the cases need several runs"
    rows = circuit.packed()
    reads = [i for i in range(len(rows)) if rows[i]["kind"] != OP_ID and max(rows[i]["p_theta"], rows[i]["p_phi"], rows[i]["p_lambda"]) >= 0]
    _check_cover(circuit, plan, reads[0])
    assert len(plan["runs"]) > 1


@pytest.mark.parametrize("family", list(PLAN_CASES))
def test_a_last_layer_wrt_ends_the_plan_at_its_first_reader(family):
    circuit = PLAN_CASES[family]()
    wrt = _genome()[1] if family == "genome" else _last_gates_parameters(circuit)
    assert wrt
    rows = circuit.packed()
    stop = min(i for i in range(len(rows)) if rows[i]["kind"] != OP_ID
               and {int(rows[i]["p_theta"]), int(rows[i]["p_phi"]), int(rows[i]["p_lambda"])} & set(wrt))
    plan, full = adjoint_reference.describe(circuit, wrt), adjoint_reference.describe(circuit)
    _check_cover(circuit, plan, stop)
    assert plan["runs"][-1][1] == stop
    assert plan["n_gates"] == sum(1 for i in range(stop, len(rows)) if rows[i]["kind"] != OP_ID) < full["n_gates"]
    # a gate's run and that run's mask do not depend on wrt: the shortened plan is the front of the full one
    assert [r[0] for r in plan["runs"]] == [r[0] for r in full["runs"][: len(plan["runs"])]]
    assert plan["runs"][:-1] == full["runs"][: len(plan["runs"]) - 1] and plan["runs"][-1][2] == full["runs"][len(plan["runs"]) - 1][2]


def test_small_registers_and_empty_requests():
    circuit = CircuitIR(3).u(P(0), 0.2, P(1), 0).id(1).cu3(P(2), P(0), 0.3, 2, 0).u(0.1, 0.2, 0.3, 1)
    circuit.declare_parameters(4)
    plan = adjoint_reference.describe(circuit)
    assert plan["runs"] == [(0b111, 0, 3)] and plan["n_gates"] == 3
    assert adjoint_reference.describe(circuit, [2])["runs"] == [(0b111, 2, 3)]
    assert adjoint_reference.describe(circuit, [3]) == {**plan, "runs": [], "n_gates": 0}  # (no gate reads parameter 3)
    assert adjoint_reference.describe(circuit, [])["runs"] == []


def test_describe_argument_errors():
    lib = _lib.load()
    ops = CircuitIR(2).u(P(0), P(1), P(2), 1).packed()
    out = np.zeros(4, dtype=np.uint64)
    first, last = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32)
    wrt = np.array([3], dtype=np.int32)

    def call(n_qubits, n_params, n_wrt, wrt_ptr):
        return lib.qsv_adjoint_describe(n_qubits, len(ops), _lib.as_ptr(ops), n_params, n_wrt, wrt_ptr, 4, _lib.as_ptr(out),
                                        _lib.as_ptr(first), _lib.as_ptr(last), None, None, None)

    assert call(2, 3, -1, None) == 1
    assert call(2, 2, -1, None) == _lib.QSV_E_ARG  # (a slot reads parameter 2)
    assert call(1, 3, -1, None) == _lib.QSV_E_ARG  # (the target is qubit 1)
    assert call(2, 3, 1, _lib.as_ptr(wrt)) == _lib.QSV_E_ARG  # (wrt names parameter 3)
