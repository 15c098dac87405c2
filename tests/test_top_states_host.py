"""Exact readout, the parts that need no GPU: the host restatement of the selection (tests/top_states_reference.py) on
hand-made arrays, ``most_probable_states`` and the solver's ``eigenstate`` / ``eigenstate_values`` with an oracle-backed
stand-in for the device, and the C ABI's declaration."""

import re

import numpy as np
import pytest

import helpers
from oracle import statevector_oracle as so
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import StatevectorDevice, most_probable_states
from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration, EVQEResult
from queasars_amd.ir import CircuitIR, PauliOperator
from top_states_reference import TOL_FP64, check_top, expected_top


# ---- the reference helper ------------------------------------------------------------------------------------------


def test_expected_top_orders_by_probability_then_index():
    probs = np.asarray([0.1, 0.3, 0.0, 0.3, 0.2, 0.0, 0.1, 0.0])
    states, got = expected_top(probs, 8)
    assert states.dtype == np.uint64 and states.tolist() == [1, 3, 4, 0, 6, 2, 5, 7]
    assert got.tolist() == [0.3, 0.3, 0.2, 0.1, 0.1, 0.0, 0.0, 0.0]
    states, got = expected_top(probs, 2)
    assert states.tolist() == [1, 3] and got.tolist() == [0.3, 0.3]
    # a basis state: one and then zeros in index order (the tie rule)
    basis = np.zeros(16)
    basis[5] = 1.0
    assert expected_top(basis, 4)[0].tolist() == [5, 0, 1, 2]
    for k in (0, 9):
        with pytest.raises(ValueError):
            expected_top(probs, k)


def test_check_top_accepts_the_expected_answer_and_rounding_near_ties():
    rng = np.random.default_rng(3)
    probs = rng.random(64)
    probs[[7, 9, 40]] = probs[11]  # exact ties
    probs /= probs.sum()
    for k in (1, 5, 64):
        states, got = expected_top(probs, k)
        check_top(states, got, probs, k, TOL_FP64)
    # a device that rounds differently may swap two states that are within tol of each other, also across the cut
    probs = np.asarray([0.5, 0.25 + 4e-14, 0.25 - 4e-14, 0.0])
    check_top(np.asarray([0, 2, 1], dtype=np.uint64), np.asarray([0.5, 0.25, 0.25 - 1e-14]), probs, 3, TOL_FP64)
    check_top(np.asarray([0, 2], dtype=np.uint64), np.asarray([0.5, 0.25]), probs, 2, TOL_FP64)


@pytest.mark.parametrize(
    "states, got, why",
    [
        ([1, 1, 4], [0.3, 0.3, 0.2], "twice"),
        ([1, 3, 8], [0.3, 0.3, 0.2], "out of range"),
        ([1, 3, 4], [0.3, 0.3, 0.2 + 1e-9], "wrong probability"),
        ([1, 4, 3], [0.3, 0.2, 0.3], "not sorted"),
        ([3, 1, 4], [0.3, 0.3, 0.2], "tie in descending index"),
        ([1, 3, 0], [0.3, 0.3, 0.1], "state 4 left out"),
    ],
)
def test_check_top_rejects_wrong_answers(states, got, why):
    probs = np.asarray([0.1, 0.3, 0.0, 0.3, 0.2, 0.0, 0.1, 0.0])
    with pytest.raises(AssertionError):
        check_top(np.asarray(states, dtype=np.uint64), np.asarray(got), probs, 3, TOL_FP64)


# ---- the C ABI and the Python layer --------------------------------------------------------------------------------


def test_qsv_top_states_is_declared_and_bound():
    header = (helpers.ROOT / "include" / "qsv.h").read_text()
    assert re.search(r"\bint qsv_top_states\(", header)
    assert "qsv_top_states" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["qsv_top_states"][1]) == 9
    assert StatevectorDevice.MAX_TOP_STATES == 1024


def test_null_handle_is_an_argument_error_without_a_device():
    assert _lib.load().qsv_top_states(None, 0, None, None, None, 1, None, None, None) == _lib.QSV_E_ARG


class OracleDevice:
    """What the solver and most_probable_states use of a StatevectorDevice, from the oracle's probabilities."""

    def __init__(self, n_qubits, table=None):
        self.n_qubits = n_qubits
        self.table = table
        self.calls = []

    def top_states(self, circuits, parameter_values, k, with_values=False):
        self.calls.append((len(circuits), k, with_values))
        picked = [expected_top(so.probabilities(helpers.oracle_state(c, p)), k) for c, p in zip(circuits, parameter_values)]
        states = np.asarray([s for s, _ in picked], dtype=np.uint64).reshape(len(picked), k)
        probs = np.asarray([p for _, p in picked], dtype=np.float64).reshape(len(picked), k)
        return states, probs, self.table[states.astype(np.int64)] if with_values else None


def test_most_probable_states_formats_bitstrings_with_qubit_zero_last():
    n = 5
    x = (np.pi, 0.0, np.pi)
    flipped = CircuitIR(n).u(*x, 0).u(*x, 3)  # the basis state with qubits 0 and 3 set: index 9
    half = CircuitIR(n).u(np.pi / 2, 0.0, np.pi, 4)  # (|00000> + |10000>) / sqrt 2
    idle = CircuitIR(n).id(2)
    device = OracleDevice(n)
    got = most_probable_states(device, [flipped, half, idle], [[], [], []], 3)
    assert device.calls == [(3, 3, False)]
    assert [len(row) for row in got] == [3, 3, 3]
    assert next(iter(got[0])) == "01001" and got[0]["01001"] == pytest.approx(1.0, abs=1e-15)
    assert set(list(got[1])[:2]) == {"00000", "10000"} and list(got[1])[2] == "00001"  # (then exact zeros in index order)
    assert got[1]["00000"] == pytest.approx(0.5, abs=1e-15) and got[1]["10000"] == pytest.approx(0.5, abs=1e-15)
    assert got[2] == {"00000": 1.0, "00001": 0.0, "00010": 0.0} and list(got[2]) == ["00000", "00001", "00010"]
    assert all(type(v) is float for row in got for v in row.values())


# ---- the solver ----------------------------------------------------------------------------------------------------


def hamiltonian():
    return PauliOperator.from_sparse_list(
        [("Z", [0], -1.5), ("Z", [1], -3.0), ("ZZ", [0, 1], 1.0), ("Z", [2], 1.5), ("Z", [3], 3.0), ("ZZ", [2, 3], -1.0)], 4
    )


def make_config():
    return EVQEMinimumEigensolverConfiguration(
        optimizer=SPSA(maxiter=10, learning_rate=0.4, perturbation=0.3), population_size=6, max_generations=3, random_seed=5,
        n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
        use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
        parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
    )


class OracleEvaluator:
    """An evaluator without a device."""

    def __init__(self, operator):
        self.operator = operator

    @property
    def n_qubits(self):
        return self.operator.num_qubits

    def evaluate_circuits(self, circuits, parameter_values):
        return [helpers.oracle_expectation(c, p, self.operator) for c, p in zip(circuits, parameter_values)]


class DeviceEvaluator(OracleEvaluator):
    """... with a device and nothing else: the solver reads the states from the device, without values."""

    def __init__(self, operator):
        super().__init__(operator)
        self.statevector_device = OracleDevice(operator.num_qubits)


class OperatorDeviceEvaluator(DeviceEvaluator):
    """... and with a top_states of its own, as the operator evaluators have: the values of a diagonal operator come along."""

    def __init__(self, operator):
        super().__init__(operator)
        self.statevector_device.table = so.diagonal_values(operator.num_qubits, operator.z_mask.tolist(), operator.coeffs.real.tolist())

    def top_states(self, circuits, parameter_values, k):
        return self.statevector_device.top_states(circuits, parameter_values, k, with_values=self.operator.is_diagonal())


def _same_run(a, b):
    assert a.eigenvalue == b.eigenvalue
    assert a.best_individual == b.best_individual
    assert a.generations == b.generations
    assert a.circuit_evaluations == b.circuit_evaluations
    assert a.best_expectation_values == b.best_expectation_values


def test_result_fields_default_to_none():
    fields = EVQEResult.__dataclass_fields__
    assert fields["eigenstate"].default is None and fields["eigenstate_values"].default is None


def test_eigenstate_is_read_once_after_the_run_and_leaves_it_unchanged():
    op = hamiltonian()
    plain_evaluator = OperatorDeviceEvaluator(op)
    plain = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(plain_evaluator)
    assert plain.eigenstate is None and plain.eigenstate_values is None
    assert plain_evaluator.statevector_device.calls == []

    evaluator = OperatorDeviceEvaluator(op)
    result = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(evaluator, eigenstate_states=5)
    _same_run(plain, result)  # (no random stream used, not counted in circuit_evaluations)
    assert evaluator.statevector_device.calls == [(1, 5, True)]
    best = result.best_individual
    probs = so.probabilities(helpers.oracle_state(best.get_parameterized_quantum_circuit(), list(best.parameter_values)))
    states, want = expected_top(probs, 5)
    assert list(result.eigenstate) == [format(int(s), "04b") for s in states]
    assert list(result.eigenstate.values()) == want.tolist()
    table = evaluator.statevector_device.table
    assert list(result.eigenstate_values) == list(result.eigenstate)
    assert list(result.eigenstate_values.values()) == [float(table[int(s)]) for s in states]

    # an evaluator that only has a device: the states without values
    bare = DeviceEvaluator(op)
    from_device = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(bare, eigenstate_states=5)
    _same_run(plain, from_device)
    assert bare.statevector_device.calls == [(1, 5, False)]
    assert from_device.eigenstate == result.eigenstate and from_device.eigenstate_values is None

    # a non-diagonal operator: no values either
    general = PauliOperator.from_sparse_list([("Z", [0], 1.0), ("X", [1], 0.5)], 4)
    mixed = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(OperatorDeviceEvaluator(general), eigenstate_states=2)
    assert len(mixed.eigenstate) == 2 and mixed.eigenstate_values is None


def test_eigenstate_needs_an_evaluator_with_a_device():
    with pytest.raises(ValueError):
        EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(OracleEvaluator(hamiltonian()), eigenstate_states=4)
