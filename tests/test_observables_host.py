"""Several observables per evaluation, the parts that need no GPU: the C ABI's declarations and argument errors, the shape
rule of GpuEstimator pubs, and aux operators in the EVQE solver (with an oracle-backed evaluator)."""

import ctypes as C
import re

import numpy as np
import pytest

import helpers
from queasars_amd import _lib
from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration
from queasars_amd.ir import PauliOperator
from oracle import statevector_oracle as so
from queasars_amd.circuit_evaluation.circuit_evaluation import StatevectorDevice, _diagonal_values
from queasars_amd.primitives import pub_broadcast, pub_layout

NEW_FUNCTIONS = ("qsv_observables_create", "qsv_observables_destroy", "qsv_eval_observables")


def test_new_functions_are_declared_and_bound():
    header = (helpers.ROOT / "include" / "qsv.h").read_text()
    for name in NEW_FUNCTIONS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES


def test_null_handle_is_an_argument_error_without_a_device():
    lib = _lib.load()
    out = C.c_int(0)
    assert lib.qsv_eval_observables(None, 1, 0, None, None, None, None) == _lib.QSV_E_ARG
    assert lib.qsv_observables_create(None, 1, None, None, None, None, None, C.byref(out)) == _lib.QSV_E_ARG
    assert lib.qsv_observables_destroy(None, 1) == _lib.QSV_E_ARG


@pytest.mark.parametrize(
    "observables, values, expected",
    [((), (7,), ()), ((3,), (7,), (3,)), ((2, 1), (4, 7), (2, 4)), ((3,), (2, 3, 7), (2, 3)), ((1,), (0,), (1,))],
)
def test_pub_broadcast_shapes(observables, values, expected):
    assert pub_broadcast(observables, values) == expected


def test_pub_broadcast_rejects_incompatible_shapes():
    with pytest.raises(ValueError):
        pub_broadcast((2,), (3, 7))
    with pytest.raises(ValueError):
        pub_broadcast((4, 2), (3, 1, 7))


def test_pub_layout_spreads_bindings_and_observables():
    layout = pub_layout([["a"], ["b"], ["a"]], np.asarray([[0.5, 1.0], [0.0, 2.0], [0.5, 1.0], [3.0, 3.0]]))
    assert layout.shape == (3, 4) and layout.observables == ["a", "b", "a"]
    rows = layout.rows[layout.binding_index]
    assert rows.shape == (3, 4, 2)
    np.testing.assert_array_equal(rows[1, 2], [0.5, 1.0])
    np.testing.assert_array_equal(rows[2, 3], [3.0, 3.0])
    assert len(layout.rows) == 3  # (the repeated binding is evaluated once)
    assert [[layout.observables[j] for j in row] for row in layout.observable_index.tolist()] == [["a"] * 4, ["b"] * 4, ["a"] * 4]
    wide = pub_layout(["a", "b", "c"], np.zeros((2, 3, 5)))
    assert wide.shape == (2, 3) and wide.binding_index.shape == (2, 3) and wide.observable_index.tolist() == [[0, 1, 2]] * 2


@pytest.mark.parametrize("values", [None, [], np.zeros((3, 0))])
def test_pub_layout_without_parameter_values(values):
    layout = pub_layout(["a", "b"] if values is None or len(values) == 0 else [["a"], ["b"]], values)
    assert layout.rows.shape == (1, 0)  # one empty binding
    assert layout.shape == ((2,) if values is None or len(values) == 0 else (2, 3))
    assert (layout.binding_index == 0).all()


def test_pub_layout_of_no_bindings():
    layout = pub_layout(["a"], np.zeros((0, 4)))
    assert layout.shape == (0,) and layout.rows.shape == (0, 4)


def test_diagonal_values_of_samples_match_the_oracle_table():
    rng = np.random.default_rng(4)
    n = 7
    op = PauliOperator.from_sparse_list([("I", [0], 0.75), ("Z", [2], -1.5), ("ZZ", [0, 6], 2.0), ("ZZZ", [1, 3, 5], 0.5)], n)
    table = so.diagonal_values(n, op.z_mask.tolist(), op.coeffs.real.tolist())
    states = rng.integers(0, 1 << n, size=(5, 40)).astype(np.uint64)
    np.testing.assert_allclose(_diagonal_values(op, states), table[states.astype(np.int64)], rtol=0, atol=1e-12)


def test_observable_sets_reject_what_is_not_a_pauli_operator():
    from collections import OrderedDict
    from types import SimpleNamespace

    stand_in = SimpleNamespace(_n_qubits=4, _observable_sets=OrderedDict())
    with pytest.raises(ValueError):
        StatevectorDevice._observable_set(stand_in, ["ZZII"])
    with pytest.raises(ValueError):
        StatevectorDevice._observable_set(stand_in, [PauliOperator.from_sparse_list([("Z", [4], 1.0)], 5)])


# ---- aux operators in the solver -----------------------------------------------------------------------------------


class OracleEvaluator:
    def __init__(self, operator):
        self.operator = operator
        self.observable_calls = 0

    @property
    def n_qubits(self):
        return self.operator.num_qubits

    def evaluate_circuits(self, circuits, parameter_values):
        return [helpers.oracle_expectation(c, p, self.operator) for c, p in zip(circuits, parameter_values)]


class OracleObservablesEvaluator(OracleEvaluator):
    def evaluate_observables(self, circuits, parameter_values, operators):
        self.observable_calls += 1
        return [[helpers.oracle_expectation(c, p, op) for op in operators] for c, p in zip(circuits, parameter_values)]


def hamiltonian():
    return PauliOperator.from_sparse_list(
        [("Z", [0], -1.5), ("Z", [1], -3.0), ("ZZ", [0, 1], 1.0), ("Z", [2], 1.5), ("Z", [3], 3.0), ("ZZ", [2, 3], -1.0)], 4
    )


def aux_list():
    return [
        PauliOperator.from_sparse_list([("Z", [0], 1.0)], 4),
        PauliOperator.from_sparse_list([("XY", [1, 2], 0.5), ("ZZ", [0, 3], -2.0), ("Y", [3], 0.25)], 4),
        PauliOperator.from_sparse_list([("X", [2], 1.0), ("X", [2], 1.0)], 4),
    ]


def make_config():
    return EVQEMinimumEigensolverConfiguration(
        optimizer=SPSA(maxiter=10, learning_rate=0.4, perturbation=0.3), population_size=6, max_generations=3, random_seed=5,
        n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
        use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
        parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
    )


def _same_run(a, b):
    assert a.eigenvalue == b.eigenvalue
    assert a.best_individual == b.best_individual
    assert a.generations == b.generations
    assert a.circuit_evaluations == b.circuit_evaluations
    assert a.best_expectation_values == b.best_expectation_values
    assert a.median_expectation_values == b.median_expectation_values
    assert a.mean_expectation_values == b.mean_expectation_values


def _oracle_aux(result, operators):
    ind = result.best_individual
    circuit = ind.get_parameterized_quantum_circuit()
    return [helpers.oracle_expectation(circuit, list(ind.parameter_values), op) for op in operators]


def test_aux_operators_leave_the_run_unchanged_and_are_evaluated_at_the_best_individual():
    op = hamiltonian()
    plain = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(OracleObservablesEvaluator(op))
    assert plain.aux_operators_evaluated is None
    ops = aux_list()

    evaluator = OracleObservablesEvaluator(op)
    as_list = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(evaluator, aux_operators=ops)
    _same_run(plain, as_list)
    assert evaluator.observable_calls == 1
    assert isinstance(as_list.aux_operators_evaluated, list) and len(as_list.aux_operators_evaluated) == len(ops)
    np.testing.assert_allclose(as_list.aux_operators_evaluated, _oracle_aux(as_list, ops), rtol=0, atol=1e-12)

    named = {"z0": ops[0], "mixed": ops[1], "twice_x": ops[2]}
    as_dict = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(OracleObservablesEvaluator(op), aux_operators=named)
    _same_run(plain, as_dict)
    assert isinstance(as_dict.aux_operators_evaluated, dict) and list(as_dict.aux_operators_evaluated) == list(named)
    np.testing.assert_allclose(list(as_dict.aux_operators_evaluated.values()), _oracle_aux(as_dict, ops), rtol=0, atol=1e-12)


def test_aux_operators_need_an_operator_evaluator_over_the_same_register():
    op = hamiltonian()
    with pytest.raises(ValueError):
        EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(OracleEvaluator(op), aux_operators=aux_list())
    wide = PauliOperator.from_sparse_list([("Z", [4], 1.0)], 5)
    with pytest.raises(ValueError):
        EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(OracleObservablesEvaluator(op), aux_operators={"w": wide})
