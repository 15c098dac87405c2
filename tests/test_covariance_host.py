"""The covariance matrix of an observable set, the parts that need no GPU: the two references against each other and their
symmetry and positivity, the C ABI's declaration, the Python entry points' argument checks, GpuEstimator(shots=N,
joint_moments=True) on a NumPy-backed evaluator, and ``aux_operators_covariance`` in the EVQE solver."""

import re

import numpy as np
import pytest

import covariance_reference as cr
import helpers
import variance_reference as vr
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe.solver import EVQEMinimumEigensolver, EVQEResult
from queasars_amd.ir import PauliOperator
from queasars_amd.primitives import GpuEstimator, pub_broadcast
from test_observables_host import OracleObservablesEvaluator, _same_run, aux_list, hamiltonian, make_config
from test_variance_host import BINDINGS, NumpyEvaluator, _circuit, _exact, _observables, general_operator


def observables(n: int) -> list:
    return [general_operator(n), helpers.random_ising_operator(n, seed=n), helpers.random_pauli_operator(n, 9, seed=3),
            PauliOperator.from_sparse_list([("X", [0], 1.0), ("X", [0], 0.5), ("YY", [1, n - 1], -0.25)], n),
            helpers.random_ising_operator(n, seed=n)]


# ---- the references ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [6, 8])
def test_dense_and_matrix_free_references_agree(n):
    ops = observables(n)
    _, _, states = cr.population(n, 3, 4, 2)
    for state in states:
        (dense_values, dense), (free_values, free) = cr.dense_moments(ops, state), cr.moments(ops, state)
        assert np.abs(dense_values - free_values).max() <= 1e-12 and np.abs(dense - free).max() <= 1e-11
        assert np.abs(free).min() > 1e-6  # (no entry vanishes: the agreement is not 0 = 0)
        for k, op in enumerate(ops):  # the diagonal is the variance reference's number
            assert abs(free[k, k] - vr.moments(op, state)[1]) <= 1e-11
        assert free[1, 4] == pytest.approx(free[1, 1], abs=1e-12)  # (observables 1 and 4 are the same operator)


@pytest.mark.parametrize("n", [3, 7, 10])
def test_the_reference_is_symmetric_and_positive_semidefinite_on_random_states(n):
    ops = observables(n)
    rng = np.random.default_rng(n)
    for _ in range(4):
        state = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
        state /= np.linalg.norm(state)
        _, cov = cr.moments(ops, state)
        scale = float(np.outer(cr.spreads(ops), cr.spreads(ops)).max())
        assert np.abs(cov - cov.T).max() <= 1e-14 * scale  # (a matrix product's rounding; the device's matrix is symmetric bit for bit)
        assert np.linalg.eigvalsh(cov).min() >= -1e-13 * scale
        w = rng.uniform(-1.0, 1.0, size=len(ops))
        assert w @ cov @ w == pytest.approx(vr.moments(cr.combined(ops, w), state)[1], abs=1e-11 * scale)


def test_the_reference_on_known_states():
    n = 4
    plus = np.full(1 << n, 0.25, dtype=np.complex128)
    z = [PauliOperator.from_sparse_list([("Z", [q], 1.0)], n) for q in range(n)]
    x = [PauliOperator.from_sparse_list([("X", [q], 1.0)], n) for q in range(n)]
    assert np.abs(cr.moments(z, plus)[1] - np.eye(n)).max() <= 1e-15
    assert np.abs(cr.moments(x, plus)[1]).max() <= 1e-15
    bell = np.zeros(1 << n, dtype=np.complex128)
    bell[0] = bell[3] = np.sqrt(0.5)
    values, cov = cr.moments([z[0], z[1], PauliOperator.from_sparse_list([("ZZ", [0, 1], 1.0)], n)], bell)
    assert np.abs(values - [0.0, 0.0, 1.0]).max() <= 1e-15
    assert cov[0, 1] == pytest.approx(1.0, abs=1e-15) and np.abs(cov[2]).max() <= 1e-15 and np.abs(cov[:, 2]).max() <= 1e-15


# ---- the C ABI ---------------------------------------------------------------------------------------------------------


def test_the_entry_point_is_declared_and_bound():
    header = (helpers.ROOT / "include" / "qsv.h").read_text()
    assert re.search(r"\bint qsv_observables_covariance\(", header)
    assert re.search(r"#define QSV_COVARIANCE_MAX_OBSERVABLES 64\b", header)
    assert StatevectorDevice.MAX_COVARIANCE_OBSERVABLES == 64
    assert "qsv_observables_covariance" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["qsv_observables_covariance"][1]) == 8
    assert _lib.load().qsv_observables_covariance(None, 0, 0, None, None, None, None, None) == _lib.QSV_E_ARG  # (no handle)


# ---- argument checks that come before the library ------------------------------------------------------------------------


def test_the_device_checks_its_arguments_before_it_calls_the_library():
    dev = object.__new__(StatevectorDevice)  # (no handle: every check below comes before the library is called)
    dev._n_qubits = 3
    ops = _observables()
    with pytest.raises(ValueError, match="same length"):
        dev.observable_covariances([_circuit()], [], ops)
    with pytest.raises(ValueError, match="at least one"):
        dev.observable_covariances([], [], [])
    with pytest.raises(ValueError, match="64"):
        dev.observable_covariances([], [], [ops[0]] * 65)
    with pytest.raises(ValueError, match="PauliOperator"):
        dev.observable_covariances([], [], [ops[0], "ZZI"])
    with pytest.raises(ValueError, match="qubits"):
        dev.observable_covariances([], [], [PauliOperator.from_sparse_list([("Z", [0], 1.0)], 4)])
    assert callable(getattr(OperatorCircuitEvaluator, "evaluate_covariances", None))


# ---- GpuEstimator(shots=N, joint_moments=True) -----------------------------------------------------------------------------


class NumpyCovarianceEvaluator(NumpyEvaluator):
    def evaluate_covariances(self, circuits, values, operators, with_values=False):
        self.log.append(("evaluate_covariances", len(circuits), len(operators)))
        exact, cov = cr.reference(list(operators), [helpers.oracle_state(c, v) for c, v in zip(circuits, values)])
        return (exact, cov) if with_values else cov


class StubEstimator(GpuEstimator):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.log = []

    def _evaluator(self, operator):
        return NumpyCovarianceEvaluator(operator, self.log)


def test_joint_moments_take_an_array_pubs_numbers_from_one_call():
    circuit, (op_a, op_b) = _circuit(), _observables()
    shots, seed = 1024, 7
    pubs = [(circuit, op_a, BINDINGS[0]), (circuit, [[op_a], [op_b]], BINDINGS), (circuit, op_b, BINDINGS[1], 0.5)]
    estimator = StubEstimator(shots=shots, seed=seed, joint_moments=True)
    results = estimator.run(pubs, precision=0.25).result()
    default = StubEstimator(shots=shots, seed=seed)
    for result, other in zip(results, default.run(pubs, precision=0.25).result()):
        assert result.data.stds.shape == result.data.evs.shape == other.data.evs.shape
        np.testing.assert_allclose(result.data.stds, other.data.stds, rtol=0, atol=1e-13)
        np.testing.assert_allclose(result.data.evs, other.data.evs, rtol=0, atol=1e-12)  # (the same draws, entry by entry)
        assert result.metadata == other.metadata == {"target_precision": 0.0, "shots": shots}
    array = results[1]
    assert array.data.evs.shape == pub_broadcast((2, 1), BINDINGS.shape) == (2, 3)
    expected = np.asarray([[_exact(circuit, op, b) for b in BINDINGS] for op in (op_a, op_b)])
    np.testing.assert_allclose(array.data.stds, np.sqrt(expected[..., 1] / shots), rtol=0, atol=1e-13)
    # the array pub: one call over its two distinct bindings and two distinct observables; the single pubs as before
    assert sorted(estimator.log) == [("evaluate_covariances", 2, 2), ("evaluate_variances", 1), ("evaluate_variances", 1)]
    assert ("evaluate_covariances", 2, 2) not in default.log and len(default.log) == 4


def test_joint_moments_split_more_observables_than_a_set_holds():
    circuit = _circuit()
    rng = np.random.default_rng(0)
    ops = [PauliOperator.from_sparse_list([("X", [0], float(c)), ("ZZ", [1, 2], 0.5)], 3) for c in rng.uniform(0.5, 1.5, size=70)]
    estimator = StubEstimator(shots=100, seed=1, joint_moments=True)
    result = estimator.run([(circuit, ops, BINDINGS[0])]).result()[0]
    assert result.data.stds.shape == (70,)
    assert estimator.log == [("evaluate_covariances", 1, 64), ("evaluate_covariances", 1, 6)]
    expected = np.asarray([_exact(circuit, op, BINDINGS[0])[1] for op in ops])
    np.testing.assert_allclose(result.data.stds, np.sqrt(expected / 100), rtol=0, atol=1e-13)


def test_joint_moments_belong_to_the_shot_noise():
    with pytest.raises(ValueError, match="shots"):
        GpuEstimator(joint_moments=True)
    assert GpuEstimator(shots=5)._joint_moments is False


# ---- the solver ----------------------------------------------------------------------------------------------------------


class OracleCovarianceEvaluator(OracleObservablesEvaluator):
    covariance_calls = 0

    def evaluate_covariances(self, circuits, parameter_values, operators, with_values=False):
        self.covariance_calls += 1
        values, cov = cr.reference(list(operators), [helpers.oracle_state(c, p) for c, p in zip(circuits, parameter_values)])
        return (values, cov) if with_values else cov


def test_the_result_has_no_covariance_unless_asked_for():
    result = EVQEResult(eigenvalue=0.0, best_individual=object(), generations=0, circuit_evaluations=[])
    assert result.aux_operators_covariance is None and result.aux_operators_variance is None


def test_aux_operators_covariance_needs_aux_operators_and_an_evaluator_that_has_it():
    solver = EVQEMinimumEigensolver(make_config())
    with pytest.raises(ValueError, match="aux_operators"):
        solver.compute_minimum_eigenvalue(OracleCovarianceEvaluator(hamiltonian()), aux_operators_covariance=True)
    with pytest.raises(ValueError, match="aux_operators"):
        solver.compute_minimum_eigenvalue(OracleCovarianceEvaluator(hamiltonian()), aux_operators=[], aux_operators_covariance=True)
    with pytest.raises(ValueError, match="evaluate_covariances"):
        solver.compute_minimum_eigenvalue(OracleObservablesEvaluator(hamiltonian()), aux_operators=aux_list(), aux_operators_covariance=True)


def test_aux_operators_covariance_is_one_call_at_the_best_individual_and_leaves_the_run_unchanged():
    op, ops = hamiltonian(), aux_list()
    plain_evaluator = OracleCovarianceEvaluator(op)
    plain = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(plain_evaluator, aux_operators=ops)
    assert plain.aux_operators_covariance is None and plain.aux_operators_variance is None and plain_evaluator.covariance_calls == 0
    evaluator = OracleCovarianceEvaluator(op)
    asked = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(evaluator, aux_operators=ops, aux_operators_covariance=True)
    _same_run(plain, asked)
    assert asked.aux_operators_evaluated == plain.aux_operators_evaluated
    assert evaluator.covariance_calls == 1
    best = asked.best_individual
    state = helpers.oracle_state(best.get_parameterized_quantum_circuit(), list(best.parameter_values))
    matrix = asked.aux_operators_covariance
    assert isinstance(matrix, np.ndarray) and matrix.shape == (3, 3) and matrix.dtype == np.float64
    assert np.abs(matrix - cr.dense_moments(ops, state)[1]).max() <= 1e-12
    assert isinstance(asked.aux_operators_variance, list) and asked.aux_operators_variance == [float(v) for v in np.diagonal(matrix)]
    # a dict: the matrix in list(aux_operators) order, the variances under the dict's keys
    named = {"second": ops[1], "first": ops[0], "third": ops[2]}
    by_name = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(
        OracleCovarianceEvaluator(op), aux_operators=named, aux_operators_covariance=True)
    _same_run(plain, by_name)
    order = [1, 0, 2]
    assert np.abs(by_name.aux_operators_covariance - matrix[np.ix_(order, order)]).max() <= 1e-13
    assert list(by_name.aux_operators_variance) == ["second", "first", "third"]
    assert by_name.aux_operators_variance == pytest.approx({"second": matrix[1, 1], "first": matrix[0, 0], "third": matrix[2, 2]}, abs=1e-13)
    assert list(by_name.aux_operators_variance.values()) == [float(v) for v in np.diagonal(by_name.aux_operators_covariance)]
