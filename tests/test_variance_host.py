"""The operator's variance, the parts that need no GPU: the two references against each other, the C ABI's declaration, the shot
noise of GpuEstimator(shots=N) on a NumPy-backed evaluator, and ``eigenvalue_variance`` in the EVQE solver."""

import re

import numpy as np
import pytest

import helpers
import variance_reference as vr
from queasars_amd import _lib
from queasars_amd.evqe.solver import EVQEMinimumEigensolver, EVQEResult
from queasars_amd.ir import CircuitIR, ParamRef, PauliOperator
from queasars_amd.primitives import GpuEstimator, pub_broadcast
from test_observables_host import OracleEvaluator, _same_run, hamiltonian, make_config


def general_operator(n: int) -> PauliOperator:
    """Strings with one, two and three Y factors among X, Z and identity terms, one coefficient with an imaginary part."""
    return PauliOperator.from_sparse_list(
        [("I", [0], 0.4), ("Z", [1], -0.7), ("ZZ", [0, n - 1], 0.9), ("X", [2], 0.6), ("Y", [0], -1.1), ("XY", [1, 3], 0.8),
         ("YY", [2, n - 1], 0.5 + 0.3j), ("YZY", [0, 1, 2], -0.45), ("YYY", [n - 3, n - 2, n - 1], 0.35), ("XZ", [n - 1, 0], 0.25)], n)


# ---- the references ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [6, 8])
@pytest.mark.parametrize("kind", ["ising", "general"])
def test_dense_and_matrix_free_references_agree(n, kind):
    op = helpers.random_ising_operator(n, seed=n) if kind == "ising" else general_operator(n)
    _, _, states = vr.population(n, 3, 4, 2)
    for state in states:
        dense, free = vr.dense_moments(op, state), vr.moments(op, state)
        assert abs(dense[0] - free[0]) <= 1e-12 and abs(dense[1] - free[1]) <= 1e-12, (dense, free)
        assert free[1] > 1e-3  # (no eigenstate: the agreement is not 0 = 0)


def test_matrix_free_reference_reads_labels_as_the_oracle_does():
    n = 7
    op = general_operator(n)
    circuits, params, states = vr.population(n, 3, 4, 2)
    for c, p, state in zip(circuits, params, states):
        assert abs(vr.moments(op, state)[0] - helpers.oracle_expectation(c, p, op)) <= 1e-13


def test_references_on_an_eigenstate_and_a_known_spread():
    state = np.zeros(8, dtype=np.complex128)
    state[5] = 1.0
    diagonal = PauliOperator.from_sparse_list([("Z", [0], 1.5), ("ZZ", [1, 2], -2.0), ("I", [0], 0.25)], 3)
    assert vr.moments(diagonal, state) == pytest.approx((-1.5 + 2.0 + 0.25, 0.0), abs=1e-15)
    field = PauliOperator.from_sparse_list([("X", [0], 0.5), ("X", [1], -2.0), ("X", [2], 1.0)], 3)
    zero = np.zeros(8, dtype=np.complex128)
    zero[0] = 1.0
    assert vr.moments(field, zero) == pytest.approx((0.0, 0.25 + 4.0 + 1.0), abs=1e-15)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------


def test_the_entry_point_is_declared_and_bound():
    header = (helpers.ROOT / "include" / "qsv.h").read_text()
    assert re.search(r"\bint qsv_variance_circuits\(", header)
    assert "qsv_variance_circuits" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["qsv_variance_circuits"][1]) == 7
    assert _lib.load().qsv_variance_circuits(None, 0, None, None, None, None, None) == _lib.QSV_E_ARG  # (no handle)


# ---- GpuEstimator(shots=N) -----------------------------------------------------------------------------------------------


class NumpyEvaluator:
    """What GpuEstimator asks of an OperatorCircuitEvaluator, from the NumPy oracle; every call is noted in `log`."""

    def __init__(self, operator, log):
        self.operator, self.log = operator, log

    def _pairs(self, circuits, values):
        return [vr.moments(self.operator, helpers.oracle_state(c, v)) for c, v in zip(circuits, values)]

    def evaluate_circuits(self, circuits, values):
        self.log.append(("evaluate_circuits", len(circuits)))
        return [p[0] for p in self._pairs(circuits, values)]

    def evaluate_variances(self, circuits, values, with_values=False):
        self.log.append(("evaluate_variances", len(circuits)))
        pairs = self._pairs(circuits, values)
        variances = [p[1] for p in pairs]
        return ([p[0] for p in pairs], variances) if with_values else variances


class StubEstimator(GpuEstimator):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.log = []

    def _evaluator(self, operator):
        return NumpyEvaluator(operator, self.log)


def _circuit(n=3):
    c = CircuitIR(n)
    p = [ParamRef(0), ParamRef(1)]
    return c.u(p[0], 0.3, -0.2, 0).cu3(0.9, 0.1, 0.4, 0, 1).u(p[1], -0.5, 0.7, 2).cu3(1.3, 0.2, -0.1, 2, 1)


def _observables(n=3):
    return [PauliOperator.from_sparse_list([("X", [0], 1.0), ("ZZ", [1, 2], 0.5)], n),
            PauliOperator.from_sparse_list([("Y", [1], -0.75), ("Z", [0], 1.25), ("XX", [0, 2], 0.5)], n)]


BINDINGS = np.asarray([[0.4, 1.1], [2.0, -0.6], [0.4, 1.1]])


def _exact(circuit, op, binding):
    return vr.moments(op, helpers.oracle_state(circuit, list(binding)))


def test_shots_give_each_entry_its_own_standard_deviation_and_draw():
    circuit, (op_a, op_b) = _circuit(), _observables()
    shots, seed = 1024, 7
    estimator = StubEstimator(shots=shots, seed=seed)
    pubs = [(circuit, op_a, BINDINGS[0]), (circuit, [[op_a], [op_b]], BINDINGS), (circuit, op_b, BINDINGS[1], 0.5)]
    results = estimator.run(pubs, precision=0.25).result()
    draws = np.random.default_rng(seed)
    expected = [np.asarray(_exact(circuit, op_a, BINDINGS[0])),
                np.asarray([[_exact(circuit, op, b) for b in BINDINGS] for op in (op_a, op_b)]),
                np.asarray(_exact(circuit, op_b, BINDINGS[1]))]
    for result, moments in zip(results, expected):
        exact, variances = moments[..., 0], moments[..., 1]
        stds = result.data.stds
        assert stds.shape == result.data.evs.shape == exact.shape
        np.testing.assert_allclose(stds, np.sqrt(np.maximum(variances, 0.0) / shots), rtol=0, atol=1e-15)
        assert (stds > 1e-3).all()
        normal = draws.standard_normal(size=exact.shape)
        np.testing.assert_allclose((result.data.evs - exact) / stds, normal, rtol=0, atol=1e-10)
        assert result.metadata["shots"] == shots
    assert results[1].data.evs.shape == pub_broadcast((2, 1), BINDINGS.shape) == (2, 3)
    # one call per distinct observable of the array pub over its two distinct bindings, one per operator of the single pubs
    assert sorted(estimator.log) == [("evaluate_variances", 1), ("evaluate_variances", 1), ("evaluate_variances", 2), ("evaluate_variances", 2)]


def test_a_negative_variance_from_rounding_is_no_noise():
    class Rounded(NumpyEvaluator):
        def evaluate_variances(self, circuits, values, with_values=False):
            return ([1.0] * len(circuits), [-1e-17] * len(circuits))

    class Estimator(GpuEstimator):
        def _evaluator(self, operator):
            return Rounded(operator, [])

    result = Estimator(shots=10, seed=1).run([(_circuit(), _observables()[0], BINDINGS[0])]).result()[0]
    assert float(result.data.stds) == 0.0 and float(result.data.evs) == 1.0


def test_shots_must_be_positive():
    for shots in (0, -5):
        with pytest.raises(ValueError):
            GpuEstimator(shots=shots)


def test_without_shots_the_calls_and_the_draws_are_todays():
    circuit, (op_a, op_b) = _circuit(), _observables()
    estimator = StubEstimator(seed=3)
    pubs = [(circuit, op_a, BINDINGS[0]), (circuit, op_b, BINDINGS[1], 0.5), (circuit, op_a, BINDINGS[1])]
    results = estimator.run(pubs, precision=0.1).result()
    assert estimator.log == [("evaluate_circuits", 2), ("evaluate_circuits", 1)]  # (batched per distinct operator; no variance call)
    draws = np.random.default_rng(3)
    for result, (_, op, binding, *own) in zip(results, pubs):
        p = own[0] if own else 0.1
        assert float(result.data.evs) == _exact(circuit, op, binding)[0] + float(draws.normal(0.0, p))
        assert result.metadata == {"target_precision": p}
        assert not hasattr(result.data, "stds")
    exact = StubEstimator(seed=3).run(pubs[:1]).result()[0]
    assert float(exact.data.evs) == _exact(circuit, op_a, BINDINGS[0])[0] and exact.metadata == {"target_precision": 0.0}


# ---- the solver ----------------------------------------------------------------------------------------------------------


class OracleVarianceEvaluator(OracleEvaluator):
    variance_calls = 0

    def evaluate_variances(self, circuits, parameter_values, with_values=False):
        self.variance_calls += 1
        pairs = [vr.moments(self.operator, helpers.oracle_state(c, p)) for c, p in zip(circuits, parameter_values)]
        variances = [p[1] for p in pairs]
        return ([p[0] for p in pairs], variances) if with_values else variances


def test_the_result_has_no_variance_unless_asked_for():
    individual = object()
    assert EVQEResult(eigenvalue=0.0, best_individual=individual, generations=0, circuit_evaluations=[]).eigenvalue_variance is None


def test_eigenvalue_variance_needs_an_evaluator_that_has_it():
    with pytest.raises(ValueError, match="evaluate_variances"):
        EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(OracleEvaluator(hamiltonian()), eigenvalue_variance=True)


def test_eigenvalue_variance_is_one_call_at_the_best_individual_and_leaves_the_run_unchanged():
    op = hamiltonian()
    plain_evaluator = OracleVarianceEvaluator(op)
    plain = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(plain_evaluator)
    assert plain.eigenvalue_variance is None and plain_evaluator.variance_calls == 0
    evaluator = OracleVarianceEvaluator(op)
    asked = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(evaluator, eigenvalue_variance=True)
    _same_run(plain, asked)
    assert evaluator.variance_calls == 1
    best = asked.best_individual
    state = helpers.oracle_state(best.get_parameterized_quantum_circuit(), list(best.parameter_values))
    assert asked.eigenvalue_variance == pytest.approx(vr.dense_moments(op, state)[1], abs=1e-12)
    assert asked.eigenvalue_variance >= -1e-12
