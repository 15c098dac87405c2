"""The Fubini-Study metric without a device: tests/metric_reference.py's two constructions against each other,
against the closed form of one ``u`` gate and against second differences of the fidelity; the ``NaturalGradient`` optimiser on a
stand-in evaluator; and ``metric_tensors`` of the evaluators on tests/test_evaluator_layer_host.py's recording device, held to
the two rules that file holds every ``evaluate_*`` method to (it is behind the initial state per call; it installs no operator)."""

import math

import numpy as np
import pytest

import circuit_families as cf
import dense_gradient
import metric_reference as mr
import test_evaluator_layer_host as layer
from queasars_amd.evqe import solver
from queasars_amd.evqe.solver import NaturalGradient
from queasars_amd.ir import CircuitIR, ParamRef, PauliOperator

CASES = {
    "ladder(6)": lambda: cf.ladder(6),
    "generic(6, 24)": lambda: cf.generic(6, 24),
    "generic(11, 40)": lambda: cf.generic(11, 40),
    "all_pairs(5)": lambda: cf.all_pairs(5),
    "star(5)": lambda: cf.star(5),
    "generic(4, 30), much shared and literal": lambda: cf.generic(4, 30, share=0.4, literal=0.3, seed=3),
}


def case(name):
    circuit, values = CASES[name]()
    return circuit, values[:circuit.num_parameters]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_constructions_agree(name):
    circuit, values = case(name)
    back, fore = mr.backward(circuit, values), mr.forward(circuit, values)
    assert back.shape == (circuit.num_parameters,) * 2
    err = float(np.abs(back - fore).max())
    print(f"{name}: {circuit.num_parameters} parameters, largest |backward - forward| {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("name", sorted(CASES))
def test_symmetric_and_positive_semidefinite(name):
    circuit, values = case(name)
    g = mr.backward(circuit, values)
    assert np.abs(g - g.T).max() <= 1e-15
    assert np.linalg.eigvalsh(0.5 * (g + g.T)).min() >= -1e-12


def test_one_u_gate_on_the_zero_state():
    """psi = (cos(theta/2), e^(i phi) sin(theta/2)): G = diag(1/4, sin^2(theta)/4, 0) -- lambda does nothing to |0>."""
    circuit = CircuitIR(1).u(ParamRef(0), ParamRef(1), ParamRef(2), 0)
    for theta, phi, lam in [(0.7, -1.1, 2.3), (2.9, 0.4, -0.2), (0.0, 1.0, 1.0)]:
        want = np.diag([0.25, math.sin(theta) ** 2 / 4.0, 0.0])
        for build in (mr.backward, mr.forward):
            assert np.abs(build(circuit, [theta, phi, lam]) - want).max() <= 1e-15


@pytest.mark.parametrize("name", ["ladder(6)", "generic(6, 24)", "all_pairs(5)"])
def test_the_quadratic_form_is_the_second_difference_of_the_fidelity(name):
    circuit, values = case(name)
    g = mr.backward(circuit, values)
    rng = np.random.default_rng(5)
    for _ in range(3):
        v = rng.normal(size=circuit.num_parameters)
        v /= np.linalg.norm(v)
        want = mr.fidelity_second_difference(circuit, values, v, eps=1e-3)
        # (the difference quotient's own error: O(eps^2) times fourth derivatives of a function bounded by 1, and rounding / eps^2)
        assert abs(float(v @ g @ v) - want) <= 5e-6 * max(1.0, float(np.sum(mr.slot_counts(circuit))) ** 2 / 100.0)


def test_shared_literal_and_unread_parameters():
    circuit, values = cf.generic(5, 40, share=0.4, literal=0.3, seed=11)
    counts = mr.slot_counts(circuit)
    assert counts.max() >= 2 and any(int(row["p_theta"]) < 0 for row in circuit.packed())  # (shared and literal slots)
    circuit.declare_parameters(circuit.num_parameters + 2)  # (two parameters nothing reads)
    values = values[:circuit.num_parameters - 2] + [0.3, -0.4]
    back, fore = mr.backward(circuit, values), mr.forward(circuit, values)
    assert np.abs(back - fore).max() <= 1e-12
    assert not back[-2:].any() and not back[:, -2:].any()
    assert back[int(np.argmax(counts)), int(np.argmax(counts))] > 0
    # a subset, in another order and with a parameter named twice, is that submatrix of the full one
    wrt = [3, 0, circuit.num_parameters - 1, 3]
    assert np.abs(mr.backward(circuit, values, wrt) - back[np.ix_(wrt, wrt)]).max() <= 1e-14
    assert np.abs(mr.forward(circuit, values, wrt) - back[np.ix_(wrt, wrt)]).max() <= 1e-12


# ---- the optimiser ----------------------------------------------------------------------------------------------------------


class DenseEvaluator:
    """Gradients from tests/dense_gradient.py and metrics from tests/metric_reference.py, with what the driver asked for."""

    n_qubits = 2
    gradient_method = "parameter_shift"

    def __init__(self, operator):
        self.h = dense_gradient.dense_operator(operator)
        self.gradient_calls, self.metric_calls = [], []

    def value(self, circuit, point):
        return dense_gradient.expectation(circuit, point, self.h)

    def evaluate_gradients(self, circuits, parameter_values, wrt=None):
        self.gradient_calls.append((list(circuits), [list(p) for p in parameter_values], wrt))
        return [dense_gradient.gradient(c, p, self.h)[list(w)] for c, p, w in zip(circuits, parameter_values, wrt)]

    def metric_tensors(self, circuits, parameter_values, wrt=None):
        self.metric_calls.append((list(circuits), [list(p) for p in parameter_values], wrt))
        return [mr.backward(c, p, w) for c, p, w in zip(circuits, parameter_values, wrt)]


def two_qubit_circuit():
    return CircuitIR(2).u(ParamRef(0), ParamRef(1), 0.0, 0).u(ParamRef(2), 0.3, 0.0, 1).cu3(ParamRef(3), 0.0, 0.0, 0, 1)


OPERATOR = PauliOperator(["ZZ", "XI", "IX"], [1.0, 0.5, -0.7])


def test_a_step_is_the_regularised_solve():
    circuit, x0 = two_qubit_circuit(), [0.4, -0.3, 1.1, 0.6]
    optimizer = NaturalGradient(maxiter=1, learning_rate=0.2, regularization=1e-2)
    evaluator = DenseEvaluator(OPERATOR)
    run = optimizer.new_run(x0, seed=None)
    solver._minimize_batched(evaluator, [(circuit, run)])
    g, metric = dense_gradient.gradient(circuit, x0, evaluator.h), mr.backward(circuit, x0)
    want = np.asarray(x0) - 0.2 * np.linalg.solve(metric + 1e-2 * np.eye(4), g)
    assert np.abs(run.x - want).max() <= 1e-15 and run.done and run.iteration == 1
    assert run.nfev == sum(circuit.gradient_terms())
    assert len(evaluator.gradient_calls) == len(evaluator.metric_calls) == 1


def test_runs_advance_together_and_stop_each_on_its_own():
    circuit = two_qubit_circuit()
    evaluator = DenseEvaluator(OPERATOR)
    short = NaturalGradient(maxiter=2, learning_rate=0.2, regularization=1e-2)
    long = NaturalGradient(maxiter=200, learning_rate=0.2, regularization=1e-2, tol=1e-4)
    runs = [short.new_run([0.4, -0.3, 1.1, 0.6], None), long.new_run([0.4, -0.3, 1.1, 0.6], None), long.new_run([], None)]
    assert runs[2].done  # (nothing to search)
    solver._minimize_batched(evaluator, [(circuit, run) for run in runs])
    assert runs[0].iteration == 2 and all(run.done for run in runs)
    assert 2 < runs[1].iteration < 200, runs[1].iteration  # (stopped by tol)
    # one call of each kind per iteration, for all the runs still running
    assert len(evaluator.gradient_calls) == len(evaluator.metric_calls) == runs[1].iteration
    assert [len(call[0]) for call in evaluator.metric_calls] == [2, 2] + [1] * (runs[1].iteration - 2)
    for (gc, gp, gw), (mc, mp, mw) in zip(evaluator.gradient_calls, evaluator.metric_calls):
        assert gp == mp and gw == mw and all(a is b for a, b in zip(gc, mc))
    start = evaluator.value(circuit, [0.4, -0.3, 1.1, 0.6])
    assert evaluator.value(circuit, runs[1].x) < evaluator.value(circuit, runs[0].x) < start
    # a stationary point: the last update was below tol and the gradient before it was (G + rho I) update / learning_rate, with
    # |G| <= trace G <= 4 slots x 1/4 -- so it was below 1.01 * 1e-4 / 0.2, and one such step moves it by less than itself
    assert np.linalg.norm(dense_gradient.gradient(circuit, runs[1].x, evaluator.h)) < 2 * 1.01 * 1e-4 / 0.2


def test_an_embedded_run_is_differentiated_by_its_own_parameters():
    circuit = two_qubit_circuit()
    evaluator = DenseEvaluator(OPERATOR)
    run = NaturalGradient(maxiter=1, learning_rate=0.1, regularization=1e-3).new_run([1.1, 0.6], None)
    base = np.asarray([0.4, -0.3, 0.0, 0.0])
    run.embed = (base, np.asarray([2, 3]))
    solver._minimize_batched(evaluator, [(circuit, run)])
    (_, points, wrt), = evaluator.metric_calls
    assert wrt == [[2, 3]] and points == [[0.4, -0.3, 1.1, 0.6]] and run.x.shape == (2,)


def test_what_the_optimiser_refuses():
    with pytest.raises(ValueError, match="regularization must be positive"):
        NaturalGradient(regularization=0.0)

    class NoMetric:
        n_qubits = 2

        def evaluate_gradients(self, *args):
            raise AssertionError("not reached")

    run = NaturalGradient(maxiter=1).new_run([0.1] * 4, None)
    with pytest.raises(ValueError, match="needs an evaluator with metric_tensors"):
        solver._minimize_batched(NoMetric(), [(two_qubit_circuit(), run)])
    adam = solver.Adam(maxiter=1).new_run([0.1] * 4, None)
    with pytest.raises(ValueError, match="cannot share a search"):
        solver._minimize_batched(DenseEvaluator(OPERATOR), [(two_qubit_circuit(), run), (two_qubit_circuit(), adam)])
    assert NaturalGradient(maxiter=3).n_circuit_evaluations_for(4) == solver.Adam(maxiter=3).n_circuit_evaluations_for(4)


# ---- the evaluators' method, on the recording device ------------------------------------------------------------------------


class MetricRecordingDevice(layer.RecordingDevice):
    def metric_tensors(self, circuits, parameter_values, wrt=None):
        n = self._note("metric_tensors", circuits)
        return [np.zeros((c.num_parameters, c.num_parameters)) for c in circuits[:n]]


EVALUATORS = {"operator": layer.operator_evaluator, "sampler": layer.sampler_evaluator}


def test_the_method_is_no_evaluate_method():
    """tests/test_evaluator_layer_host.py lists every ``evaluate_*`` method: this one is held to its rules here instead."""
    for cls in (layer.OperatorCircuitEvaluator, layer.OperatorSamplerCircuitEvaluator):
        assert callable(getattr(cls, "metric_tensors")) and not hasattr(cls, "evaluate_metric_tensors")


@pytest.mark.parametrize("kind", sorted(EVALUATORS))
def test_metric_tensors_leaves_another_evaluators_operator_in_place(kind):
    device = MetricRecordingDevice()
    ev = EVALUATORS[kind](device)
    layer.leave_another_operator(device)
    got = ev.metric_tensors(layer.make_circuits(), layer.VALUES)
    assert [m.shape for m in got] == [(2, 2), (0, 0), (3, 3)]
    assert [c.name for c in device.calls] == ["metric_tensors"]
    assert device.installed == [] and device._operator is layer.OTHER and not device.operator_lock.held()


@pytest.mark.parametrize("kind", sorted(EVALUATORS))
def test_metric_tensors_is_behind_the_initial_state_and_sees_a_circuit_edited_in_place(kind):
    device = MetricRecordingDevice()
    ev = EVALUATORS[kind](device, layer.INITIAL)
    circuits = layer.make_circuits()
    device.calls.clear()
    ev.metric_tensors(circuits, layer.VALUES)
    assert all(layer.same_circuit(got, layer.INITIAL.compose(c)) for got, c in zip(device.calls[0].circuits, circuits))
    assert ev._composed_lists is None  # (no list kept by identity)
    circuits[0].u(ParamRef(0), 0.2, ParamRef(1), 2)  # the same object, one gate longer
    circuits[2] = CircuitIR(layer.N_QUBITS).u(ParamRef(0), ParamRef(1), ParamRef(2), 0)
    device.calls.clear()
    ev.metric_tensors(circuits, layer.VALUES)
    assert all(layer.same_circuit(got, layer.INITIAL.compose(c)) for got, c in zip(device.calls[0].circuits, circuits))
    # circuits on a kept state are passed through as they are
    kept = [c.continue_from(layer.FakeKept()) for c in layer.make_circuits()]
    device.calls.clear()
    ev.metric_tensors(kept, layer.VALUES)
    assert all(got is c for got, c in zip(device.calls[0].circuits, kept))
    with pytest.raises(ValueError):
        ev.metric_tensors(circuits, layer.VALUES[:2])
