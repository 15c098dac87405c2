"""Deflated (VQD) costs without a device: the NumPy reference against finite differences and against the plain
adjoint reference, the evaluator's layer on the recording stand-in of tests/test_evaluator_layer_host.py, and the driver
``evqe.deflation.compute_eigenvalues`` with a solver that records what it is given."""

import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import adjoint_reference
import circuit_families as cf
import deflation_reference as dr
import helpers
import test_evaluator_layer_host as layer
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import DeflatedOperatorCircuitEvaluator, KeptState, OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe import deflation
from queasars_amd.evqe.solver import EVQEResult
from queasars_amd.ir import PauliOperator

ROOT = Path(__file__).resolve().parent.parent


# ---- the header and the binding ------------------------------------------------------------------------------------------------


def test_header_binding_and_build_list_know_the_entry_points():
    header = (ROOT / "include" / "qsv.h").read_text()
    assert re.search(r"\bint qsv_deflated_gradient_circuits\(", header) and re.search(r"\bint qsv_deflated_gradient_device\(", header)
    assert len(_lib.SIGNATURES["qsv_deflated_gradient_circuits"][1]) == 14
    assert len(_lib.SIGNATURES["qsv_deflated_gradient_device"][1]) == 16
    from queasars_amd import _build

    assert "deflation.hip" in _build.SOURCES and "deflation.hpp" in _build.HEADERS
    lib = _lib.load()
    assert hasattr(lib, "qsv_deflated_gradient_circuits") and hasattr(lib, "qsv_deflated_gradient_device")


# ---- the reference -----------------------------------------------------------------------------------------------------------


def _case(n: int):
    """(circuit, point, operator, kept states, betas): a circuit with a shared parameter, a general operator, three kept states of
    other circuits, weights of mixed sign and size."""
    circuit, params = cf.generic(n, 30, share=0.3, literal=0.2, seed=n)
    operator = helpers.random_pauli_operator(n, 12, seed=n)
    kept = [helpers.oracle_state(*cf.generic(n, 20, seed=100 + n + k)) for k in range(3)]
    return circuit, params, operator, kept, [3.0, -0.75, 11.5]


@pytest.mark.parametrize("n", (3, 4, 5, 6))
def test_the_reference_gradient_is_the_derivative_of_the_reference_cost(n):
    circuit, params, operator, kept, betas = _case(n)
    gradient, value, energy, c = dr.gradient_and_terms(circuit, params, operator, kept, betas)
    cost, energy_again, c_again = dr.terms(circuit, params, operator, kept, betas)
    assert abs(value - cost) < 1e-12 * dr.scale(operator, betas)  # Re<psi|lambda_G> = C
    assert energy == energy_again and np.array_equal(c, c_again)
    assert abs(cost - energy - sum(b * abs(x) ** 2 for b, x in zip(betas, c))) < 1e-12 * dr.scale(operator, betas)
    fd = dr.finite_differences(circuit, params, operator, kept, betas, h=1e-6)
    worst = float(np.abs(gradient - fd).max())
    # h = 1e-6: truncation h^2 |C'''| / 6 ~ 1e-12 * scale, rounding eps * scale / h ~ 2e-10 * scale: 1e-7 * scale has margin
    tolerance = 1e-7 * dr.scale(operator, betas)
    print(f"n = {n}: largest |sweep - central difference| {worst:.3e}, allowed {tolerance:.3e}")
    assert worst < tolerance and float(np.abs(gradient).max()) > 1e-3
    # the penalty matters: without the kept states the gradient is another one
    assert float(np.abs(gradient - adjoint_reference.gradient(circuit, params, operator)).max()) > 1e-3


@pytest.mark.parametrize("n", (3, 6))
def test_without_kept_states_the_reference_is_the_adjoint_reference(n):
    circuit, params, operator, _, _ = _case(n)
    gradient, value, energy, c = dr.gradient_and_terms(circuit, params, operator, [], [])
    want, want_value = adjoint_reference.gradient_and_value(circuit, params, operator)
    assert np.array_equal(gradient, want) and value == want_value == energy and c.shape == (0,)


def test_the_deflated_matrix_bounds_the_cost_from_below():
    circuit, params, operator, kept, betas = _case(4)
    low = float(np.linalg.eigvalsh(dr.deflated_matrix(operator, kept, betas))[0])
    rng = np.random.default_rng(4)
    for _ in range(5):
        point = rng.uniform(-np.pi, np.pi, len(params)).tolist()
        assert dr.cost(circuit, point, operator, kept, betas) >= low - 1e-10


# ---- the evaluator on the recording stand-in ---------------------------------------------------------------------------------


class DeflationDevice(layer.RecordingDevice):
    """The recording stand-in with what the deflated evaluator asks of a device: kept states that are real ``KeptState`` objects
    of this stand-in, ``_kept_id``'s check as the device makes it, and ``deflated_gradients`` / ``metric_tensors``."""

    MAX_OVERLAP_STATES = StatevectorDevice.MAX_OVERLAP_STATES
    _kept_id = StatevectorDevice._kept_id
    _count = 0

    def __init__(self, n_qubits=layer.N_QUBITS):
        super().__init__(n_qubits)
        DeflationDevice._count += 1
        self._serial = ("deflation stand-in", DeflationDevice._count)
        self._dead_states = []

    def keep_states(self, circuits, parameter_values):
        first = sum(len(call.circuits) for call in self.calls if call.name == "keep_states")
        return [KeptState(self, first + i) for i in range(self._note("keep_states", circuits))]

    def deflated_gradients(self, circuits, parameter_values, kept_states, betas, wrt=None, with_values=False, with_overlaps=False):
        n = self._note("deflated_gradients", circuits)
        self.calls[-1].kept, self.calls[-1].betas, self.calls[-1].wrt = list(kept_states), list(betas), wrt
        for kept in kept_states:
            self._kept_id(kept)
        out = ([np.zeros(c.num_parameters if wrt is None else 0) for c in circuits],)
        out += (np.zeros(n), np.zeros(n)) if with_values else ()
        out += (np.zeros((n, len(kept_states)), dtype=complex),) if with_overlaps else ()
        return out if len(out) > 1 else out[0]

    def metric_tensors(self, circuits, parameter_values, wrt=None):
        return [np.zeros((c.num_parameters,) * 2) for c in circuits[: self._note("metric_tensors", circuits)]]


DEFLATED_GUARDED = {
    "evaluate_circuits": lambda ev, c, v: ev.evaluate_circuits(c, v),
    "evaluate_gradients": lambda ev, c, v: ev.evaluate_gradients(c, v),
    "evaluate_deflation_terms": lambda ev, c, v: ev.evaluate_deflation_terms(c, v),
}


def deflated_evaluator(device, initial=None, betas=None, n_kept=2):
    kept = device.keep_states(layer.make_circuits()[:n_kept], layer.VALUES[:n_kept])
    return DeflatedOperatorCircuitEvaluator(layer.NON_DIAGONAL, kept, betas, initial, statevector_device=device), kept


def test_every_public_evaluate_method_of_the_deflated_evaluator_is_listed():
    import inspect

    public = {name for name, _ in inspect.getmembers(DeflatedOperatorCircuitEvaluator, inspect.isfunction) if name.startswith("evaluate_")}
    assert public == set(DEFLATED_GUARDED)


@pytest.mark.parametrize("name", sorted(DEFLATED_GUARDED))
def test_the_methods_install_the_operator_through_the_guard(name):
    device = DeflationDevice()
    ev, kept = deflated_evaluator(device)
    layer.leave_another_operator(device)
    DEFLATED_GUARDED[name](ev, layer.make_circuits(), layer.VALUES)
    layer.assert_guarded(device, layer.NON_DIAGONAL)
    (call,) = device.calls
    assert call.name == "deflated_gradients" and call.kept == kept
    # the default weights: 2 sum |c| of the operator for every kept state
    assert call.betas == [2.0 * (0.5 + 1.0 + 0.25)] * 2
    assert call.wrt is None if name == "evaluate_gradients" else call.wrt == []  # (the value-only call sweeps nothing)


def test_metric_tensors_is_inherited_and_reads_no_operator():
    device = DeflationDevice()
    ev, _ = deflated_evaluator(device, layer.INITIAL)
    layer.leave_another_operator(device)
    circuits = layer.make_circuits()
    metrics = ev.metric_tensors(circuits, layer.VALUES)
    assert [m.shape for m in metrics] == [(2, 2), (0, 0), (3, 3)]
    assert device.installed == [] and device._operator is layer.OTHER
    assert all(layer.same_circuit(got, layer.INITIAL.compose(c)) for got, c in zip(device.calls[0].circuits, circuits))


@pytest.mark.parametrize("name", sorted(DEFLATED_GUARDED))
def test_the_methods_compose_behind_the_initial_state_per_call(name):
    device = DeflationDevice()
    ev, _ = deflated_evaluator(device, layer.INITIAL)
    circuits = layer.make_circuits()
    device.calls.clear()
    DEFLATED_GUARDED[name](ev, circuits, layer.VALUES)
    assert all(layer.same_circuit(got, layer.INITIAL.compose(c)) for got, c in zip(device.calls[0].circuits, circuits))
    assert ev._composed_lists is None  # (no list is kept by identity)
    circuits[0] = layer.make_circuits()[2]  # a list changed in place is seen
    DEFLATED_GUARDED[name](ev, circuits, [layer.VALUES[2]] + layer.VALUES[1:])
    assert layer.same_circuit(device.calls[1].circuits[0], layer.INITIAL.compose(circuits[0]))


def test_none_pairs_are_dropped():
    device = DeflationDevice()
    ev, _ = deflated_evaluator(device, layer.INITIAL)
    circuits = layer.make_circuits()
    device.calls.clear()
    assert len(ev.evaluate_circuits([circuits[0], None, circuits[2]], [layer.VALUES[0], layer.VALUES[1], None])) == 1
    assert len(ev.evaluate_gradients([None, circuits[2]], [layer.VALUES[1], layer.VALUES[2]])) == 1
    assert [len(call.circuits) for call in device.calls] == [1, 1]
    assert layer.same_circuit(device.calls[1].circuits[0], layer.INITIAL.compose(circuits[2]))


def test_kept_states_of_another_device_and_released_ones_are_refused():
    device, other = DeflationDevice(), DeflationDevice()
    foreign = other.keep_states(layer.make_circuits()[:1], layer.VALUES[:1])
    with pytest.raises(ValueError, match="not kept on this device"):
        DeflatedOperatorCircuitEvaluator(layer.NON_DIAGONAL, foreign, statevector_device=device)
    mine = device.keep_states(layer.make_circuits()[:1], layer.VALUES[:1])
    mine[0].release()
    with pytest.raises(ValueError, match="not kept on this device"):
        DeflatedOperatorCircuitEvaluator(layer.NON_DIAGONAL, mine, statevector_device=device)
    with pytest.raises(ValueError, match="KeptState"):
        DeflatedOperatorCircuitEvaluator(layer.NON_DIAGONAL, [layer.FakeKept()], statevector_device=device)
    good = device.keep_states(layer.make_circuits()[:2], layer.VALUES[:2])
    with pytest.raises(ValueError, match="one weight per kept state"):
        DeflatedOperatorCircuitEvaluator(layer.NON_DIAGONAL, good, [1.0], statevector_device=device)
    # without a device of its own the evaluator takes the kept states' device
    assert DeflatedOperatorCircuitEvaluator(layer.NON_DIAGONAL, good).statevector_device is device
    ev = DeflatedOperatorCircuitEvaluator(layer.NON_DIAGONAL, good, [1.0, -2.0], statevector_device=device)
    assert ev.betas == [1.0, -2.0] and ev.kept_states == good
    assert ev.device_resident_search_possible() is False and ev.gradient_method == "adjoint"
    assert not hasattr(ev, "keep_states")  # (a layer search from a kept state is refused by the library: the solver never asks)
    # a state released after the evaluator was made is refused at the call
    good[1].release()
    with pytest.raises(ValueError, match="not kept on this device"):
        ev.evaluate_circuits(layer.make_circuits(), layer.VALUES)


def test_the_device_methods_check_their_arguments_before_any_call():
    """``StatevectorDevice._deflation_arguments`` on the stand-in: no library is reached."""
    device = DeflationDevice()
    kept = device.keep_states(layer.make_circuits()[:2], layer.VALUES[:2])
    ids, weights = StatevectorDevice._deflation_arguments(device, kept, [0.5, -3.0])
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1] and weights.dtype == np.float64 and weights.tolist() == [0.5, -3.0]
    for bad, sentence in (([1.0], "one weight per kept state"), ([1.0, float("nan")], "finite"), ([float("inf"), 1.0], "finite")):
        with pytest.raises(ValueError, match=sentence):
            StatevectorDevice._deflation_arguments(device, kept, bad)
    with pytest.raises(ValueError, match="at most 64"):
        StatevectorDevice._deflation_arguments(device, kept * 33, [1.0] * 66)
    ids, weights = StatevectorDevice._deflation_arguments(device, [], [])
    assert ids.shape == (0,) and weights.shape == (0,)


# ---- the driver --------------------------------------------------------------------------------------------------------------


class FakeIndividual:
    def __init__(self, run):
        self.parameter_values = (0.1 * (run + 1), 0.2)
        self._circuit = layer.make_circuits()[0]

    def get_parameterized_quantum_circuit(self, shared=True):
        return self._circuit


class RecordingSolver:
    share_circuits = True

    def __init__(self):
        self.runs = []

    def compute_minimum_eigenvalue(self, evaluator, **kwargs):
        run = len(self.runs)
        self.runs.append(SimpleNamespace(evaluator=evaluator, kwargs=kwargs))
        return EVQEResult(eigenvalue=-1.0 - run, best_individual=FakeIndividual(run), generations=1, circuit_evaluations=[1])


def _drive(k, **options):
    device = DeflationDevice()
    ev = OperatorCircuitEvaluator(layer.NON_DIAGONAL, initial_state_circuit=layer.INITIAL, statevector_device=device)
    solver = RecordingSolver()
    results = deflation.compute_eigenvalues(solver, ev, k, **options)
    return device, ev, solver, results


def test_the_driver_makes_k_runs_each_against_the_states_kept_before_it():
    device, ev, solver, results = _drive(3, max_generations=2)
    assert len(results) == 3 and len(solver.runs) == 3
    assert all(run.kwargs == {"max_generations": 2} for run in solver.runs)
    assert solver.runs[0].evaluator is ev
    kept_calls = [call for call in device.calls if call.name == "keep_states"]
    assert len(kept_calls) == 3  # (one state kept after each run, behind the evaluator's initial state)
    assert all(layer.same_circuit(call.circuits[0], layer.INITIAL.compose(layer.make_circuits()[0])) for call in kept_calls)
    for j, run in enumerate(solver.runs[1:], start=1):
        deflated = run.evaluator
        assert isinstance(deflated, DeflatedOperatorCircuitEvaluator) and deflated.statevector_device is device
        assert deflated.operator is layer.NON_DIAGONAL and deflated.initial_state_circuit is layer.INITIAL
        assert len(deflated.kept_states) == j and [k._serial for k in deflated.kept_states] == [device._serial] * j
        assert deflated.betas == [2.0 * 1.75] * j  # the default: 2 sum |c|
    assert solver.runs[2].evaluator.kept_states[:1] == solver.runs[1].evaluator.kept_states
    # what each result carries
    assert results[0].deflated_value == results[0].eigenvalue == -1.0 and results[0].overlaps_with_previous.shape == (0,)
    for j in (1, 2):
        assert results[j].eigenvalue == 0.0 and results[j].deflated_value == 0.0  # (the stand-in's zeros, not the solver's -1 - j)
        assert results[j].overlaps_with_previous.shape == (j,) and results[j].overlaps_with_previous.dtype == np.complex128
    # released at the end
    assert all(r.kept_state is None for r in results) and sorted(device._dead_states) == [0, 1, 2]
    assert all(k._id < 0 for k in solver.runs[2].evaluator.kept_states)


def test_the_driver_keeps_the_states_when_asked_and_takes_weights():
    device, _, solver, results = _drive(3, betas=[4.0, -1.0], keep=True)
    assert device._dead_states == [] and [r.kept_state._id for r in results] == [0, 1, 2]
    assert solver.runs[1].evaluator.betas == [4.0] and solver.runs[2].evaluator.betas == [4.0, -1.0]
    _, _, solver, _ = _drive(2, betas=7.0)
    assert solver.runs[1].evaluator.betas == [7.0]
    with pytest.raises(ValueError, match="needs as many"):
        _drive(3, betas=[1.0])
    with pytest.raises(ValueError, match="at least 1"):
        _drive(0)


def test_the_driver_releases_what_it_kept_when_a_run_fails():
    device = DeflationDevice()
    ev = OperatorCircuitEvaluator(layer.NON_DIAGONAL, statevector_device=device)

    class FailingSolver(RecordingSolver):
        def compute_minimum_eigenvalue(self, evaluator, **kwargs):
            if len(self.runs) == 1:
                raise RuntimeError("the second run fails")
            return super().compute_minimum_eigenvalue(evaluator, **kwargs)

    with pytest.raises(RuntimeError, match="second run"):
        deflation.compute_eigenvalues(FailingSolver(), ev, 3)
    assert device._dead_states == [0]


def test_an_operator_of_complex_coefficients_counts_their_moduli_in_the_default_weight():
    device = DeflationDevice()
    kept = device.keep_states(layer.make_circuits()[:1], layer.VALUES[:1])
    ev = DeflatedOperatorCircuitEvaluator(PauliOperator(["XIZ", "ZZI"], [0.3 + 0.4j, -2.0]), kept, statevector_device=device)
    assert ev.betas == [2.0 * 2.5]
