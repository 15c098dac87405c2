"""Folded-spectrum and variance costs without a device: the NumPy restatement (tests/folded_reference.py)
against the dense derivative of (H - c)^2 and against central differences of the cost -- in mode *mean* of the variance itself,
which checks that holding E fixed in the seed loses nothing --; the two prototypes against the binding;
``FoldedSpectrumCircuitEvaluator`` against the two rules of DESIGN.md 5.2 on the recording stand-in; the drivers of
``evqe/spectrum.py`` on a recording solver, and ``minimize_variance``'s refusal of NFT.

Inputs: n in {3, 4, 5, 6, 8}; a circuit with a shared parameter (``circuit_families.generic``) and an EVQE individual; a general
operator of 12 random strings and an Ising operator; targets inside and outside the spectrum and ``None`` (the mean)."""

import ctypes as C
import inspect
import re
from functools import lru_cache
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import circuit_families as cf
import dense_gradient
import folded_reference as fr
import helpers
import test_evaluator_layer_host as layer
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import FoldedSpectrumCircuitEvaluator, OperatorCircuitEvaluator
from queasars_amd.circuit_evaluation.circuit_evaluation import StatevectorDevice, _OperatorEvaluator
from queasars_amd.evqe import spectrum
from queasars_amd.evqe.solver import NFT, SPSA, Adam, EVQEResult

ROOT = Path(__file__).resolve().parent.parent
SIZES = (3, 4, 5, 6, 8)
STEP = 1e-6


@lru_cache(maxsize=None)
def operator(n: int, kind: str):
    return helpers.random_ising_operator(n, seed=n) if kind == "ising" else helpers.random_pauli_operator(n, 12, seed=n)


@lru_cache(maxsize=None)
def circuits(n: int):
    shared, values = cf.generic(n, 30, share=0.3, literal=0.2, seed=n)
    assert min(shared.gradient_terms(), default=0) < 0  # (a parameter that several angle slots read)
    _, made, params = helpers.population_circuits(n, 2, 1, n)
    return ((shared, list(values)), (made[0], list(params[0])))


def targets(n: int, kind: str):
    """Inside the spectrum, outside it (below the lowest eigenvalue's bound), and the mean."""
    width = fr.spread(operator(n, kind))
    return (0.25 * width, -1.5 * width, None)


@lru_cache(maxsize=None)
def case(n: int, kind: str, which: int, target):
    circuit, params = circuits(n)[which]
    return fr.folded(circuit, params, operator(n, kind), target)


# ---- the reference -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ("general", "ising"))
@pytest.mark.parametrize("n", SIZES)
def test_the_reference_is_the_dense_gradient_of_the_folded_matrix(n, kind):
    """Allowance 1e-12 (sum |c_k| + |c|)^2: both sides are fp64 sweeps of at most ~40 gates over the same seed, whose norm the
    factor bounds; the measured figures are DESIGN.md 4.21's (at most 2e-3 of it)."""
    op = operator(n, kind)
    worst = 0.0
    for which, (circuit, params) in enumerate(circuits(n)):
        for target in targets(n, kind):
            got = case(n, kind, which, target)
            matrix = fr.folded_matrix(op, got.centre)
            dense = dense_gradient.gradient(circuit, params, matrix)
            scale = fr.seed_norm(op, got.centre)
            error = float(np.abs(dense - got.gradient).max(initial=0.0))
            worst = max(worst, error / scale)
            assert error <= 1e-12 * scale, (which, target, error, scale)
            # the centred cost is the expectation value of the dense matrix
            assert abs(got.cost - dense_gradient.expectation(circuit, params, matrix)) <= 1e-12 * scale
            assert abs(got.energy - dense_gradient.expectation(circuit, params, dense_gradient.dense_operator(op))) <= 1e-12 * fr.spread(op)
            assert got.cost >= 0.0
    print(f"n = {n}, {kind}: reference against the dense gradient of (H - c)^2, over (sum|c_k| + |c|)^2: {worst:.3e}")


@pytest.mark.parametrize("kind", ("general", "ising"))
@pytest.mark.parametrize("n", SIZES)
def test_the_reference_is_the_derivative_of_the_cost(n, kind):
    """Central differences, h = 1e-6, of the centred cost; with ``target=None`` of the variance itself, E moving with the point:
    the seed holds E fixed, and d/dc <(H - c)^2> = -2 (E - c) = 0 at c = E says that this loses nothing.  Allowance
    1e-7 (sum |c_k| + |c|)^2: truncation h^2 |F'''| / 6 ~ 1e-12 and rounding eps / h ~ 2e-10 of that scale (the measured figures
    are DESIGN.md 4.21's, at most 3e-10 of it: a factor of 300 and more in hand)."""
    op = operator(n, kind)
    worst = {True: 0.0, False: 0.0}
    for which, (circuit, params) in enumerate(circuits(n)):
        for target in targets(n, kind):
            got = case(n, kind, which, target)
            differences = fr.finite_differences(circuit, params, op, target, h=STEP)
            scale = fr.seed_norm(op, got.centre)
            error = float(np.abs(differences - got.gradient).max(initial=0.0))
            worst[target is None] = max(worst[target is None], error / scale)
            assert error <= 1e-7 * scale, (which, target, error, scale)
    print(f"n = {n}, {kind}: reference against central differences over (sum|c_k| + |c|)^2: target {worst[False]:.3e}, mean {worst[True]:.3e}")
    # not a test of zeros; the two modes differ; and the fixed target at E is the mean
    circuit, params = circuits(n)[0]
    mean = case(n, kind, 0, None)
    assert float(np.abs(mean.gradient).max()) > 1e-3
    assert float(np.abs(mean.gradient - case(n, kind, 0, targets(n, kind)[0]).gradient).max()) > 1e-3
    at_e = fr.folded(circuit, params, op, mean.energy)
    assert np.array_equal(at_e.gradient, mean.gradient) and at_e.cost == mean.cost


def test_the_folded_minimum_is_the_eigenvalue_nearest_the_target():
    n = 4
    op = operator(n, "general")
    values = np.linalg.eigvalsh(dense_gradient.dense_operator(op))
    target = float(values[len(values) // 2]) + 0.01
    folded = np.linalg.eigvalsh(fr.folded_matrix(op, target))
    assert abs(folded[0] - float(((values - target) ** 2).min())) < 1e-12  # (the folded minimum is the eigenvalue nearest the target)
    rng = np.random.default_rng(4)
    circuit, params = circuits(n)[0]
    for _ in range(5):
        point = rng.uniform(-np.pi, np.pi, len(params)).tolist()
        assert fr.cost(circuit, point, op, target) >= folded[0] - 1e-10
        assert fr.cost(circuit, point, op, None) >= 0.0


# ---- the C ABI --------------------------------------------------------------------------------------------------------------


def prototype(name: str) -> list:
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qsv.h").read_text(), flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert found, name
    return [" ".join(argument.split()) for argument in found.group(1).split(",")]


def ctype_of(argument: str):
    if "*" in argument:
        return C.c_void_p
    kind = argument.rsplit(" ", 1)[0]
    return {"int": C.c_int, "double": C.c_double}[kind]


@pytest.mark.parametrize("name,arguments", [
    ("qsv_folded_gradient_circuits", ["h", "centre", "target", "n_evals", "circuit_ids", "param_offsets", "params", "wrt_offsets", "wrt",
                                      "out", "out_values", "out_energies"]),
    ("qsv_folded_gradient_device", ["h", "centre", "target", "n_evals", "circuit_ids", "width", "device_values", "ready_event",
                                    "wrt_offsets", "wrt", "out_width", "device_out", "device_out_values", "device_out_energies"]),
])
def test_the_prototypes_match_the_binding_argument_by_argument(name, arguments):
    declared = prototype(name)
    assert [re.split(r"[ *]", a)[-1] for a in declared] == arguments
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(declared)
    for argument, bound in zip(declared, argtypes):
        assert ctype_of(argument) is bound, (name, argument)


def test_the_build_list_and_the_library_know_the_kernels():
    from queasars_amd import _build

    assert "folded.hip" in _build.SOURCES and "folded.hpp" in _build.HEADERS
    lib = _lib.load()
    assert hasattr(lib, "qsv_folded_gradient_circuits") and hasattr(lib, "qsv_folded_gradient_device")


# ---- the evaluator on the recording stand-in -----------------------------------------------------------------


class FoldedDevice(layer.RecordingDevice):
    """The recording stand-in with what the folded evaluator asks of a device."""

    def folded_gradients(self, circuits, parameter_values, target=None, wrt=None, with_values=False, with_energies=False):
        n = self._note("folded_gradients", circuits)
        self.calls[-1].target, self.calls[-1].wrt = target, wrt
        out = ([np.zeros(c.num_parameters if wrt is None else 0) for c in circuits],)
        out += ((np.zeros(n),) if with_values else ()) + ((np.zeros(n),) if with_energies else ())
        return out if len(out) > 1 else out[0]

    def metric_tensors(self, circuits, parameter_values, wrt=None):
        return [np.zeros((c.num_parameters,) * 2) for c in circuits[: self._note("metric_tensors", circuits)]]


GUARDED = {
    "evaluate_circuits": lambda ev, c, v: ev.evaluate_circuits(c, v),
    "evaluate_gradients": lambda ev, c, v: ev.evaluate_gradients(c, v),
    "evaluate_values_and_gradients": lambda ev, c, v: ev.evaluate_values_and_gradients(c, v, [0]),
    "evaluate_energies": lambda ev, c, v: ev.evaluate_energies(c, v),
}
WRT_SEEN = {"evaluate_circuits": [], "evaluate_gradients": None, "evaluate_values_and_gradients": [0], "evaluate_energies": []}


def test_the_class_and_every_public_evaluate_method_of_it():
    assert issubclass(FoldedSpectrumCircuitEvaluator, _OperatorEvaluator) and not issubclass(FoldedSpectrumCircuitEvaluator, OperatorCircuitEvaluator)
    public = {name for name, _ in inspect.getmembers(FoldedSpectrumCircuitEvaluator, inspect.isfunction) if name.startswith("evaluate_")}
    assert public == set(GUARDED)
    assert FoldedSpectrumCircuitEvaluator.metric_tensors is _OperatorEvaluator.metric_tensors
    ev = FoldedSpectrumCircuitEvaluator(layer.NON_DIAGONAL, 0.5, statevector_device=FoldedDevice())
    assert ev.target == 0.5 and ev.gradient_method == "adjoint"
    assert not ev.device_resident_search_possible() and not ev.device_resident_search_by_default
    assert FoldedSpectrumCircuitEvaluator(layer.NON_DIAGONAL, statevector_device=FoldedDevice()).target is None
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            FoldedSpectrumCircuitEvaluator(layer.NON_DIAGONAL, bad, statevector_device=FoldedDevice())
    with pytest.raises(ValueError, match="different number of qubits"):
        FoldedSpectrumCircuitEvaluator(layer.NON_DIAGONAL, 0.5, statevector_device=FoldedDevice(4))
    with pytest.raises(ValueError, match="free parameters"):
        FoldedSpectrumCircuitEvaluator(layer.NON_DIAGONAL, 0.5, layer.make_circuits()[0], statevector_device=FoldedDevice())


@pytest.mark.parametrize("target", (0.5, None))
@pytest.mark.parametrize("name", sorted(GUARDED))
def test_the_methods_install_the_operator_through_the_guard(name, target):
    device = FoldedDevice()
    ev = FoldedSpectrumCircuitEvaluator(layer.NON_DIAGONAL, target, statevector_device=device)
    layer.leave_another_operator(device)
    GUARDED[name](ev, layer.make_circuits(), layer.VALUES)
    layer.assert_guarded(device, layer.NON_DIAGONAL)
    (call,) = device.calls  # (evaluate_values_and_gradients: ONE call)
    assert call.name == "folded_gradients" and call.target == target and call.wrt == WRT_SEEN[name]


def test_metric_tensors_is_inherited_and_reads_no_operator():
    device = FoldedDevice()
    ev = FoldedSpectrumCircuitEvaluator(layer.NON_DIAGONAL, 0.5, layer.INITIAL, statevector_device=device)
    layer.leave_another_operator(device)
    circuits = layer.make_circuits()
    assert [m.shape for m in ev.metric_tensors(circuits, layer.VALUES)] == [(2, 2), (0, 0), (3, 3)]
    assert device.installed == [] and device._operator is layer.OTHER
    assert all(layer.same_circuit(got, layer.INITIAL.compose(c)) for got, c in zip(device.calls[0].circuits, circuits))


@pytest.mark.parametrize("name", sorted(GUARDED))
def test_the_methods_compose_behind_the_initial_state_per_call_and_drop_none_pairs(name):
    device = FoldedDevice()
    ev = FoldedSpectrumCircuitEvaluator(layer.NON_DIAGONAL, None, layer.INITIAL, statevector_device=device)
    circuits = layer.make_circuits()
    GUARDED[name](ev, circuits, layer.VALUES)
    assert all(layer.same_circuit(got, layer.INITIAL.compose(c)) for got, c in zip(device.calls[-1].circuits, circuits))
    assert ev._composed_lists is None  # (no list is kept by identity)
    circuits[0] = layer.make_circuits()[2]  # a list changed in place is seen
    GUARDED[name](ev, circuits, [layer.VALUES[2]] + layer.VALUES[1:])
    assert layer.same_circuit(device.calls[-1].circuits[0], layer.INITIAL.compose(circuits[0]))
    GUARDED[name](ev, [circuits[0], None, circuits[2]], [layer.VALUES[2], layer.VALUES[1], None])
    assert len(device.calls[-1].circuits) == 1


def test_the_counts_the_host_drivers_read():
    ev = FoldedSpectrumCircuitEvaluator(layer.NON_DIAGONAL, 0.5, statevector_device=FoldedDevice())
    gradients = ev.evaluate_gradients(layer.make_circuits(), layer.VALUES)
    assert [len(g) for g in gradients] == [2, 0, 3]
    assert ev.last_gradient_evaluations == 3 and ev.last_gradient_evaluation_counts == [1, 1, 1]
    values, gradients = ev.evaluate_values_and_gradients(layer.make_circuits()[:2], layer.VALUES[:2])
    assert values.shape == (2,) and len(gradients) == 2 and ev.last_gradient_evaluation_counts == [1, 1]
    assert ev.evaluate_energies(layer.make_circuits(), layer.VALUES).shape == (3,)
    assert isinstance(ev.evaluate_circuits(layer.make_circuits(), layer.VALUES), list)


def test_the_device_methods_check_the_target_before_any_call():
    assert StatevectorDevice._folded_centre(None) == (1, 0.0)
    assert StatevectorDevice._folded_centre(-2) == (0, -2.0)
    for bad in (float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            StatevectorDevice._folded_centre(bad)


# ---- the drivers -------------------------------------------------------------------------------------------------------------


class FakeIndividual:
    parameter_values = (0.1, 0.2)

    def get_parameterized_quantum_circuit(self, shared=True):
        return layer.make_circuits()[0]


class RecordingSolver:
    share_circuits = True

    def __init__(self, optimizer):
        self.configuration = SimpleNamespace(optimizer=optimizer)
        self.runs = []

    def compute_minimum_eigenvalue(self, evaluator, **kwargs):
        self.runs.append(SimpleNamespace(evaluator=evaluator, kwargs=kwargs))
        return EVQEResult(eigenvalue=-7.0, best_individual=FakeIndividual(), generations=1, circuit_evaluations=[1])


def _drive(function, optimizer, *args, **options):
    device = FoldedDevice()
    ev = OperatorCircuitEvaluator(layer.NON_DIAGONAL, initial_state_circuit=layer.INITIAL, statevector_device=device)
    solver = RecordingSolver(optimizer)
    device.calls.clear()
    return device, ev, solver, function(solver, ev, *args, **options)


@pytest.mark.parametrize("optimizer", (SPSA(), NFT(), Adam()))
def test_compute_eigenvalue_near_runs_the_solver_on_a_folded_evaluator(optimizer):
    device, ev, solver, result = _drive(spectrum.compute_eigenvalue_near, optimizer, 0.75, max_generations=2)
    (run,) = solver.runs
    folded = run.evaluator
    assert run.kwargs == {"max_generations": 2}
    assert isinstance(folded, FoldedSpectrumCircuitEvaluator) and folded.target == 0.75
    assert folded.statevector_device is device and folded.operator is layer.NON_DIAGONAL and folded.initial_state_circuit is layer.INITIAL
    # the stand-in's zeros, not the solver's -7: the energy, the cost and the centred variance at the best individual
    assert result.eigenvalue == 0.0 and result.folded_value == 0.0 and result.eigenvalue_variance == 0.0
    assert [(call.name, call.target, call.wrt) for call in device.calls] == [
        ("folded_gradients", 0.75, []), ("folded_gradients", 0.75, []), ("folded_gradients", None, [])]
    assert all(call.held and call.operator is layer.NON_DIAGONAL for call in device.calls)
    assert all(layer.same_circuit(call.circuits[0], layer.INITIAL.compose(layer.make_circuits()[0])) for call in device.calls)
    with pytest.raises(ValueError, match="minimize_variance"):
        spectrum.compute_eigenvalue_near(solver, ev, None)


@pytest.mark.parametrize("optimizer", (SPSA(), Adam()))
def test_minimize_variance_runs_the_solver_on_the_variance(optimizer):
    device, _, solver, result = _drive(spectrum.minimize_variance, optimizer)
    assert solver.runs[0].evaluator.target is None
    assert result.eigenvalue == 0.0 and result.folded_value == 0.0 and result.eigenvalue_variance == 0.0
    assert [(call.name, call.target) for call in device.calls] == [("folded_gradients", None)] * 2


def test_minimize_variance_refuses_nft_and_says_why():
    device = FoldedDevice()
    ev = OperatorCircuitEvaluator(layer.NON_DIAGONAL, statevector_device=device)
    solver = RecordingSolver(NFT())
    with pytest.raises(ValueError, match="second harmonic.*NFT"):
        spectrum.minimize_variance(solver, ev)
    assert solver.runs == []
