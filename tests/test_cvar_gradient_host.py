"""Exact CVaR gradients without a device: the NumPy restatement of the rule (tests/cvar_gradient_reference.py)
against the dense derivative of the clipped operator, against central differences of the reference's CVaR and against the
reference's value; the two prototypes against the binding; ``ExactCVaRCircuitEvaluator`` against the two rules of DESIGN.md 5.2
on a recording stand-in for the device, its pickle, and the solver's host Adam driver on a NumPy stand-in of the evaluator.

Inputs: ``population_circuits(7, 2, 3, seed)`` for seeds 0 - 3, an Ising operator and a tie-free random diagonal,
alpha in {0.05, 0.25, 0.5, 0.9}: 96 cases, built once."""

import inspect
import pickle
import re
import threading
from functools import lru_cache
from pathlib import Path
from types import SimpleNamespace

import ctypes as C
import numpy as np
import pytest

import cvar_gradient_reference as ref
import dense_gradient
import helpers
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import ExactCVaRCircuitEvaluator, OperatorSamplerCircuitEvaluator
from queasars_amd.circuit_evaluation.circuit_evaluation import StatevectorDevice
from queasars_amd.evqe import solver
from queasars_amd.ir import CircuitIR, ParamRef, PauliOperator

ROOT = Path(__file__).resolve().parent.parent
N = 7
OPERATOR_SEED = 4  # (of both operators: with it no case lies within 1e-4 of a kink, which the central differences need and assert)
ALPHAS = (0.05, 0.25, 0.5, 0.9)
OPERATORS = ("ising", "tie-free")
STEP = 1e-6


@lru_cache(maxsize=None)
def operator(kind: str) -> PauliOperator:
    if kind == "ising":
        return helpers.random_ising_operator(N, seed=OPERATOR_SEED)
    op = helpers.random_pauli_operator(N, 4 * N, seed=OPERATOR_SEED, alphabet="IZ")
    assert len(np.unique(ref.diagonal_values(op))) == 1 << N  # (tie-free)
    return op


@lru_cache(maxsize=None)
def circuits():
    out = []
    for seed in range(4):
        _, made, params = helpers.population_circuits(N, 2, 3, seed)
        out += [(c, list(p)) for c, p in zip(made, params)]
    return tuple(out)


@lru_cache(maxsize=None)
def cases():
    """{(circuit index, operator, alpha): CVaRCase}, computed once, never written to."""
    return {(i, kind, alpha): ref.cvar_gradient(c, p, operator(kind), alpha)
            for i, (c, p) in enumerate(circuits()) for kind in OPERATORS for alpha in ALPHAS}


def cvar_of(probabilities: np.ndarray, values: np.ndarray, alpha: float) -> float:
    from queasars_amd.circuit_evaluation.expectation_calculation import _get_expectation

    return _get_expectation([(i, float(p), float(v)) for i, (p, v) in enumerate(zip(probabilities, values))], alpha)


# ---- the reference ----------------------------------------------------------------------------------------------------------


def test_the_reference_is_the_dense_gradient_of_the_clipped_operator():
    worst = 0.0
    for (i, kind, alpha), case in cases().items():
        if i % 3:  # (the dense derivative runs the circuit once per angle slot: a third of the circuits, every operator and alpha)
            continue
        circuit, params = circuits()[i]
        dense = dense_gradient.gradient(circuit, params, np.diag(case.weights).astype(np.complex128))
        worst = max(worst, float(np.max(np.abs(dense - case.gradient))))
        assert np.allclose(dense, case.gradient, rtol=0.0, atol=1e-12), (i, kind, alpha)
    print(f"reference against the dense gradient of diag(w): {worst:.3e}")


def test_the_reference_is_the_derivative_of_the_numpy_cvar():
    """Central differences (h = 1e-6) of ``_get_expectation`` on the oracle state's distribution.  Away from a kink the CVaR is
    differentiable and a step of 1e-6 moves the gathered mass by about 1e-6: every case must have a kink margin above 1e-4."""
    margins = [case.kink_margin for case in cases().values()]
    print(f"smallest kink margin: {min(margins):.3e}")
    assert min(margins) > 1e-4
    values = {kind: ref.diagonal_values(operator(kind)) for kind in OPERATORS}
    worst = 0.0
    for i, (circuit, params) in enumerate(circuits()):
        got = {key: np.zeros(circuit.num_parameters) for key in ((kind, alpha) for kind in OPERATORS for alpha in ALPHAS)}
        for p in range(circuit.num_parameters):
            shifted = []
            for sign in (1.0, -1.0):
                point = list(params)
                point[p] += sign * STEP
                psi = helpers.oracle_state(circuit, point)
                shifted.append(psi.real ** 2 + psi.imag ** 2)
            for kind, alpha in got:
                got[(kind, alpha)][p] = (cvar_of(shifted[0], values[kind], alpha) - cvar_of(shifted[1], values[kind], alpha)) / (2 * STEP)
        for (kind, alpha), differences in got.items():
            error = float(np.max(np.abs(differences - cases()[(i, kind, alpha)].gradient), initial=0.0))
            worst = max(worst, error)
            assert error <= 1e-7, (i, kind, alpha, error)
    print(f"reference against central differences: {worst:.3e}")


def test_the_reference_value_is_the_numpy_cvar():
    worst = 0.0
    for (i, kind, alpha), case in cases().items():
        circuit, params = circuits()[i]
        worst = max(worst, abs(case.value - ref.numpy_cvar(circuit, params, operator(kind), alpha)))
    assert worst <= 1e-12
    # the stopping rule firing by itself: half of the mass of a uniform superposition, summed, falls one rounding short of 0.5
    circuit = CircuitIR(4)
    for q in range(4):
        circuit.u(np.pi / 2, 0.0, 0.0, q)
    z = PauliOperator(["ZIII"], [1.0])
    case = ref.cvar_gradient(circuit, [], z, 0.5)
    assert 0.0 < case.left_out < 1e-15 and case.threshold == -1.0
    assert abs(case.value - ref.numpy_cvar(circuit, [], z, 0.5)) <= 1e-12
    print(f"reference value against _get_expectation: {worst:.3e}; left out by the stopping rule: {case.left_out:.3e}")


def test_the_margins_and_the_boundary_of_a_hand_made_distribution():
    p = np.array([0.1, 0.2, 0.3, 0.4])
    v = np.array([3.0, 1.0, 2.0, 1.0])  # ascending by (value, index): states 1, 3, 2, 0 with cumulative mass 0.2, 0.6, 0.9, 1.0
    b, t, s, kink, identification = ref.boundary(p, v, 0.5)
    assert (b, t, s) == (1, 1.0, 0.0) and kink == pytest.approx(0.1) and identification == pytest.approx(0.1 + 1e-8 + 5e-6)
    b, t, s, kink, identification = ref.boundary(p, v, 0.600004)  # (0.6 is within the tolerance below alpha: the stop fires)
    assert (b, t) == (1, 1.0) and s == pytest.approx(4e-6) and kink < 0 < identification
    b, t, s, _, _ = ref.boundary(p * 0.5, v, 0.9)  # (nothing reaches the target: the last rank)
    assert (b, t) == (3, 3.0) and s == pytest.approx(0.4)


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
    ("qsv_cvar_gradient_circuits", ["h", "alpha", "n_evals", "circuit_ids", "param_offsets", "params", "wrt_offsets", "wrt", "out",
                                    "out_values", "out_thresholds"]),
    ("qsv_cvar_gradient_device", ["h", "alpha", "n_evals", "circuit_ids", "width", "device_values", "ready_event", "wrt_offsets", "wrt",
                                  "out_width", "device_out", "device_out_values", "device_out_thresholds"]),
])
def test_the_prototypes_match_the_binding_argument_by_argument(name, arguments):
    declared = prototype(name)
    assert [re.split(r"[ *]", a)[-1] for a in declared] == arguments
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(declared)
    for argument, bound in zip(declared, argtypes):
        assert ctype_of(argument) is bound, (name, argument)


# ---- the evaluator on a recording stand-in ------------------------------------------------------------------


class OwnedLock:
    def __init__(self):
        self._lock, self._owner, self._depth = threading.RLock(), None, 0

    def __enter__(self):
        self._lock.acquire()
        self._owner, self._depth = threading.get_ident(), self._depth + 1
        return True

    acquire = __enter__

    def release(self):
        self._depth -= 1
        if self._depth == 0:
            self._owner = None
        self._lock.release()

    def __exit__(self, *exc):
        self.release()

    def held(self) -> bool:
        return self._depth > 0 and self._owner == threading.get_ident()


class RecordingDevice:
    """What the CVaR evaluator asks of a ``StatevectorDevice``, answered with zeros of the right shapes and written down."""

    MAX_CVAR_SHOTS = StatevectorDevice.MAX_CVAR_SHOTS
    _serial = ("recording", 2)

    def __init__(self, n_qubits=3):
        self.n_qubits, self.device_index = n_qubits, 0
        self._operator, self.operator_lock = None, OwnedLock()
        self.installed, self.calls = [], []

    def __reduce__(self):
        return (RecordingDevice, (self.n_qubits,))

    def set_operator(self, operator):
        self.installed.append(operator)
        self._operator = operator

    def _note(self, name, circuits, **said):
        self.calls.append(SimpleNamespace(name=name, circuits=circuits, operator=self._operator, held=self.operator_lock.held(), **said))
        return len(circuits)

    def cvar_gradients(self, circuits, parameter_values, alpha, wrt=None, with_values=False, with_thresholds=False):
        n = self._note("cvar_gradients", circuits, alpha=alpha, wrt=wrt)
        out = ([np.zeros(c.num_parameters) for c in circuits],) + ((np.zeros(n),) if with_values else ()) + \
              ((np.zeros(n),) if with_thresholds else ())
        return out if len(out) > 1 else out[0]

    def exact_cvar_batch(self, circuits, parameter_values, alpha):
        return [0.0] * self._note("exact_cvar_batch", circuits)

    def metric_tensors(self, circuits, parameter_values, wrt=None):
        self._note("metric_tensors", circuits)
        return [np.zeros((c.num_parameters, c.num_parameters)) for c in circuits]


DIAGONAL = PauliOperator(["ZIZ", "IZI"], [1.0, -0.5])
OTHER = PauliOperator(["ZZZ"], [1.0])
INITIAL = CircuitIR(3).u(1.0, 0.2, 0.3, 0).u(0.5, 0.6, 0.7, 1).u(0.9, 1.0, 1.1, 2)
VALUES = [[0.1, 0.2], [], [0.3, 0.4, 0.5]]
NEW_METHODS = {
    "evaluate_gradients": lambda ev, c, v: ev.evaluate_gradients(c, v),
    "evaluate_values_and_gradients": lambda ev, c, v: ev.evaluate_values_and_gradients(c, v, [0]),
    "evaluate_thresholds": lambda ev, c, v: ev.evaluate_thresholds(c, v),
}
INHERITED = {"evaluate_circuits", "evaluate_device_to_device", "evaluate_observables"}


def make_circuits():
    return [CircuitIR(3).u(ParamRef(0), 0.1, ParamRef(1), 0).cu3(0.3, 0.2, 0.1, 0, 1), CircuitIR(3).u(0.4, 0.5, 0.6, 2),
            CircuitIR(3).u(ParamRef(0), ParamRef(1), ParamRef(2), 1).cu3(0.7, 0.8, 0.9, 1, 2)]


def same_circuit(a: CircuitIR, b: CircuitIR) -> bool:
    return bytes(a._bytes) == bytes(b._bytes) and a.num_parameters == b.num_parameters


def test_the_class_is_the_exact_sampler_evaluator_with_three_more_methods():
    assert issubclass(ExactCVaRCircuitEvaluator, OperatorSamplerCircuitEvaluator)
    public = {name for name, _ in inspect.getmembers(ExactCVaRCircuitEvaluator, inspect.isfunction) if name.startswith("evaluate_")}
    assert public == INHERITED | set(NEW_METHODS)
    for name in INHERITED:  # (the parent's own functions: the parent's bits)
        assert getattr(ExactCVaRCircuitEvaluator, name) is getattr(OperatorSamplerCircuitEvaluator, name)
    ev = ExactCVaRCircuitEvaluator(DIAGONAL, 0.25, statevector_device=RecordingDevice())
    assert ev._shots is None and ev.alpha == 0.25 and ev.gradient_method == "adjoint"
    assert callable(ev.metric_tensors) and not ev.device_resident_search_by_default
    with pytest.raises(ValueError, match="alpha"):
        ExactCVaRCircuitEvaluator(DIAGONAL, 0.0, statevector_device=RecordingDevice())
    with pytest.raises(ValueError, match="diagonal"):
        ExactCVaRCircuitEvaluator(PauliOperator(["XII"], [1.0]), 0.5, statevector_device=RecordingDevice())


@pytest.mark.parametrize("name", sorted(NEW_METHODS))
def test_a_new_method_reaches_the_device_under_the_lock_with_its_own_operator(name):
    device = RecordingDevice()
    ev = ExactCVaRCircuitEvaluator(DIAGONAL, 0.25, statevector_device=device)
    device.set_operator(OTHER)  # (another evaluator on the same device went last)
    device.installed.clear()
    device.calls.clear()
    NEW_METHODS[name](ev, make_circuits(), VALUES)
    (call,) = device.calls
    assert call.name == "cvar_gradients" and call.held and call.operator is DIAGONAL and call.alpha == 0.25
    assert device.installed == [DIAGONAL] and not device.operator_lock.held()
    assert call.wrt == {"evaluate_gradients": None, "evaluate_values_and_gradients": [0], "evaluate_thresholds": []}[name]


@pytest.mark.parametrize("name", sorted(NEW_METHODS))
def test_a_new_method_composes_behind_the_initial_state_per_call_and_drops_none_pairs(name):
    device = RecordingDevice()
    ev = ExactCVaRCircuitEvaluator(DIAGONAL, 0.25, initial_state_circuit=INITIAL, statevector_device=device)
    circuits = make_circuits()
    NEW_METHODS[name](ev, circuits, VALUES)
    assert all(same_circuit(got, INITIAL.compose(c)) for got, c in zip(device.calls[-1].circuits, circuits))
    assert ev._composed_lists is None  # (no list is kept by identity)
    circuits[0] = CircuitIR(3).u(ParamRef(0), ParamRef(1), 0.25, 2)  # (a list changed in place is seen)
    NEW_METHODS[name](ev, circuits, VALUES)
    assert same_circuit(device.calls[-1].circuits[0], INITIAL.compose(circuits[0]))
    NEW_METHODS[name](ev, [circuits[0], None, circuits[2]], [VALUES[0], VALUES[1], None])
    assert len(device.calls[-1].circuits) == 1


def test_the_counts_the_host_drivers_read():
    ev = ExactCVaRCircuitEvaluator(DIAGONAL, 0.25, statevector_device=RecordingDevice())
    gradients = ev.evaluate_gradients(make_circuits(), VALUES)
    assert [len(g) for g in gradients] == [2, 0, 3]
    assert ev.last_gradient_evaluations == 3 and ev.last_gradient_evaluation_counts == [1, 1, 1]
    values, gradients = ev.evaluate_values_and_gradients(make_circuits()[:2], VALUES[:2])
    assert values.shape == (2,) and len(gradients) == 2 and ev.last_gradient_evaluation_counts == [1, 1]
    assert ev.evaluate_thresholds(make_circuits(), VALUES).shape == (3,)


def test_a_pickled_evaluator_travels_with_empty_caches():
    ev = ExactCVaRCircuitEvaluator(DIAGONAL, 0.25, initial_state_circuit=INITIAL, statevector_device=RecordingDevice())
    circuits = make_circuits()  # (the cache holds a caller's circuits weakly: they live as long as this list)
    ev.evaluate_gradients(circuits, VALUES)
    assert len(ev._composed) == 3
    ev._last_matrix = ("a weak reference to a tensor of this process",)
    restored = pickle.loads(pickle.dumps(ev))
    assert type(restored) is ExactCVaRCircuitEvaluator and restored.alpha == 0.25 and restored._shots is None
    assert restored._composed_lists is None and restored._last_matrix is None and len(restored._composed) == 0
    assert restored.n_qubits == 3 and same_circuit(restored._initial_state_circuit, INITIAL)
    assert len(restored.evaluate_gradients(make_circuits(), VALUES)) == 3


# ---- the solver's host driver -------------------------------------------------------------------------------------------------


class NumpyCVaREvaluator:
    """What ``_minimize_adam`` reads of ``ExactCVaRCircuitEvaluator``, computed by the NumPy reference."""

    gradient_method = "adjoint"

    def __init__(self, operator, alpha):
        self.operator, self.alpha = operator, alpha
        self.last_gradient_evaluations, self.last_gradient_evaluation_counts = 0, []

    def evaluate_circuits(self, circuits, parameter_values):
        return [ref.numpy_cvar(c, p, self.operator, self.alpha) for c, p in zip(circuits, parameter_values)]

    def evaluate_gradients(self, circuits, parameter_values, wrt=None):
        wrt = [list(range(c.num_parameters)) for c in circuits] if wrt is None else wrt
        out = [ref.cvar_gradient(c, p, self.operator, self.alpha).gradient[np.asarray(w, dtype=np.int64)]
               for c, p, w in zip(circuits, parameter_values, wrt)]
        self.last_gradient_evaluations, self.last_gradient_evaluation_counts = len(out), [1] * len(out)
        return out


def test_the_host_adam_driver_lowers_the_cvar():
    ev = NumpyCVaREvaluator(operator("ising"), 0.25)
    config = solver.Adam(maxiter=15, lr=0.05)
    solver._require_gradients(ev, config)
    jobs = [(c, config.new_run(list(p), None)) for c, p in circuits()[:3]]
    before = np.asarray(ev.evaluate_circuits([c for c, _ in jobs], [run.x.tolist() for _, run in jobs]))
    solver._minimize_adam(ev, jobs)
    after = np.asarray(ev.evaluate_circuits([c for c, _ in jobs], [run.x.tolist() for _, run in jobs]))
    assert all(run.done and run.nfev == run.iteration for _, run in jobs)
    print("CVaR before", before, "after", after)
    assert (after < before).all()
