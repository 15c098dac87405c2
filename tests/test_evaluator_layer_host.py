"""The Python layer over the library, without a device: the operator guard, the composition behind an initial state, what an
evaluator pickles, and the ``wrt`` normaliser.  A recording stand-in takes the place of the
``StatevectorDevice``: for every call it notes the circuits it was given, the operator installed at that moment and whether
the calling thread held ``operator_lock``."""

import inspect
import pickle
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from queasars_amd.circuit_evaluation import circuit_evaluation as ce
from queasars_amd.circuit_evaluation.circuit_evaluation import (
    OperatorCircuitEvaluator,
    OperatorSamplerCircuitEvaluator,
    StatevectorDevice,
)
from queasars_amd.ir import CircuitIR, ParamRef, PauliOperator

N_QUBITS = 3


class OwnedLock:
    """A re-entrant lock that knows whether the calling thread holds it."""

    def __init__(self):
        self._lock, self._owner, self._depth = threading.RLock(), None, 0

    def acquire(self, *args, **kwargs):
        got = self._lock.acquire(*args, **kwargs)
        if got:
            self._owner, self._depth = threading.get_ident(), self._depth + 1
        return got

    def release(self):
        self._depth -= 1
        if self._depth == 0:
            self._owner = None
        self._lock.release()

    __enter__ = acquire

    def __exit__(self, *exc):
        self.release()

    def held(self) -> bool:
        return self._depth > 0 and self._owner == threading.get_ident()


class FakeKept:
    n_qubits = N_QUBITS

    def release(self):
        pass


class RecordingDevice:
    """What an evaluator asks of a ``StatevectorDevice``, answered with zeros of the right shapes and written down."""

    MAX_CVAR_SHOTS = StatevectorDevice.MAX_CVAR_SHOTS
    _serial = ("recording", 1)
    last_gradient_evaluations = 0

    def __init__(self, n_qubits=N_QUBITS):
        self.n_qubits, self.device_index = n_qubits, 0
        self._operator, self.operator_lock = None, OwnedLock()
        self.installed, self.calls = [], []
        self.sweep_first = False  # (circuit_cost sends the batch's first circuit to the adjoint sweep)

    def __reduce__(self):
        return (RecordingDevice, (self.n_qubits,))

    def set_operator(self, operator):
        self.installed.append(operator)
        self._operator = operator

    def _register_many(self, circuits):
        pass

    def forget_last_batch(self):
        pass

    def _note(self, name, circuits):
        self.calls.append(SimpleNamespace(name=name, circuits=circuits, operator=self._operator, held=self.operator_lock.held()))
        return len(circuits)

    def circuit_cost(self, circuit):
        first = self.sweep_first and not any(c.name == "circuit_cost" for c in self.calls)
        self._note("circuit_cost", [circuit])
        return {"route": "gate passes" if first else "one tile"}

    def expectation_values(self, circuits, parameter_values):
        return np.zeros(self._note("expectation_values", circuits))

    def expectation_values_to_device(self, circuits, parameter_values, device_pointer):
        self._note("expectation_values_to_device", circuits)

    def expectation_values_of_device_parameters(self, circuits, *rest):
        return np.zeros(self._note("expectation_values_of_device_parameters", circuits))

    def variances(self, circuits, parameter_values):
        n = self._note("variances", circuits)
        return np.zeros(n), np.zeros(n)

    def observable_values(self, circuits, parameter_values, operators):
        return np.zeros((self._note("observable_values", circuits), len(operators)))

    def observable_covariances(self, circuits, parameter_values, operators):
        n, m = self._note("observable_covariances", circuits), len(operators)
        return np.zeros((n, m)), np.zeros((n, m, m))

    def overlaps(self, circuits, parameter_values, kept_states, with_operator=False):
        s = np.zeros((self._note("overlaps", circuits), len(kept_states)), dtype=complex)
        return (s, s.copy()) if with_operator else s

    def keep_states(self, circuits, parameter_values):
        return [FakeKept() for _ in range(self._note("keep_states", circuits))]

    def gradients(self, circuits, parameter_values, wrt=None):
        return [np.zeros(c.num_parameters) for c in circuits[: self._note("gradients", circuits)]]

    def adjoint_gradients(self, circuits, parameter_values, wrt=None):
        return [np.zeros(c.num_parameters) for c in circuits[: self._note("adjoint_gradients", circuits)]]

    def gradients_of_device_parameters(self, circuits, *rest):
        return self._note("gradients_of_device_parameters", circuits)

    def adjoint_gradients_of_device_parameters(self, circuits, *rest):
        return self._note("adjoint_gradients_of_device_parameters", circuits)

    def gradient_plan(self, circuits, width, out_width, wrt=None):
        self._note("gradient_plan", circuits)
        device = self

        class Plan:
            n_shifted, closed = 4, False

            def __init__(self):
                self.width, self.out_width = width, out_width

            def run(self, matrix_ptr, event, out_ptr):
                return device._note("gradient_plan.run", circuits) and self.n_shifted

        return Plan()

    def cvar_of_device_parameters(self, circuits, *rest):
        self._note("cvar_of_device_parameters", circuits)

    def top_states(self, circuits, parameter_values, k, with_values=False):
        n = self._note("top_states", circuits)
        return np.zeros((n, k), dtype=np.uint64), np.zeros((n, k)), np.zeros((n, k)) if with_values else None

    def sample_batch(self, circuits, parameter_values, shots, seed, with_values=False):
        n = self._note("sample_batch", circuits)
        return np.zeros((n, shots), dtype=np.uint64), np.zeros((n, shots)) if with_values else None

    def sample_cvar_batch(self, circuits, parameter_values, shots, seed, alpha):
        return [0.0] * self._note("sample_cvar_batch", circuits)

    def exact_cvar_batch(self, circuits, parameter_values, alpha):
        return [0.0] * self._note("exact_cvar_batch", circuits)


class FakeTensor:
    """As much of a contiguous float64 device tensor as the evaluators look at before they hand its pointer on."""

    _base, _version, is_cuda = None, 0, False

    def __init__(self, *shape):
        import torch

        self.shape, self.dtype, self.device = shape, torch.float64, SimpleNamespace(index=0)

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 4096


@pytest.fixture
def any_matrix_will_do(monkeypatch):
    monkeypatch.setattr(ce, "_is_device_matrix", lambda *args, **kwargs: True)


def make_circuits():
    """Three circuits of 2, 0 and 3 parameters."""
    return [
        CircuitIR(N_QUBITS).u(ParamRef(0), 0.1, ParamRef(1), 0).cu3(0.3, 0.2, 0.1, 0, 1),
        CircuitIR(N_QUBITS).u(0.4, 0.5, 0.6, 2),
        CircuitIR(N_QUBITS).u(ParamRef(0), ParamRef(1), ParamRef(2), 1).cu3(0.7, 0.8, 0.9, 1, 2),
    ]


VALUES = [[0.1, 0.2], [], [0.3, 0.4, 0.5]]
INITIAL = CircuitIR(N_QUBITS).u(1.0, 0.2, 0.3, 0).u(0.5, 0.6, 0.7, 1).u(0.9, 1.0, 1.1, 2)
NON_DIAGONAL = PauliOperator(["XIZ", "ZZI", "IYY"], [0.5, -1.0, 0.25])
DIAGONAL = PauliOperator(["ZIZ", "IZI"], [1.0, -0.5])
OTHER = PauliOperator(["ZZZ"], [1.0])
OBSERVABLES = [PauliOperator(["ZII"], [1.0]), PauliOperator(["IXI"], [1.0])]


def matrix_and_out(width=3):
    return FakeTensor(3, 3), FakeTensor(3, width)


def _plan_run(ev, circuits, values):
    matrix, out = matrix_and_out()
    return ev.gradient_plan(circuits, matrix, out).run(matrix, out)


# every method of OperatorCircuitEvaluator that reads the operator set on the device ...
OPERATOR_GUARDED = {
    "evaluate_circuits": lambda ev, c, v: ev.evaluate_circuits(c, v),
    "evaluate_variances": lambda ev, c, v: ev.evaluate_variances(c, v),
    "evaluate_overlaps": lambda ev, c, v: ev.evaluate_overlaps(c, v, [FakeKept()], with_operator=True),
    "evaluate_subspace_matrices": lambda ev, c, v: ev.evaluate_subspace_matrices(c, v),
    "evaluate_device_parameters": lambda ev, c, v: ev.evaluate_device_parameters(c, FakeTensor(3, 3), ready=True),
    "evaluate_gradients": lambda ev, c, v: ev.evaluate_gradients(c, v),
    "evaluate_gradients_device_to_device": lambda ev, c, v: ev.evaluate_gradients_device_to_device(c, *matrix_and_out()),
    "evaluate_device_to_device": lambda ev, c, v: ev.evaluate_device_to_device(c, FakeTensor(3, 3), FakeTensor(3)),
    "evaluate_circuits_to_device": lambda ev, c, v: ev.evaluate_circuits_to_device(c, v, 4096),
    "gradient_plan": lambda ev, c, v: ev.gradient_plan(c, *matrix_and_out()),
    "gradient_plan.run": _plan_run,
    "circuit_costs": lambda ev, c, v: ev.circuit_costs(c),
    "top_states": lambda ev, c, v: ev.top_states(c, v, 2),
}
# ... and those that do not: the operator that was on the device is still there afterwards
OPERATOR_UNGUARDED = {
    "evaluate_observables": lambda ev, c, v: ev.evaluate_observables(c, v, OBSERVABLES),
    "evaluate_covariances": lambda ev, c, v: ev.evaluate_covariances(c, v, OBSERVABLES),
    "keep_states": lambda ev, c, v: ev.keep_states(c, v),
}
SAMPLER_GUARDED = {
    "evaluate_circuits": lambda ev, c, v: ev.evaluate_circuits(c, v),
    "evaluate_device_to_device": lambda ev, c, v: ev.evaluate_device_to_device(c, FakeTensor(3, 3), FakeTensor(3)),
    "top_states": lambda ev, c, v: ev.top_states(c, v, 2),
}
# (evaluate_observables of the sampler evaluator saves, sets each observable and restores: not the guard)
SAMPLER_UNGUARDED = {"evaluate_observables": lambda ev, c, v: ev.evaluate_observables(c, v, [DIAGONAL, OTHER])}
BY_IDENTITY = [("operator", "evaluate_device_to_device"), ("operator", "evaluate_gradients_device_to_device"),
               ("sampler", "evaluate_device_to_device")]
SAMPLER_MODES = {"exact mean": (None, 1.0), "exact cvar": (None, 0.5), "device cvar": (8, 0.5),
                 "host cvar": (StatevectorDevice.MAX_CVAR_SHOTS + 1, 0.5)}


def operator_evaluator(device, initial=None, operator=NON_DIAGONAL, method="parameter_shift"):
    return OperatorCircuitEvaluator(operator, initial_state_circuit=initial, statevector_device=device, gradient_method=method)


def sampler_evaluator(device, initial=None, shots=8, alpha=0.5):
    return OperatorSamplerCircuitEvaluator(shots, DIAGONAL, alpha=alpha, initial_state_circuit=initial, seed=1,
                                           statevector_device=device)


def leave_another_operator(device):
    """Another evaluator on the same device went last."""
    device.set_operator(OTHER)
    device.installed.clear()
    device.calls.clear()


# ---- the guard ------------------------------------------------------------------------------------------------------------


def assert_guarded(device, operator):
    assert device.calls, "the method never reached the device"
    for call in device.calls:
        if call.name == "keep_states":  # (of evaluate_subspace_matrices: runs the circuits, reads no operator)
            continue
        assert call.held, f"{call.name} ran outside operator_lock"
        assert call.operator is operator, f"{call.name} ran under another evaluator's operator"
    assert device.installed == [operator]
    assert not device.operator_lock.held()


# (gradient_method is read by evaluate_gradients and evaluate_gradients_device_to_device alone)
OPERATOR_GUARD_CASES = [(name, "parameter_shift") for name in sorted(OPERATOR_GUARDED)] + \
                       [(name, method) for name in ("evaluate_gradients", "evaluate_gradients_device_to_device")
                        for method in ("adjoint", "auto")]


@pytest.mark.parametrize("name,method", OPERATOR_GUARD_CASES)
def test_operator_evaluator_reaches_the_device_under_the_lock_with_its_own_operator(name, method, any_matrix_will_do):
    device = RecordingDevice()
    device.sweep_first = name == "evaluate_gradients"  # ("auto": a mixed batch on the host; the device form takes it whole)
    operator = DIAGONAL if name == "top_states" else NON_DIAGONAL  # (top_states installs a diagonal operator only)
    ev = operator_evaluator(device, operator=operator, method=method)
    leave_another_operator(device)
    OPERATOR_GUARDED[name](ev, make_circuits(), VALUES)
    assert_guarded(device, operator)


def test_top_states_of_a_non_diagonal_operator_installs_nothing_but_holds_the_lock():
    device = RecordingDevice()
    ev = operator_evaluator(device)
    leave_another_operator(device)
    _states, _probabilities, values = ev.top_states(make_circuits(), VALUES, 2)
    assert values is None and device.installed == [] and device._operator is OTHER
    assert [c.held for c in device.calls] == [True]


# (evaluate_device_to_device refuses more than MAX_CVAR_SHOTS shots)
SAMPLER_GUARD_CASES = [(name, mode) for name in sorted(SAMPLER_GUARDED) for mode in sorted(SAMPLER_MODES)
                       if (name, mode) != ("evaluate_device_to_device", "host cvar")]


@pytest.mark.parametrize("name,mode", SAMPLER_GUARD_CASES)
def test_sampler_evaluator_reaches_the_device_under_the_lock_with_its_own_operator(name, mode):
    shots, alpha = SAMPLER_MODES[mode]
    device = RecordingDevice()
    ev = sampler_evaluator(device, shots=shots, alpha=alpha)
    leave_another_operator(device)
    SAMPLER_GUARDED[name](ev, make_circuits(), VALUES)
    assert_guarded(device, DIAGONAL)


@pytest.mark.parametrize("name", sorted(OPERATOR_UNGUARDED))
def test_methods_that_do_not_read_the_operator_leave_the_one_that_was_there(name):
    device = RecordingDevice()
    ev = operator_evaluator(device)
    leave_another_operator(device)
    OPERATOR_UNGUARDED[name](ev, make_circuits(), VALUES)
    assert device.calls and device.installed == [] and device._operator is OTHER


@pytest.mark.parametrize("mode", sorted(SAMPLER_MODES))
def test_sampler_observables_restore_the_operator_that_was_there(mode):
    shots, alpha = SAMPLER_MODES[mode]
    device = RecordingDevice()
    ev = sampler_evaluator(device, shots=shots, alpha=alpha)
    leave_another_operator(device)
    rows = SAMPLER_UNGUARDED["evaluate_observables"](ev, make_circuits(), VALUES)
    assert np.shape(rows) == (3, 2) and device._operator is OTHER


def test_every_public_evaluate_method_is_in_the_lists():
    for cls, listed in ((OperatorCircuitEvaluator, {**OPERATOR_GUARDED, **OPERATOR_UNGUARDED}),
                        (OperatorSamplerCircuitEvaluator, {**SAMPLER_GUARDED, **SAMPLER_UNGUARDED})):
        public = {name for name, _ in inspect.getmembers(cls, inspect.isfunction) if name.startswith("evaluate_")}
        assert public <= set(listed), f"{cls.__name__}: not covered here: {sorted(public - set(listed))}"


def test_the_device_guard_installs_only_what_is_not_there_and_releases_on_failure():
    device = RecordingDevice()
    with StatevectorDevice.with_operator(device, DIAGONAL) as inside:
        assert inside is device and device.operator_lock.held() and device._operator is DIAGONAL
        with StatevectorDevice.with_operator(device, DIAGONAL):  # (re-entrant, and nothing to install)
            pass
        assert device.operator_lock.held()
    assert device.installed == [DIAGONAL] and not device.operator_lock.held()

    def refuse(operator):
        raise ValueError("no")

    device.set_operator = refuse
    with pytest.raises(ValueError, match="no"):
        with StatevectorDevice.with_operator(device, OTHER):
            pass
    assert not device.operator_lock.held()


# ---- composition ----------------------------------------------------------------------------------------------------------


def same_circuit(a: CircuitIR, b: CircuitIR) -> bool:
    return bytes(a._bytes) == bytes(b._bytes) and a.num_parameters == b.num_parameters and a._kept_state is b._kept_state


def batches_seen(device, n):
    """The batches of ``n`` circuits the device was handed (circuit_costs asks one circuit at a time: those as one batch)."""
    batches = [call.circuits for call in device.calls if len(call.circuits) == n]
    singles = [call.circuits[0] for call in device.calls if call.name == "circuit_cost"]
    if len(singles) == n:
        batches.append(singles)
    assert batches, "the method never handed the device the batch"
    return batches


def all_methods(kind):
    guarded, unguarded = (OPERATOR_GUARDED, OPERATOR_UNGUARDED) if kind == "operator" else (SAMPLER_GUARDED, SAMPLER_UNGUARDED)
    return {**guarded, **unguarded}


def make_evaluator(kind, device, name, initial):
    if kind == "sampler":
        return sampler_evaluator(device, initial)
    return operator_evaluator(device, initial, operator=DIAGONAL if name == "top_states" else NON_DIAGONAL)


EVERY_METHOD = [("operator", name) for name in sorted(all_methods("operator"))] + \
               [("sampler", name) for name in sorted(all_methods("sampler"))]


@pytest.mark.parametrize("kind,name", EVERY_METHOD)
def test_every_method_hands_the_device_the_circuits_behind_the_initial_state(kind, name, any_matrix_will_do):
    device = RecordingDevice()
    ev = make_evaluator(kind, device, name, INITIAL)
    circuits = make_circuits()
    device.calls.clear()
    all_methods(kind)[name](ev, circuits, VALUES)
    batches = batches_seen(device, len(circuits))
    for batch in batches:
        assert all(same_circuit(got, INITIAL.compose(c)) for got, c in zip(batch, circuits))


# (keep_states and evaluate_subspace_matrices keep their circuits' states: the device refuses circuits that continue one)
@pytest.mark.parametrize("kind,name", [pair for pair in EVERY_METHOD if pair[1] not in ("evaluate_subspace_matrices", "keep_states")])
def test_circuits_on_a_kept_state_are_passed_through_as_they_are(kind, name, any_matrix_will_do):
    device = RecordingDevice()
    ev = make_evaluator(kind, device, name, INITIAL)
    circuits = [c.continue_from(FakeKept()) for c in make_circuits()]
    device.calls.clear()
    all_methods(kind)[name](ev, circuits, VALUES)
    batches = batches_seen(device, len(circuits))
    assert all(got is c for batch in batches for got, c in zip(batch, circuits))


@pytest.mark.parametrize("kind,name", BY_IDENTITY)
def test_the_by_identity_methods_hand_over_the_same_composed_list_object(kind, name, any_matrix_will_do):
    device = RecordingDevice()
    ev = make_evaluator(kind, device, name, INITIAL)
    circuits = make_circuits()
    device.calls.clear()
    for _ in range(2):
        all_methods(kind)[name](ev, circuits, VALUES)
    first, second = device.calls
    assert first.circuits is second.circuits and first.circuits is not circuits
    all_methods(kind)[name](ev, list(circuits), VALUES)  # (another list object: composed anew)
    assert device.calls[2].circuits is not first.circuits


@pytest.mark.parametrize("kind,name", [pair for pair in EVERY_METHOD if pair not in BY_IDENTITY])
def test_no_other_method_keeps_a_list_by_identity(kind, name, any_matrix_will_do):
    device = RecordingDevice()
    ev = make_evaluator(kind, device, name, INITIAL)
    all_methods(kind)[name](ev, make_circuits(), VALUES)
    assert ev._composed_lists is None


@pytest.mark.parametrize("name", ["evaluate_variances", "evaluate_covariances", "evaluate_overlaps"])
def test_a_list_changed_in_place_is_seen(name):
    """The one intended change of behaviour: these three kept the composed list by the identity of the caller's list."""
    device = RecordingDevice()
    ev = operator_evaluator(device, INITIAL)
    circuits = make_circuits()
    call = all_methods("operator")[name]
    call(ev, circuits, VALUES)
    circuits[0] = CircuitIR(N_QUBITS).u(ParamRef(0), ParamRef(1), 0.25, 2)
    device.calls.clear()
    call(ev, circuits, VALUES)
    assert same_circuit(device.calls[0].circuits[0], INITIAL.compose(circuits[0]))


def test_none_pairs_are_dropped_before_the_device_sees_the_batch():
    circuits = make_circuits()
    for ev in (operator_evaluator(RecordingDevice(), INITIAL), sampler_evaluator(RecordingDevice(), INITIAL)):
        ev._device.calls.clear()
        assert len(ev.evaluate_circuits([circuits[0], None, circuits[2]], [VALUES[0], VALUES[1], None])) == 1
        (call,) = ev._device.calls
        assert len(call.circuits) == 1 and same_circuit(call.circuits[0], INITIAL.compose(circuits[0]))


# ---- pickle ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["operator", "sampler"])
def test_a_pickled_evaluator_travels_with_empty_caches(kind):
    ev = make_evaluator(kind, RecordingDevice(), "evaluate_circuits", INITIAL)
    circuits = make_circuits()
    ev.evaluate_device_to_device(circuits, FakeTensor(3, 3), FakeTensor(3))
    assert ev._composed_lists is not None and ev._composed_lists[0] is circuits and len(ev._composed) == 3
    ev._last_matrix = ("a weak reference to a tensor of this process",)
    restored = pickle.loads(pickle.dumps(ev))
    assert restored._composed_lists is None and restored._last_matrix is None and len(restored._composed) == 0
    assert ev._composed_lists is not None and ev._last_matrix is not None  # (the original keeps its own)
    assert restored.n_qubits == N_QUBITS and same_circuit(restored._initial_state_circuit, INITIAL)


# ---- wrt ------------------------------------------------------------------------------------------------------------------

WRT_SENTENCE = "wrt must be None, one list of parameter indices, or one list per circuit"


def test_the_wrt_normaliser_on_every_form():
    assert ce._wrt_per_circuit(3, None) is None
    assert ce._wrt_per_circuit(3, [0, 1]) == [[0, 1]] * 3
    assert ce._wrt_per_circuit(3, []) == [[], [], []]
    assert ce._wrt_per_circuit(3, (np.int64(1),)) == [[1]] * 3
    assert ce._wrt_per_circuit(3, [[1, 0], [], [2]]) == [[1, 0], [], [2]]
    assert ce._wrt_per_circuit(0, None) is None and ce._wrt_per_circuit(0, []) == []
    with pytest.raises(ValueError, match=WRT_SENTENCE):
        ce._wrt_per_circuit(3, [[0], [1]])


def test_wrt_arguments_for_circuits_of_2_0_and_3_parameters():
    circuits = make_circuits()
    assert [c.num_parameters for c in circuits] == [2, 0, 3]

    def check(wrt, offsets, flat, counts):
        got = StatevectorDevice._wrt_arguments(circuits, wrt)
        if offsets is None:
            assert got[0] is None and got[1] is None
        else:
            assert got[0].dtype == np.int64 and got[0].tolist() == offsets
            assert got[1].dtype == np.int32 and got[1].tolist() == flat
        assert got[2].dtype == np.int64 and got[2].tolist() == counts

    check(None, None, None, [2, 0, 3])
    check([0], [0, 1, 2, 3], [0, 0, 0], [1, 1, 1])
    check([1, 0], [0, 2, 4, 6], [1, 0, 1, 0, 1, 0], [2, 2, 2])
    check([], [0, 0, 0, 0], [0], [0, 0, 0])  # (one padding entry: the library is never handed an empty array)
    check([[1, 0], [], [2]], [0, 2, 2, 3], [1, 0, 2], [2, 0, 1])
    with pytest.raises(ValueError, match=WRT_SENTENCE):
        StatevectorDevice._wrt_arguments(circuits, [[0], [1]])
