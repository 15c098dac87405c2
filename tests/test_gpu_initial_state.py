"""GPU test of ``initial_state_circuit=``: an evaluator built with an initial state returns, from EVERY method, the bits an
evaluator built without one returns for ``initial.compose(circuit)``.  The second evaluator lives on a device of its own, so
nothing the first one registered or cached can answer for it.  4 qubits, 3 circuits of 2, 0 and 3 parameters, fp64; one
parameter is read by two angle slots, so ``gradient_method="auto"`` splits the batch between the adjoint sweep and parameter
shift.  The comparison is exact: both sides run the same kernels on the same gates.  Run on the MI355X box with -m gpu."""

import numpy as np
import pytest

from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, OperatorSamplerCircuitEvaluator, StatevectorDevice
from queasars_amd.ir import CircuitIR, ParamRef, PauliOperator

pytestmark = pytest.mark.gpu

N = 4
P = ParamRef
INITIAL = CircuitIR(N).u(0.9, 0.2, 0.3, 0).u(0.5, 0.6, 0.7, 1).u(1.3, 1.0, 1.1, 2).u(0.4, 0.8, 1.2, 3)
VALUES = [[0.37, -0.81], [], [1.21, 0.45, -0.63]]
NON_DIAGONAL = PauliOperator(["XIZI", "ZZII", "IYYI", "IIXX", "ZIIZ"], [0.5, -1.0, 0.25, 0.75, -0.4])
DIAGONAL = PauliOperator(["ZIZI", "IZII", "ZZIZ", "IIIZ"], [1.0, -0.5, 0.3, 0.2])
OBSERVABLES = [PauliOperator(["ZIII"], [1.0]), PauliOperator(["IXIY", "ZZII"], [1.0, 0.5]), PauliOperator(["IIZZ"], [-2.0])]
DIAGONAL_OBSERVABLES = [PauliOperator(["ZIII"], [1.0]), PauliOperator(["IZZI", "IIIZ"], [1.0, 0.5])]
PLAN_WRT = [[0, 1], [], [1, 2]]  # (parameter 0 of the third circuit has no shift rule: two slots read it)


def make_circuits():
    return [
        CircuitIR(N).u(P(0), 0.3, P(1), 0).cu3(0.5, 0.1, 0.2, 0, 1).u(0.2, 0.4, 0.6, 3),
        CircuitIR(N).u(0.7, 0.1, 0.9, 2).cu3(1.1, 0.3, 0.5, 2, 3),
        CircuitIR(N).u(P(0), P(1), 0.4, 1).cu3(P(2), 0.2, P(0), 1, 2),
    ]


def same_bits(a, b) -> bool:
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)) and any(isinstance(x, (tuple, list, dict, np.ndarray)) for x in a):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None or isinstance(a, (str, bool)):
        return a is b or a == b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def devices():
    return StatevectorDevice(N, dtype="fp64"), StatevectorDevice(N, dtype="fp64")


class Pair:
    """Evaluator A (initial state, the caller's circuits) and evaluator B (none, the composed circuits, its own device)."""

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.circuits = make_circuits()
        self.composed = [INITIAL.compose(c) for c in self.circuits]

    def check(self, call, what):
        got, want = call(self.a, self.circuits), call(self.b, self.composed)
        assert same_bits(got, want), f"{what}: {got!r} != {want!r}"
        return got


@pytest.fixture
def operator_pair(devices):
    return Pair(OperatorCircuitEvaluator(NON_DIAGONAL, initial_state_circuit=INITIAL, statevector_device=devices[0],
                                         gradient_method="auto"),
                OperatorCircuitEvaluator(NON_DIAGONAL, statevector_device=devices[1], gradient_method="auto"))


def sampler_pair(devices, shots, alpha):
    return Pair(OperatorSamplerCircuitEvaluator(shots, DIAGONAL, alpha=alpha, initial_state_circuit=INITIAL, seed=11,
                                                statevector_device=devices[0]),
                OperatorSamplerCircuitEvaluator(shots, DIAGONAL, alpha=alpha, seed=11, statevector_device=devices[1]))


def point_matrix():
    """The points as rows of a device matrix, one entry wider than the longest vector (rows need not be aligned), complete."""
    import torch

    matrix = torch.zeros((len(VALUES), 4), dtype=torch.float64, device="cuda")
    for i, p in enumerate(VALUES):
        matrix[i, : len(p)] = torch.tensor(p, dtype=torch.float64)
    torch.cuda.synchronize()
    return matrix


def read_back(tensor) -> np.ndarray:
    import torch

    torch.cuda.synchronize()
    return tensor.cpu().numpy()


def test_host_methods_of_the_operator_evaluator(operator_pair):
    pair = operator_pair
    values = pair.check(lambda ev, c: ev.evaluate_circuits(c, VALUES), "evaluate_circuits")
    assert len(values) == 3 and len(set(values)) == 3  # (three different states: nothing here is trivially equal)
    pair.check(lambda ev, c: ev.evaluate_circuits([c[0], None, c[2]], [VALUES[0], VALUES[1], VALUES[2]]), "None pairs")
    pair.check(lambda ev, c: ev.evaluate_variances(c, VALUES, with_values=True), "evaluate_variances")
    pair.check(lambda ev, c: ev.evaluate_observables(c, VALUES, OBSERVABLES), "evaluate_observables")
    pair.check(lambda ev, c: ev.evaluate_covariances(c, VALUES, OBSERVABLES, with_values=True), "evaluate_covariances")
    pair.check(lambda ev, c: ev.evaluate_subspace_matrices(c, VALUES), "evaluate_subspace_matrices")
    pair.check(lambda ev, c: ev.top_states(c, VALUES, 5), "top_states")
    pair.check(lambda ev, c: ev.circuit_costs(c), "circuit_costs")

    def overlaps(ev, c):
        kept = ev.keep_states(c[:2], VALUES[:2])
        try:
            return ev.evaluate_overlaps(c, VALUES, kept), ev.evaluate_overlaps(c, VALUES, kept, with_operator=True)
        finally:
            for state in kept:
                state.release()

    pair.check(overlaps, "keep_states / evaluate_overlaps")

    def continued(ev, c):
        (state,) = ev.keep_states(c[:1], VALUES[:1])
        layer = CircuitIR(N).u(P(0), 0.1, 0.2, 1).cu3(0.3, P(1), 0.5, 1, 3).continue_from(state)
        try:
            return ev.evaluate_circuits([layer, layer], [[0.3, -0.2], [1.4, 0.6]])
        finally:
            state.release()

    pair.check(continued, "a circuit on a kept state")


def test_gradients_of_the_operator_evaluator(operator_pair):
    import torch

    pair = operator_pair
    gradients = pair.check(lambda ev, c: ev.evaluate_gradients(c, VALUES), "evaluate_gradients")
    assert [g.shape for g in gradients] == [(2,), (0,), (3,)]
    assert pair.a.last_gradient_evaluation_counts == pair.b.last_gradient_evaluation_counts
    assert pair.a.last_gradient_evaluation_counts[2] == 1  # (the shared parameter sent the third circuit to the sweep)
    pair.check(lambda ev, c: ev.evaluate_gradients(c, VALUES, PLAN_WRT), "evaluate_gradients, wrt per circuit")
    matrix = point_matrix()

    def device_to_device(ev, c):
        rows = []
        for _ in range(2):  # (the same list twice: the second call takes the composed list kept by identity)
            out = torch.full((3, 5), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ev.evaluate_gradients_device_to_device(c, matrix, out)
            rows.append(read_back(out))
        assert same_bits(rows[0], rows[1])
        return rows[0]

    rows = pair.check(device_to_device, "evaluate_gradients_device_to_device")
    assert all(same_bits(rows[i, : len(g)], g) for i, g in enumerate(gradients))

    def planned(ev, c):
        out = torch.full((3, 3), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        plan = ev.gradient_plan(c, matrix, out, PLAN_WRT)
        try:
            plan.run(matrix, out)
            return read_back(out)
        finally:
            plan.close()

    pair.check(planned, "gradient_plan")


def test_device_matrix_methods_of_the_operator_evaluator(operator_pair):
    import torch

    pair = operator_pair
    matrix = point_matrix()
    values = pair.check(lambda ev, c: ev.evaluate_circuits(c, VALUES), "evaluate_circuits")
    assert same_bits(pair.check(lambda ev, c: ev.evaluate_circuits(c, matrix), "evaluate_circuits of a matrix"), values)
    assert same_bits(pair.check(lambda ev, c: ev.evaluate_device_parameters(c, matrix), "evaluate_device_parameters"),
                     np.asarray(values))

    def device_to_device(ev, c):
        seen = []
        for _ in range(2):  # (the same list twice)
            out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ev.evaluate_device_to_device(c, matrix, out)
            seen.append(read_back(out))
        assert same_bits(seen[0], seen[1])
        return seen[0]

    assert same_bits(pair.check(device_to_device, "evaluate_device_to_device"), np.asarray(values))

    def to_device(ev, c):
        out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert ev.evaluate_circuits_to_device(c, VALUES, out.data_ptr()) is True
        return read_back(out)

    assert same_bits(pair.check(to_device, "evaluate_circuits_to_device"), np.asarray(values))


@pytest.mark.parametrize("shots,alpha", [(None, 1.0), (None, 0.4), (64, 0.4), (64, 1.0), (StatevectorDevice.MAX_CVAR_SHOTS + 1, 0.4)])
def test_the_sampler_evaluator(devices, shots, alpha):
    import torch

    pair = sampler_pair(devices, shots, alpha)
    pair.check(lambda ev, c: ev.evaluate_circuits(c, VALUES), "evaluate_circuits")
    pair.check(lambda ev, c: ev.evaluate_circuits([None, c[1], c[2]], VALUES), "None pairs")
    pair.check(lambda ev, c: ev.evaluate_observables(c, VALUES, DIAGONAL_OBSERVABLES), "evaluate_observables")
    pair.check(lambda ev, c: ev.top_states(c, VALUES, 5), "top_states")
    if shots is not None and shots > StatevectorDevice.MAX_CVAR_SHOTS:
        return  # (evaluate_device_to_device refuses what the host sorts)
    matrix = point_matrix()

    def device_to_device(ev, c):
        seen = []
        for _ in range(2):  # (the same list twice; with shots each call draws the evaluator's next seed)
            out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ev.evaluate_device_to_device(c, matrix, out)
            seen.append(read_back(out))
        return seen

    seen = pair.check(device_to_device, "evaluate_device_to_device")
    if shots is None:
        assert same_bits(seen[0], seen[1])
        assert same_bits(seen[0], np.asarray(pair.a.evaluate_circuits(pair.circuits, VALUES)))
