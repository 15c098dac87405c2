"""GPU tests of the folded-spectrum and variance costs (include/qsv.h: qsv_folded_gradient_circuits / qsv_folded_gradient_device;
DESIGN.md 4.21).

Sizes: n = 6 (fewer amplitudes than a workgroup's threads), n = 12 (two tiles of 2^11, two workgroups' shares) and n = 14 (eight
tiles, eight workgroups' shares).  Operators: an Ising operator (no x-mask group: the fused diagonal pass), a general operator (a
diagonal part and four x-mask groups -- one mask bit 0 alone, one bit n - 1 alone, so the gather crosses lanes and crosses tiles --
with strings of an odd number of Y factors) and one x-mask group of many strings (tests/operator_families.py).  Circuits:
``population_circuits(n, 2, 3, seed)`` for seeds 0 and 1 and one unstructured circuit with a parameter that several angle slots
read (tests/circuit_families.py).  Centres: a target inside the spectrum, one outside it, and each evaluation's own mean.

The reference is tests/folded_reference.py, which tests/test_folded_host.py holds to the dense derivative of (H - c)^2 and to
central differences.  fp64 bound: EXP_TOL * max(1, (sum |c_k| + |c|)^2) with EXP_TOL = 1e-10 of tests/test_gpu_adjoint.py: the
sweep is linear in its seed, whose norm (sum |c_k| + |c|)^2 bounds.  Run on the MI355X box with -m gpu."""

import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import adjoint_reference
import circuit_families as cf
import dense_gradient
import folded_reference as fr
import helpers
import operator_families as of
import variance_reference as vr
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import (
    CircuitEvaluatorException,
    FoldedSpectrumCircuitEvaluator,
    OperatorCircuitEvaluator,
    StatevectorDevice,
)
from queasars_amd.ir import CircuitIR, ParamRef, PauliOperator

pytestmark = pytest.mark.gpu

P = ParamRef
EXP_TOL = 1e-10
SIZES = (6, 12, 14)
OPERATORS = ("ising", "general", "one group")
CENTRES = ("inside", "outside", "mean")


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def assert_same_bits(got, want, what=""):
    assert len(got) == len(want), what
    for e, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), f"{what}: circuit {e}"


def assert_same_call(got, want, what):
    assert_same_bits(got[0], want[0], what + ": gradients")
    assert np.array_equal(bits(got[1]), bits(want[1])), what + ": costs"
    assert np.array_equal(bits(got[2]), bits(want[2])), what + ": energies"


# ---- the cases, built once --------------------------------------------------------------------------------------------------


@lru_cache(maxsize=None)
def operator(n: int, kind: str) -> PauliOperator:
    if kind == "ising":
        return helpers.random_ising_operator(n, seed=n)
    if kind == "one group":
        # The mask is qubits 0 and n - 1: the gather crosses lanes and tiles at once.  (one_group's "random" mask covers ten of twelve
        # qubits; under it <H> and its gradient vanish identically on two-layer individuals, and the plain fp32 sweep's error, the
        # yardstick of the fp32 test, with them.)
        return of.one_group(n, {6: 40, 12: of.K_CHUNK + 1, 14: 64}[n], (1 << (n - 1)) | 1)
    rng = np.random.default_rng(n)
    low, high, wide = 1, 1 << (n - 1), (1 << (n - 1)) | 0b110
    terms = [(0, 0b11, 0.8), (0, high | 1, -0.6), (0, 1 << (n // 2), 0.45), (0, 0, 0.3),       # the diagonal part (with an identity)
             (low, 0, 0.7), (low, low | 0b100, -0.35), (low, high, 0.25),                       # X_0, Y_0 Z_2 (ny = 1), X_0 Z_(n-1)
             (high, 0, -0.55), (high, high, 0.4), (high, 0b11, 0.2),                             # X_(n-1), Y_(n-1) (ny = 1), X_(n-1) Z_0 Z_1
             (wide, 0, 0.5), (wide, 0b010, -0.3), (wide, 0b110, 0.15), (wide, wide, 0.35),      # ny = 0, 1, 2, 3
             (0b11, 0b01, 0.6), (0b11, 0b11, -0.25)]                                             # Y_0 X_1 (ny = 1), Y_0 Y_1
    op = of.from_masks(n, [(x, z, c * float(rng.uniform(0.5, 1.5))) for x, z, c in terms])
    has_diagonal, groups = of.groups_of(op)
    assert has_diagonal and len(groups) == 4
    assert any(bin(x & z).count("1") & 1 for x, z, _ in of.masks_of(op))
    return op


@lru_cache(maxsize=None)
def evaluations(n: int):
    """[(circuit, parameters)]: six individuals and the circuit with a shared parameter."""
    out = []
    for seed in range(2):
        _, circuits, params = helpers.population_circuits(n, 2, 3, seed)
        out += [(c, list(p)) for c, p in zip(circuits, params)]
    shared, values = cf.generic(n, 40, share=0.3, literal=0.2)
    assert min(shared.gradient_terms(), default=0) < 0  # (a parameter that several angle slots read)
    out.append((shared, list(values)))
    return tuple(out)


def target_of(n: int, kind: str, centre: str):
    width = fr.spread(operator(n, kind))
    return {"inside": 0.2 * width, "outside": -1.5 * width, "mean": None}[centre]


@lru_cache(maxsize=None)
def reference(n: int, kind: str, centre: str):
    """The FoldedCase of every evaluation: computed once, shared, never written to."""
    out = []
    for circuit, params in evaluations(n):
        case = fr.folded(circuit, params, operator(n, kind), target_of(n, kind, centre))
        case.gradient.setflags(write=False)
        out.append(case)
    return tuple(out)


@lru_cache(maxsize=None)
def stage(n: int, kind: str, dtype: str = "fp64") -> StatevectorDevice:
    device = StatevectorDevice(n, dtype=dtype)
    device.set_operator(operator(n, kind))
    return device


def host_call(device, circuits, params, target, wrt=None):
    """(gradients, costs, energies) of the host entry point."""
    return device.folded_gradients(list(circuits), list(params), target, wrt, with_values=True, with_energies=True)


def device_call(device, circuits, params, target, wrt=None):
    """The same from the device entry point: points in a padded matrix of an odd row length, everything read back after one
    synchronise; the padding behind a row's entries is zeros."""
    import torch

    n = len(circuits)
    width = max(len(p) for p in params) + 1
    width += 1 - width % 2
    matrix = torch.zeros((n, width), dtype=torch.float64, device="cuda")
    for e, p in enumerate(params):
        matrix[e, : len(p)] = torch.tensor(p, dtype=torch.float64)
    counts = [c.num_parameters if wrt is None else len(wrt if np.ndim(wrt[0]) == 0 else wrt[e]) for e, c in enumerate(circuits)]
    out_width = max(counts) + 3
    out = torch.full((n, out_width), float("nan"), dtype=torch.float64, device="cuda")
    values = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    energies = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    device.folded_gradients_of_device_parameters(list(circuits), matrix.data_ptr(), width, 0, out.data_ptr(), out_width, target, wrt,
                                                 values.data_ptr(), energies.data_ptr())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for e, count in enumerate(counts):
        assert np.array_equal(bits(host[e, count:]), np.zeros(out_width - count, dtype=np.uint64)), f"padding of row {e}"
    return [host[e, :count].copy() for e, count in enumerate(counts)], values.cpu().numpy(), energies.cpu().numpy()


# ---- 1. fp64 against the reference -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n", SIZES)
def test_fp64_matches_the_reference(n, kind):
    device, op = stage(n, kind), operator(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    gathers = kind != "ising"
    worst_g = worst_v = worst_e = 0.0  # (errors over their bounds: rows, cost, energy)
    for centre in CENTRES:
        target, want = target_of(n, kind, centre), reference(n, kind, centre)
        gradients, costs, energies = host_call(device, circuits, params, target)
        stats = device.adjoint_stats()
        for e, case in enumerate(want):
            bound = EXP_TOL * max(1.0, fr.seed_norm(op, case.centre))
            error_g = float(np.abs(gradients[e] - case.gradient).max(initial=0.0))
            error_v, error_e = abs(costs[e] - case.cost), abs(energies[e] - case.energy)
            print(f"n = {n}, {kind}, {centre}, evaluation {e}: rows {error_g:.3e} cost {error_v:.3e} energy {error_e:.3e} bound {bound:.3e}")
            worst_g, worst_v, worst_e = max(worst_g, error_g / bound), max(worst_v, error_v / bound), max(worst_e, error_e / bound)
            assert error_g <= bound and error_v <= bound and error_e <= bound, (centre, e, error_g, error_v, error_e, bound)
            assert costs[e] >= 0.0
        # the counters: the residual and the seed pass are a state sweep each (an operator of its diagonal alone: one for both)
        device.adjoint_gradients(circuits, params)
        plain = device.adjoint_stats()
        assert stats["n_state_sweeps"] == plain["n_state_sweeps"] + len(circuits) * (2 if gathers else 1)
        assert stats["n_gates"] == plain["n_gates"] and stats["n_runs"] == plain["n_runs"] > 0
        # the value-only call launches no run, and returns the same cost and energy
        _, only_costs, only_energies = host_call(device, circuits, params, target, wrt=[])
        stats = device.adjoint_stats()
        assert stats["n_runs"] == 0 and stats["n_gates"] == 0 and stats["n_state_sweeps"] == 2 * len(circuits)
        assert np.array_equal(bits(only_costs), bits(costs)) and np.array_equal(bits(only_energies), bits(energies))
        assert np.abs(energies - device.expectation_values(circuits, params)).max() <= EXP_TOL * max(1.0, fr.spread(op))
    print(f"n = {n}, {kind}: largest error over its bound: rows {worst_g:.3e}, cost {worst_v:.3e}, energy {worst_e:.3e}")
    # not a test of zeros, and not the plain gradient
    case = reference(n, kind, "mean")[0]
    plain = adjoint_reference.gradient(circuits[0], params[0], op)
    assert float(np.abs(case.gradient).max()) > 1e-3 and float(np.abs(case.gradient - plain).max()) > 1e-3


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n", SIZES)
def test_the_centred_cost_is_the_variance(n, kind):
    device, op = stage(n, kind), operator(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    _, want = vr.reference(op, [helpers.oracle_state(c, p) for c, p in zip(circuits, params)])
    _, costs, _ = host_call(device, circuits, params, None, wrt=[])
    _, one_pass = device.variances(circuits, params)
    tolerance = vr.tol_fp64(op)
    print(f"n = {n}, {kind}: centred cost against variance_reference {np.abs(costs - want).max():.3e}, against evaluate_variances "
          f"{np.abs(costs - one_pass).max():.3e}, allowed {tolerance:.3e}")
    assert np.abs(costs - want).max() <= tolerance and np.abs(costs - one_pass).max() <= tolerance


# ---- 2. single precision -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n", (6, 12))
def test_fp32_within_four_times_the_plain_sweeps_error(n, kind):
    """The allowance: four times the error of the existing fp32 adjoint sweep on the same circuits under the same operator, measured
    in the same run against its fp64 reference, times max(1, (sum |c_k| + |c|)^2 / sum |c_k|): the seed's norm over the
    operator's, as DESIGN.md 4.20 scales its own."""
    device, op = stage(n, kind, "fp32"), operator(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    plain = device.adjoint_gradients(circuits, params)
    plain_error = max(float(np.abs(g - adjoint_reference.gradient(c, p, op)).max(initial=0.0)) for g, c, p in zip(plain, circuits, params))
    worst = worst_v = 0.0
    for centre in CENTRES:
        want = reference(n, kind, centre)
        gradients, costs, energies = host_call(device, circuits, params, target_of(n, kind, centre))
        for e, case in enumerate(want):
            allowance = 4.0 * max(1.0, fr.seed_norm(op, case.centre) / fr.spread(op)) * plain_error
            error = float(np.abs(gradients[e] - case.gradient).max(initial=0.0))
            worst, worst_v = max(worst, error / allowance), max(worst_v, abs(costs[e] - case.cost) / allowance)
            assert error <= allowance, (centre, e, error, allowance)
            assert costs[e] >= 0.0
    print(f"n = {n}, {kind}, fp32: plain sweep error {plain_error:.3e}; folded rows' error over their allowance {worst:.3e}, cost {worst_v:.3e}")


# ---- 3. exact edges ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", SIZES)
def test_the_plus_state_is_an_eigenstate_of_the_sum_of_x(n):
    """|+...+> under sum_j X_j (eigenvalue n): the variance and its gradient vanish, to the bound."""
    op = PauliOperator(["I" * q + "X" + "I" * (n - 1 - q) for q in range(n)], [1.0] * n)
    device = StatevectorDevice(n)
    device.set_operator(op)
    circuit = CircuitIR(n)
    for q in range(n):
        circuit.u(P(2 * q), P(2 * q + 1), 0.0, q)
    point = [np.pi / 2, 0.0] * n
    bound = EXP_TOL * max(1.0, fr.seed_norm(op, float(n)))
    for call in (host_call, device_call):
        gradients, costs, energies = call(device, [circuit], [point], None)
        print(f"n = {n}, {call.__name__}: variance {costs[0]:.3e}, largest row entry {np.abs(gradients[0]).max():.3e}, E - n {energies[0] - n:.3e}")
        assert 0.0 <= costs[0] <= bound and np.abs(gradients[0]).max() <= bound and abs(energies[0] - n) <= bound
    device.close()


@pytest.mark.parametrize("n", SIZES)
def test_a_basis_state_at_its_own_value_costs_nothing_and_never_less(n):
    device, op = stage(n, "ising"), operator(n, "ising")
    for state in (0, 5, (1 << n) - 1, (1 << (n - 1)) | 2):
        circuit = CircuitIR(n)
        for q in range(n):
            circuit.u(np.pi * ((state >> q) & 1), 0.0, 0.0, q)
        circuit.u(P(0), 0.0, P(1), 1)  # (at theta = 0: a phase on the basis state)
        point = [0.0, 0.4]
        value = float(device.expectation_values([circuit], [point])[0])
        bound = EXP_TOL * max(1.0, fr.seed_norm(op, value))
        for target in (value, None):
            gradients, costs, energies = host_call(device, [circuit], [point], target)
            assert 0.0 <= costs[0] <= bound and abs(energies[0] - value) <= bound, (state, target, costs[0])
            assert np.abs(gradients[0]).max() <= bound


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n", (6, 12))
def test_the_target_at_the_mean_is_the_mean(n, kind):
    device, op = stage(n, kind), operator(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    mean = host_call(device, circuits, params, None)
    for e, case in enumerate(reference(n, kind, "mean")):
        at_e = host_call(device, circuits[e:e + 1], params[e:e + 1], case.energy)
        bound = EXP_TOL * max(1.0, fr.seed_norm(op, case.energy))
        assert float(np.abs(at_e[0][0] - mean[0][e]).max(initial=0.0)) <= bound and abs(at_e[1][0] - mean[1][e]) <= bound
        assert abs(at_e[2][0] - mean[2][e]) <= bound


# ---- 4. bit contracts --------------------------------------------------------------------------------------------------------


def _pool(n: int):
    """Fourteen evaluations: the seven circuits at two points each."""
    return [(c, [float(v) * (1.0 - 0.25 * variant) + 0.3 * variant for v in p]) for variant in range(2) for c, p in evaluations(n)]


@pytest.mark.parametrize("n,kind,centre", [(6, "general", "mean"), (6, "ising", "inside"), (12, "one group", "inside"), (14, "general", "mean"),
                                           (14, "ising", "mean")])
def test_a_mixed_batch_larger_than_the_launch_group(n, kind, centre):
    target = target_of(n, kind, centre)
    device = StatevectorDevice(n, group=4)
    assert int(device._lib.qsv_group_size(device._handle)) == 4
    device.set_operator(operator(n, kind))
    pool = _pool(n)[:11]  # (two full launch groups and one of three)
    circuits, params = [c for c, _ in pool], [p for _, p in pool]
    batch = host_call(device, circuits, params, target)
    alone = [host_call(device, [c], [p], target) for c, p in pool]
    want = ([a[0][0] for a in alone], np.asarray([a[1][0] for a in alone]), np.asarray([a[2][0] for a in alone]))
    assert_same_call(batch, want, "eleven against each evaluation alone")
    back = host_call(device, circuits[::-1], params[::-1], target)
    assert_same_call(([g for g in back[0][::-1]], back[1][::-1], back[2][::-1]), batch, "other positions in the launch groups")
    assert_same_call(device_call(device, circuits, params, target), batch, "the device entry point")
    assert_same_call(host_call(stage(n, kind), circuits, params, target), batch, "another device, another group size")
    allocations = device.adjoint_stats()["n_allocations"]
    for _ in range(2):
        assert_same_call(host_call(device, circuits, params, target), batch, "the same call again")
    assert device.adjoint_stats()["n_allocations"] == allocations
    device.close()


@pytest.mark.parametrize("kind", ("ising", "general"))
@pytest.mark.parametrize("n", (6, 14))
def test_wrt_entries_are_the_bits_of_the_full_gradient(n, kind):
    device = stage(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)[:4]))
    for target in (target_of(n, kind, "inside"), None):
        full, costs, energies = host_call(device, circuits, params, target)
        wrt = [[3, 1], [0], [], [5, 2, 4]]
        for call in (host_call, device_call):
            got = call(device, circuits, params, target, wrt)
            assert_same_call(got, ([g[np.asarray(w, dtype=np.int64)] for g, w in zip(full, wrt)], costs, energies), call.__name__)
        last = [circuits[0].num_parameters - 1]
        assert_same_bits(device.folded_gradients(circuits[:1], params[:1], target, last), [full[0][-1:]], "one list for all circuits")


# ---- 5. the neighbours keep their bits ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ("ising", "general"))
def test_folded_calls_leave_a_replayed_batch_the_adjoint_sweep_and_the_variance_their_bits(kind):
    n = 12
    op = operator(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    evaluator = OperatorCircuitEvaluator(op, gradient_method="adjoint")
    dev = evaluator.statevector_device
    before = evaluator.evaluate_circuits(circuits, params)
    replays = dev.replayed_pushes()
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert dev.replayed_pushes() == replays + 1  # (the second call did replay)
    gradients = evaluator.evaluate_gradients(circuits, params)
    variances = evaluator.evaluate_variances(circuits, params, with_values=True)
    for target in (target_of(n, kind, "inside"), None):
        folded = FoldedSpectrumCircuitEvaluator(op, target, statevector_device=dev)
        values, rows = folded.evaluate_values_and_gradients(circuits, params)
        assert folded.evaluate_circuits(circuits, params) == values.tolist()
        assert_same_bits(folded.evaluate_gradients(circuits, params), rows, "evaluate_gradients")
        assert evaluator.evaluate_circuits(circuits, params) == before
        assert evaluator.evaluate_circuits(circuits, params) == before
        assert_same_bits(evaluator.evaluate_gradients(circuits, params), gradients, "the adjoint sweep after a folded call")
        assert evaluator.evaluate_variances(circuits, params, with_values=True) == variances
    assert dev.replayed_pushes() > replays + 1


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------


def _raw(dev, circuits, params, centre, target, wrt=None):
    """qsv_folded_gradient_circuits as the C ABI returns it: (return code, message)."""
    ids, offsets, flat = dev._batch_arguments(circuits, params)
    wrt_offsets, wrt_flat, counts = StatevectorDevice._wrt_arguments(circuits, wrt)
    out, values = np.full(max(1, int(counts.sum())), np.nan), np.full(len(circuits), np.nan)
    rc = dev._lib.qsv_folded_gradient_circuits(
        dev._handle, int(centre), float(target), len(circuits), _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(flat),
        None if wrt_offsets is None else _lib.as_ptr(wrt_offsets), None if wrt_flat is None else _lib.as_ptr(wrt_flat),
        _lib.as_ptr(out), _lib.as_ptr(values), None)
    return rc, _lib.last_error(dev._lib, dev._handle)


def test_refusals_leave_the_handle_working():
    import torch

    n, kind, target = 6, "general", 0.5
    circuits, params = (list(x) for x in zip(*evaluations(n)[:3]))
    dev = StatevectorDevice(n)
    want = stage(n, kind).folded_gradients(circuits, params, target)
    width = max(c.num_parameters for c in circuits)
    matrix = torch.zeros((len(circuits), width), dtype=torch.float64, device="cuda")
    out = torch.zeros((len(circuits), width), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def device_form(**pointers):
        return dev.folded_gradients_of_device_parameters(circuits, matrix.data_ptr(), width, 0, out.data_ptr(), width, target, **pointers)

    def refused(code, word, circuits=circuits, params=params, centre=0, target=target, wrt=None):
        rc, message = _raw(dev, circuits, params, centre, target, wrt)
        assert rc == code and word in message, (rc, message)

    refused(_lib.QSV_E_STATE, "no operator set (call qsv_set_operator first)")
    with pytest.raises(CircuitEvaluatorException, match="no operator set"):
        dev.folded_gradients(circuits, params, target)
    with pytest.raises(CircuitEvaluatorException, match="no operator set"):
        device_form()
    dev.set_operator(operator(n, kind))
    assert_same_bits(dev.folded_gradients(circuits, params, target), want, "after the refusals")
    for centre in (-1, 2):
        refused(_lib.QSV_E_ARG, "centre must be 0 (the target) or 1 (each evaluation's own mean)", centre=centre)
    for bad in (float("nan"), float("inf")):
        refused(_lib.QSV_E_ARG, "target is not finite", target=bad)
        refused(_lib.QSV_E_ARG, "target is not finite", centre=1, target=bad)
        with pytest.raises(ValueError, match="finite"):
            dev.folded_gradients(circuits, params, bad)
    refused(_lib.QSV_E_ARG, "wrt index", wrt=[[circuits[0].num_parameters], [], []])
    kept = dev.keep_states(circuits[:1], params[:1])
    continued = CircuitIR(n).u(P(0), 0.0, 0.0, 2).continue_from(kept[0])
    refused(_lib.QSV_E_UNSUPPORTED, "folded-spectrum costs of a circuit on a kept state are not built", circuits=[continued], params=[[0.4]])
    with pytest.raises(ValueError, match="kept state"):
        dev.folded_gradients([continued], [[0.4]], target)
    assert dev._lib.qsv_folded_gradient_circuits(dev._handle, 0, target, 0, None, None, None, None, None, None, None, None) == _lib.QSV_OK
    # host pointers and a row too short, at the device entry point
    host = np.zeros(8)
    with pytest.raises(ValueError, match="device_out_values is not memory of this handle's device"):
        device_form(values_ptr=host.ctypes.data)
    with pytest.raises(ValueError, match="device_out_energies is not memory of this handle's device"):
        device_form(energies_ptr=host.ctypes.data)
    with pytest.raises(ValueError, match="out_width 1 is too small"):
        dev.folded_gradients_of_device_parameters(circuits, matrix.data_ptr(), width, 0, out.data_ptr(), 1, target)
    # inside an open batch, from the thread that holds it: both entry points
    ids, offsets, flat = dev._batch_arguments(circuits, params)
    counts = np.diff(offsets).astype(np.int64)
    values = np.zeros(len(circuits))
    assert dev._lib.qsv_eval_begin(dev._handle, len(circuits), _lib.as_ptr(ids), _lib.as_ptr(counts)) == _lib.QSV_OK
    refused(_lib.QSV_E_STATE, "(qsv_folded_gradient_circuits goes between batches)")
    rc = dev._lib.qsv_folded_gradient_device(dev._handle, 0, target, len(circuits), _lib.as_ptr(ids), width, C.c_void_p(matrix.data_ptr()), None,
                                             None, None, width, C.c_void_p(out.data_ptr()), None, None)
    assert rc == _lib.QSV_E_STATE and "(qsv_folded_gradient_device goes between batches)" in _lib.last_error(dev._lib, dev._handle)
    assert dev._lib.qsv_eval_push(dev._handle, 0, len(circuits), _lib.as_ptr(flat)) == _lib.QSV_OK
    assert dev._lib.qsv_eval_end(dev._handle, _lib.as_ptr(values)) == _lib.QSV_OK
    assert_same_bits(dev.folded_gradients(circuits, params, target), want, "after the open batch")
    # another operator, another kind of pass
    dev.set_operator(operator(n, "ising"))
    assert_same_bits(dev.folded_gradients(circuits, params, target), stage(n, "ising").folded_gradients(circuits, params, target), "another operator")
    dev.close()


def test_a_register_above_28_qubits_is_refused():
    """A 29-qubit fp32 handle (one state slot of 4 GiB), asked before the operator is looked for."""
    n = 29
    dev = StatevectorDevice(n, dtype="fp32")
    circuit = CircuitIR(n).u(0.3, 0.2, 0.1, 0)
    rc, message = _raw(dev, [circuit], [[]], 1, 0.0)
    assert rc == _lib.QSV_E_UNSUPPORTED and "28 qubits" in message and "29" in message, (rc, message)
    with pytest.raises(ValueError, match="28 qubits"):
        dev.folded_gradients([circuit], [[]])
    dev.close()


# ---- 7. the evaluator and the drivers ---------------------------------------------------------------------------------------


def test_the_evaluator_behind_an_initial_state():
    n, kind = 6, "general"
    op = operator(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    initial = CircuitIR(n)
    for q in range(n):
        initial.u(0.3 + 0.1 * q, 0.2, -0.1, q)
    for target in (0.4, None):
        ev = FoldedSpectrumCircuitEvaluator(op, target, initial_state_circuit=initial)
        values, gradients = ev.evaluate_values_and_gradients(circuits, params)
        energies = ev.evaluate_energies(circuits, params)
        for e, (c, p) in enumerate(zip(circuits, params)):
            case = fr.folded(initial.compose(c), p, op, target)
            bound = EXP_TOL * max(1.0, fr.seed_norm(op, case.centre))
            assert float(np.abs(gradients[e] - case.gradient).max(initial=0.0)) <= bound
            assert abs(values[e] - case.cost) <= bound and abs(energies[e] - case.energy) <= bound
        assert ev.evaluate_circuits(circuits, params) == values.tolist()
        assert ev.last_gradient_evaluations == len(circuits) and ev.last_gradient_evaluation_counts == [1] * len(circuits)
        assert len(ev.metric_tensors(circuits[:2], params[:2])) == 2


def _solver(optimizer, population_size=4, max_generations=2, randomize=True):
    from queasars_amd.evqe.solver import EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    return EVQEMinimumEigensolver(EVQEMinimumEigensolverConfiguration(
        optimizer=optimizer, population_size=population_size, max_generations=max_generations, random_seed=5,
        n_initial_layers=2, randomize_initial_population_parameters=randomize, speciation_genetic_distance_threshold=2,
        use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
        parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
    ))


def test_a_short_search_towards_an_interior_eigenvalue_and_a_variance_polish():
    """n = 8, a general operator of ten strings whose spectrum NumPy diagonalises.  ``compute_eigenvalue_near`` with Adam, aimed
    at the eigenvalue in the middle of the spectrum, must end below the best folded cost of its initial population;
    ``minimize_variance`` started at the best individual of a short energy search (as the initial state of the polish, whose own
    layers start at the identity) must not raise the variance.  No threshold on convergence: the figures are printed."""
    from queasars_amd.evqe import EVQEPopulation, spectrum
    from queasars_amd.evqe.solver import Adam

    n = 8
    op = helpers.random_pauli_operator(n, 10, seed=8)
    spectrum_values = np.linalg.eigvalsh(dense_gradient.dense_operator(op))
    target = float(spectrum_values[len(spectrum_values) // 2])
    evaluator = OperatorCircuitEvaluator(op, gradient_method="adjoint")
    solver = _solver(Adam(maxiter=10, lr=0.05))
    folded = FoldedSpectrumCircuitEvaluator(op, target, statevector_device=evaluator.statevector_device)
    population = EVQEPopulation.random_population(n, 2, 4, True, random_seed=solver._population_seed)
    start = folded.evaluate_circuits([ind.get_parameterized_quantum_circuit() for ind in population.individuals],
                                     [list(ind.parameter_values) for ind in population.individuals])
    result = spectrum.compute_eigenvalue_near(solver, evaluator, target)
    print(f"target {target:.6f} (spectrum {spectrum_values[0]:.4f} .. {spectrum_values[-1]:.4f}): the initial population's folded cost "
          f"{np.round(start, 4)}, the result's {result.folded_value:.6f} at E = {result.eigenvalue:.6f}, variance {result.eigenvalue_variance:.6f}")
    assert result.generations == 2 and 0.0 <= result.folded_value < min(start)
    assert abs(result.folded_value - (result.eigenvalue_variance + (result.eigenvalue - target) ** 2)) <= 1e-10 * fr.seed_norm(op, target)
    assert evaluator.statevector_device.adjoint_stats()["n_runs"] == 0  # (the result's figures: value-only calls)
    # the polish
    energy = _solver(Adam(maxiter=10, lr=0.05)).compute_minimum_eigenvalue(evaluator)
    best = energy.best_individual
    reached = helpers.bound_copy(best.get_parameterized_quantum_circuit(), list(best.parameter_values))
    polished_from = OperatorCircuitEvaluator(op, initial_state_circuit=reached, statevector_device=evaluator.statevector_device)
    before = FoldedSpectrumCircuitEvaluator(op, None, statevector_device=evaluator.statevector_device).evaluate_circuits([reached], [[]])[0]
    polish = spectrum.minimize_variance(_solver(Adam(maxiter=10, lr=0.001), population_size=2, max_generations=1, randomize=False), polished_from)
    print(f"the energy search's best: E = {energy.eigenvalue:.6f}, variance {before:.6f}; polished: E = {polish.eigenvalue:.6f}, "
          f"variance {polish.eigenvalue_variance:.6f}")
    assert 0.0 <= polish.eigenvalue_variance <= before and polish.folded_value == polish.eigenvalue_variance
