"""GPU tests of the exact CVaR gradients (include/qsv.h: qsv_cvar_gradient_circuits / qsv_cvar_gradient_device).

Sizes: n = 6 (fewer states than one workgroup's threads), n = 12 (exactly one chunk of the threshold search, two tiles of the
sweep) and n = 14 (four chunks, eight tiles).  Circuits: ``population_circuits(n, 2, 3, seed)`` for seeds 0 - 2 and one
unstructured circuit with a parameter that several angle slots read.  Operators: an Ising operator, the same with its
coefficients rounded (the boundary lies inside a tie) and a tie-free random diagonal.  alpha in {0.05, 0.25, 0.5, 0.9}.

The reference is tests/cvar_gradient_reference.py, which tests/test_cvar_gradient_host.py holds to the dense derivative and to
central differences.  It names a boundary state from cumulative sums; every comparison first asserts that the case's
identification margin is above 1e-9 (fp64) or 1e-6 (fp32): further from a change of the boundary than the sums' rounding.

fp64 bound: EXP_TOL * max(1, |w|_inf) with EXP_TOL = 1e-10 of tests/test_gpu_adjoint.py and |w|_inf = max_i max(t - v_i, 0) / alpha:
the sweep is linear in its seed, so its error scales with the seed's norm.  Run on the MI355X box with -m gpu."""

import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import adjoint_reference
import circuit_families as cf
import cvar_gradient_reference as ref
import helpers
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import (
    CircuitEvaluatorException,
    ExactCVaRCircuitEvaluator,
    OperatorSamplerCircuitEvaluator,
    StatevectorDevice,
)
from queasars_amd.ir import CircuitIR, ParamRef, PauliOperator

pytestmark = pytest.mark.gpu

P = ParamRef
EXP_TOL = 1e-10
SIZES = (6, 12, 14)
ALPHAS = (0.05, 0.25, 0.5, 0.9)
OPERATORS = ("ising", "rounded", "tie-free")
MARGIN = {"fp64": 1e-9, "fp32": 1e-6}


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def assert_same_bits(got, want, what=""):
    assert len(got) == len(want), what
    for e, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), f"{what}: circuit {e}"


def assert_same_call(got, want, what):
    assert_same_bits(got[0], want[0], what + ": gradients")
    assert np.array_equal(bits(got[1]), bits(want[1])), what + ": values"
    assert np.array_equal(bits(got[2]), bits(want[2])), what + ": thresholds"


# ---- the cases, built once --------------------------------------------------------------------------------------------------


@lru_cache(maxsize=None)
def operator(n: int, kind: str) -> PauliOperator:
    ising = helpers.random_ising_operator(n, seed=n)
    if kind == "ising":
        return ising
    if kind == "rounded":
        op = PauliOperator(list(ising.labels), np.round(ising.coeffs.real))
        assert len(np.unique(ref.diagonal_values(op))) < (1 << n) // 4  # (ties)
        return op
    op = helpers.random_pauli_operator(n, 4 * n, seed=n, alphabet="IZ")
    assert len(np.unique(ref.diagonal_values(op))) == 1 << n
    return op


@lru_cache(maxsize=None)
def evaluations(n: int):
    """[(circuit, parameters)]: nine individuals and the circuit with a shared parameter."""
    out = []
    for seed in range(3):
        _, circuits, params = helpers.population_circuits(n, 2, 3, seed)
        out += [(c, list(p)) for c, p in zip(circuits, params)]
    shared, values = cf.generic(n, 40, share=0.3, literal=0.2)
    assert min(shared.gradient_terms(), default=0) < 0  # (a parameter that several angle slots read)
    out.append((shared, list(values)))
    return tuple(out)


@lru_cache(maxsize=None)
def reference(n: int, kind: str, alpha: float, dtype: str = "fp64"):
    """The CVaRCase of every evaluation: computed once, shared, never written to.  "fp32": the boundary as a single-precision
    handle finds it, from the probabilities of the rounded state; everything else in double precision."""
    out = []
    for circuit, params in evaluations(n):
        case = ref.cvar_gradient(circuit, params, operator(n, kind), alpha, np.complex128 if dtype == "fp64" else np.complex64)
        case.gradient.setflags(write=False)
        out.append(case)
    return tuple(out)


@lru_cache(maxsize=None)
def stage(n: int, kind: str, dtype: str = "fp64") -> StatevectorDevice:
    device = StatevectorDevice(n, dtype=dtype)
    device.set_operator(operator(n, kind))
    return device


def host_call(device, circuits, params, alpha, wrt=None):
    """(gradients, values, thresholds) of the host entry point."""
    return device.cvar_gradients(list(circuits), list(params), alpha, wrt, with_values=True, with_thresholds=True)


def device_call(device, circuits, params, alpha, wrt=None):
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
    thresholds = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    device.cvar_gradients_of_device_parameters(list(circuits), matrix.data_ptr(), width, 0, out.data_ptr(), out_width, alpha, wrt,
                                               values.data_ptr(), thresholds.data_ptr())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for e, count in enumerate(counts):
        assert np.array_equal(bits(host[e, count:]), np.zeros(out_width - count, dtype=np.uint64)), f"padding of row {e}"
    return [host[e, :count].copy() for e, count in enumerate(counts)], values.cpu().numpy(), thresholds.cpu().numpy()


# ---- 1. fp64 against the reference -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n", SIZES)
def test_fp64_matches_the_reference(n, kind):
    device = stage(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    worst_g = worst_v = worst_x = 0.0  # (errors over their bounds: gradient, value, value against the exact CVaR)
    chunks = set()
    for alpha in ALPHAS:
        want = reference(n, kind, alpha)
        margin = min(case.identification_margin for case in want)
        assert margin > MARGIN["fp64"], (alpha, margin)
        gradients, values, thresholds = host_call(device, circuits, params, alpha)
        exact = np.asarray(device.exact_cvar_batch(circuits, params, alpha))
        for e, case in enumerate(want):
            bound = EXP_TOL * max(1.0, case.weight_norm)
            error_g = float(np.abs(gradients[e] - case.gradient).max(initial=0.0))
            error_v, error_x = abs(values[e] - case.value), abs(values[e] - exact[e])
            worst_g, worst_v, worst_x = max(worst_g, error_g / bound), max(worst_v, error_v / bound), max(worst_x, error_x / bound)
            assert error_g <= bound and error_v <= bound and error_x <= bound, (alpha, e, error_g, error_v, error_x, bound)
            assert thresholds[e] == case.threshold, (alpha, e)
            chunks.add(case.boundary // 4096)
        # the counters: the seed pass is the one state sweep the H application is; the value-only call sweeps nothing
        stats = device.adjoint_stats()
        device.adjoint_gradients(circuits, params)
        plain = device.adjoint_stats()
        assert all(stats[key] == plain[key] for key in ("n_state_sweeps", "n_gates", "n_runs"))
        _, only_values, only_thresholds = host_call(device, circuits, params, alpha, wrt=[])
        stats = device.adjoint_stats()
        assert stats["n_state_sweeps"] == len(circuits) and stats["n_runs"] == 0 and stats["n_gates"] == 0
        assert np.array_equal(bits(only_values), bits(values)) and np.array_equal(bits(only_thresholds), bits(thresholds))
    print(f"n = {n}, {kind}: largest error over its bound: gradient {worst_g:.3e}, value {worst_v:.3e}, value against exact_cvar_batch "
          f"{worst_x:.3e}; boundary chunks {sorted(chunks)}")
    # not a test of zeros, and not the plain gradient
    case = reference(n, kind, 0.25)[0]
    plain = adjoint_reference.gradient(circuits[0], params[0], operator(n, kind))
    assert float(np.abs(case.gradient).max()) > 1e-3 and float(np.abs(case.gradient - plain).max()) > 1e-3


def test_the_boundaries_at_fourteen_qubits_fall_in_every_chunk():
    chunks = {case.boundary // 4096 for kind in OPERATORS for alpha in ALPHAS for case in reference(14, kind, alpha)}
    assert chunks == {0, 1, 2, 3}


# ---- 2. single precision -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n", (6, 12))
def test_fp32_within_four_times_the_plain_sweeps_error(n, kind):
    """The allowance: four times the error of the existing fp32 adjoint sweep on the same circuits under the same operator, measured
    in the same run against its fp64 reference, times max(1, |w|_inf / max |v|): the seed's norm over the operator's.  Four is the
    spread between cases that tests/test_gpu_adjoint.py reports for single precision (1.0e-8 to 4.0e-8)."""
    device = stage(n, kind, "fp32")
    op = operator(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    plain = device.adjoint_gradients(circuits, params)
    plain_error = max(float(np.abs(g - adjoint_reference.gradient(c, p, op)).max(initial=0.0)) for g, c, p in zip(plain, circuits, params))
    largest = float(np.abs(ref.diagonal_values(op)).max())
    worst, worst_v = 0.0, 0.0
    for alpha in ALPHAS:
        want, seen = reference(n, kind, alpha), reference(n, kind, alpha, "fp32")
        margin = min(min(a.identification_margin, b.identification_margin) for a, b in zip(want, seen))
        assert margin > MARGIN["fp32"], (alpha, margin)
        gradients, values, thresholds = host_call(device, circuits, params, alpha)
        for e, case in enumerate(want):
            allowance = 4.0 * max(1.0, case.weight_norm / largest) * plain_error
            error = float(np.abs(gradients[e] - case.gradient).max(initial=0.0))
            worst, worst_v = max(worst, error / allowance), max(worst_v, abs(values[e] - case.value) / allowance)
            assert error <= allowance, (alpha, e, error, allowance)
            assert thresholds[e] == case.threshold, (alpha, e)
    print(f"n = {n}, {kind}, fp32: plain sweep error {plain_error:.3e}; CVaR gradient error over its allowance {worst:.3e}, value {worst_v:.3e}")


# ---- 3. bit contracts --------------------------------------------------------------------------------------------------------


def _pool(n: int):
    """Twenty evaluations: the ten circuits at two points each."""
    return [(c, [float(v) * (1.0 - 0.25 * variant) + 0.3 * variant for v in p]) for variant in range(2) for c, p in evaluations(n)]


@pytest.mark.parametrize("n,kind", [(6, "rounded"), (12, "ising"), (14, "tie-free")])
def test_a_row_is_the_same_bits_alone_and_in_any_batch(n, kind):
    device = stage(n, kind)
    alpha = 0.25
    pool = _pool(n)
    alone = [host_call(device, [c], [p], alpha) for c, p in pool]
    rng = np.random.default_rng(n)
    for size in (1, 7, 20):
        order = rng.permutation(len(pool))[:size].tolist()
        circuits, params = [pool[i][0] for i in order], [pool[i][1] for i in order]
        want = ([alone[i][0][0] for i in order], np.asarray([alone[i][1][0] for i in order]), np.asarray([alone[i][2][0] for i in order]))
        assert_same_call(host_call(device, circuits, params, alpha), want, f"a batch of {size}, host")
        assert_same_call(device_call(device, circuits, params, alpha), want, f"a batch of {size}, device")
    allocations = device.adjoint_stats()["n_allocations"]
    for _ in range(2):
        assert_same_call(host_call(device, [pool[0][0]], [pool[0][1]], alpha), alone[0], "the same call again")
    assert device.adjoint_stats()["n_allocations"] == allocations


def test_a_mixed_batch_larger_than_the_launch_group():
    n, kind, alpha = 6, "ising", 0.5
    device = StatevectorDevice(n, group=4)
    assert int(device._lib.qsv_group_size(device._handle)) == 4
    device.set_operator(operator(n, kind))
    pool = _pool(n)[:11]  # (two full launch groups and one of three)
    circuits, params = [c for c, _ in pool], [p for _, p in pool]
    batch = host_call(device, circuits, params, alpha)
    alone = [host_call(device, [c], [p], alpha) for c, p in pool]
    want = ([a[0][0] for a in alone], np.asarray([a[1][0] for a in alone]), np.asarray([a[2][0] for a in alone]))
    assert_same_call(batch, want, "eleven against each evaluation alone")
    back = host_call(device, circuits[::-1], params[::-1], alpha)
    assert_same_call(([g for g in back[0][::-1]], back[1][::-1], back[2][::-1]), batch, "other positions in the launch groups")
    assert_same_call(device_call(device, circuits, params, alpha), batch, "the device entry point")
    assert_same_call(host_call(stage(n, kind), circuits, params, alpha), batch, "another device, another group size")
    device.close()


@pytest.mark.parametrize("n", (6, 14))
def test_wrt_entries_are_the_bits_of_the_full_gradient(n):
    device = stage(n, "ising")
    circuits, params = (list(x) for x in zip(*evaluations(n)[:4]))
    full, values, thresholds = host_call(device, circuits, params, 0.5)
    wrt = [[3, 1], [0], [], [5, 2, 4]]
    for call in (host_call, device_call):
        got = call(device, circuits, params, 0.5, wrt)
        assert_same_call(got, ([g[np.asarray(w, dtype=np.int64)] for g, w in zip(full, wrt)], values, thresholds), call.__name__)
    last = [circuits[0].num_parameters - 1]
    assert_same_bits(device.cvar_gradients(circuits[:1], params[:1], 0.5, last), [full[0][-1:]], "one list for all circuits")


@pytest.mark.parametrize("alpha", (1.0, 1.0 - 5e-6))
@pytest.mark.parametrize("n", (6, 12))
def test_alpha_one_is_the_plain_adjoint_call(n, alpha):
    device = stage(n, "tie-free")
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    want, want_values = device.adjoint_gradients(circuits, params, return_values=True)
    top = float(ref.diagonal_values(operator(n, "tie-free")).max())
    for call in (host_call, device_call):
        gradients, values, thresholds = call(device, circuits, params, alpha)
        assert_same_bits(gradients, want, call.__name__)
        assert np.array_equal(bits(values), bits(want_values)) and np.array_equal(thresholds, np.full(len(circuits), top))
    wrt = [[1, 0]] * len(circuits)
    assert_same_bits(device.cvar_gradients(circuits, params, alpha, wrt), device.adjoint_gradients(circuits, params, wrt), "wrt")


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", (6, 12))
def test_the_state_zero_with_the_minimum_elsewhere(n):
    """|0...0> from id gates alone, and from a gate whose angles do nothing to it: every state below v_0 carries no mass, so the
    boundary is state 0, the seed is zero and the value is v_0."""
    device, values = stage(n, "ising"), ref.diagonal_values(operator(n, "ising"))
    assert int(np.argmin(values)) != 0
    idle = CircuitIR(n)
    for q in range(n):
        idle.id(q)
    phases = CircuitIR(n).u(0.0, P(0), P(1), 1).cu3(P(2), P(0), 0.3, 1, 0)  # (the control is never set)
    for alpha in ALPHAS:
        gradients, got, thresholds = host_call(device, [idle, phases], [[], [0.4, -0.7, 1.1]], alpha)
        assert gradients[0].shape == (0,) and np.array_equal(gradients[1], np.zeros(3))
        assert np.array_equal(got, np.full(2, values[0])) and np.array_equal(thresholds, np.full(2, values[0]))


@pytest.mark.parametrize("n", (6, 12))
def test_more_than_alpha_of_the_mass_on_the_lowest_state(n):
    device, values = stage(n, "tie-free"), ref.diagonal_values(operator(n, "tie-free"))
    lowest = int(np.argmin(values))
    circuit = CircuitIR(n)
    for q in range(n):
        circuit.u(np.pi * ((lowest >> q) & 1), 0.0, 0.0, q)
    circuit.u(P(0), P(1), 0.0, n - 1)  # (cos^2(0.1) = 0.990 of the mass stays)
    gradients, got, thresholds = host_call(device, [circuit], [[0.2, 0.5]], 0.9)
    assert np.array_equal(gradients[0], np.zeros(2)) and thresholds[0] == values[lowest] and got[0] == values[lowest]
    case = ref.cvar_gradient(circuit, [0.2, 0.5], operator(n, "tie-free"), 0.9)
    assert case.boundary == 0 and not case.gradient.any()


def stopped_early(n: int, kind: str, alpha: float, short: float):
    """(circuit, parameters) whose two lowest occupied states hold ``alpha - short`` of the mass: with ``short`` inside the
    tolerance of the stopping rule the accumulation ends there, below alpha, and leaves ``short`` out.  The state is a product
    of rotations of qubits 0 and 1 on top of the operator's lowest state x, so four states are occupied; which of x ^ 1, x ^ 2,
    x ^ 3 comes second in value decides which angle is solved for."""
    values = ref.diagonal_values(operator(n, kind))
    x = int(np.argmin(values))
    second = min((1, 2, 3), key=lambda flip: (values[x ^ flip], x ^ flip))
    wanted = alpha - short
    if second == 3:  # stay^2 = cos^2(theta / 2) per qubit: wanted = a b + (1 - a)(1 - b)
        a = 0.95
        b = (wanted - (1.0 - a)) / (2.0 * a - 1.0)
    else:  # the qubit that x and the second state differ in takes any angle, the other one holds `wanted`
        a, b = (0.848, wanted) if second == 1 else (wanted, 0.848)
    circuit = CircuitIR(n)
    for q in range(n):
        circuit.u(np.pi * ((x >> q) & 1), 0.0, 0.0, q)
    circuit.u(P(0), 0.0, 0.0, 0).u(P(1), 0.0, 0.0, 1)
    return circuit, [2.0 * float(np.arccos(np.sqrt(a))), 2.0 * float(np.arccos(np.sqrt(b)))]


@pytest.mark.parametrize("n", (6, 12))
def test_the_stopping_rule_fires_below_alpha(n):
    """s > 0: the value is t (1 - s / alpha) + Re<psi|lambda>, the reference's accumulation, and what exact_cvar_batch returns."""
    kind, alpha, short = "tie-free", 0.9, 3e-6
    device = stage(n, kind)
    circuit, params = stopped_early(n, kind, alpha, short)
    case = ref.cvar_gradient(circuit, params, operator(n, kind), alpha)
    assert case.boundary > 0 and abs(case.left_out - short) < 1e-12 and case.identification_margin > 1e-6
    assert float(np.abs(case.gradient).max()) > 1e-3 and abs(case.threshold * case.left_out / alpha) > 1e-7  # (s is seen in the value)
    gradients, values, thresholds = host_call(device, [circuit], [params], alpha)
    bound = EXP_TOL * max(1.0, case.weight_norm)
    assert float(np.abs(gradients[0] - case.gradient).max()) <= bound and thresholds[0] == case.threshold
    assert abs(values[0] - case.value) <= bound and abs(values[0] - device.exact_cvar_batch([circuit], [params], alpha)[0]) <= bound
    assert_same_call(device_call(device, [circuit], [params], alpha), (gradients, values, thresholds), "the device entry point")


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------


def _raw(dev, circuits, params, alpha, wrt=None):
    """qsv_cvar_gradient_circuits as the C ABI returns it: (return code, message)."""
    ids, offsets, flat = dev._batch_arguments(circuits, params)
    wrt_offsets, wrt_flat, counts = StatevectorDevice._wrt_arguments(circuits, wrt)
    out, values = np.full(max(1, int(counts.sum())), np.nan), np.full(len(circuits), np.nan)
    rc = dev._lib.qsv_cvar_gradient_circuits(
        dev._handle, float(alpha), len(circuits), _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(flat),
        None if wrt_offsets is None else _lib.as_ptr(wrt_offsets), None if wrt_flat is None else _lib.as_ptr(wrt_flat),
        _lib.as_ptr(out), _lib.as_ptr(values), None)
    return rc, _lib.last_error(dev._lib, dev._handle)


def test_refusals_leave_the_handle_working():
    import torch

    n, kind, alpha = 6, "ising", 0.25
    circuits, params = (list(x) for x in zip(*evaluations(n)[:3]))
    dev = StatevectorDevice(n)
    want = stage(n, kind).cvar_gradients(circuits, params, alpha)
    width = max(c.num_parameters for c in circuits)
    matrix = torch.zeros((len(circuits), width), dtype=torch.float64, device="cuda")
    out = torch.zeros((len(circuits), width), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def device_form(**pointers):
        return dev.cvar_gradients_of_device_parameters(circuits, matrix.data_ptr(), width, 0, out.data_ptr(), width, alpha, **pointers)

    def refused(code, word, circuits=circuits, params=params, alpha=alpha, wrt=None):
        rc, message = _raw(dev, circuits, params, alpha, wrt)
        assert rc == code and word in message, (rc, message)

    sentence = "the exact CVaR needs a diagonal operator (call qsv_set_operator with I/Z terms only)"
    refused(_lib.QSV_E_STATE, sentence)  # (no operator)
    dev.set_operator(helpers.random_pauli_operator(n, 9, seed=2))
    refused(_lib.QSV_E_STATE, sentence)
    with pytest.raises(CircuitEvaluatorException, match="needs a diagonal operator"):
        dev.cvar_gradients(circuits, params, alpha)
    with pytest.raises(CircuitEvaluatorException, match="needs a diagonal operator"):
        device_form()
    dev.set_operator(operator(n, kind))
    assert_same_bits(dev.cvar_gradients(circuits, params, alpha), want, "after the refusals")
    refused(_lib.QSV_E_ARG, "alpha must be in (0, 1]", alpha=0.0)
    refused(_lib.QSV_E_ARG, "alpha must be in (0, 1]", alpha=1.5)
    refused(_lib.QSV_E_ARG, "alpha must be in (0, 1]", alpha=float("nan"))
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match="alpha"):
            dev.cvar_gradients(circuits, params, bad)
    refused(_lib.QSV_E_ARG, "wrt index", wrt=[[circuits[0].num_parameters], [], []])
    kept = dev.keep_states(circuits[:1], params[:1])
    continued = CircuitIR(n).u(P(0), 0.0, 0.0, 2).continue_from(kept[0])
    refused(_lib.QSV_E_UNSUPPORTED, "CVaR gradients of a circuit on a kept state are not built", circuits=[continued], params=[[0.4]])
    with pytest.raises(ValueError, match="kept state"):
        dev.cvar_gradients([continued], [[0.4]], alpha)
    assert dev._lib.qsv_cvar_gradient_circuits(dev._handle, alpha, 0, None, None, None, None, None, None, None, None) == _lib.QSV_OK
    # host pointers and a row too short, at the device entry point
    host = np.zeros(8)
    with pytest.raises(ValueError, match="device_out_values is not memory of this handle's device"):
        device_form(values_ptr=host.ctypes.data)
    with pytest.raises(ValueError, match="device_out_thresholds is not memory of this handle's device"):
        device_form(thresholds_ptr=host.ctypes.data)
    with pytest.raises(ValueError, match="out_width 1 is too small"):
        dev.cvar_gradients_of_device_parameters(circuits, matrix.data_ptr(), width, 0, out.data_ptr(), 1, alpha)
    # inside an open batch, from the thread that holds it: both entry points
    ids, offsets, flat = dev._batch_arguments(circuits, params)
    counts = np.diff(offsets).astype(np.int64)
    values = np.zeros(len(circuits))
    assert dev._lib.qsv_eval_begin(dev._handle, len(circuits), _lib.as_ptr(ids), _lib.as_ptr(counts)) == _lib.QSV_OK
    refused(_lib.QSV_E_STATE, "(qsv_cvar_gradient_circuits goes between batches)")
    rc = dev._lib.qsv_cvar_gradient_device(dev._handle, alpha, len(circuits), _lib.as_ptr(ids), width, C.c_void_p(matrix.data_ptr()), None,
                                           None, None, width, C.c_void_p(out.data_ptr()), None, None)
    assert rc == _lib.QSV_E_STATE and "(qsv_cvar_gradient_device goes between batches)" in _lib.last_error(dev._lib, dev._handle)
    assert dev._lib.qsv_eval_push(dev._handle, 0, len(circuits), _lib.as_ptr(flat)) == _lib.QSV_OK
    assert dev._lib.qsv_eval_end(dev._handle, _lib.as_ptr(values)) == _lib.QSV_OK
    assert_same_bits(dev.cvar_gradients(circuits, params, alpha), want, "after the open batch")
    # a new operator is sorted again
    dev.set_operator(operator(n, "tie-free"))
    assert_same_bits(dev.cvar_gradients(circuits, params, alpha), stage(n, "tie-free").cvar_gradients(circuits, params, alpha), "another operator")
    dev.close()


# ---- 6. the evaluator and the solver ----------------------------------------------------------------------------------------


def test_the_evaluator_is_the_exact_sampler_evaluator_with_gradients():
    n, kind, alpha = 6, "ising", 0.25
    op = operator(n, kind)
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    initial = CircuitIR(n)
    for q in range(n):
        initial.u(0.3 + 0.1 * q, 0.2, -0.1, q)
    ev = ExactCVaRCircuitEvaluator(op, alpha, initial_state_circuit=initial)
    parent = OperatorSamplerCircuitEvaluator(None, op, alpha=alpha, initial_state_circuit=initial, statevector_device=ev.statevector_device)
    assert ev.evaluate_circuits(circuits, params) == parent.evaluate_circuits(circuits, params)
    values, gradients = ev.evaluate_values_and_gradients(circuits, params)
    want = [ref.cvar_gradient(initial.compose(c), p, op, alpha) for c, p in zip(circuits, params)]
    for e, case in enumerate(want):
        bound = EXP_TOL * max(1.0, case.weight_norm)
        assert float(np.abs(gradients[e] - case.gradient).max(initial=0.0)) <= bound and abs(values[e] - case.value) <= bound
    assert np.array_equal(ev.evaluate_thresholds(circuits, params), np.asarray([case.threshold for case in want]))
    assert_same_bits(ev.evaluate_gradients(circuits, params), gradients, "evaluate_gradients")
    assert ev.last_gradient_evaluations == len(circuits) and ev.last_gradient_evaluation_counts == [1] * len(circuits)
    assert len(ev.metric_tensors(circuits[:2], params[:2])) == 2


def _jssp_operator():
    import jssp_instances as inst
    from queasars_amd.job_shop_scheduling import JSSPDomainWallHamiltonianEncoder

    encoder = JSSPDomainWallHamiltonianEncoder(inst.small_asymmetric(), makespan_limit=4, **inst.NOTEBOOK_PENALTIES)
    assert encoder.n_qubits == 5
    return encoder.get_problem_hamiltonian()


def _solver(optimizer):
    from queasars_amd.evqe.solver import EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    return EVQEMinimumEigensolver(EVQEMinimumEigensolverConfiguration(
        optimizer=optimizer, population_size=4, max_generations=2, random_seed=5,
        n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
        use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
        parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
    ))


@pytest.mark.parametrize("optimizer", ("adam", "natural gradient"))
def test_compute_minimum_eigenvalue_on_a_small_jssp_hamiltonian(optimizer):
    from queasars_amd.evqe import EVQEPopulation
    from queasars_amd.evqe.solver import Adam, NaturalGradient

    op, alpha = _jssp_operator(), 0.5
    chosen = Adam(maxiter=6, lr=0.05) if optimizer == "adam" else NaturalGradient(maxiter=6, learning_rate=1e-3, regularization=1.0)
    solver = _solver(chosen)
    ev = ExactCVaRCircuitEvaluator(op, alpha)
    population = EVQEPopulation.random_population(ev.n_qubits, 2, 4, True, random_seed=solver._population_seed)
    start = ev.evaluate_circuits([ind.get_parameterized_quantum_circuit() for ind in population.individuals],
                                 [list(ind.parameter_values) for ind in population.individuals])
    result = solver.compute_minimum_eigenvalue(ev)
    print(f"{optimizer}: the initial population's CVaR {np.round(start, 3)}, the result's {result.eigenvalue:.6f}")
    assert result.generations == 2 and np.isfinite(result.eigenvalue) and result.eigenvalue <= min(start)
    assert ev.statevector_device.adjoint_stats()["n_runs"] >= 1
    # the same configuration on the plain sampler evaluator is still turned away
    with pytest.raises(ValueError, match="needs an evaluator with evaluate_gradients"):
        _solver(chosen).compute_minimum_eigenvalue(OperatorSamplerCircuitEvaluator(None, op, alpha=alpha, statevector_device=ev.statevector_device))
