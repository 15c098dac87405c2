"""GPU tests of the deflated (VQD) costs (include/qsv.h: qsv_deflated_gradient_circuits / qsv_deflated_gradient_device; DESIGN.md
4.18) against tests/deflation_reference.py.

Sizes: n = 6 (less than one tile), n = T (exactly the sweep's tile) and n = T + 2 (four tiles, several workgroups).  Kept states:
K = 1, 3, 16, 17 (crosses the 16-wide block of the overlap panels) and 64 (the limit), weights of mixed sign and size.
fp64 tolerances: gradients 1e-10 * max(1, sum |beta|) -- the project's adjoint tolerance scaled to this cost --, values, energies
and overlaps 1e-12 * (sum |c| + sum |beta|).  Run on the MI355X box with -m gpu."""

from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import adjoint_reference
import circuit_families as cf
import deflation_reference as dr
import dense_gradient
import helpers
import test_gpu_adjoint as tga
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import (
    CircuitEvaluatorException,
    DeflatedOperatorCircuitEvaluator,
    OperatorCircuitEvaluator,
    StatevectorDevice,
)
from queasars_amd.ir import CircuitIR, ParamRef

pytestmark = pytest.mark.gpu

P = ParamRef
T = tga.T
SIZES = (6, T, T + 2)
KEPT = (1, 3, 16, 17, 64)
OPERATORS = ("ising", "general")
FP32_FLOOR = 2e-6  # the project's floor, relative to the cost's scale

bits = tga.bits


def cbits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.complex128)).view(np.uint64)


# ---- the cases, built once ---------------------------------------------------------------------------------------------------


@lru_cache(maxsize=None)
def unread(n: int):
    """A circuit with two parameters that no gate reads, and one that two slots read."""
    circuit = CircuitIR(n).u(P(0), P(1), 0.3, 0).cu3(P(3), 0.2, P(1), 0, n - 1).u(P(0), 0.1, 0.2, n // 2)
    circuit.declare_parameters(6)
    return circuit, [0.3, -1.1, 9.0, 0.7, 8.0, 7.0]


@lru_cache(maxsize=None)
def evaluations(n: int):
    """[(circuit, point)]: the generic family (a parameter several slots read), the ladder, an EVQE individual, and a circuit
    with parameters no gate reads."""
    by_name = {name: (c, p) for name, c, p in tga.cases(n)}
    assert tga._has_shared(by_name["generic"][0])
    return (by_name["generic"], by_name["ladder"], by_name["individual 0"], unread(n))


@lru_cache(maxsize=None)
def kept_circuits(n: int):
    """64 (circuit, point) pairs whose states are kept, and their oracle states: first the evaluated circuits themselves at
    slightly perturbed points, so that overlaps of order one occur at every K (the overlaps of unrelated circuits fall with the
    register: 0.03 at the most at n = 13), then a random population."""
    rng = np.random.default_rng(900 + n)
    near = [(c, [float(v + rng.normal(0.0, 0.05)) for v in p]) for c, p in evaluations(n)]
    _, circuits, params = helpers.population_circuits(n, 2, 64 - len(near), seed=900 + n)
    circuits = [c for c, _ in near] + list(circuits)
    params = [p for _, p in near] + [list(p) for p in params]
    states = [helpers.oracle_state(c, p) for c, p in zip(circuits, params)]
    return circuits, params, states


@lru_cache(maxsize=None)
def weights(n: int) -> tuple:
    """64 weights of mixed sign and size: magnitudes from 0.05 to 20, every third one negative."""
    rng = np.random.default_rng(n)
    magnitudes = np.exp(rng.uniform(np.log(0.05), np.log(20.0), size=64))
    return tuple(float(m) * (-1.0 if k % 3 == 1 else 1.0) for k, m in enumerate(magnitudes))


@lru_cache(maxsize=None)
def stage(n: int, kind: str, dtype: str = "fp64"):
    """One device per (register, operator, type) with the 64 kept states on it."""
    device = StatevectorDevice(n, dtype=dtype)
    plain = OperatorCircuitEvaluator(tga.operator(n, kind), statevector_device=device, gradient_method="adjoint")
    circuits, params, _ = kept_circuits(n)
    return SimpleNamespace(device=device, plain=plain, kept=device.keep_states(circuits, params), operator=tga.operator(n, kind))


@lru_cache(maxsize=None)
def reference(n: int, kind: str, k: int):
    """[(gradient, C, E, c)] of evaluations(n) against the first k kept states: computed once, shared, never written to."""
    out = []
    for circuit, params in evaluations(n):
        gradient, value, energy, c = dr.gradient_and_terms(circuit, params, tga.operator(n, kind), kept_circuits(n)[2][:k], weights(n)[:k])
        gradient.setflags(write=False)
        c.setflags(write=False)
        out.append((gradient, value, energy, c))
    return tuple(out)


def host_call(device, circuits, params, kept, betas, wrt=None):
    """(gradients, costs, energies, overlaps) of the host entry point."""
    return device.deflated_gradients(list(circuits), list(params), kept, betas, wrt, with_values=True, with_overlaps=True)


def device_call(device, circuits, params, kept, betas, wrt=None):
    """The same from the device entry point: points in a padded matrix of an odd row length, everything read back after one
    synchronise; the padding behind a row's entries is zeros."""
    import torch

    n, k = len(circuits), len(kept)
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
    overlaps = torch.full((n, max(1, k), 2), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    device.deflated_gradients_of_device_parameters(list(circuits), matrix.data_ptr(), width, 0, out.data_ptr(), out_width, kept, betas, wrt,
                                                   values.data_ptr(), energies.data_ptr(), overlaps.data_ptr() if k else 0)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for e, count in enumerate(counts):
        assert np.array_equal(bits(host[e, count:]), np.zeros(out_width - count, dtype=np.uint64)), f"padding of row {e}"
    s = overlaps.cpu().numpy()[:, :k, :]
    return ([host[e, :count].copy() for e, count in enumerate(counts)], values.cpu().numpy(), energies.cpu().numpy(),
            np.ascontiguousarray(s[..., 0] + 1j * s[..., 1]).reshape(n, k))


def assert_same_call(got, want, what):
    tga.assert_same_bits(got[0], want[0], what + ": gradients")
    assert np.array_equal(bits(got[1]), bits(want[1])), what + ": costs"
    assert np.array_equal(bits(got[2]), bits(want[2])), what + ": energies"
    assert got[3].shape == want[3].shape and np.array_equal(cbits(got[3]), cbits(want[3])), what + ": overlaps"


# ---- 1. fp64 against the reference -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("k", KEPT)
@pytest.mark.parametrize("n", SIZES)
def test_fp64_matches_the_reference(n, k, kind):
    st = stage(n, kind)
    circuits, params = zip(*evaluations(n))
    betas = weights(n)[:k]
    want = reference(n, kind, k)
    gradients, costs, energies, overlaps = host_call(st.device, circuits, params, st.kept[:k], betas)
    scale = dr.scale(st.operator, betas)
    worst_g = max(float(np.abs(g - w[0]).max(initial=0.0)) for g, w in zip(gradients, want))
    worst_c = float(np.abs(costs - np.asarray([w[1] for w in want])).max())
    worst_e = float(np.abs(energies - np.asarray([w[2] for w in want])).max())
    worst_s = max(float(max(np.abs((s - w[3]).real).max(), np.abs((s - w[3]).imag).max())) for s, w in zip(overlaps, want))
    tol_g = 1e-10 * max(1.0, float(np.abs(betas).sum()))
    print(f"n = {n}, K = {k}, {kind}: |dgrad| {worst_g:.3e} (allowed {tol_g:.3e}), |dC| {worst_c:.3e}, |dE| {worst_e:.3e}, "
          f"|dc| {worst_s:.3e} (allowed {1e-12 * scale:.3e}); sum |c| + sum |beta| = {scale:.1f}")
    assert worst_g < tol_g
    assert worst_c < 1e-12 * scale and worst_e < 1e-12 * scale and worst_s < 1e-12 * scale
    # not a test of zeros: the penalties move the gradient, and the parameters no gate reads have entry 0.0
    plain = [adjoint_reference.gradient(c, p, st.operator) for c, p in zip(circuits, params)]
    assert max(float(np.abs(w[0] - g).max()) for w, g in zip(want, plain)) > 1e-3
    assert np.array_equal(bits(gradients[3][[2, 4, 5]]), np.zeros(3, dtype=np.uint64))
    # the counters: one more state sweep per evaluation for the update, none in the value-only call
    stats = st.device.adjoint_stats()
    st.plain.evaluate_gradients(list(circuits), list(params))
    plain_stats = st.device.adjoint_stats()
    assert stats["n_state_sweeps"] == plain_stats["n_state_sweeps"] + len(circuits)
    assert stats["n_gates"] == plain_stats["n_gates"] and stats["n_runs"] == plain_stats["n_runs"]
    _, only_costs, _, _ = host_call(st.device, circuits, params, st.kept[:k], betas, wrt=[])
    stats = st.device.adjoint_stats()
    assert stats["n_state_sweeps"] == len(circuits) and stats["n_runs"] == 0 and stats["n_gates"] == 0
    assert np.array_equal(bits(only_costs), bits(costs))  # (the value does not depend on what is swept)


# ---- 2. bit contracts --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", SIZES)
def test_without_kept_states_it_is_the_adjoint_call(n):
    st = stage(n, "general")
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    want, want_values = st.device.adjoint_gradients(circuits, params, return_values=True)
    got = host_call(st.device, circuits, params, [], [])
    tga.assert_same_bits(got[0], want, "K = 0, host")
    assert np.array_equal(bits(got[1]), bits(want_values)) and np.array_equal(bits(got[2]), bits(want_values))
    assert got[3].shape == (len(circuits), 0)
    assert_same_call(device_call(st.device, circuits, params, [], []), got, "K = 0, device")
    wrt = [[1, 0], [2], [], [5, 3]]
    tga.assert_same_bits(st.device.deflated_gradients(circuits, params, [], [], wrt), st.device.adjoint_gradients(circuits, params, wrt), "K = 0, wrt")


@pytest.mark.parametrize("k", (3, 17, 64))
@pytest.mark.parametrize("n", SIZES)
def test_the_overlaps_are_the_bits_of_the_overlap_call(n, k):
    st = stage(n, "ising")
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    _, _, _, overlaps = host_call(st.device, circuits, params, st.kept[:k], weights(n)[:k])
    want = st.device.overlaps(circuits, params, st.kept[:k])
    assert np.array_equal(cbits(overlaps), cbits(want))


def _pool(n: int):
    """33 evaluations: the eleven cases of tests/test_gpu_adjoint.py at three points each."""
    out = []
    for variant in range(3):
        for _, circuit, params in tga.cases(n):
            out.append((circuit, [float(v) * (1.0 - 0.25 * variant) + 0.3 * variant for v in params]))
    return out


@pytest.mark.parametrize("n,k", [(6, 17), (T, 3)])
def test_a_row_is_the_same_bits_alone_and_in_any_batch(n, k):
    st = stage(n, "general")
    kept, betas = st.kept[:k], weights(n)[:k]
    pool = _pool(n)
    alone = [host_call(st.device, [c], [p], kept, betas) for c, p in pool]
    rng = np.random.default_rng(n)
    for size in (1, 5, 17, 33):
        order = rng.permutation(len(pool))[:size].tolist()
        circuits, params = [pool[i][0] for i in order], [pool[i][1] for i in order]
        want = ([alone[i][0][0] for i in order], np.asarray([alone[i][1][0] for i in order]), np.asarray([alone[i][2][0] for i in order]),
                np.asarray([alone[i][3][0] for i in order]).reshape(size, k))
        assert_same_call(host_call(st.device, circuits, params, kept, betas), want, f"a batch of {size}, host")
        if size in (5, 33):
            assert_same_call(device_call(st.device, circuits, params, kept, betas), want, f"a batch of {size}, device")
    again = host_call(st.device, [pool[0][0]], [pool[0][1]], kept, betas)
    assert_same_call(again, alone[0], "the same call again")


def test_a_batch_larger_than_the_launch_group_at_six_qubits():
    n, k = 6, 17
    device = StatevectorDevice(n, group=4)
    group = int(device._lib.qsv_group_size(device._handle))
    assert group == 4
    device.set_operator(tga.operator(n, "general"))
    kc, kp, _ = kept_circuits(n)
    kept, betas = device.keep_states(kc[:k], kp[:k]), weights(n)[:k]
    pool = _pool(n)[: group + 3]
    circuits, params = [c for c, _ in pool], [p for _, p in pool]
    batch = host_call(device, circuits, params, kept, betas)
    alone = [host_call(device, [c], [p], kept, betas) for c, p in pool]
    want = ([a[0][0] for a in alone], np.asarray([a[1][0] for a in alone]), np.asarray([a[2][0] for a in alone]),
            np.asarray([a[3][0] for a in alone]).reshape(len(pool), k))
    assert_same_call(batch, want, "group + 3 against each evaluation alone")
    back = host_call(device, circuits[::-1], params[::-1], kept, betas)
    assert_same_call(([g for g in back[0][::-1]], back[1][::-1], back[2][::-1], back[3][::-1]), batch, "other positions in the launch groups")
    assert_same_call(device_call(device, circuits, params, kept, betas), batch, "the device entry point")
    # the same bits as on a device with the default launch group
    st = stage(n, "general")
    assert_same_call(host_call(st.device, circuits, params, st.kept[:k], betas), batch, "another device, another group size")
    device.close()


@pytest.mark.parametrize("n", (6, T + 2))
def test_wrt_entries_are_the_bits_of_the_full_gradient(n):
    k = 16
    st = stage(n, "general")
    kept, betas = st.kept[:k], weights(n)[:k]
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    full = host_call(st.device, circuits, params, kept, betas)
    rng = np.random.default_rng(5)
    ragged = [rng.permutation(c.num_parameters)[: 1 + e].tolist() for e, c in enumerate(circuits)]
    ragged[1] = []
    permuted = [rng.permutation(c.num_parameters).tolist() for c in circuits]
    last = [tga._last_gates_parameters(c) for c in circuits]
    for name, wrt in (("one list for all", [2, 0]), ("ragged", ragged), ("permuted", permuted), ("last gates", last)):
        want_rows = [f[np.asarray(wrt if np.ndim(wrt[0]) == 0 else wrt[e], dtype=np.int64)] for e, f in enumerate(full[0])]
        for entry, call in (("host", host_call), ("device", device_call)):
            got = call(st.device, circuits, params, kept, betas, wrt)
            assert_same_call(got, (want_rows,) + tuple(full[1:]), f"{name} / {entry}")


def test_a_repeated_kept_state_is_one_state_with_the_weights_added():
    n = T
    st = stage(n, "general")
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    a, b = st.kept[0], st.kept[1]
    twice = host_call(st.device, circuits, params, [a, b, a], [1.5, -0.7, 2.25])
    once = host_call(st.device, circuits, params, [a, b], [3.75, -0.7])
    assert np.array_equal(cbits(twice[3][:, 0]), cbits(twice[3][:, 2])) and np.array_equal(cbits(twice[3][:, :2]), cbits(once[3]))
    assert max(float(np.abs(g - w).max()) for g, w in zip(twice[0], once[0])) < 1e-10 * 4.45
    assert float(np.abs(twice[1] - once[1]).max()) < 1e-12 * dr.scale(st.operator, [3.75, -0.7])
    assert np.array_equal(bits(twice[2]), bits(once[2]))


# ---- 3. exact cases on a diagonal operator -----------------------------------------------------------------------------------


def _basis_circuit(n: int):
    circuit = CircuitIR(n)
    for q in range(n):
        circuit.u(P(q), 0.0, 0.0, q)
    return circuit


def _basis_point(n: int, state: int) -> list:
    return [np.pi if (state >> q) & 1 else 0.0 for q in range(n)]


def test_exact_costs_at_basis_states_of_a_diagonal_operator():
    n = 6
    op = tga.operator(n, "ising")
    spectrum = np.real(np.diag(dense_gradient.dense_operator(op)))  # brute force: the operator is diagonal
    order = np.argsort(spectrum, kind="stable")
    ground, excited = int(order[0]), int(order[1])
    plain = OperatorCircuitEvaluator(op)
    circuit = _basis_circuit(n)
    kept = plain.keep_states([circuit], [_basis_point(n, ground)])
    ev = DeflatedOperatorCircuitEvaluator(op, kept)
    beta = 2.0 * dr.spread(op)
    assert ev.betas == [beta] and ev.statevector_device is plain.statevector_device
    points = [_basis_point(n, excited), _basis_point(n, ground)]
    costs = ev.evaluate_circuits([circuit, circuit], points)
    gradients = ev.evaluate_gradients([circuit, circuit], points)
    energies, overlaps = ev.evaluate_deflation_terms([circuit, circuit], points)
    tol = 1e-12 * (dr.spread(op) + beta)
    print(f"E_0 = {spectrum[ground]:.6f}, E_1 = {spectrum[excited]:.6f}, beta = {beta:.3f}: costs {costs}, "
          f"largest |gradient| {max(float(np.abs(g).max()) for g in gradients):.3e}")
    assert abs(costs[0] - spectrum[excited]) < tol and abs(costs[1] - (spectrum[ground] + beta)) < tol
    assert abs(energies[0] - spectrum[excited]) < tol and abs(energies[1] - spectrum[ground]) < tol
    assert abs(overlaps[0, 0]) < 1e-12 and abs(abs(overlaps[1, 0]) - 1.0) < 1e-12
    assert all(float(np.abs(g).max()) < 1e-10 * max(1.0, beta) for g in gradients)
    assert costs[0] < costs[1]  # with the default weight the kept ground state is no longer the minimum


# ---- 4. the lower bound ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", OPERATORS)
def test_the_cost_is_bounded_by_the_deflated_matrix(kind):
    n, k = 6, 3
    st = stage(n, kind)
    kc, kp, _ = kept_circuits(n)
    dense = [st.device.statevector(c, p) for c, p in zip(kc[:k], kp[:k])]
    for betas in ([7.0, 2.5, 11.0], [4.0, -3.0, 0.5]):
        low = float(np.linalg.eigvalsh(dr.deflated_matrix(st.operator, dense, betas))[0])
        pool = _pool(n)
        ev = DeflatedOperatorCircuitEvaluator(st.operator, st.kept[:k], betas)
        costs = np.asarray(ev.evaluate_circuits([c for c, _ in pool], [p for _, p in pool]))
        print(f"{kind}, betas {betas}: lowest eigenvalue {low:.6f}, smallest cost {costs.min():.6f}")
        assert np.all(costs >= low - 1e-10)


# ---- 5. single precision -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n,k", [(6, 17), (T, 64), (T + 2, 3)])
def test_fp32_within_four_times_the_plain_sweeps_error(n, k, kind):
    """The allowance: four times the error of the plain fp32 adjoint sweep on the same circuits and points under the operator alone,
    scaled by (sum |c| + sum |beta|) / sum |c|, and never less than 2e-6 * (sum |c| + sum |beta|).

    Measured on the MI355X (largest error / allowance over the six cases): see DESIGN.md 4.18."""
    st = stage(n, kind, "fp32")
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    betas = weights(n)[:k]
    spread, scale = dr.spread(st.operator), dr.scale(st.operator, betas)
    plain = st.plain.evaluate_gradients(circuits, params)
    plain_error = max(float(np.abs(g - adjoint_reference.gradient(c, p, st.operator)).max(initial=0.0)) for g, c, p in zip(plain, circuits, params))
    allowance = max(4.0 * plain_error * scale / spread, FP32_FLOOR * scale)
    want = reference(n, kind, k)
    gradients, costs, energies, overlaps = host_call(st.device, circuits, params, st.kept[:k], betas)
    error_g = max(float(np.abs(g - w[0]).max(initial=0.0)) for g, w in zip(gradients, want))
    error_c = float(np.abs(costs - np.asarray([w[1] for w in want])).max())
    error_e = float(np.abs(energies - np.asarray([w[2] for w in want])).max())
    print(f"n = {n}, K = {k}, {kind}, fp32: plain sweep error {plain_error:.3e}; deflated gradient error {error_g:.3e}, cost {error_c:.3e}, "
          f"energy {error_e:.3e}; allowance {allowance:.3e} (scale {scale:.1f}, sum |c| {spread:.1f})")
    assert error_g <= allowance and error_c <= allowance and error_e <= allowance


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------


def _raw(dev, circuits, params, prefix_ids, betas, n_states=None, n_evals=None, ids_given=True, betas_given=True, wrt=None, out_given=True):
    """qsv_deflated_gradient_circuits as the C ABI returns it: (return code, message, gradient entries back to back, costs)."""
    n = len(circuits)
    ids, offsets, flat = dev._batch_arguments(circuits, params) if n else (np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1))
    prefix = np.asarray(list(prefix_ids) + [0], dtype=np.int32)
    weights_ = np.asarray(list(betas) + [0.0], dtype=np.float64)
    k = len(prefix_ids) if n_states is None else n_states
    wrt_offsets, wrt_flat, counts = StatevectorDevice._wrt_arguments(circuits, wrt) if n else (None, None, np.zeros(0, np.int64))
    out = np.full(max(1, int(counts.sum())), np.nan)
    values = np.full(max(1, n), np.nan)
    rc = dev._lib.qsv_deflated_gradient_circuits(
        dev._handle, k, _lib.as_ptr(prefix) if ids_given else None, _lib.as_ptr(weights_) if betas_given else None,
        n if n_evals is None else n_evals, _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(flat),
        None if wrt_offsets is None else _lib.as_ptr(wrt_offsets), None if wrt_flat is None else _lib.as_ptr(wrt_flat),
        _lib.as_ptr(out) if out_given else None, _lib.as_ptr(values), None, None)
    return rc, _lib.last_error(dev._lib, dev._handle), out, values


def test_refusals_leave_the_handle_working():
    n, k = 6, 3
    op = tga.operator(n, "general")
    circuits, params = (list(x) for x in zip(*evaluations(n)))
    kc, kp, _ = kept_circuits(n)
    dev = StatevectorDevice(n)
    kept = dev.keep_states(kc[:k], kp[:k])
    ids, betas = [s._id for s in kept], list(weights(n)[:k])
    want = reference(n, "general", k)

    def works():
        rc, message, out, values = _raw(dev, circuits, params, ids, betas)
        assert rc == _lib.QSV_OK, message
        assert float(np.abs(out - np.concatenate([w[0] for w in want])).max()) < 1e-10 * max(1.0, float(np.abs(betas).sum()))
        assert float(np.abs(values - np.asarray([w[1] for w in want])).max()) < 1e-12 * dr.scale(op, betas)

    def refused(code, word, **kwargs):
        rc, message, _, _ = _raw(dev, kwargs.pop("circuits", circuits), kwargs.pop("params", params), kwargs.pop("prefix_ids", ids),
                                 kwargs.pop("betas", betas), **kwargs)
        assert rc == code and word in message, (rc, message)

    refused(_lib.QSV_E_STATE, "no operator set")
    with pytest.raises(CircuitEvaluatorException, match="no operator set"):
        dev.deflated_gradients(circuits, params, kept, betas)
    dev.set_operator(op)
    works()
    refused(_lib.QSV_E_ARG, "prefix_ids", ids_given=False)
    refused(_lib.QSV_E_ARG, "betas is null", betas_given=False)
    refused(_lib.QSV_E_ARG, "n_states", n_states=-1)
    refused(_lib.QSV_E_ARG, "betas[1] is not finite", betas=[1.0, float("nan"), 2.0])
    refused(_lib.QSV_E_ARG, "betas[2] is not finite", betas=[1.0, 2.0, float("inf")])
    refused(_lib.QSV_E_ARG, "unknown kept state 9999", prefix_ids=[ids[0], 9999, ids[1]])
    refused(_lib.QSV_E_UNSUPPORTED, "n_states", prefix_ids=[ids[0]] * 65, betas=[1.0] * 65)
    refused(_lib.QSV_E_ARG, "wrt index", wrt=[[circuits[0].num_parameters], [], [], []])
    refused(_lib.QSV_E_ARG, "wrt index", wrt=[[-1], [], [], []])
    refused(_lib.QSV_E_ARG, "out is null", out_given=False)
    refused(_lib.QSV_E_ARG, "bad arguments", n_evals=-1)
    works()
    gone = dev.keep_states(kc[5:6], kp[5:6])[0]
    gone_id = gone._id
    gone.release()
    assert dev.kept_state_count() == k  # (the release has reached the library)
    refused(_lib.QSV_E_ARG, f"unknown kept state {gone_id}", prefix_ids=[ids[0], gone_id, ids[1]])
    continued = CircuitIR(n).u(P(0), 0.0, 0.0, 2).continue_from(kept[0])
    refused(_lib.QSV_E_UNSUPPORTED, "kept state", circuits=[continued], params=[[0.4]])
    with pytest.raises(ValueError, match="kept state"):
        dev.deflated_gradients([continued], [[0.4]], kept, betas)
    assert _raw(dev, [], [], ids, betas, n_evals=0)[0] == _lib.QSV_OK
    # out_width too small, at the device entry point
    import torch

    matrix = torch.zeros((1, circuits[0].num_parameters), dtype=torch.float64, device="cuda")
    out = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="out_width 2 is too small"):
        dev.deflated_gradients_of_device_parameters([circuits[0]], matrix.data_ptr(), circuits[0].num_parameters, 0, out.data_ptr(), 2, kept, betas)
    host = np.zeros(4)
    with pytest.raises(ValueError, match="device_out_values is not memory of this handle's device"):
        dev.deflated_gradients_of_device_parameters([circuits[0]], matrix.data_ptr(), circuits[0].num_parameters, 0, out.data_ptr(), 2, kept, betas,
                                                    wrt=[[0]], values_ptr=host.ctypes.data)
    # inside an open batch, from the thread that holds it
    batch_ids, offsets, flat = dev._batch_arguments(circuits, params)
    counts = np.diff(offsets).astype(np.int64)
    values = np.zeros(len(circuits))
    assert dev._lib.qsv_eval_begin(dev._handle, len(circuits), _lib.as_ptr(batch_ids), _lib.as_ptr(counts)) == _lib.QSV_OK
    refused(_lib.QSV_E_STATE, "(qsv_deflated_gradient_circuits goes between batches)")
    assert dev._lib.qsv_eval_push(dev._handle, 0, len(circuits), _lib.as_ptr(flat)) == _lib.QSV_OK
    assert dev._lib.qsv_eval_end(dev._handle, _lib.as_ptr(values)) == _lib.QSV_OK
    assert float(np.abs(values - np.asarray([w[2] for w in want])).max()) < 1e-12 * dr.scale(op, betas)
    works()
    dev.close()


def test_a_register_above_28_qubits_is_refused():
    """A 29-qubit fp32 handle: asked before the kept states are looked up, so the handle needs to hold none (and no operator)."""
    n = 29
    dev = StatevectorDevice(n, dtype="fp32")
    circuit = CircuitIR(n).u(P(0), 0.2, 0.1, 0)
    rc, message, _, _ = _raw(dev, [circuit], [[0.3]], [12345], [1.0])
    assert rc == _lib.QSV_E_UNSUPPORTED and "28 qubits" in message and "29" in message, (rc, message)
    dev.close()


# ---- 7. the driver on the device ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("optimizer", ("spsa", "adam"))
def test_compute_eigenvalues_on_a_four_qubit_operator(optimizer):
    from queasars_amd.evqe import deflation
    from queasars_amd.evqe.solver import SPSA, Adam, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    n = 4
    op = helpers.random_pauli_operator(n, 12, seed=44)
    chosen = SPSA(maxiter=8, learning_rate=0.4, perturbation=0.3) if optimizer == "spsa" else Adam(maxiter=4)
    config = EVQEMinimumEigensolverConfiguration(
        optimizer=chosen, population_size=4, max_generations=1, random_seed=5,
        n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
        use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
        parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
    )
    ev = OperatorCircuitEvaluator(op, gradient_method="adjoint")
    device = ev.statevector_device
    results = deflation.compute_eigenvalues(EVQEMinimumEigensolver(config), ev, 3)
    assert len(results) == 3 and device.kept_state_count() == 0  # (released at the end)
    beta = 2.0 * float(np.abs(op.coeffs).sum())
    lowest = float(np.linalg.eigvalsh(dense_gradient.dense_operator(op))[0])
    dense = []
    for j, result in enumerate(results):
        overlaps = result.overlaps_with_previous
        assert overlaps.shape == (j,)
        recomputed = result.eigenvalue + beta * float(np.sum(np.abs(overlaps) ** 2))
        print(f"{optimizer}, run {j}: eigenvalue {result.eigenvalue:.6f}, deflated value {result.deflated_value:.6f}, |overlaps| {np.abs(overlaps)}")
        assert abs(result.deflated_value - recomputed) < 1e-12 * (dr.spread(op) + j * beta)
        assert result.eigenvalue >= lowest - 1e-10
        bound = float(np.linalg.eigvalsh(dr.deflated_matrix(op, dense, [beta] * j))[0])
        assert result.deflated_value >= bound - 1e-10
        best = result.best_individual
        dense.append(device.statevector(best.get_parameterized_quantum_circuit(), list(best.parameter_values)))
