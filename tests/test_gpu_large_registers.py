"""The consumers of whole final states -- variance, covariance, overlaps and matrix elements, adjoint gradients, the k most probable
states -- at the register sizes people run them at: 20 to 28 qubits, where the geometry (reg_bits 4, tiles of 12 and 13 qubits,
low_bits 3), the launch groups (128 down to 1), every consumer's grid cap and the byte offsets (slots and kept states beyond
4 GiB, one state of 4 GiB) differ from everything the other modules reach.

(a) n = 20, fp64 and fp32, and (b) n = 21, 22, fp64: non-product circuits of the benchmark population against full states from the
C oracle and the existing *_reference helpers, under the project's own bounds.  (c) n = 24, (d) n = 25 and n = 24 fp32, (e) n = 28:
product circuits on interleaved blocks against tests/factorised_reference.py (held to the full-state references on the host by
tests/test_factorised_reference_host.py, which also checks, at these sizes and seeds, that variances, overlaps, gradients and
top-state gaps are large enough for an indexing error to show).  No state of 24 qubits or more is copied to the host.

Bounds from n = 24 on: the derivations of the project's bounds name sums of 2^13 to 2^17 terms and do not carry to 2^24 .. 2^28, so
each bound is FOUR times the largest error measured against the factorised reference on an MI355X over this module's seeds (the
kernels are deterministic; the margin is for other seeds), and never above the ceiling 1e-9 (fp64; times max(1, sum|c|) for values,
T and gradients, times its square -- S_a S_b for a covariance entry -- for variances and covariances), which an indexing error
exceeds by six decades under the conditions the host module checks.  Errors are relative to those scales.

Measured on an MI355X (largest error per regime, relative to the scales above; "-": the regime does not run the consumer):

    regime                     E        V        C        S        T        G        P (beyond 1e-13 relative)
    n24, group 20 (20 evals)   7.8e-16  1.2e-16  1.7e-15  -        -        -        0
    n24, two groups (10)       6.9e-16  8.0e-17  1.2e-15  1.3e-15  9.2e-17  5.3e-17  0
    n24, 18 kept states        -        -        -        1.1e-15  6.7e-17  -        -
    n25                        8.9e-16  8.3e-17  1.7e-15  3.9e-16  1.4e-16  1.2e-16  0
    n28                        1.7e-16  1.8e-17  1.5e-15  1.4e-15  6.8e-17  1.9e-17  0
    worst, fp64                8.9e-16  1.2e-16  1.7e-15  1.4e-15  1.4e-16  1.2e-16  0
    bound, fp64 (4 x worst)    3.6e-15  4.8e-16  6.9e-15  5.8e-15  5.6e-16  4.9e-16  the bound of E
    n24 fp32                   1.4e-07  1.6e-08  2.9e-07  1.2e-07  1.2e-09  2.0e-08  3.5e-10
    bound, fp32 (4 x measured) 5.8e-07  6.4e-08  1.2e-06  4.7e-07  4.9e-09  7.9e-08  the bound of E

All of these are rounding of the last few bits: no bound comes near its ceiling, and the errors do not grow from 2^24 to 2^28
terms.  A top state's probability is held to 1e-13 relative plus the bound of E (the state error bound); the state lists are
compared exactly, every rank.  fp32: no fp64 ceiling applies and no state can be copied out to measure e_s as the project's fp32
rule asks, so the ceiling is 1e-4, a decade below what an indexing error moves.

n = 20 .. 22 under the project's own bounds, measured on an MI355X: fp64 |dE| <= 3.5e-15 (allowed 1e-10), |dVar| <= 6.4e-14 (allowed
4e-10 .. 7e-9), |dC| / (S_a S_b) <= 7.4e-15 (1e-11), |dS| <= 2.3e-15 (1e-11), |dT| <= 7.2e-15 (7e-11 .. 2.7e-10), gradients 7.0e-15
(1e-10), probabilities 1.4e-17 (1e-13): three decades of room or more everywhere.  n = 20 fp32: e_s = 3.0e-7, so the floor of 2e-6 decides;
largest errors relative to the scales |dE| 2.6e-8, |dVar| 4.8e-9, |dC| 2.8e-8, |dS| 1.8e-7, |dT| 2.4e-8, gradients 2.2e-8,
probabilities 5.4e-9.

Resident memory at n = 28: 19.1 GiB of device memory were in use at the end of the test beyond what was in use at its start --
the 4 GiB state slot (group 1), 8 GiB of two kept states, and the scratch of the adjoint sweep and of the reductions (not broken
down here).  Host time: the full-state references of n = 22 take 7 s and those of n = 20, which both dtypes share,
4 s (the device's part is well under a second); every other test takes three seconds or less.
"""

from __future__ import annotations

import time

import numpy as np
import pytest

import covariance_reference as cr
import factorised_reference as fr
import helpers
import overlap_reference as ovr
import shift_rules
import top_states_reference as tsr
import variance_reference as vr
from oracle import statevector_oracle as so
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10  # (tests/test_gpu_adjoint.py: gradients and values against the reference)
CEILING = 1e-9
FP32_CEILING = 1e-4  # (the conditions of the host module put an indexing error at 1e-3 or more: a decade below that)

# regime: {quantity: bound}, relative to the quantity's scale (see the header); E value, V variance, C covariance entry, S overlap,
# T matrix element, G gradient entry, P probability of a top state
FP64 = dict(E=3.6e-15, V=4.8e-16, C=6.9e-15, S=5.8e-15, T=5.6e-16, G=4.9e-16)
FP32 = dict(E=5.8e-7, V=6.4e-8, C=1.2e-6, S=4.7e-7, T=4.9e-9, G=7.9e-8)
for _bounds in (FP64, FP32):
    _bounds["P"] = _bounds["E"]  # (what a probability may be off beyond 1e-13 relative: the state error bound)
BOUNDS = {name: FP32 if "fp32" in name else FP64 for name in fr.LARGE_CASES}
assert all(b <= (FP32_CEILING if "fp32" in name else CEILING) for name, bounds in BOUNDS.items() for b in bounds.values())


def _scale(op) -> float:
    return max(1.0, fr.spread(op))


def _held(regime, quantity, error, bound=None):
    """Print a case's largest error (relative to its scale) next to its bound, then hold it to the bound."""
    bound = BOUNDS[regime][quantity] if bound is None else bound
    print(f"MEASURED {regime} | {quantity} | {error:.3e} | bound {bound:.3e}")
    assert error <= bound, (regime, quantity, error, bound)


class _Handles:
    """One handle per (n, dtype, group), shared within the module."""

    def __init__(self):
        self.devices = {}

    def get(self, n, dtype="fp64", group=0):
        key = (n, dtype, group)
        if key not in self.devices:
            self.devices[key] = StatevectorDevice(n, dtype=dtype, group=group)
        return self.devices[key]

    def close(self, n, dtype="fp64", group=0):
        dev = self.devices.pop((n, dtype, group), None)
        if dev is not None:
            dev.close()


@pytest.fixture(scope="module")
def handles():
    h = _Handles()
    yield h
    for dev in h.devices.values():
        dev.close()


# ---- (a), (b): full states from the C oracle -----------------------------------------------------------------------------------

_FULL: dict = {}
WRT_PER_CIRCUIT = 4


def _pick_by_launch_form(dev):
    """One circuit of each form a 20-qubit handle launches, from the benchmark's populations: {name: (circuit, parameters)}."""
    ising = helpers.random_ising_operator(20, seed=2020)
    ev = OperatorCircuitEvaluator(ising, statevector_device=dev)
    picked: dict = {}
    for layers in (4, 5):
        _, circuits, params = helpers.population_circuits(20, layers, 64, seed=0)
        ev.circuit_costs(circuits)
        for c, p in zip(circuits, params):
            form, launched = dev.circuit_form(c), dev.circuit_launch_form(c)
            if not form["one_launch"]:
                continue
            reduced = launched["n_virtual"] != form["n_virtual"]
            if launched["halves"]:
                name = "half sides"
            elif form["n_keys"] == 3 and reduced:
                name = "three-key reduced side"
            elif reduced:
                name = "final control"
            else:
                name = "one launch"
            picked.setdefault(name, (c, p, launched))
    for name in ("one launch", "half sides", "three-key reduced side", "final control"):
        assert name in picked, (name, list(picked))
        print(f"n=20 {name}: {picked[name][2]}")
    _, circuits, params = helpers.population_circuits(20, 8, 8, seed=0)
    ev.circuit_costs(circuits)
    through = [i for i, c in enumerate(circuits) if dev.circuit_cost(c)["route"] == "gate passes"]
    assert through, "no eight-layer circuit goes through the gate passes"
    picked["eight layers"] = (circuits[through[0]], params[through[0]], None)
    return {name: (c, p) for name, (c, p, _) in picked.items()}


def _full_case(n, c_oracle, dev):
    """Circuits, points, oracle states and every reference of the size, computed once and shared by the dtypes."""
    if n in _FULL:
        return _FULL[n]
    if n == 20:
        chosen = list(_pick_by_launch_form(dev).values())
    else:
        _, c4, p4 = helpers.population_circuits(n, 4, 1, seed=n)
        _, c8, p8 = helpers.population_circuits(n, 8, 1, seed=n)
        chosen = [(c4[0], p4[0]), (c8[0], p8[0])]
    circuits, params = [c for c, _ in chosen], [list(p) for _, p in chosen]
    rng = np.random.default_rng(77 + n)
    kept_params = [[float(v + rng.normal(0.0, 0.05)) for v in p] for p in params]  # (overlap_reference.population's perturbation)
    blocks = fr.interleaved_blocks(n, (n - 2 * (n // 3), n // 3, n // 3), seed=n)
    # (above 20 qubits shorter operators: every string costs the host's reference a tenth of a second per state)
    terms, pairs, most = (24, 24, 4) if n == 20 else (12, 6, 2)
    case = dict(circuits=circuits, params=params, kept_params=kept_params, general=fr.general_operator(n, blocks, n, n_terms=terms),
                ising=fr.ising_operator(n, blocks, n, n_pairs=pairs), observables=fr.observable_set(n, blocks, 17, n, max_terms=most))
    case["states"] = [c_oracle.simulate(c, p) for c, p in zip(circuits, params)]
    case["kept_states"] = [c_oracle.simulate(c, p) for c, p in zip(circuits, kept_params)]
    case["want_s"] = ovr.overlaps(case["kept_states"], case["states"])
    assert np.abs(case["want_s"]).max() >= 0.5 and np.abs(case["want_s"]).min() <= 0.1
    for name in ("general", "ising"):
        op = case[name]
        applied = [vr.apply_strings(op, s) for s in case["states"]]
        values = np.asarray([float(np.real(np.vdot(s, lam))) for s, lam in zip(case["states"], applied)])
        case[name, "values"] = values
        case[name, "variances"] = np.asarray([float(np.real(np.vdot(lam, lam))) for lam in applied]) - values ** 2
        case[name, "want_t"] = ovr.overlaps(case["kept_states"], applied)
    # (a split circuit and, at n = 20, the eight-layer one: every row costs the host seconds)
    case["cov_rows"] = [0, len(circuits) - 1] if n == 20 else [0]
    case["cov"] = cr.reference(case["observables"], [case["states"][i] for i in case["cov_rows"]])
    # gradients by a few parameters per circuit -- the second, the last and two in between --, from the shift rules on the C
    # oracle's expectation values (tests/shift_rules.py: the rules of include/qsv.h restated)
    case["wrt"], case["gradients"] = [], []
    scratch = np.zeros(2 << n)
    for c, p in zip(circuits, params):
        terms = c.gradient_terms()
        usable = [k for k, t in enumerate(terms) if t > 0]
        wrt = sorted({usable[int(j)] for j in np.linspace(1, len(usable) - 1, WRT_PER_CIRCUIT)})
        points = shift_rules.shifted_points(terms, p, wrt)
        values = [c_oracle.evaluate(c, point, case["general"], None, scratch) for point in points]
        case["wrt"].append(wrt)
        case["gradients"].append(shift_rules.combine(terms, values, wrt))
    case["probabilities"] = [so.probabilities(s) for s in case["states"]]
    _FULL[n] = case
    return case


def _run_full_regime(n, dtype, c_oracle, handles):
    dev = handles.get(n, dtype)
    case = _full_case(n, c_oracle, handles.get(n, "fp64"))
    circuits, params = case["circuits"], case["params"]
    regime = f"n{n} {dtype}"
    if dtype == "fp64":
        rel = None
    else:
        # the project's rule for fp32 handles: the handle's own statevector() error on the same circuits
        e_s = max(float(np.linalg.norm(dev.statevector(c, p) - s)) for c, p, s in zip(circuits, params, case["states"]))
        rel = ovr.tol_fp32(e_s)
        print(f"{regime}: e_s = {e_s:.3e}, allowed relative error {rel:.3e}")
    kept = dev.keep_states(circuits, case["kept_params"])
    s_first = None
    for name in ("general", "ising"):
        op = case[name]
        ev = OperatorCircuitEvaluator(op, statevector_device=dev, gradient_method="adjoint")
        values, variances = (np.asarray(v) for v in ev.evaluate_variances(circuits, params, with_values=True))
        _held(regime, f"E {name}", float(np.abs(values - case[name, "values"]).max()), vr.TOL_VALUES if rel is None else rel * _scale(op))
        _held(regime, f"V {name}", float(np.abs(variances - case[name, "variances"]).max()),
              vr.tol_fp64(op) if rel is None else rel * _scale(op) ** 2)
        s, t = ev.evaluate_overlaps(circuits, params, kept, with_operator=True)
        _held(regime, f"S {name}", ovr.max_component_error(s, case["want_s"]), ovr.TOL_S if rel is None else rel)
        _held(regime, f"T {name}", ovr.max_component_error(t, case[name, "want_t"]), ovr.tol_t(op) if rel is None else rel * _scale(op))
        assert s_first is None or s.tobytes() == s_first.tobytes()
        s_first = s
    ev = OperatorCircuitEvaluator(case["general"], statevector_device=dev, gradient_method="adjoint")
    got = ev.evaluate_gradients(circuits, params, wrt=case["wrt"])
    err = max(float(np.abs(g - w).max()) for g, w in zip(got, case["gradients"]))
    assert max(float(np.abs(w).max()) for w in case["gradients"]) > 1e-3
    _held(regime, "G general", err, EXP_TOL if rel is None else rel * _scale(case["general"]))
    ops = case["observables"]
    rows = case["cov_rows"]
    values, cov = ev.evaluate_covariances([circuits[i] for i in rows], [params[i] for i in rows], ops, with_values=True)
    scale = np.maximum(1.0, cr.spreads(ops))
    rel_c = float((np.abs(cov - case["cov"][1]) / np.outer(scale, scale)).max())
    _held(regime, "C", rel_c, 1e-11 if rel is None else rel)  # (cr.tol_fp64: 1e-11 S_a S_b)
    if rel is None:
        assert np.all(np.abs(cov - case["cov"][1]) <= cr.tol_fp64(ops))
    _held(regime, "E observables", float(np.abs(values - case["cov"][0]).max()), cr.TOL_VALUES if rel is None else rel * float(scale.max()))
    # the k most probable states, split and unsplit circuits in one call
    dev.set_operator(case["ising"])
    sampled = [dev.circuit_form(c)["split_sampled"] for c in circuits]
    print(f"{regime}: read from side tables: {sampled}")
    if n == 20 and dtype == "fp64":
        assert any(sampled) and not all(sampled), sampled
    tol = tsr.TOL_FP64 if rel is None else max(tsr.FP32_REL, rel)
    for k in (8, 1024):
        states, probs, _ = dev.top_states(circuits, params, k)
        for i in range(len(circuits)):
            tsr.check_top(states[i], probs[i], case["probabilities"][i], k, tol)
        index = states.astype(np.int64)
        _held(regime, f"P k={k}", max(float(np.abs(probs[i] - case["probabilities"][i][index[i]]).max()) for i in range(len(circuits))), tol)
    for state in kept:
        state.release()


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_n20_against_full_states(dtype, c_oracle, handles):
    """(a): one circuit of each launch form and an eight-layer one, all five consumers, both dtypes."""
    _run_full_regime(20, dtype, c_oracle, handles)


@pytest.mark.parametrize("n", [21, 22])
def test_the_13_qubit_tile_against_full_states(n, c_oracle, handles):
    """(b): tile_bits = 13; at n = 22 the adjoint sweep runs at its workgroup cap."""
    _run_full_regime(n, "fp64", c_oracle, handles)
    handles.close(n)
    _FULL.pop(n, None)


# ---- (c) - (e): the factorised reference ---------------------------------------------------------------------------------------


def _check_moments(regime, ev, case, rows, op, name):
    circuits, params = [case.circuits[i] for i in rows], [case.params[i] for i in rows]
    values, variances = (np.asarray(v) for v in ev.evaluate_variances(circuits, params, with_values=True))
    want = np.asarray([fr.moments(op, case.factorised(i)) for i in rows])
    _held(regime, "E", float(np.abs(values - want[:, 0]).max()) / _scale(op))
    _held(regime, "V", float(np.abs(variances - want[:, 1]).max()) / _scale(op) ** 2)
    assert np.all(want[:, 1] >= 1e-3 * fr.spread(op) ** 2), name
    return values, variances


def _check_covariances(regime, ev, case, rows, m):
    ops = case.observables[m]
    values, cov = ev.evaluate_covariances([case.circuits[i] for i in rows], [case.params[i] for i in rows], ops, with_values=True)
    scale = np.maximum(1.0, np.asarray([fr.spread(o) for o in ops]))
    want = [fr.covariance(ops, case.factorised(i)) for i in rows]
    _held(regime, "E", max(float((np.abs(values[j] - w[0]) / scale).max()) for j, w in enumerate(want)))
    _held(regime, "C", max(float((np.abs(cov[j] - w[1]) / np.outer(scale, scale)).max()) for j, w in enumerate(want)))
    assert cov.tobytes() == np.ascontiguousarray(np.swapaxes(cov, -1, -2)).tobytes()
    return values, cov


def _check_top(regime, dev, case, rows, k=fr.TOP_K):
    states, probs, _ = dev.top_states([case.circuits[i] for i in rows], [case.params[i] for i in rows], k)
    worst = 0.0
    for j, i in enumerate(rows):
        want_states, want_probs, gap = fr.top_states(case.factorised(i), k)
        assert gap >= fr.gap_floor(regime)
        assert states[j].tolist() == want_states.tolist(), (regime, i)  # (every rank: the host module guarantees the gaps)
        excess = np.abs(probs[j] - want_probs) - 1e-13 * want_probs
        worst = max(worst, float(excess.max()))
    _held(regime, "P", max(worst, 0.0))
    return states, probs


def _check_overlaps(regime, ev, case, rows, kept, kept_index, op):
    s, t = ev.evaluate_overlaps([case.circuits[i] for i in rows], [case.params[i] for i in rows], kept, with_operator=True)
    want_s = np.asarray([[fr.overlap(case.kept_factorised(j), case.factorised(i)) for j in kept_index] for i in rows])
    want_t = np.asarray([[fr.element(op, case.kept_factorised(j), case.factorised(i)) for j in kept_index] for i in rows])
    _held(regime, "S", ovr.max_component_error(s, want_s))
    _held(regime, "T", ovr.max_component_error(t, want_t) / _scale(op))
    return s, t, want_s


def _check_gradients(regime, ev, case, i, op):
    pc, p = case.evals[i]
    got, = ev.evaluate_gradients([pc.circuit], [list(p)])
    want = fr.gradient(op, pc, p)
    assert got.shape == want.shape and np.mean(np.abs(want) > 1e-3 * fr.spread(op)) >= 0.25
    _held(regime, "G", float(np.abs(got - want).max()) / _scale(op))
    return got


def _evaluators(dev, case):
    return {name: OperatorCircuitEvaluator(op, statevector_device=dev, gradient_method="adjoint") for name, op in
            (("general", case.general), ("ising", case.ising))}


def test_n24_state_slots_beyond_4_gib(handles):
    """(c) A handle with group = 20: 5 GiB of state slots; positions 16 .. 19 of a batch of 20 lie beyond 4 GiB."""
    regime = "n24 group 20"
    case = fr.large_case(regime)
    dev = handles.get(24, group=20)
    group = int(dev._lib.qsv_group_size(dev._handle))
    assert group == 20 and (group - 1) * (1 << 24) * 16 >= 1 << 32
    assert 16 * (1 << 24) * 16 >= 1 << 32  # (slot 16 starts at 4 GiB)
    rows = list(range(20))
    evs = _evaluators(dev, case)
    start = time.perf_counter()
    _check_moments(regime, evs["general"], case, rows, case.general, "general")
    _check_moments(regime, evs["ising"], case, rows, case.ising, "ising")
    _check_covariances(regime, evs["general"], case, rows, 17)
    _check_top(regime, dev, case, rows)
    print(f"{regime}: {time.perf_counter() - start:.2f} s with the host references")
    handles.close(24, group=20)


def test_n24_two_launch_groups_and_the_same_bits(handles):
    """(c) The default handle (group 8) on a batch of 10: two launch groups; evaluation 0 again at position 9 returns the same
    bits from every consumer."""
    regime = "n24 two groups"
    case = fr.large_case(regime)
    dev = handles.get(24)
    group = int(dev._lib.qsv_group_size(dev._handle))
    assert group < 10 <= 2 * group, group
    rows = list(range(9)) + [0]
    evs = _evaluators(dev, case)
    values, variances = _check_moments(regime, evs["general"], case, rows, case.general, "general")
    assert values[9].tobytes() == values[0].tobytes() and variances[9].tobytes() == variances[0].tobytes()
    values, variances = _check_moments(regime, evs["ising"], case, rows, case.ising, "ising")
    assert values[9].tobytes() == values[0].tobytes() and variances[9].tobytes() == variances[0].tobytes()
    values, cov = _check_covariances(regime, evs["general"], case, rows, 17)
    assert values[9].tobytes() == values[0].tobytes() and cov[9].tobytes() == cov[0].tobytes()
    states, probs = _check_top(regime, dev, case, rows)
    assert states[9].tobytes() == states[0].tobytes() and probs[9].tobytes() == probs[0].tobytes()
    kept = dev.keep_states([pc.circuit for pc in case.kept], [pc.params for pc in case.kept])
    s, t, want_s = _check_overlaps(regime, evs["general"], case, rows, kept, [0, 1], case.general)
    assert s[9].tobytes() == s[0].tobytes() and t[9].tobytes() == t[0].tobytes()
    assert np.abs(want_s).max() >= 0.5 and np.abs(want_s).min() <= 0.1
    for state in kept:
        state.release()
    pc, p = case.evals[0]
    ev = evs["general"]
    got = ev.evaluate_gradients([c for c in (pc.circuit, case.circuits[1], pc.circuit)], [list(p), case.params[1], list(p)])
    assert got[2].tobytes() == got[0].tobytes()
    _check_gradients(regime, ev, case, 0, case.general)
    _check_gradients(regime, evs["ising"], case, 0, case.ising)


def test_n24_kept_states_beyond_4_gib(handles):
    """(c) Eighteen kept states of 256 MiB: the slots of the last two start at and beyond 4 GiB; then a recycled slot."""
    regime = "n24 kept beyond 4 GiB"
    case = fr.large_case(regime)
    dev = handles.get(24)
    assert dev.kept_state_count() == 0
    assert 16 * (1 << 24) * 16 >= 1 << 32 and 17 * (1 << 24) * 16 > 1 << 32  # (kept slots 16 and 17, handed out in order)
    kept = dev.keep_states([pc.circuit for pc in case.kept], [pc.params for pc in case.kept])
    assert len(kept) == 18 and dev.kept_state_count() == 18
    ev = OperatorCircuitEvaluator(case.general, statevector_device=dev)
    rows = list(range(4))
    index = [0, 15, 16, 17]
    s, t, want_s = _check_overlaps(regime, ev, case, rows, [kept[j] for j in index], index, case.general)
    assert abs(want_s[2, 3]) >= 0.5 and abs(want_s[3, 2]) >= 0.5 and np.abs(want_s).min() <= 0.1
    # a recycled slot: state 3 is destroyed and state 17's circuit kept again in its place, at evaluation 2's perturbed point
    kept[3].release()
    assert dev.kept_state_count() == 17
    pc, p = case.evals[2]
    assert pc is case.kept[17]
    kept[3] = dev.keep_states([pc.circuit], [list(p)])[0]
    case._factorised["kept", 3] = case.factorised(2)
    index = [0, 3, 16, 17]
    s, t, want_s = _check_overlaps(regime, ev, case, rows, [kept[j] for j in index], index, case.general)
    assert abs(want_s[2, 1] - 1.0) <= 1e-12  # (evaluation 2 is the new state 3 itself)
    for state in kept:
        state.release()
    assert dev.kept_state_count() == 0
    handles.close(24)


def _all_five(regime, dev, rows, m):
    case = fr.large_case(regime)
    evs = _evaluators(dev, case)
    start = time.perf_counter()
    _check_moments(regime, evs["general"], case, rows, case.general, "general")
    _check_moments(regime, evs["ising"], case, rows, case.ising, "ising")
    print(f"{regime}: variances {time.perf_counter() - start:.2f} s")
    start = time.perf_counter()
    _check_covariances(regime, evs["general"], case, rows[:2], m)
    print(f"{regime}: covariances {time.perf_counter() - start:.2f} s")
    start = time.perf_counter()
    kept = dev.keep_states([pc.circuit for pc in case.kept], [pc.params for pc in case.kept])
    _, _, want_s = _check_overlaps(regime, evs["general"], case, rows, kept, [0, 1], case.general)
    _check_overlaps(regime, evs["ising"], case, rows[:1], kept, [0, 1], case.ising)
    assert np.abs(want_s).max() >= 0.5 and np.abs(want_s).min() <= 0.1
    for state in kept:
        state.release()
    print(f"{regime}: overlaps {time.perf_counter() - start:.2f} s")
    start = time.perf_counter()
    _check_gradients(regime, evs["general"], case, 0, case.general)
    print(f"{regime}: gradients {time.perf_counter() - start:.2f} s")
    start = time.perf_counter()
    _check_top(regime, dev, case, rows)
    print(f"{regime}: top states {time.perf_counter() - start:.2f} s")


def test_n25_low_bits_3(handles):
    """(d) fp64 beyond 256 MiB per state: low_bits = lane_bits = 3."""
    _all_five("n25", handles.get(25), [0, 1, 2], 33)
    handles.close(25)


def test_n24_fp32(handles):
    """(d) An fp32 handle at 24 qubits (low_bits = 3 from n = 20 on)."""
    _all_five("n24 fp32", handles.get(24, "fp32"), [0, 1, 2], 33)
    handles.close(24, "fp32")


def test_n28_the_documented_limit(handles):
    """(e) One state is 4 GiB: two evaluations, a general and an Ising operator, 17 observables, two kept states, k = 16."""
    import torch

    free_before = torch.cuda.mem_get_info()[0]
    dev = handles.get(28)
    _all_five("n28", dev, [0, 1], 17)
    print(f"n28: device memory in use beyond the start of the test: {(free_before - torch.cuda.mem_get_info()[0]) / 2 ** 30:.2f} GiB")
    handles.close(28)
