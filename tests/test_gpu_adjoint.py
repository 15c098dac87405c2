"""GPU tests of the adjoint gradients (include/qsv.h: qsv_adjoint_gradient_circuits / qsv_adjoint_gradient_device).

Sizes: n = 6 (one tile, n < T), n = T and n = T + 2 (four tiles on two workgroups: the tile loop and the sum over workgroups).
fp64 within 1e-10 (the project's EXP_TOL) of the NumPy sweep of tests/adjoint_reference.py, which tests/test_adjoint_plan.py
holds to the dense derivative.  Run on the MI355X box with -m gpu."""

import json
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import adjoint_reference
import circuit_families as cf
import dense_gradient
import helpers
import operator_families as of
from queasars_amd.circuit_evaluation import CircuitEvaluatorException, OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe import solver
from queasars_amd.ir import OP_CU3, OP_ID, CircuitIR, ParamRef

pytestmark = pytest.mark.gpu

P = ParamRef
EXP_TOL = 1e-10
SHIFT_TOL = 2e-10  # against parameter shift on the same device: two fp64 results, each within EXP_TOL of the exact value
# Single precision, relative to sum |c_k|.  Measured on the MI355X on the cases of this file (largest error against
# adjoint_reference over the three sizes and both operators, divided by sum |c_k|): the existing fp32 parameter-shift gradients
# FP32_SHIFT_MEASURED, the sweep FP32_SWEEP_MEASURED.  The sweep is allowed four times the parameter-shift error -- it rounds
# every gate twice, on two states, where a shifted evaluation rounds it once on one -- and never less than the project's 2e-6.
FP32_SHIFT_MEASURED = 4.041e-8  # (n = 6 under the Ising operator; the other cases 1.0e-8 .. 2.5e-8)
FP32_SWEEP_MEASURED = 5.567e-8  # (the same case; the others 2.0e-8 .. 3.9e-8)
FP32_REL = max(4.0 * FP32_SHIFT_MEASURED, 2e-6)

T = adjoint_reference.describe(CircuitIR(1).u(P(0), 0.0, 0.0, 0))["tile_bits"]
LOW = adjoint_reference.describe(CircuitIR(1).u(P(0), 0.0, 0.0, 0))["low_bits"]
SIZES = (6, T, T + 2)
OPERATORS = ("ising", "general")


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def assert_same_bits(got, want, what=""):
    assert len(got) == len(want), what
    for e, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), f"{what}: circuit {e}"


# ---- the cases, built once --------------------------------------------------------------------------------------------------


def _band(n: int, lo: int, hi: int) -> int:
    return sum(1 << q for q in range(lo, min(hi, n)))


@lru_cache(maxsize=None)
def operator(n: int, kind: str):
    """"ising": diagonal.  "general": about 40 strings -- X / Y / Z factors confined to the qubits below c, to those between c and
    T and to those at or above T (operator_families.placed), strings across the bands, and a Z-only group."""
    if kind == "ising":
        return helpers.random_ising_operator(n, seed=n)
    bands = [m for m in (_band(n, 0, LOW), _band(n, LOW, T), _band(n, T, n)) if m]
    terms = []
    for mask in bands:
        terms += of.masks_of(of.placed(n, mask, 0, "a", "general", n_terms=10))
    for a, b in zip(bands, bands[1:]):
        terms += of.masks_of(of.placed(n, a, b, "across", "general", n_terms=5))
    rng = np.random.default_rng(n)
    terms += [(0, int(z), float(c)) for z, c in zip(rng.integers(1, 1 << n, size=8), rng.uniform(-1.0, 1.0, size=8))]
    merged = {}
    for x, z, c in terms:
        merged[(x, z)] = merged.get((x, z), 0.0) + complex(c).real
    op = of.from_masks(n, [(x, z, c) for (x, z), c in merged.items()])
    assert any(int(x) for x in op.x_mask) and any(not int(x) for x in op.x_mask)
    return op


def spread(op) -> float:
    return float(np.abs(op.coeffs.real).sum())


def _swept_gates(circuit) -> int:
    """The gates a full gradient's sweep visits: the non-id gates from the first one that reads a parameter on."""
    rows = circuit.packed()
    rows = rows[rows["kind"] != OP_ID]
    reads = np.maximum(np.maximum(rows["p_theta"], rows["p_phi"]), rows["p_lambda"]) >= 0
    return int(len(rows) - np.argmax(reads)) if reads.any() else 0


def _has_shared(circuit) -> bool:
    return min(circuit.gradient_terms(), default=0) < 0


@lru_cache(maxsize=None)
def cases(n: int):
    """[(name, circuit, parameters)]: the families, and a five-individual EVQE population."""
    made = [("ladder", cf.ladder(n)), ("star out", cf.star(n)), ("star in", cf.star(n, fan_in=True)),
            ("rotation_runs", cf.rotation_runs(n)), ("generic", cf.generic(n, 60, share=0.3, literal=0.2)),
            ("two_blocks", cf.two_blocks(n, 2))]
    out = [(name, c, p) for name, (c, p) in made]
    _, circuits, params = helpers.population_circuits(n, 3, 5, seed=n)
    out += [(f"individual {i}", c, list(p)) for i, (c, p) in enumerate(zip(circuits, params))]
    assert _has_shared(dict((name, c) for name, c, _ in out)["generic"])
    if n > T:  # targets and controls at or above T, controls above and below their targets
        rows = np.concatenate([c.packed() for _, c, _ in out])
        cu3 = rows[rows["kind"] == OP_CU3]
        assert (rows["target"][rows["kind"] != OP_ID] >= T).any() and (cu3["control"] >= T).any()
        assert (cu3["control"] > cu3["target"]).any() and (cu3["control"] < cu3["target"]).any()
    return tuple(out)


@lru_cache(maxsize=None)
def reference(n: int, kind: str):
    """[(gradient, value)] of cases(n) under operator(n, kind): computed once, shared, never written to."""
    out = []
    for _, circuit, params in cases(n):
        gradient, value = adjoint_reference.gradient_and_value(circuit, params, operator(n, kind))
        gradient.setflags(write=False)
        out.append((gradient, value))
    return tuple(out)


@lru_cache(maxsize=None)
def evaluator(n: int, kind: str, method: str = "adjoint", dtype: str = "fp64"):
    return OperatorCircuitEvaluator(operator(n, kind), dtype=dtype, gradient_method=method)


def device_gradients(ev, circuits, params, wrt=None):
    """The device entry point: points in a padded matrix of an odd row length, gradients (and padding) read back after one
    synchronise."""
    import torch

    width = max(len(p) for p in params) + 1
    width += 1 - width % 2
    matrix = torch.zeros((len(circuits), width), dtype=torch.float64, device="cuda")
    for e, p in enumerate(params):
        matrix[e, : len(p)] = torch.tensor(p, dtype=torch.float64)
    counts = [c.num_parameters if wrt is None else len(wrt if np.ndim(wrt[0]) == 0 else wrt[e]) for e, c in enumerate(circuits)]
    out_width = max(counts) + 3
    out = torch.full((len(circuits), out_width), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ev.evaluate_gradients_device_to_device(circuits, matrix, out, wrt)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for e, k in enumerate(counts):
        assert np.array_equal(bits(host[e, k:]), np.zeros(out_width - k, dtype=np.uint64)), f"padding of row {e}"
    return [host[e, :k].copy() for e, k in enumerate(counts)]


# ---- 1. values ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n", SIZES)
def test_fp64_gradients_are_the_reference_sweep(n, kind):
    names, circuits, params = zip(*cases(n))
    want = reference(n, kind)
    ev = evaluator(n, kind)
    got = ev.evaluate_gradients(list(circuits), list(params))
    assert ev.last_gradient_evaluations == len(circuits)
    worst = max(float(np.abs(g - w).max(initial=0.0)) for g, (w, _) in zip(got, want))
    print(f"n = {n}, {kind}: largest deviation from the reference {worst:.3e} (sum |c| = {spread(operator(n, kind)):.1f})")
    assert worst < EXP_TOL
    assert max(float(np.abs(w).max(initial=0.0)) for w, _ in want) > 1e-3  # (not gradients of zeros)
    stats = ev.statevector_device.adjoint_stats()
    assert stats["n_gates"] == sum(_swept_gates(c) for c in circuits) and stats["n_runs"] >= 1
    # circuits without a shared parameter: also against parameter shift on the same device
    plain = [i for i, c in enumerate(circuits) if not _has_shared(c)]
    assert len(plain) >= len(circuits) - 2
    shift = evaluator(n, kind, "parameter_shift").evaluate_gradients([circuits[i] for i in plain], [params[i] for i in plain])
    worst_shift = max(float(np.abs(got[i] - s).max(initial=0.0)) for i, s in zip(plain, shift))
    print(f"n = {n}, {kind}: largest deviation from parameter shift {worst_shift:.3e}")
    assert worst_shift < SHIFT_TOL


# ---- 2. a shared parameter ---------------------------------------------------------------------------------------------------


def test_a_shared_parameter_is_summed_where_parameter_shift_refuses():
    circuit = CircuitIR(6)
    for q in range(6):
        circuit.u(P(q % 3), P(3), 0.25 * q, q)
    circuit.cu3(P(0), P(4), P(4), 0, 5).cu3(P(1), 0.3, P(2), 4, 1).u(P(5), P(0), P(3), 2)
    params = np.random.default_rng(6).uniform(-np.pi, np.pi, 6).tolist()
    for kind in OPERATORS:
        with pytest.raises(ValueError, match="more than one angle slot"):
            evaluator(6, kind, "parameter_shift").evaluate_gradients([circuit], [params])
        got = evaluator(6, kind).evaluate_gradients([circuit], [params])[0]
        want = dense_gradient.gradient(circuit, params, dense_gradient.dense_operator(operator(6, kind)))
        assert float(np.abs(got - want).max()) < EXP_TOL and float(np.abs(want).max()) > 1e-3


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", SIZES)
def test_a_row_depends_on_nothing_but_its_circuit_and_point(n):
    device = StatevectorDevice(n, group=4)
    group = int(device._lib.qsv_group_size(device._handle))
    assert group == 4
    ev = OperatorCircuitEvaluator(operator(n, "general"), statevector_device=device, gradient_method="adjoint")
    _, circuits, params = (list(x) for x in zip(*cases(n)[: group + 3]))
    assert len(circuits) == group + 3
    batch = ev.evaluate_gradients(circuits, params)
    alone = [ev.evaluate_gradients([c], [p])[0] for c, p in zip(circuits, params)]
    assert_same_bits(batch, alone, "a batch of group + 3 against each evaluation alone")
    assert_same_bits(ev.evaluate_gradients(circuits[::-1], params[::-1])[::-1], batch, "other positions in the launch groups")
    assert_same_bits(device_gradients(ev, circuits, params), batch, "the device entry point")
    assert_same_bits(ev.evaluate_gradients(circuits, params), batch, "the same call again")
    device.close()


# ---- 4. wrt ------------------------------------------------------------------------------------------------------------------


def _last_gates_parameters(circuit, count=4):
    rows = [row for row in circuit.packed() if row["kind"] != OP_ID][-count:]
    return sorted({int(row[name]) for row in rows for name in ("p_theta", "p_phi", "p_lambda") if row[name] >= 0})


@pytest.mark.parametrize("n", (6, T + 2))
def test_wrt_entries_are_the_bits_of_the_full_gradient(n):
    ev = evaluator(n, "general")
    _, circuits, params = (list(x) for x in zip(*cases(n)))
    full = ev.evaluate_gradients(circuits, params)
    rng = np.random.default_rng(5)
    ragged = [rng.permutation(c.num_parameters)[: 1 + e % 7].tolist() for e, c in enumerate(circuits)]
    ragged[3] = []
    permuted = [rng.permutation(c.num_parameters).tolist() for c in circuits]
    last = [_last_gates_parameters(c) for c in circuits]
    for name, wrt in (("one list for all", [2, 0]), ("ragged", ragged), ("permuted", permuted), ("last gates", last)):
        for entry in ("host", "device"):
            got = ev.evaluate_gradients(circuits, params, wrt) if entry == "host" else device_gradients(ev, circuits, params, wrt)
            want = [f[np.asarray(wrt if np.ndim(wrt[0]) == 0 else wrt[e], dtype=np.int64)] for e, f in enumerate(full)]
            assert_same_bits(got, want, f"{name} / {entry}")
    # the sweep of a last-gates wrt stops early
    device = ev.statevector_device
    ev.evaluate_gradients(circuits, params)
    whole = device.adjoint_stats()
    ev.evaluate_gradients(circuits, params, last)
    short = device.adjoint_stats()
    assert 0 < short["n_gates"] < whole["n_gates"] and short["n_state_sweeps"] <= whole["n_state_sweeps"]
    if n > T:
        assert short["n_state_sweeps"] < whole["n_state_sweeps"] and short["n_runs"] < whole["n_runs"]


def test_a_parameter_no_gate_reads_has_entry_zero():
    circuit = CircuitIR(6).u(P(0), P(1), 0.3, 0).cu3(P(3), 0.2, P(1), 0, 4)
    circuit.declare_parameters(6)  # (2, 4 and 5 are read by nothing)
    params = [0.3, -1.1, 9.0, 0.7, 8.0, 7.0]
    ev = evaluator(6, "general")
    got = ev.evaluate_gradients([circuit], [params])[0]
    assert got.shape == (6,) and np.array_equal(bits(got[[2, 4, 5]]), np.zeros(3, dtype=np.uint64))
    assert np.abs(got[[0, 1, 3]]).min() > 0.0
    assert np.array_equal(bits(ev.evaluate_gradients([circuit], [params], [[5, 1]])[0]), bits(got[[5, 1]]))
    assert ev.evaluate_gradients([circuit], [params], [[4]])[0].tolist() == [0.0]
    assert ev.statevector_device.adjoint_stats()["n_gates"] == 0


# ---- 5. the by-product -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n", SIZES)
def test_the_values_are_the_expectation_values(n, kind):
    ev = evaluator(n, kind)
    _, circuits, params = (list(x) for x in zip(*cases(n)))
    _, values = ev.statevector_device.adjoint_gradients(circuits, params, wrt=[[] for _ in circuits], return_values=True)
    want = np.asarray(ev.evaluate_circuits(circuits, params))
    worst = float(np.abs(values - want).max())
    print(f"n = {n}, {kind}: largest deviation of the by-product from evaluate_circuits {worst:.3e}")
    assert worst < EXP_TOL
    assert float(np.abs(values - np.asarray([v for _, v in reference(n, kind)])).max()) < EXP_TOL


# ---- 6. single precision -----------------------------------------------------------------------------------------------------


def fp32_errors(n: int, kind: str) -> tuple[float, float]:
    """(largest error of the fp32 parameter-shift gradients, of the fp32 sweep) against the reference, over sum |c_k|."""
    _, circuits, params = (list(x) for x in zip(*cases(n)))
    want = [w for w, _ in reference(n, kind)]
    scale = spread(operator(n, kind))
    sweep = evaluator(n, kind, "adjoint", "fp32").evaluate_gradients(circuits, params)
    plain = [i for i, c in enumerate(circuits) if not _has_shared(c)]
    shift = evaluator(n, kind, "parameter_shift", "fp32").evaluate_gradients([circuits[i] for i in plain], [params[i] for i in plain])
    shift_error = max(float(np.abs(s - want[i]).max(initial=0.0)) for i, s in zip(plain, shift)) / scale
    sweep_error = max(float(np.abs(g - w).max(initial=0.0)) for g, w in zip(sweep, want)) / scale
    return shift_error, sweep_error


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("n", SIZES)
def test_fp32_gradients_within_four_times_the_parameter_shift_error(n, kind):
    shift_error, sweep_error = fp32_errors(n, kind)
    print(f"n = {n}, {kind}: fp32 error over sum |c_k|: parameter shift {shift_error:.3e}, sweep {sweep_error:.3e}")
    assert sweep_error < FP32_REL


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------


def test_refusals():
    (_, circuit, params), (_, other, other_params) = cases(6)[0], cases(6)[1]
    bare = StatevectorDevice(6)
    with pytest.raises(CircuitEvaluatorException, match="no operator set"):
        bare.adjoint_gradients([circuit], [params])
    bare.close()
    ev = evaluator(6, "general")
    device = ev.statevector_device
    with pytest.raises(ValueError, match="wrt index"):
        ev.evaluate_gradients([circuit], [params], [[circuit.num_parameters]])
    with pytest.raises(ValueError, match="wrt index"):
        ev.evaluate_gradients([circuit], [params], [[-1]])
    # out_width too small, at the C ABI
    import torch

    matrix = torch.zeros((1, circuit.num_parameters), dtype=torch.float64, device="cuda")
    out = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="out_width 2 is too small"):
        device.adjoint_gradients_of_device_parameters([circuit], matrix.data_ptr(), circuit.num_parameters, 0, out.data_ptr(), 2)
    with pytest.raises(ValueError, match="rows of 2 entries"):
        ev.evaluate_gradients_device_to_device([circuit], matrix, out)
    # a circuit on a kept state
    kept = ev.keep_states([circuit], [params])
    continued = CircuitIR(6).u(P(0), P(1), P(2), 3).continue_from(kept[0])
    with pytest.raises(ValueError, match="kept state"):
        ev.evaluate_gradients([continued], [[0.1, 0.2, 0.3]])
    kept[0].release()
    # noise is emulated on the host
    noisy = OperatorCircuitEvaluator(operator(6, "general"), estimator_precision=0.1, statevector_device=device, gradient_method="adjoint")
    with pytest.raises(ValueError, match="estimator_precision"):
        noisy.evaluate_gradients([circuit], [params])
    with pytest.raises(ValueError, match="gradient_method"):
        OperatorCircuitEvaluator(operator(6, "general"), statevector_device=device, gradient_method="finite differences")
    # ... and the handle still works
    got = ev.evaluate_gradients([other], [other_params])[0]
    assert float(np.abs(got - reference(6, "general")[1][0]).max()) < EXP_TOL


# ---- 8. "auto" ---------------------------------------------------------------------------------------------------------------


def test_auto_sends_each_circuit_to_its_method():
    n = 14  # (the smallest register with a split route and gate passes: tests/test_gpu_operator_families.py)
    op = helpers.random_ising_operator(n, seed=n)
    device = StatevectorDevice(n)
    auto = OperatorCircuitEvaluator(op, statevector_device=device, gradient_method="auto")
    sweep = OperatorCircuitEvaluator(op, statevector_device=device, gradient_method="adjoint")
    shift = OperatorCircuitEvaluator(op, statevector_device=device, gradient_method="parameter_shift")
    default = OperatorCircuitEvaluator(op, statevector_device=device)
    split_c, split_p = cf.two_blocks(n, 2)
    pass_c, pass_p = cf.generic(n, 200, share=0.0)
    shared_c, shared_p = cf.two_blocks(n, 2, seed=1)
    shared_c.u(P(0), P(1), 0.5, 3)  # (two_blocks again, with two parameters read a second time: still a split circuit)
    routes = [cost["route"] for cost in auto.circuit_costs([split_c, pass_c, shared_c])]
    assert routes[0].startswith("split") and routes[1] == "gate passes", routes
    assert not _has_shared(split_c) and not _has_shared(pass_c) and _has_shared(shared_c)
    circuits, params = [split_c, pass_c, shared_c, split_c], [split_p, pass_p, shared_p, [0.5 * x for x in split_p]]
    got = auto.evaluate_gradients(circuits, params)
    assert auto.last_gradient_evaluation_counts[1:3] == [1, 1] and auto.last_gradient_evaluation_counts[0] == sum(split_c.gradient_terms())
    assert auto.last_gradient_evaluations == 2 + 2 * sum(split_c.gradient_terms())
    by_sweep = sweep.evaluate_gradients(circuits[1:3], params[1:3])
    by_shift = shift.evaluate_gradients([circuits[0], circuits[3]], [params[0], params[3]])
    assert_same_bits(got, [by_shift[0], by_sweep[0], by_sweep[1], by_shift[1]], "auto against the per-method calls")
    wrt = [[3, 1], [0], [1, 0, 5], []]
    assert_same_bits(auto.evaluate_gradients(circuits, params, wrt), [g[np.asarray(w, dtype=np.int64)] for g, w in zip(got, wrt)], "auto with wrt")
    assert_same_bits(device_gradients(auto, circuits, params), got, "auto, device to device")
    # "parameter_shift" is what it was: the bits of an evaluator built with defaults
    assert default.gradient_method == "parameter_shift"
    assert_same_bits(shift.evaluate_gradients([split_c, pass_c], [split_p, pass_p]), default.evaluate_gradients([split_c, pass_c], [split_p, pass_p]),
                     "parameter_shift against the default")
    assert shift.last_gradient_evaluations == default.last_gradient_evaluations == sum(split_c.gradient_terms()) + sum(pass_c.gradient_terms())
    device.close()


# ---- 9. the host Adam driver -------------------------------------------------------------------------------------------------


def test_the_host_adam_driver_runs_on_the_sweep():
    from queasars_amd.evqe.serialization import population_from_dict

    data = json.loads((Path(__file__).resolve().parent / "golden" / "population_n6.json").read_text())
    population = population_from_dict(data["population"])
    circuits = [ind.get_parameterized_quantum_circuit() for ind in population.individuals]
    ev = OperatorCircuitEvaluator(helpers.random_ising_operator(6, seed=3), gradient_method="adjoint")
    config = solver.Adam(maxiter=5)
    jobs = [(c, config.new_run(list(ind.parameter_values), None)) for c, ind in zip(circuits, population.individuals)]
    before = np.asarray(ev.evaluate_circuits(circuits, [run.x.tolist() for _, run in jobs]))
    solver._minimize_adam(ev, jobs)
    stats = ev.statevector_device.adjoint_stats()
    assert stats["n_state_sweeps"] >= 2 * len(jobs) and stats["n_gates"] > 0 and stats["n_runs"] >= 1
    assert all(run.done and run.iteration == 5 and run.nfev == 5 and np.isfinite(run.x).all() for _, run in jobs)
    after = np.asarray(ev.evaluate_circuits(circuits, [run.x.tolist() for _, run in jobs]))
    assert np.isfinite(before).all() and np.isfinite(after).all()
    from queasars_amd.evqe import device_search

    assert not device_search.possible_adam(ev, config, len(jobs))  # (a device-resident Adam search stays parameter shift)
