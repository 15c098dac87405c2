"""GPU tests on operators outside the benchmark's shapes (tests/operator_families.py): pauli_groups_kernel past its first chunk
of a group's terms, observable rows on both sides of kObsChunk, factor_term_side / factor_term_value on strings that live on
one side, on the keys or in the low six bits of a side only, the quadratic route with couplings placed relative to the cut,
the two CVaRs on values of D that tie by the thousand, the all-X / all-Y / all-Z strings and the lowest and highest pivots,
and operators with more x-mask groups than a launch has rows of workgroups.  The CPU half (tests/test_operator_families.py)
shows that the families reach those regimes and that both oracles read a Pauli string as Kronecker products do.

Bounds are the project's own: an fp64 expectation value within 1e-10 * max(1, sum |c_k| / 50) of the oracle (NumPy's through
14 qubits, the plain-C one above), a single string's value within 1e-12, fp32 within 2e-6 * sum |c_k| on circuits of at most
128 plan factors.  Every test prints the largest deviation it saw."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import circuit_families as cf
import helpers
import operator_families as of
from oracle import statevector_oracle as so
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, OperatorSamplerCircuitEvaluator, StatevectorDevice
from queasars_amd.ir import OP_CU3
from test_gpu_circuit_families import FP32_MAX_FACTORS, FP32_REL
from test_operator_families import c_expectation

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10  # (times max(1, sum |c_k| / 50): tests/test_gpu_configs.py)
TERM_TOL = 1e-12  # (one string's value: tests/test_gpu_observables.py)
ROUTE_ONE_TILE, ROUTE_SPLIT_ONE_LAUNCH, ROUTE_SPLIT, ROUTE_PASSES = 0, 1, 2, 3
SPLIT_ROUTES = (ROUTE_SPLIT_ONE_LAUNCH, ROUTE_SPLIT)
NUMPY_ORACLE_UP_TO = 14

_CIRCUITS: dict = {}  # n -> [(name, circuit, parameters)], made once
_STATES: dict = {}  # id(circuit) -> (circuit, oracle state): computed once, shared, never written to


def _circuits(n: int):
    """The smallest registers at which each route exists: one tile (10), a split of two keys and gate passes (14), three keys
    (17), the one-launch route under quadratic operators and factor_terms under general ones (20)."""
    if n not in _CIRCUITS:
        made = {10: [("generic 200", cf.generic(10, 200)), ("ladder", cf.ladder(10))],
                14: [("two_blocks 2", cf.two_blocks(14, 2)), ("generic 200", cf.generic(14, 200))],
                17: [("two_blocks 3", cf.two_blocks(17, 3))],
                20: [(f"two_blocks {b}", cf.two_blocks(20, b)) for b in (1, 2, 3)] + [("generic 200", cf.generic(20, 200))]}[n]
        _CIRCUITS[n] = [(name, c, p) for name, (c, p) in made]
    return _CIRCUITS[n]


def _state(circuit, params, c_oracle):
    key = id(circuit)
    if key not in _STATES:
        n = circuit.n_qubits
        state = helpers.oracle_state(circuit, params) if n <= NUMPY_ORACLE_UP_TO else c_oracle.simulate(circuit, params)
        state.setflags(write=False)
        _STATES[key] = (circuit, state)
    return _STATES[key][1]


def _oracle_value(circuit, params, op, c_oracle) -> float:
    state = _state(circuit, params, c_oracle)
    if circuit.n_qubits <= NUMPY_ORACLE_UP_TO:
        return so.pauli_expectation(state, op.x_mask.tolist(), op.z_mask.tolist(), op.coeffs.tolist()).real
    return c_expectation(c_oracle, state, op)


def _spread(op) -> float:
    return float(np.abs(op.coeffs.real).sum())  # (the imaginary parts do not enter real(<H>))


def _bound(op) -> float:
    return EXP_TOL * max(1.0, _spread(op) / 50.0)


def _is_quadratic(op) -> bool:
    return not op.x_mask.any() and max(bin(int(z)).count("1") for z in op.z_mask) <= 2


def _sides(n: int) -> tuple[int, int]:
    """The two sides of the split form of the size's two_blocks circuit without its key qubits: circuit_form's mask_x / mask_y
    (under an Ising operator; between them they hold every qubit) less the controls of the gates that cross from one to the
    other -- so that ``placed`` finds the keys in neither.  The two halves of the register where the size has no split circuit."""
    name, c, p = _circuits(n)[0]
    if not name.startswith("two_blocks"):
        return (1 << (n // 2)) - 1, ((1 << n) - 1) & ~((1 << (n // 2)) - 1)
    dev = StatevectorDevice(n)
    try:
        OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=n), statevector_device=dev).circuit_costs([c])
        form = dev.circuit_form(c)
    finally:
        dev.close()
    mask_x, mask_y = form["mask_x"], form["mask_y"]
    assert form["route"] in SPLIT_ROUTES and mask_x and mask_y and not mask_x & mask_y and mask_x | mask_y == (1 << n) - 1, form
    keys = 0
    for kind, target, control, *_ in c.bound_ops(p):
        if kind == OP_CU3 and ((mask_x >> int(control)) & 1) != ((mask_x >> int(target)) & 1):
            keys |= 1 << int(control)
    assert 1 <= bin(keys).count("1") <= 3, (bin(keys), form)
    return mask_x & ~keys, mask_y & ~keys


def _placed_families(n: int, mask_a: int, mask_b: int) -> dict:
    made = {}
    for where in ("a", "b", "across", "rest"):
        for kind in ("quadratic", "general"):
            for part in (None,) if kind == "quadratic" or where == "rest" else (None, "low6", "high"):
                try:
                    made[f"placed {where} {kind}" + (f" {part}" if part else "")] = of.placed(n, mask_a, mask_b, where, kind, part)
                except ValueError:  # (no qubit there: a side of six qubits has no "high" part, two halves leave no "rest")
                    pass
    return made


def _physical_families(n: int) -> dict:
    k = 10 if n <= NUMPY_ORACLE_UP_TO else 8  # (a few hundred terms where the oracle sweeps 2^17 and 2^20 amplitudes per term)
    made = {"transverse_ising": of.transverse_ising(n, True), "heisenberg": of.heisenberg(n, True), "hopping": of.hopping(n, 12),
            "parities": of.parities(n), f"all_z_strings {k}": of.all_z_strings(k, n), "unweighted_cut": of.unweighted_cut(n, 3),
            "one_group 257 low": of.one_group(n, of.K_CHUNK + 1, "low"), "one_group 257 high": of.one_group(n, of.K_CHUNK + 1, "high")}
    made["untidy unweighted_cut"] = of.untidy(made["unweighted_cut"])
    made["untidy heisenberg"] = of.untidy(made["heisenberg"])
    return made


def _check_on_every_route(n, families, c_oracle, dtype="fp64"):
    """Each operator under OperatorCircuitEvaluator on the size's circuits: alone, in a batch and in the batch reversed the same
    bits; the oracle; a handle that does not split.  Returns {operator: routes} and the largest deviations."""
    cases = _circuits(n)
    names, circuits, params = [x[0] for x in cases], [x[1] for x in cases], [x[2] for x in cases]
    if dtype == "fp32":
        keep = [i for i, c in enumerate(circuits) if cf.plan_stats(c)["n_factors"] <= FP32_MAX_FACTORS]
        assert keep, "no circuit of the size has few enough factors for the fp32 bound"
        names, circuits, params = [names[i] for i in keep], [circuits[i] for i in keep], [params[i] for i in keep]
    dev, plain = StatevectorDevice(n, dtype=dtype), StatevectorDevice(n, dtype=dtype)
    plain.set_option("split", 0)
    routes, worst = {}, {"oracle": 0.0, "unsplit handle": 0.0}
    try:
        for name, op in families.items():
            ev = OperatorCircuitEvaluator(op, statevector_device=dev)
            ev.circuit_costs(circuits)
            forms = [dev.circuit_form(c) for c in circuits]
            routes[name] = [f["route"] for f in forms]
            for cname, form in zip(names, forms):
                if cname.startswith("two_blocks"):
                    assert form["route"] in SPLIT_ROUTES, (name, cname, form)
                    if n == 20 and _is_quadratic(op):
                        assert form["route"] == ROUTE_SPLIT_ONE_LAUNCH, (name, cname, form)
                else:
                    assert form["route"] == (ROUTE_ONE_TILE if n == 10 else ROUTE_PASSES), (name, cname, form)
            got = ev.evaluate_circuits(circuits, params)
            assert ev.evaluate_circuits(circuits[::-1], params[::-1]) == got[::-1], name
            for i, (c, p) in enumerate(zip(circuits, params)):
                assert ev.evaluate_circuits([c], [p])[0] == got[i], (name, names[i])
            bound = FP32_REL * _spread(op) if dtype == "fp32" else _bound(op)
            scale = bound / (FP32_REL if dtype == "fp32" else EXP_TOL)
            for i, (c, p) in enumerate(zip(circuits, params)):
                err = abs(got[i] - _oracle_value(c, p, op, c_oracle))
                worst["oracle"] = max(worst["oracle"], err / scale)
                assert err < bound, (name, names[i], forms[i], got[i], err, bound)
            ref = OperatorCircuitEvaluator(op, statevector_device=plain).evaluate_circuits(circuits, params)
            err = float(np.abs(np.asarray(got) - np.asarray(ref)).max())
            worst["unsplit handle"] = max(worst["unsplit handle"], err / scale)
            assert err < (2 * bound if dtype == "fp32" else bound), (name, err, bound)  # (fp32: each within its bound of the oracle)
    finally:
        dev.close()
        plain.close()
    print(f"\nn = {n} {dtype}, circuits {names}: routes per operator")
    for name, r in routes.items():
        print(f"   {name:32s} " + ", ".join(_lib.ROUTE_NAMES[x] for x in r))
    unit = "sum |c_k|" if dtype == "fp32" else "max(1, sum |c_k| / 50)"
    print(f"   largest deviation per unit of {unit}: " + ", ".join(f"{k}: {v:.2e}" for k, v in worst.items()))
    return routes


# ---- a. expectation values on every route ---------------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["physical", "placed"])
@pytest.mark.parametrize("n", [10, 14, 17, 20])
def test_expectation_values_of_every_family_on_every_route(n, which, c_oracle):
    """Every family under OperatorCircuitEvaluator on the size's circuits.  "physical": transverse-field Ising, Heisenberg,
    hopping terms, the parity strings, every Z string on ten (eight) qubits, the unweighted cut, one group of 257 strings under
    the lowest and the highest pivot, and an untidy copy of a quadratic and of a general one.  "placed": quadratic and general
    terms inside side x, inside side y, across the cut and on the keys of the size's split circuit (its circuit_form masks), the
    general ones also confined to the low six or to the other qubits of a side."""
    families = _physical_families(n) if which == "physical" else _placed_families(n, *_sides(n))
    if which == "placed":  # (a side of at most six qubits has no "high" part, the two halves of a register leave no "rest")
        assert {"placed a quadratic", "placed b general", "placed across quadratic", "placed across general low6"} <= set(families)
        assert n < 14 or {"placed rest quadratic", "placed rest general"} <= set(families), list(families)
        assert n < 17 or {"placed a general high", "placed b general high"} & set(families), list(families)
    routes = _check_on_every_route(n, families, c_oracle)
    kinds = {"quadratic": [k for k, op in families.items() if _is_quadratic(op)],
             "diagonal": [k for k, op in families.items() if not op.x_mask.any() and not _is_quadratic(op)],
             "general": [k for k, op in families.items() if op.x_mask.any()]}
    assert kinds["quadratic"] and kinds["general"] and (which == "placed" or kinds["diagonal"]), kinds
    assert all(len(r) == len(_circuits(n)) for r in routes.values())


# ---- b. one group across the chunk boundary ---------------------------------------------------------------------------------


@pytest.mark.parametrize("x_name", of.X_MASK_NAMES)
@pytest.mark.parametrize("n", [10, 14])
def test_one_group_across_the_chunk_boundary(n, x_name, c_oracle):
    """pauli_groups_kernel on one group of 255, 256, 257, 513, 512, 513 (and, at ten qubits, all 1024) strings under one x mask
    -- one chunk not full, one full, a second of one string, a third, partial one --, on a handle that does not split: the
    oracle decides; the operator cut into two at term kChunk must also add up to the whole (which chunk a failure is in)."""
    cases = _circuits(n)
    circuits, params = [x[1] for x in cases], [x[2] for x in cases]
    dev = StatevectorDevice(n)
    dev.set_option("split", 0)
    worst = {"oracle": 0.0, "two parts": 0.0}
    try:
        for count in of.GROUP_COUNTS + ((1 << n,) if n == 10 else ()):
            op = of.one_group(n, count, x_name)
            assert of.groups_of(op) == (0, [(of.x_mask_of(n, x_name), count)])
            got = np.asarray(OperatorCircuitEvaluator(op, statevector_device=dev).evaluate_circuits(circuits, params))
            assert [dev.circuit_form(c)["route"] for c in circuits] == [ROUTE_ONE_TILE if n == 10 else ROUTE_PASSES] * len(circuits)
            want = np.asarray([_oracle_value(c, p, op, c_oracle) for c, p in zip(circuits, params)])
            err = float(np.abs(got - want).max())
            worst["oracle"] = max(worst["oracle"], err / (_bound(op) / EXP_TOL))
            terms = of.masks_of(op)
            parts = [of.from_masks(n, terms[:of.K_CHUNK]), of.from_masks(n, terms[of.K_CHUNK:])] if count > of.K_CHUNK else []
            summed = sum(np.asarray(OperatorCircuitEvaluator(part, statevector_device=dev).evaluate_circuits(circuits, params)) for part in parts)
            apart = float(np.abs(got - summed).max()) if parts else 0.0
            worst["two parts"] = max(worst["two parts"], apart / (_bound(op) / EXP_TOL))
            assert err < _bound(op) and apart < _bound(op), (count, x_name, err, apart, got, want, summed)
    finally:
        dev.close()
    print(f"\nn = {n}, x mask {x_name}: largest deviation per unit of max(1, sum |c_k| / 50): " + ", ".join(f"{k}: {v:.2e}" for k, v in worst.items()))


# ---- c. observable sets across the row boundary -----------------------------------------------------------------------------


@pytest.mark.parametrize("x_name", ["high", "random"])
@pytest.mark.parametrize("n", [10, 14])
def test_observable_sets_across_the_row_boundary(n, x_name):
    """observable_values with every string of all_z_strings(10, n) (two full rows of the diagonal group), of a group of kObsChunk
    (one full row) and of kObsChunk + 1 strings (a full row and a row of one, which carries its own `parts`) as an observable of
    its own: each value within 1e-12 of the oracle's -- on the one-tile route (10 qubits), on the gate passes and on a split
    circuit's side tables (14: split_term_values_kernel).  The same sets as two observables of many terms each against the
    one-operator evaluator (1e-12)."""
    cases = _circuits(n)
    names, circuits, params = [x[0] for x in cases], [x[1] for x in cases], [x[2] for x in cases]
    sets = {"all_z_strings": of.all_z_strings(10, n), "one_group 512": of.one_group(n, of.K_OBS_CHUNK, x_name),
            "one_group 513": of.one_group(n, of.K_OBS_CHUNK + 1, x_name)}
    states = [helpers.oracle_state(c, p) for c, p in zip(circuits, params)]
    dev = StatevectorDevice(n)
    worst = {}
    try:
        dev.set_operator(helpers.random_ising_operator(n, seed=n))  # (the routes are read under it; the sets do not use it)
        forms = [dev.circuit_form(c) for c in circuits]
        if n == 10:
            assert [f["route"] for f in forms] == [ROUTE_ONE_TILE] * len(circuits), forms
        else:
            assert forms[0]["route"] in SPLIT_ROUTES and 1 <= forms[0]["n_keys"] <= 2 and forms[1]["route"] == ROUTE_PASSES, forms
        for name, op in sets.items():
            strings = of.single_strings(op)
            got = dev.observable_values(circuits, params, strings)
            assert got.shape == (len(circuits), len(op))
            for row, state, cname in zip(got, states, names):
                want = np.asarray([so.pauli_term_expectation(state, int(x), int(z)).real for x, z in zip(op.x_mask, op.z_mask)])
                err = float(np.abs(row - want).max())
                worst[name, cname] = err
                assert err < TERM_TOL, (name, cname, int(np.abs(row - want).argmax()), err)
            terms = of.masks_of(op)
            halves = [of.from_masks(n, terms[:300]), of.from_masks(n, terms[300:])]
            assert of.rows_of(halves) == of.rows_of(strings)
            pair = dev.observable_values(circuits, params, halves)
            for m, half in enumerate(halves):
                want = np.asarray(OperatorCircuitEvaluator(half, statevector_device=dev).evaluate_circuits(circuits, params))
                err = float(np.abs(pair[:, m] - want).max())
                worst[name, f"observable {m} of two"] = err
                assert err < TERM_TOL, (name, m, err)
    finally:
        dev.close()
    print(f"\nn = {n}, x mask {x_name}: largest deviations")
    for key, err in worst.items():
        print(f"   {key}: {err:.2e}")


# ---- d. degenerate D ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [10, 14, 17])
def test_exact_cvar_on_tied_values(n, c_oracle):
    """The exact-probability CVaR under unweighted_cut -- integer values of D, a dozen of them over 2^n states -- against
    so.cvar_expectation fed the oracle's probabilities and D (1e-10), for alpha = 1, 0.5, 0.05 and one awkward value: a split
    circuit (14, 17: side tables) and unsplittable ones (10, 14: the probabilities of the last pass)."""
    cases = _circuits(n)
    circuits, params = [x[1] for x in cases], [x[2] for x in cases]
    op = of.unweighted_cut(n, 3)
    table = so.diagonal_values(n, op.z_mask.tolist(), op.coeffs.real.tolist())
    assert len(set(table.tolist())) <= n + 2
    probs = [np.abs(_state(c, p, c_oracle)) ** 2 for c, p in zip(circuits, params)]
    worst = 0.0
    for alpha in (1.0, 0.5, 0.05, 0.3217):
        ev = OperatorSamplerCircuitEvaluator(None, op, alpha=alpha)
        try:
            got = ev.evaluate_circuits(circuits, params)
            assert got == ev.evaluate_circuits(circuits[::-1], params[::-1])[::-1]
            if n >= 14:
                assert ev.statevector_device.circuit_form(circuits[0])["split_sampled"]
            for i, pr in enumerate(probs):
                if np.isclose(alpha, 1):
                    want = float(np.dot(pr, table))
                else:
                    want = so.cvar_expectation(list(zip(range(1 << n), pr.tolist(), table.tolist())), alpha)
                worst = max(worst, abs(got[i] - want))
                assert abs(got[i] - want) < EXP_TOL, (n, alpha, cases[i][0], got[i], want)
        finally:
            ev.statevector_device.close()
    print(f"\nn = {n}: exact CVaR on {len(set(table.tolist()))} distinct values of D, largest |value - oracle| = {worst:.2e}")


@pytest.mark.parametrize("shots,alpha", [(512, 0.5), (37, 0.25), (4096, 0.05)])
def test_sampled_cvar_on_tied_values(shots, alpha):
    """qsv_sample_cvar_batch sorts sample values on the device that are nearly all ties: the host CVaR of the same samples
    (test_cvar_on_the_device_equals_the_host_cvar_of_the_same_samples' rule, unchanged), split and unsplit circuits."""
    from queasars_amd.circuit_evaluation.circuit_evaluation import _cvar_of_sample_matrix

    worst = 0.0
    for n in (10, 14, 17):
        cases = _circuits(n)
        circuits, params = [x[1] for x in cases], [x[2] for x in cases]
        dev = StatevectorDevice(n)
        try:
            dev.set_operator(of.unweighted_cut(n, 3))
            got = dev.sample_cvar_batch(circuits, params, shots, 99, alpha)
            _, values = dev.sample_batch(circuits, params, shots, 99, with_values=True)
            assert len(np.unique(values)) <= n + 2 and np.all(values == np.round(values))
            want = _cvar_of_sample_matrix(values, alpha)
            err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
            worst = max(worst, err)
            assert err < 1e-12 * max(1.0, float(np.abs(values).max())), (n, got, want)
        finally:
            dev.close()
    print(f"\n{shots} shots, alpha {alpha}: largest |device CVaR - host CVaR of the same samples| = {worst:.2e}")


# ---- e. gradients ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("circuit_name", ["two_blocks", "generic"])
def test_gradients_under_a_general_and_a_placed_quadratic_operator(circuit_name):
    """evaluate_gradients at 14 qubits under heisenberg and under quadratic terms across the cut, on the split circuit and on an
    unstructured one, within 1e-10 of the derivative of the gate matrices (operator_families.adjoint_gradient: dense_gradient's
    quantity without its 2^n x 2^n matrix, which ends at eight qubits; the CPU half holds the two together).  The generic circuit
    is drawn without shared parameters, as test_gradients_of_generic_circuits draws it: a shared one has no shift rule."""
    n = 14
    c, p = cf.two_blocks(n, 2) if circuit_name == "two_blocks" else cf.generic(n, 200, share=0.0)
    assert -1 not in c.gradient_terms()
    for name, op in (("heisenberg", of.heisenberg(n, True)), ("placed across quadratic", of.placed(n, *_sides(n), "across", "quadratic"))):
        ev = OperatorCircuitEvaluator(op)
        try:
            got = ev.evaluate_gradients([c], [p])[0]
            route = ev.statevector_device.circuit_form(c)["route"]
            want = of.adjoint_gradient(c, p, op)
            err = float(np.abs(got - want).max())
            print(f"\n{circuit_name} under {name} ({_lib.ROUTE_NAMES[route]}, {len(want)} parameters): |gradient - reference| = {err:.2e}")
            assert got.shape == want.shape and err < EXP_TOL
        finally:
            ev.statevector_device.close()


# ---- f. single precision --------------------------------------------------------------------------------------------------------


def test_expectation_values_in_single_precision(c_oracle):
    """Every family at 14 qubits on an fp32 handle, on the circuits of at most 128 plan factors, under 2e-6 * sum |c_k|."""
    n = 14
    families = {**_physical_families(n), **_placed_families(n, *_sides(n))}
    _check_on_every_route(n, families, c_oracle, dtype="fp32")


# ---- more x-mask groups, or observable rows, than a launch has rows of workgroups ------------------------------------------


def _max_grid_y() -> int:
    """The device's largest gridDim.y, from the runtime (hipDeviceGetAttribute; 29 and 30 are hipDeviceAttributeMaxGridDimX and
    ..Y of hip_runtime_api.h, checked against each other and, by the caller, against what the library accepts)."""
    import torch

    with open("/proc/self/maps") as f:  # (the runtime torch and libqsv share, wherever it was loaded from)
        loaded = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert loaded, "no HIP runtime in this process"
    hip = C.CDLL(loaded[0])
    gx, gy = C.c_int(0), C.c_int(0)
    device = torch.cuda.current_device()
    assert hip.hipDeviceGetAttribute(C.byref(gx), 29, device) == 0 and hip.hipDeviceGetAttribute(C.byref(gy), 30, device) == 0
    assert gx.value >= gy.value >= 1024, (gx.value, gy.value)
    return gy.value


def _many_masks(n: int, count: int):
    """`count` strings with an x mask of its own each: the nonzero masks of lowest weight first, every third with a Y on its
    lowest qubit (both parities of ny)."""
    masks = sorted(range(1, 1 << n), key=lambda x: (bin(x).count("1"), x))[:count]
    rng = cf._rng("many masks", n, count)
    return [(x, (x & -x) if k % 3 == 2 else 0, float(c)) for k, (x, c) in enumerate(zip(masks, rng.uniform(-1.0, 1.0, size=count)))]


@pytest.mark.parametrize("n", [10, 14])
def test_slices_of_groups_and_rows_give_the_same_bits(n):
    """Option "max_grid_y" (x-mask groups, or observable rows, per launch): 1, 3 and 7 give the bits of one launch, for
    expectation values of operators of many groups and for an observable set of many rows; the device's own limit is the
    largest value the library takes."""
    limit = _max_grid_y()
    cases = _circuits(n)
    circuits, params = [x[1] for x in cases], [x[2] for x in cases]
    ops = [of.heisenberg(n, True), of.hopping(n, 30), helpers.random_pauli_operator(n, 40, seed=n)]
    strings = of.single_strings(of.one_group(n, of.K_OBS_CHUNK + 1, "random")) + of.single_strings(of.hopping(n, 30))
    assert len(of.rows_of(strings)) > 30 and all(len(of.groups_of(op)[1]) >= n - 1 for op in ops)
    dev = StatevectorDevice(n)
    dev.set_option("split", 0)
    try:
        dev.set_option("max_grid_y", limit)
        with pytest.raises(ValueError, match="max_grid_y"):
            dev.set_option("max_grid_y", limit + 1)
        whole = [OperatorCircuitEvaluator(op, statevector_device=dev).evaluate_circuits(circuits, params) for op in ops]
        whole_values = dev.observable_values(circuits, params, strings)
        for per_launch in (1, 3, 7, 0):
            dev.set_option("max_grid_y", per_launch)
            for op, want in zip(ops, whole):
                assert OperatorCircuitEvaluator(op, statevector_device=dev).evaluate_circuits(circuits, params) == want, per_launch
            assert np.array_equal(dev.observable_values(circuits, params, strings), whole_values), per_launch
    finally:
        dev.close()


def test_more_groups_and_rows_than_the_largest_grid(c_oracle):
    """A general operator with one more x-mask group than the device's largest gridDim.y, and an observable set with as many
    rows as a set may have (65536: one more than that limit, or the limit itself): qsv_set_operator and qsv_observables_create
    take them (a return code other than QSV_OK raises), the launches go in slices, the operator's value is the plain-C oracle's
    under the fp64 bound, and the set's values are the one-operator evaluator's and add up to it.  (17 qubits have 833 x masks of weight up to three: the masks run up to weight nine.)"""
    n = 17
    limit = _max_grid_y()
    assert limit + 1 < (1 << n), limit
    _, c, p = _circuits(n)[0]
    terms = _many_masks(n, limit + 1)
    op = of.from_masks(n, terms)
    assert len(of.groups_of(op)[1]) == limit + 1
    dev = StatevectorDevice(n)
    dev.set_option("split", 0)  # (the state route: the split route evaluates the strings one by one, without groups)
    try:
        dev.set_operator(of.parities(n))
        before = dev.expectation_values([c], [p])[0]
        ev = OperatorCircuitEvaluator(op, statevector_device=dev)
        got = ev.evaluate_circuits([c], [p])[0]
        want = _oracle_value(c, p, op, c_oracle)
        print(f"\nn = {n}: gridDim.y <= {limit}; {limit + 1} groups: |value - oracle| = {abs(got - want):.2e}, bound {_bound(op):.2e}")
        assert abs(got - want) < _bound(op), (got, want)
        # the set's two observables against the one-operator evaluator (each has fewer groups than the limit: one launch), and
        # with the strings the set leaves out they add up to the operator the oracle has just confirmed
        count = min(limit + 1, 1 << 16)
        halves = [of.from_masks(n, terms[:count // 2]), of.from_masks(n, terms[count // 2:count])]
        assert len(of.rows_of(halves)) == count
        values = dev.observable_values([c], [p], halves)[0]
        total = float(values.sum())
        for m, half in enumerate(halves):
            alone = OperatorCircuitEvaluator(half, statevector_device=dev).evaluate_circuits([c], [p])[0]
            print(f"   {count} rows, observable {m}: |value - one-operator evaluator| = {abs(values[m] - alone):.2e}, bound {_bound(half):.2e}")
            assert abs(values[m] - alone) < _bound(half), (m, values[m], alone)
        if count < len(terms):
            total += OperatorCircuitEvaluator(of.from_masks(n, terms[count:]), statevector_device=dev).evaluate_circuits([c], [p])[0]
        assert abs(total - want) < _bound(op), (total, want)
        dev.set_operator(of.parities(n))
        assert dev.expectation_values([c], [p])[0] == before
    finally:
        dev.close()
