"""GPU tests on circuits outside the EVQE genome's shape (tests/circuit_families.py): the generated round loop, chain_matrix /
prepare_eval, the multi-pass kernel, swap rounds, multiplexed entries, the split routes, both samplers, kept states and the
gradients on plans the CPU half (tests/test_circuit_families.py) shows to be chains of kMaxChain factors, passes of hundreds of
rounds, plans of eight passes, rounds of twenty entries and plans at each of prepare_eval's staging limits.

Bounds are the project's own: fp64 amplitudes 1e-12, expectation values 1e-10 against the oracle.  Single precision is asked
only of circuits whose plan has at most 128 factors -- the largest count its existing bounds (2e-5 per amplitude, 2e-6 * sum
|c_k| per expectation value) have been exercised at -- and under those bounds unchanged.  Every test prints the largest
deviation it saw."""

from __future__ import annotations

import numpy as np
import pytest

import circuit_families as cf
import dense_gradient
import helpers
from oracle import statevector_oracle as so
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from test_gpu_configs import _diagonal_operator
from test_gpu_differential import _diag_table, check_draws
from test_gpu_side_prepare import _on_and_off

pytestmark = pytest.mark.gpu

AMP_TOL = 1e-12
EXP_TOL = 1e-10
FP32_AMP_TOL = 2e-5  # (tests/test_gpu_parity.py)
FP32_REL = 2e-6  # (per unit of sum |c_k|: tests/test_gpu_configs.py)
FP32_MAX_FACTORS = 128

# two of test_statevector_other_geometries' configurations, and a compact first pass (small tiles, many outer qubits)
OTHER_GEOMETRIES = [dict(tile_bits=10, reg_bits=3, low_bits=3), dict(tile_bits=9, reg_bits=2, low_bits=2)]
COMPACT_GEOMETRY = dict(tile_bits=8, reg_bits=2, low_bits=2)

_STATES: dict = {}  # id(circuit) -> (circuit, oracle state): computed once, shared, never written to


def _families(n: int, generic_ops=(200,), bridges: int = 2):
    made = [("ladder", cf.ladder(n, 2, False)), ("ladder reversed", cf.ladder(n, 2, True)), ("star", cf.star(n, False)),
            ("fan-in", cf.star(n, True)), ("all_pairs", cf.all_pairs(n, 1)), ("rotation_runs", cf.rotation_runs(n)),
            ("ping_pong", cf.ping_pong(n)), (f"two_blocks {bridges}", cf.two_blocks(n, bridges))]
    made += [(f"generic {m}", cf.generic(n, m)) for m in generic_ops]
    return [(name, c, p) for name, (c, p) in made]


def _oracle_state(circuit, params):
    key = id(circuit)
    if key not in _STATES:
        state = helpers.oracle_state(circuit, params)
        state.setflags(write=False)
        _STATES[key] = (circuit, state)
    return _STATES[key][1]


def _expectation(state, op):
    return so.pauli_expectation(state, op.x_mask.tolist(), op.z_mask.tolist(), op.coeffs.tolist()).real


# ---- a. states -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [3, 6, 10, 13, 14, 16])
def test_statevectors_of_every_family(n):
    """StatevectorDevice.statevector against the oracle for every family, generic at 200 and 600 ops: the default geometry, two
    other geometries where the register is at least their tile, at n = 14 a compact first pass; in single precision the
    circuits of at most 128 factors."""
    cases = _families(n, generic_ops=(200, 600))
    geometries = [{}] + [g for g in OTHER_GEOMETRIES if n >= g["tile_bits"]] + ([COMPACT_GEOMETRY] if n == 14 else [])
    worst = {}
    for cfg in geometries:
        dev = StatevectorDevice(n, **cfg)
        try:
            for name, c, p in cases:
                err = float(np.abs(dev.statevector(c, p) - _oracle_state(c, p)).max())
                worst[str(cfg)] = max(worst.get(str(cfg), 0.0), err)
                assert err < AMP_TOL, (name, cfg, err)
        finally:
            dev.close()
    dev = StatevectorDevice(n, dtype="fp32")
    try:
        asked = 0
        for name, c, p in cases:
            if cf.plan_stats(c)["n_factors"] > FP32_MAX_FACTORS:
                continue
            asked += 1
            err = float(np.abs(dev.statevector(c, p) - _oracle_state(c, p)).max())
            worst["fp32"] = max(worst.get("fp32", 0.0), err)
            assert err < FP32_AMP_TOL, (name, err)
        assert asked >= 6, asked
    finally:
        dev.close()
    print(f"\nn = {n}: largest amplitude deviation per geometry: " + ", ".join(f"{k}: {v:.2e}" for k, v in worst.items()))


# ---- b. the preparation's staging regimes ----------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [10, 14])
@pytest.mark.parametrize("shape", list(cf.STAGING_SHAPES))
def test_every_staging_regime_of_the_preparation(shape, n):
    """prepare_eval at each side of each of its limits (parameters, folded gates, sines and cosines), taken alone and all
    together: in the prepare kernel (n = 10) and in the pass kernel's own preparation of a split evaluation's virtual circuits
    (n = 14: two keys, the counts are those of one side's plan).  Two parameter vectors, against the oracle; the cases of at
    most 128 factors in single precision too (float_mats)."""
    n_fold, n_trig, n_params = cf.STAGING_SHAPES[shape]
    c, p = cf.staging(n, n_fold, n_trig - n_fold, n_params, bridges=2 if n == 14 else 0)
    rng = np.random.default_rng(n_trig)
    vectors = [p, list(rng.uniform(-np.pi, np.pi, size=n_params))]
    op = helpers.random_ising_operator(n, seed=1)
    spread = float(np.abs(op.coeffs).sum())
    ref = [helpers.oracle_expectation(c, v, op) for v in vectors]
    ev = OperatorCircuitEvaluator(op)
    try:
        ev.circuit_costs([c])
        form = ev.statevector_device.circuit_form(c)
        if n == 14:
            assert form["route"] in (1, 2) and form["n_keys"] == 2 and sorted(form["n_virtual"]) == [9, 9], form
        else:
            assert form["route"] == 0, form
        got = ev.evaluate_circuits([c, c], vectors)
        err = float(np.abs(np.asarray(got) - np.asarray(ref)).max())
        print(f"\n{shape}, n = {n}: fp64 |value - oracle| = {err:.2e}")
        assert err < EXP_TOL
    finally:
        ev.statevector_device.close()
    if n_trig - n_fold <= FP32_MAX_FACTORS:
        ev32 = OperatorCircuitEvaluator(op, dtype="fp32")
        try:
            got = ev32.evaluate_circuits([c, c], vectors)
            err = float(np.abs(np.asarray(got) - np.asarray(ref)).max())
            print(f"{shape}, n = {n}: fp32 |value - oracle| = {err:.2e}, bound {FP32_REL * spread:.2e}")
            assert err < FP32_REL * spread
        finally:
            ev32.statevector_device.close()


# ---- c. operators and routes -----------------------------------------------------------------------------------------------

KINDS = ("ising", "cubic", "general", "observables")


def _operators(n: int) -> dict:
    ising = helpers.random_ising_operator(n, seed=n)
    return {"ising": ising, "cubic": _diagonal_operator(n, n, "cubic"), "general": helpers.random_pauli_operator(n, 40, seed=n),
            "observables": [ising, helpers.random_pauli_operator(n, 12, seed=n + 1)]}


def _route_cases(n: int):
    """The circuits of one register size.  n = 12 is there for the one-tile route, which no larger register of a default handle
    takes; n = 20 for the one-launch route (two_blocks with one, two and three bridges: one, two and three keys)."""
    if n == 12:
        return [("ladder", *cf.ladder(12, 2, False)), ("generic 200", *cf.generic(12, 200))]
    if n == 20:
        return [(f"two_blocks {b}", *cf.two_blocks(20, b)) for b in (1, 2, 3)] + [("ladder", *cf.ladder(20, 2, False)),
                                                                                   ("generic 200", *cf.generic(20, 200))]
    return _families(n, bridges=3 if n == 17 else 2)


def _forms(dev, op, circuits):
    ev = OperatorCircuitEvaluator(op, statevector_device=dev)
    ev.circuit_costs(circuits)  # (registers them under the operator, several at once)
    return ev, [dev.circuit_form(c) for c in circuits]


def _stratum(form):
    return (form["route"], form["n_keys"], form["amps_per_thread"], form["halves"], form["outer"], form["one_launch"])


@pytest.mark.parametrize("n", [12, 14, 16, 17, 20])
def test_operators_on_every_route(n, c_oracle):
    """Every circuit of the size under an Ising operator, a diagonal one that is not quadratic, a general one of 40 strings
    and evaluate_observables with two operators: alone, in a batch and in the batch reversed the same bits; within 1e-10 of a
    device that does not split; the first circuit of each stratum of circuit_form against the oracle (NumPy's up to 17
    qubits, the plain-C one at 20); on the one-launch route the staged preparation on, off and on again the same bits."""
    cases = _route_cases(n)
    names, circuits, params = [x[0] for x in cases], [x[1] for x in cases], [x[2] for x in cases]
    ops = _operators(n)
    dev, plain = StatevectorDevice(n), StatevectorDevice(n)
    plain.set_option("split", 0)
    worst = {}
    scratch = np.zeros(2 << n) if n == 20 else None
    try:
        for kind in KINDS:
            op = ops[kind]
            ev, forms = _forms(dev, op if kind != "observables" else op[0], circuits)
            ev_plain = OperatorCircuitEvaluator(op if kind != "observables" else op[0], statevector_device=plain)
            if kind == "observables":
                evaluate = lambda e, cs, ps: [tuple(row) for row in e.evaluate_observables(cs, ps, op)]  # noqa: E731
            else:
                evaluate = lambda e, cs, ps: e.evaluate_circuits(cs, ps)  # noqa: E731
            got = evaluate(ev, circuits, params)
            assert evaluate(ev, circuits[::-1], params[::-1]) == got[::-1], kind
            for i, (c, p) in enumerate(zip(circuits, params)):
                assert evaluate(ev, [c], [p])[0] == got[i], (kind, names[i])
            ref = evaluate(ev_plain, circuits, params)
            err = float(np.abs(np.asarray(got) - np.asarray(ref)).max())
            worst[kind, "pass path"] = err
            assert err < EXP_TOL, (kind, err)
            launched = [i for i, f in enumerate(forms) if f["one_launch"] and f["route"] == 1]
            if launched and kind != "observables":  # (the three evaluate_circuits kinds)
                cs, ps = [circuits[i] for i in launched], [params[i] for i in launched]
                assert _on_and_off(ev, lambda: evaluate(ev, cs, ps)) == [got[i] for i in launched], kind
            seen = set()
            for i, form in enumerate(forms):
                if _stratum(form) in seen:
                    continue
                seen.add(_stratum(form))
                for m, o in enumerate(op if kind == "observables" else [op]):
                    if n == 20:
                        table = c_oracle.diagonal_table(o) if not o.x_mask.any() else None
                        want = c_oracle.evaluate(circuits[i], params[i], o, table, scratch)
                    else:
                        want = _expectation(_oracle_state(circuits[i], params[i]), o)
                    value = got[i][m] if kind == "observables" else got[i]
                    err = abs(value - want)
                    key = (kind, _lib.ROUTE_NAMES[form["route"]], form["n_keys"])
                    worst[key] = max(worst.get(key, 0.0), err)
                    assert err < EXP_TOL, (kind, names[i], form, err)
    finally:
        dev.close()
        plain.close()
    print(f"\nn = {n}: largest deviations (operator, against what / route, keys):")
    for key, err in worst.items():
        print(f"   {key}: {err:.2e}")


def test_the_circuits_reach_every_route():
    """Read through circuit_form under the Ising operator, without evaluating: the circuits of test_operators_on_every_route take
    all four routes, and on the one-launch route one, two and three keys (the routes under the other operators are printed)."""
    routes, one_launch_keys = set(), set()
    for n in (12, 14, 16, 17, 20):
        circuits = [c for _, c, _ in _route_cases(n)]
        ops = _operators(n)
        dev = StatevectorDevice(n)
        try:
            for kind in ("ising", "cubic", "general"):
                _, forms = _forms(dev, ops[kind], circuits)
                print(f"\nn = {n} {kind}: " + ", ".join(f"{_lib.ROUTE_NAMES[f['route']]} ({f['n_keys']})" for f in forms))
                if kind == "ising":
                    routes |= {f["route"] for f in forms}
                    one_launch_keys |= {f["n_keys"] for f in forms if f["route"] == 1}
        finally:
            dev.close()
    assert {_lib.ROUTE_NAMES[r] for r in routes} == set(_lib.ROUTE_NAMES), routes
    assert one_launch_keys >= {1, 2, 3}, one_launch_keys


# ---- d. samplers -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family,n,bridges,split_sampled", [("generic", 14, 0, False), ("two_blocks", 14, 2, True),
                                                           ("two_blocks", 17, 3, True)])
def test_exact_draws_on_the_families(family, n, bridges, split_sampled, c_oracle):
    """sampler_draws.DrawCheck as test_exact_draws_of_both_samplers holds it: every shot of two seeds of 4096 accepted against
    the exact CDF in its sampler's order, at most 1 % off the exact draw, values D[state]; the probabilities are the C
    oracle's within 1e-14."""
    c, p = cf.generic(n, 200) if family == "generic" else cf.two_blocks(n, bridges)
    op = helpers.random_ising_operator(n, seed=n)
    spread = float(np.abs(op.coeffs).sum())
    table = _diag_table(op)
    dev, plain = StatevectorDevice(n), StatevectorDevice(n)
    plain.set_option("split", 0)
    try:
        _, forms = _forms(dev, op, [c])
        # (the splitter may find a cut of fewer keys than there are bridges: a bridge control inside a small block goes over whole)
        assert forms[0]["split_sampled"] == split_sampled and (not split_sampled or 1 <= forms[0]["n_keys"] <= bridges), forms
        dev.set_operator(op)
        plain.set_operator(op)
        probs = plain.probabilities(c, p)
        assert np.abs(probs - np.abs(c_oracle.simulate(c, p)) ** 2).max() < 1e-14
        for seed in (2, 3):
            states, values = dev.sample_batch([c], [p], 4096, seed, with_values=True)
            rep = check_draws(states, values, seed, [c], [p], forms, lambda i: probs, table, "fp64", spread)[0]
            print(f"\n{family} n = {n}, seed {seed}: {rep}")
    finally:
        dev.close()
        plain.close()


# ---- e. kept states --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", ["generic", "rotation_runs"])
def test_kept_states_of_long_circuits(family):
    """keep_states on a circuit of hundreds of factors, a ladder layer on top through continue_from: the oracle's value and
    amplitudes of the composed circuit, and the composed circuit evaluated whole on the device within 1e-10."""
    n = 14
    front, front_values = cf.generic(n, 200) if family == "generic" else cf.rotation_runs(n)
    rest, values = cf.ladder(n, 1, False, seed=1)
    whole = helpers.bound_copy(front, front_values).compose(cf.ladder(n, 1, False, seed=1)[0])
    op = helpers.random_ising_operator(n, seed=n)
    ev = OperatorCircuitEvaluator(op)
    dev = ev.statevector_device
    try:
        state = ev.keep_states([front], [front_values])[0]
        kept = rest.continue_from(state)
        points = [values, list(np.random.default_rng(3).uniform(-np.pi, np.pi, size=len(values)))]
        got = np.asarray(ev.evaluate_circuits([kept, kept], points))
        ref = np.asarray([helpers.oracle_expectation(whole, v, op) for v in points])
        on_device = np.asarray(ev.evaluate_circuits([whole, whole], points))
        amp = float(np.abs(dev.statevector(kept, values) - helpers.oracle_state(whole, values)).max())
        print(f"\n{family}: kept against the oracle {np.abs(got - ref).max():.2e}, against the whole circuit on the device "
              f"{np.abs(got - on_device).max():.2e}, amplitudes {amp:.2e}")
        assert np.abs(got - ref).max() < EXP_TOL and np.abs(got - on_device).max() < EXP_TOL and amp < AMP_TOL
    finally:
        dev.close()


# ---- f. gradients ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [6, 7, 8])
def test_gradients_of_generic_circuits(n):
    """evaluate_gradients on unstructured circuits with literal angles and with parameters no gate reads, against the dense
    derivative (tests/dense_gradient.py) within 1e-10; a parameter that several angle slots read has no shift rule: ValueError."""
    c, p = cf.generic(n, 40, share=0.0, literal=0.3, seed=n)
    c.declare_parameters(c.num_parameters + 3)
    p = p + [0.4, -1.3, 2.2]
    terms = c.gradient_terms()
    assert terms[-3:] == [0, 0, 0] and -1 not in terms and {2, 4} <= set(terms), terms
    shared, ps = cf.generic(n, 40, share=0.3, literal=0.3, seed=n)
    assert -1 in shared.gradient_terms()
    for op in (helpers.random_ising_operator(n, seed=n), helpers.random_pauli_operator(n, 12, seed=n)):
        ev = OperatorCircuitEvaluator(op)
        try:
            got = ev.evaluate_gradients([c], [p])[0]
            want = dense_gradient.gradient(c, p, dense_gradient.dense_operator(op))
            err = float(np.abs(got - want).max())
            print(f"\nn = {n}, {len(op)} strings: |gradient - dense| = {err:.2e}")
            assert got.shape == want.shape and err < EXP_TOL and np.all(got[-3:] == 0.0)
            with pytest.raises(ValueError, match="parameter"):
                ev.evaluate_gradients([shared], [ps])
        finally:
            ev.statevector_device.close()
