"""Differential GPU tests of register splitting (csrc/split.cpp) across its routes, side forms and samplers.

One seeded matrix of cases (``draw_cases``: a pure function of ``SEED``), each a population of 2 - 3 shuffled blocks of
``population_circuits`` at one register size, one operator kind, one dtype and one variant of the handle's options:

1. against the pass path (a device of the same dtype with ``split`` off; fp32 against fp64 within FP32_REL * sum |c_k|);
2. the same bits as the defaults where the design promises them (the options in ``SAME_BITS``, the batch reversed, the
   first evaluations alone: "a property of the circuit and the handle, never of the batch"), 1e-10 where an option changes
   the order of the sums;
3. the first evaluation of every stratum -- (route, keys, amplitudes per thread, half sides, swept tiles, one launch,
   operator kind, dtype), read through ``StatevectorDevice.circuit_form`` -- against the plain-C oracle;
4. (``test_the_matrix_covers_every_form``) the strata of the whole list include every route, every key count and every
   form of the one-launch route.

Samplers are held to the exact draws (tests/sampler_draws.py): every shot must be the inverse CDF of its uniform number
in the sampler's own order of states, up to rounding at a boundary.
"""

from __future__ import annotations

import numpy as np
import pytest

import helpers
from oracle import statevector_oracle as so
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe import EVQEPopulation
from queasars_amd.ir import PauliOperator
from sampler_draws import DELTA_FP32, DELTA_FP64, DrawCheck, plain_order, shot_uniform, split_order
from test_gpu_configs import _diagonal_operator

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10
FP32_REL = 2e-6
SEED = 20240917
N_CASES = 40

SIZES = (14, 16, 17, 18, 20, 21, 22)
BATCHES = (1, 2, 7, 63, 64, 65, 128, 129, 200)
KINDS = ("ising", "quadratic", "fields", "cubic", "general", "sampler", "cvar")
# options set on the handle (qsv_set_option, before the circuits are registered) or read from the environment when the
# handle is created or a circuit registered -- never one of the process-wide switches the library caches once
VARIANTS = ("defaults", "sides_r3=0", "QSV_NO_HALF_SIDES", "fused_lds_table=0", "side_diag=0", "streams=1", "chain_stream=0",
            "poll_results=0", "split_max_keys=3", "QSV_FACTOR=0", "fused_factor=0", "QSV_SIDE_SLOTS=8", "push_plan")
# (push_plan sets QSV_PUSH_PLAN, the sizes of the pushes of StatevectorDevice.expectation_values: a case of the sampler or of
# the exact CVaR -- one call of its own each -- runs the same with it as without)
SAME_BITS = {"defaults", "push_plan", "fused_lds_table=0", "side_diag=0", "streams=1", "chain_stream=0", "poll_results=0"}
OPTIONS = {"sides_r3=0": ("sides_r3", 0), "fused_lds_table=0": ("fused_lds_table", 0), "side_diag=0": ("side_diag", 0),
           "streams=1": ("streams", 1), "chain_stream=0": ("chain_stream", 0), "poll_results=0": ("poll_results", 0),
           "split_max_keys=3": ("split_max_keys", 3), "fused_factor=0": ("fused_factor", 0)}
ENVIRONMENT = {"QSV_NO_HALF_SIDES": ("QSV_NO_HALF_SIDES", "1"), "QSV_FACTOR=0": ("QSV_FACTOR", "0"),
               "QSV_SIDE_SLOTS=8": ("QSV_SIDE_SLOTS", "8")}


def _case(tag, n, blocks, kind, dtype, variant, rng_values):
    P = sum(count for _, count, _ in blocks)
    perm, op_seed, terms, shots, alpha, plan = rng_values
    name = f"{tag}-n{n}-L{'+'.join(str(L) for L, _, _ in blocks)}-P{P}-{kind}-{dtype}-{variant}"
    if variant == "push_plan":
        name += "=" + ",".join(str(s) for s in plan)
    return {"id": name, "n": n, "blocks": blocks, "perm": perm, "kind": kind, "dtype": dtype, "variant": variant,
            "op_seed": op_seed, "terms": terms, "shots": shots, "alpha": alpha, "plan": plan}


def draw_cases() -> list[dict]:
    """The matrix: ``N_CASES`` cases drawn from ``default_rng(SEED)`` (every other one at n = 20, the only size with the
    one-launch route), then the cases added by hand for strata the draw does not reach."""
    rng = np.random.default_rng(SEED)
    cases = []
    for j in range(N_CASES):
        kind = str(rng.choice(KINDS))
        # (the sampler and exact CVaR are checked against 2^n probabilities on the host: at most 20 qubits, 65 evaluations)
        small = kind in ("sampler", "cvar")
        n = 20 if j % 2 == 0 else int(rng.choice([s for s in SIZES if s != 20 and (not small or s < 20)]))
        P = int(rng.choice([b for b in BATCHES if not small or b <= 65]))
        n_blocks = min(P, int(rng.integers(2, 4)))
        cuts = np.sort(rng.choice(np.arange(1, P), size=n_blocks - 1, replace=False)) if n_blocks > 1 else np.zeros(0, int)
        counts = np.diff(np.concatenate([[0], cuts, [P]])).tolist()
        blocks = []
        for count in counts:
            L = int(rng.integers(2, 7)) if rng.random() < 0.85 else int(rng.choice([8, 9]))
            blocks.append((L, int(count), int(rng.integers(0, 1000))))
        fp32 = rng.random() < 0.2 and kind != "cvar" and (kind != "sampler" or n <= 16)
        variant = str(rng.choice(VARIANTS))
        perm = rng.permutation(P).tolist()
        plan = sorted(int(x) for x in rng.integers(1, max(2, P), size=2))
        values = (perm, int(rng.integers(0, 10_000)), int(rng.integers(6, 501)), int(rng.integers(1024, 4097)),
                  float(rng.choice([1.0, 0.5, 0.05, round(float(rng.uniform(0.01, 0.99)), 4)])), plan)
        cases.append(_case(f"d{j:02d}", n, blocks, kind, "fp32" if fp32 else "fp64", variant, values))

    def hand(tag, n, blocks, kind, variant="defaults", shots=2048, alpha=0.5, terms=6):
        P = sum(c for _, c, _ in blocks)
        cases.append(_case(tag, n, blocks, kind, "fp64", variant, (list(range(P))[::-1], 7, terms, shots, alpha, [P])))

    # route 0 (one tile): no size of the draw fits one tile
    hand("h01", 12, [(3, 5, 1), (9, 3, 2)], "ising")
    # four and five keys (the factorised expectation; the population of test_split_evaluations_with_four_and_five_keys)
    hand("h02", 20, [(6, 32, 0), (5, 8, 0)], "quadratic")
    # half sides in a push of more than 64 evaluations (slot hand-over; the benchmark's population doubled)
    hand("h03", 20, [(4, 128, 0)], "ising")
    # a swept two-tile side on the one-launch route
    hand("h04", 20, [(5, 64, 0)], "ising", "QSV_NO_HALF_SIDES")
    # a general operator and the split sampler over the n = 20 sides_r3 plans (half sides among them)
    hand("h05", 20, [(5, 64, 0)], "general")
    hand("h06", 20, [(5, 32, 0), (4, 8, 0)], "sampler")
    # half sides of one key: thirteen virtual qubits a side from twelve own qubits and one key (circuits 6, 38 and 55, 58 of
    # these populations split that way and no narrower); a push of 192
    hand("h07", 20, [(5, 64, 3), (5, 64, 7), (6, 64, 4)], "ising")
    return cases


CASES = draw_cases()
SEEN: dict[tuple, str] = {}  # stratum -> the case whose evaluation was checked against the oracle


def _population(case):
    circuits, params = [], []
    for L, count, seed in case["blocks"]:
        _, c, p = helpers.population_circuits(case["n"], L, count, seed=seed)
        circuits += c
        params += p
    return [circuits[i] for i in case["perm"]], [params[i] for i in case["perm"]]


def _operator(case):
    n, kind, seed = case["n"], case["kind"], case["op_seed"]
    if kind in ("quadratic", "fields", "cubic"):
        return _diagonal_operator(n, seed, kind)
    if kind == "general":
        base = helpers.random_pauli_operator(n, case["terms"], seed=seed, alphabet="IXYZ")
        phases = np.exp(1j * np.random.default_rng(seed).uniform(-0.3, 0.3, size=len(base)))
        return PauliOperator(base.labels, base.coeffs * phases)
    return helpers.random_ising_operator(n, seed=seed)


def _device(case, dtype, monkeypatch, variant="defaults", split=True):
    """A device with the case's variant applied; the environment stays set (in ``monkeypatch``) until the case ends,
    so that circuits registered later see it too."""
    if variant in ENVIRONMENT:
        monkeypatch.setenv(*ENVIRONMENT[variant])
    elif variant == "push_plan":
        monkeypatch.setenv("QSV_PUSH_PLAN", ",".join(str(s) for s in case["plan"]))
    elif variant == "group=3":  # (launch groups of three state slots and of eight side-table slots: a batch spans many)
        monkeypatch.setenv("QSV_SIDE_SLOTS", "8")
    dev = StatevectorDevice(case["n"], dtype=dtype, group=3 if variant == "group=3" else 0)
    if variant in OPTIONS:
        dev.set_option(*OPTIONS[variant])
    if not split:
        dev.set_option("split", 0)
    return dev


def _forms(dev, op, circuits):
    """circuit_form of every circuit (registered under ``op``), checked against circuit_cost and for consistency."""
    ev = OperatorCircuitEvaluator(op, statevector_device=dev)
    costs = ev.circuit_costs(circuits)
    names = list(_lib.ROUTE_NAMES)
    forms = []
    full = (1 << dev.n_qubits) - 1
    for c, cost in zip(circuits, costs):
        f = dev.circuit_form(c)
        assert names[f["route"]] == cost["route"] and f["n_keys"] == cost["n_keys"], (f, cost)
        if f["n_virtual"][0]:
            # (the two sides share the cut keys: virtual qubits = own qubits + keys on both; n_keys is the route's, 0 off the
            # split routes, where a circuit with a split form of more keys than the operator's kernels take runs its passes)
            keys = f["n_virtual"][0] - bin(f["mask_x"]).count("1")
            assert f["mask_x"] & f["mask_y"] == 0 and f["mask_x"] | f["mask_y"] == full, f
            assert f["n_virtual"][1] - bin(f["mask_y"]).count("1") == keys and 0 <= keys <= 5, f
            assert keys == f["n_keys"] or f["route"] not in (1, 2), f
            assert f["amps_per_thread"] in (8, 16), f
        forms.append(f)
    return forms


def _stratum(form, kind, dtype):
    return (form["route"], form["n_keys"], form["amps_per_thread"], form["halves"], form["outer"], form["one_launch"], kind, dtype)


def _diag_table(op):
    """D[i] = sum_k c_k (-1)^popcount(i & z_k) of a diagonal operator."""
    index = np.arange(1 << op.num_qubits, dtype=np.uint64)
    table = np.zeros(index.size)
    for z, c in zip(op.z_mask, op.coeffs):
        parity = index & np.uint64(z)
        for shift in (32, 16, 8, 4, 2, 1):
            parity ^= parity >> np.uint64(shift)
        table += np.where(parity & np.uint64(1), -c.real, c.real)
    return table


def check_draws(states, values, seed, circuits, params, forms, probs_of, table, dtype, spread, first_eval=0):
    """Every shot of every evaluation accepted against the exact CDF in its sampler's order; in fp64 at most 1 % of the shots
    differ from the exact draw; values == D[state].  Returns the reports."""
    reports = []
    shots = states.shape[1]
    for i, form in enumerate(forms):
        probs = probs_of(i)
        order = split_order(form["mask_x"], form["mask_y"]) if form["split_sampled"] else plain_order(len(probs).bit_length() - 1)
        check = DrawCheck(probs, order, DELTA_FP64 if dtype == "fp64" else DELTA_FP32)
        u = shot_uniform(seed, first_eval + i, np.arange(shots))
        rep = check.report(u, states[i])
        rep["split_sampled"] = form["split_sampled"]
        assert rep["rejected"] == 0, (i, form, rep)
        if dtype == "fp64":
            assert rep["differ_fraction"] <= 0.01, (i, form, rep)
        if values is not None:
            assert np.abs(values[i] - table[states[i].astype(np.int64)]).max() <= 1e-12 * spread, i
        reports.append(rep)
    return reports


def _values(dev, op, kind, circuits, params, case):
    if kind == "cvar":
        dev.set_operator(op)
        return dev.exact_cvar_batch(circuits, params, case["alpha"])
    return OperatorCircuitEvaluator(op, statevector_device=dev).evaluate_circuits(circuits, params)


def _oracle_check(c_oracle, case, op, circuit, param, got, dtype, spread):
    n, kind = case["n"], case["kind"]
    if kind == "sampler":
        return  # (checked by the caller against the oracle's probabilities)
    if kind == "cvar":
        probs = np.abs(c_oracle.simulate(circuit, param)) ** 2
        table = c_oracle.diagonal_table(op)
        alpha = case["alpha"]
        want = float(np.dot(probs, table)) if np.isclose(alpha, 1) else so.cvar_expectation(
            list(zip(range(1 << n), probs.tolist(), table.tolist())), alpha)
    else:
        diagonal = not (op.x_mask.any())
        want = c_oracle.evaluate(circuit, param, op, c_oracle.diagonal_table(op) if diagonal else None)
    tol = EXP_TOL if dtype == "fp64" else FP32_REL * spread
    assert abs(got - want) < tol, (case["id"], got, want)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_split_matrix(case, c_oracle, monkeypatch):
    n, kind, dtype, variant = case["n"], case["kind"], case["dtype"], case["variant"]
    circuits, params = _population(case)
    op = _operator(case)
    spread = float(np.abs(op.coeffs).sum())
    opened = []
    try:
        # the pass path (fp64, splitting off) and the defaults of the case's dtype, before any variant's environment
        plain = StatevectorDevice(n)
        plain.set_option("split", 0)
        opened.append(plain)
        default = StatevectorDevice(n, dtype=dtype)
        opened.append(default)
        _forms(default, op, circuits)  # (registered before a variant's environment is set)
        dev = _device(case, dtype, monkeypatch, variant) if variant != "defaults" else default
        if dev is not default:
            opened.append(dev)
        forms = _forms(dev, op, circuits)
        if kind == "sampler":
            seed = 1000 + case["op_seed"]
            dev.set_operator(op)
            states, values = dev.sample_batch(circuits, params, case["shots"], seed, with_values=True)
            if dev is not default:
                default.set_operator(op)
                base, _ = default.sample_batch(circuits, params, case["shots"], seed)
                if variant in SAME_BITS:
                    assert np.array_equal(states, base)
            plain.set_operator(op)
            table = _diag_table(op)
            check_draws(states, values, seed, circuits, params, forms, lambda i: plain.probabilities(circuits[i], params[i]),
                        table, dtype, spread)
            # the oracle: the first evaluation of every stratum against the C oracle's probabilities
            for i, form in enumerate(forms):
                key = _stratum(form, kind, dtype)
                if key in SEEN:
                    continue
                SEEN[key] = case["id"]
                probs = np.abs(c_oracle.simulate(circuits[i], params[i])) ** 2
                check_draws(states[i : i + 1], values[i : i + 1], seed, [circuits[i]], [params[i]], [form], lambda _: probs, table,
                            dtype, spread, first_eval=i)
            return
        got = _values(dev, op, kind, circuits, params, case)
        # 1. against the pass path
        ref = np.asarray(_values(plain, op, kind, circuits, params, case))
        bound = EXP_TOL if dtype == "fp64" else FP32_REL * spread
        bad = np.nonzero(~(np.abs(np.asarray(got) - ref) < bound))[0]
        if bad.size:  # (which evaluations, in which form, and which side of the comparison a second call reproduces)
            again = np.asarray(_values(dev, op, kind, circuits, params, case))
            ref_again = np.asarray(_values(plain, op, kind, circuits, params, case))
            detail = [(int(i), got[i], float(ref[i]), float(again[i]), float(ref_again[i]), forms[i]) for i in bad[:8]]
            pytest.fail(f"{case['id']}: {bad.size} evaluations off the pass path (index, got, pass path, both again, form): {detail}")
        # 2. the same bits where the design promises them; 1e-10 where the option reorders the sums
        if dev is not default:
            base = _values(default, op, kind, circuits, params, case)
            if variant in SAME_BITS:
                assert got == base
            else:
                assert np.abs(np.asarray(got) - np.asarray(base)).max() < bound
        assert _values(dev, op, kind, circuits[::-1], params[::-1], case) == got[::-1]
        for i in range(min(3, len(circuits))):
            assert _values(dev, op, kind, [circuits[i]], [params[i]], case)[0] == got[i], i
        # 3. the first evaluation of every stratum against the C oracle
        for i, form in enumerate(forms):
            key = _stratum(form, kind, dtype)
            if key in SEEN:
                continue
            SEEN[key] = case["id"]
            _oracle_check(c_oracle, case, op, circuits[i], params[i], got[i], dtype, spread)
    finally:
        for d in opened:
            d.close()


def test_the_matrix_covers_every_form(monkeypatch):
    """The strata of the whole list of cases (read through circuit_form, without evaluating): every route; keys 0 .. 5 on the
    split routes; on the one-launch route sides of 16 and of 8 amplitudes per thread, half sides of one, two and three keys
    and a swept two-tile side; a general operator and the split sampler over the n = 20 sides_r3 plans; a push of more
    than 64 evaluations that holds a half side."""
    strata = {}
    for case in CASES:
        circuits, _ = _population(case)
        op = _operator(case)
        with monkeypatch.context() as m:
            dev = _device(case, case["dtype"], m, case["variant"])
            try:
                forms = _forms(dev, op, circuits)
            finally:
                dev.close()
        for f in forms:
            strata.setdefault(_stratum(f, case["kind"], case["dtype"]) + (case["n"], len(circuits) > 64, f["split_sampled"]), case["id"])
    print(f"\n{len(strata)} strata (route, keys, amplitudes per thread, halves, outer, one launch, kind, dtype, n, push > 64, split sampled):")
    for key in sorted(strata, key=str):
        print("  ", key, strata[key])
    keys = list(strata)
    routes = {k[0] for k in keys}
    assert routes >= {0, 1, 2, 3}, routes
    assert {k[1] for k in keys if k[0] in (1, 2)} >= {0, 1, 2, 3, 4, 5}
    one = [k for k in keys if k[0] == 1]
    assert {k[2] for k in one} >= {8, 16}
    assert {k[1] for k in one if k[3]} >= {1, 2, 3}, "half sides of one, two and three keys"
    assert any(k[2] == 8 and not k[3] and max(k[4]) >= 1 for k in one), "a swept two-tile side"
    assert any(k[6] == "general" and k[8] == 20 and k[2] == 8 for k in keys), "a general operator over the sides_r3 plans"
    assert any(k[6] == "sampler" and k[8] == 20 and k[2] == 8 and k[10] for k in keys), "the split sampler over the sides_r3 plans"
    assert any(k[3] and k[9] for k in one), "a push of more than 64 evaluations holding a half side"


@pytest.mark.parametrize("n,dtype,variant", [(14, "fp64", "defaults"), (14, "fp32", "defaults"), (17, "fp64", "defaults"),
                                             (20, "fp64", "defaults"), (20, "fp64", "QSV_NO_HALF_SIDES"), (14, "fp64", "group=3")])
def test_exact_draws_of_both_samplers(n, dtype, variant, c_oracle, monkeypatch):
    """Both samplers in one mixed, shuffled batch: split-sampled circuits (zero to three keys; at n = 20 the sides_r3 plans,
    half sides, and with QSV_NO_HALF_SIDES the swept ones) and plain-sampled ones (four and five keys, unsplittable), two
    seeds of 4096 shots.  Every shot is accepted against the exact CDF in its sampler's order; in fp64 at most 1 % differ
    from the exact draw; values are D[state] within 1e-12 sum |c|.  With group=3 the batch spans many launch groups of
    both kinds, and every consumer of final states is held to the same bits as with one group (_check_many_groups)."""
    blocks = [(4, 24, 2 * n), (6, 12, 2 * n + 1), (9, 3, 2 * n + 2)]
    if n == 20:
        blocks = [(4, 16, 0), (5, 16, 0), (6, 8, 0), (9, 3, 8)]
    P = sum(c for _, c, _ in blocks)
    case = {"n": n, "blocks": blocks, "perm": np.random.default_rng(n).permutation(P).tolist(), "plan": [P]}
    circuits, params = _population(case)
    op = helpers.random_ising_operator(n, seed=n)
    spread = float(np.abs(op.coeffs).sum())
    table = _diag_table(op)
    plain = StatevectorDevice(n)
    plain.set_option("split", 0)
    dev = _device(case, dtype, monkeypatch, variant)
    try:
        forms = _forms(dev, op, circuits)
        split_keys = {f["n_keys"] for f in forms if f["split_sampled"]}
        assert len(split_keys) >= 2 and any(not f["split_sampled"] for f in forms), forms
        if n == 20:
            assert any(f["split_sampled"] and f["amps_per_thread"] == 8 for f in forms)
            assert any(f["halves"] for f in forms) == (variant == "defaults")
        dev.set_operator(op)
        plain.set_operator(op)
        probs = [plain.probabilities(c, p) for c, p in zip(circuits, params)]
        # the oracle's probabilities for one circuit of each sampler
        for want in (True, False):
            i = next(i for i, f in enumerate(forms) if f["split_sampled"] == want)
            assert np.abs(probs[i] - np.abs(c_oracle.simulate(circuits[i], params[i])) ** 2).max() < 1e-14
        total = differ = 0
        for seed in (2, 3):
            states, values = dev.sample_batch(circuits, params, 4096, seed, with_values=True)
            reports = check_draws(states, values, seed, circuits, params, forms, lambda i: probs[i], table, dtype, spread)
            total += sum(r["shots"] for r in reports)
            differ += sum(r["differ"] for r in reports)
        print(f"\nn = {n} {dtype} {variant}: {differ} of {total} shots differ from the exact draw ({sorted(split_keys)} keys split-sampled)")
        if variant == "group=3":
            _check_many_groups(dev, dtype, op, circuits, params, monkeypatch)
    finally:
        dev.close()
        plain.close()


def _check_many_groups(dev, dtype, op, circuits, params, monkeypatch):
    """Every consumer of final states on batches that span many launch groups of ``dev`` (three state slots, eight side-table
    slots), bit for bit: both samplers against a device whose launch groups hold the whole batch (a draw depends on the
    evaluation's index in its batch); the exact CVaR, kept states and the observables (split, plain and kept-state
    evaluations in one batch) against the same calls one evaluation at a time."""
    n = dev.n_qubits
    monkeypatch.delenv("QSV_SIDE_SLOTS")
    whole = StatevectorDevice(n, dtype=dtype)
    try:
        whole.set_operator(op)
        grouped, one = (d.sample_batch(circuits, params, 256, 5, with_values=True) for d in (dev, whole))
        assert np.array_equal(grouped[0], one[0]) and np.array_equal(grouped[1], one[1])
        assert dev.sample_cvar_batch(circuits, params, 256, 5, 0.5) == whole.sample_cvar_batch(circuits, params, 256, 5, 0.5)
        exact = dev.exact_cvar_batch(circuits, params, 0.5)
        assert exact == [dev.exact_cvar_batch([c], [p], 0.5)[0] for c, p in zip(circuits, params)]
        population = EVQEPopulation.random_population(n, 3, 7, True, 1)
        pairs = [ind.get_layer_search_circuits(2) for ind in population.individuals]
        values = [list(ind.get_layer_parameter_values(2)) for ind in population.individuals]
        together = dev.keep_states([front for front, _ in pairs], [[] for _ in pairs])
        alone = [dev.keep_states([front], [[]])[0] for front, _ in pairs]
        kept = [rest.continue_from(state) for (_, rest), state in zip(pairs, together)]
        for (_, rest), state, c, v in zip(pairs, alone, kept, values):
            assert np.array_equal(dev.statevector(c, v), dev.statevector(rest.continue_from(state), v))
        ops = [op, helpers.random_pauli_operator(n, 12, seed=3)]
        got = dev.observable_values(circuits + kept, params + values, ops)
        for i, (c, p) in enumerate(zip(circuits + kept, params + values)):
            assert np.array_equal(got[i], dev.observable_values([c], [p], ops)[0]), i
    finally:
        whole.close()


def test_exact_cvar_at_alpha_one_is_the_expectation_value(c_oracle):
    """qsv_exact_cvar_batch at alpha = 1 (numpy.isclose, the reference's test) is the expectation value -- not the accumulation
    loop, whose stopping rule leaves out the last 1e-5 of the mass --, and refuses decreasing parameter offsets there as at
    any other alpha."""
    n = 16
    _, circuits, params = helpers.population_circuits(n, 4, 6, seed=3)
    op = helpers.random_ising_operator(n, seed=16)
    dev = StatevectorDevice(n)
    try:
        dev.set_operator(op)
        table = c_oracle.diagonal_table(op)
        want = [c_oracle.evaluate(c, p, op, table) for c, p in zip(circuits, params)]
        for alpha in (1.0, 1.0 - 5e-6):
            got = dev.exact_cvar_batch(circuits, params, alpha)
            assert np.abs(np.asarray(got) - np.asarray(want)).max() < EXP_TOL, alpha
        ids, _, _ = dev._batch_metadata(circuits[:2])
        offsets = np.asarray([0, 5, 2], dtype=np.int64)
        values, out = np.zeros(8), np.zeros(2)
        for alpha in (1.0, 0.5):
            rc = dev._lib.qsv_exact_cvar_batch(dev._handle, 2, _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(values), alpha,
                                               _lib.as_ptr(out))
            assert rc == _lib.QSV_E_ARG, alpha
    finally:
        dev.close()
