"""A live handle walked through operators of every kind, on every consumer (tests/operator_walk.py; the CPU half is
tests/test_operator_walk.py).

One StatevectorDevice is shared by evaluators with different operators; each "is it my operator? else set_operator" is a state
transition (qsv_set_operator) on a handle that holds registered circuits, plans in the arena, side tables and a sort order of D,
recorded launches, kept states, a gradient plan and observable sets.  The walk visits the five kinds in an order that makes
every ordered pair adjacent once (21 stops) and runs every consumer at every stop.

Main assertion: every number is, BIT FOR BIT, what a reference device returns that only ever saw that kind's operator (same
dtype, default options, computed once per kind), and a revisit gives the first visit's bits -- the promise of fixed-order sums
that do not depend on batch, order or what came between (SAME_BITS, tests/test_gpu_replay.py), extended across operator changes.
Routes and launch forms must be the reference device's too.  Second assertion, at the first visit of a kind: the reference device
against the CPU oracles, at the tolerances of the modules that own them.  Mismatches are collected over the walk and reported
once, as a table of (stop, transition, consumer, circuit, got, want, route); a HIP error ends the test at once.

No consumer is compared by tolerance in place of bits.  What the walk found when it was written (HISTORY.md, after round 4,
item 7): at 14 qubits the walked handle replayed the repeated (a) calls under "ising" and "fields" from the second stop on,
and a fresh device never did -- the first batch of a handle that holds a circuit of more than three keys spoiled its own launch
record.  With `order_valid` left standing by qsv_set_operator the 14-qubit walk fails from stop 1 on ("ising" -> "fields", the
exact CVaR of every circuit, at every later visit of a diagonal kind: 56 rows); with `quadratic` left standing from stop 2 on
("fields" -> "cubic": the expectation values of every split circuit on lists and matrix, the four-key circuit's route and
launch form, parameter shift and the gradient plan: 168 rows).
"""

from __future__ import annotations

import gc
import re
import time

import numpy as np
import pytest

import adjoint_reference
import circuit_families as cf
import helpers
import operator_walk as ow
import variance_reference as vr
from oracle import statevector_oracle as so
from queasars_amd.circuit_evaluation import CircuitEvaluatorException, OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.planning import build_plan_words
from test_gpu_adjoint import EXP_TOL as GRADIENT_TOL, FP32_REL as GRADIENT_FP32_REL
from test_gpu_circuit_families import FP32_REL
from test_gpu_operator_families import EXP_TOL
from test_gpu_variance import TOL_FP32_REL

pytestmark = pytest.mark.gpu

ARMS = [(10, "fp64"), (14, "fp64"), (14, "fp32"), (20, "fp64")]
# (a) expectation values, (b) routes, (c) gradients, (d) observables, (e) variances, (f) diagonal-only consumers, (g) kept states
CONSUMERS = {10: "abcdef", 14: "abcdefg", 20: "abe"}
GRADIENT_CIRCUITS = {10: ("individual 0", "ladder"), 14: ("individual 0", "two_blocks 2")}
KEPT_LAYER = 2  # (cut after the second layer)
SHOTS, TOP_K, REFUSED = 256, 4, "CircuitEvaluatorException"
REFUSAL = re.compile(r"needs? a diagonal operator \(call qsv_set_operator with I/Z terms only\)")  # (qsv_api.hip, three places)

_STATES: dict = {}  # (n, circuit name) -> oracle state at the first parameter set: computed once, shared, never written to


def _state(n, name, circuit, params, c_oracle):
    if (n, name) not in _STATES:
        state = helpers.oracle_state(circuit, params) if n <= 14 else c_oracle.simulate(circuit, params)
        state.setflags(write=False)
        _STATES[n, name] = state
    return _STATES[n, name]


def _matrix(params):
    """The parameter vectors as rows of a device matrix (tests/test_gpu_replay.py _matrix)."""
    import torch

    width = max(1, max(len(p) for p in params))
    host = np.zeros((len(params), width))
    for i, p in enumerate(params):
        host[i, : len(p)] = p
    matrix = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return matrix


class _Handle:
    """One device, its evaluators (made at a kind's first visit, as a solver makes its aux operators' evaluators) and what it
    keeps through a walk: its own circuit objects, parameter matrices, kept states and gradient plan."""

    def __init__(self, n: int, dtype: str, walked: bool):
        self.n, self.dtype, self.walked = n, dtype, walked
        self.ops = ow.kinds(n)
        self.dev = StatevectorDevice(n, dtype=dtype)
        self.evaluators: dict = {}
        individuals, cases = ow.population(n)
        self.set_cases(cases)
        self.observables = ow.observable_set(n)
        if n in GRADIENT_CIRCUITS:
            chosen = [case for case in cases if case[0] in GRADIENT_CIRCUITS[n]]
            assert len(chosen) == 2
            self.grad_names, self.grad_circuits = [c[0] for c in chosen], [c[1] for c in chosen]
            self.grad_params = [c[2] for c in chosen]
            self.wrt = [list(range(0, c.num_parameters, 7)) for c in self.grad_circuits]  # (every seventh: all three slots, u and cu3)
            self.grad_matrix = _matrix(self.grad_params)
            self.out_width = max(len(w) for w in self.wrt) + 3
        self.plan = None
        self.kept = None
        if "g" in CONSUMERS[n]:
            cut = [ind.get_layer_search_circuits(KEPT_LAYER) for ind in individuals[:2]]
            self.fronts, self.rests = [front for front, _ in cut], [rest for _, rest in cut]
            self.kept_values = [list(ind.get_layer_parameter_values(KEPT_LAYER)) for ind in individuals[:2]]
            self.kept_names = [f"individual {i} on its kept state" for i in range(2)]

    def set_cases(self, cases, with_matrix: bool = True):
        self.names, self.circuits = [c[0] for c in cases], [c[1] for c in cases]
        self.sets = ow.parameter_sets([c[2] for c in cases], seed=self.n)
        self.matrix = _matrix(self.sets[0]) if with_matrix else None

    def evaluator(self, kind: str) -> OperatorCircuitEvaluator:
        if kind not in self.evaluators:
            self.evaluators[kind] = OperatorCircuitEvaluator(self.ops[kind], statevector_device=self.dev)
        return self.evaluators[kind]

    def register(self, kind: str):
        self.evaluator(kind).circuit_costs(self.circuits)

    def close(self):
        if self.plan is not None:
            self.plan.close()
        self.dev.close()


def _consume(h: _Handle, kind: str, letters: str) -> dict:
    """Every consumer of `letters` on `h` under the operator of `kind`, set the way the product sets it: by the kind's evaluator
    on the shared device.  {(consumer, circuit): value}."""
    import torch

    dev, ev = h.dev, h.evaluator(kind)
    names, circuits, sets = h.names, h.circuits, h.sets
    diagonal = kind in ow.DIAGONAL_KINDS
    out: dict = {}

    def rows(tag, values, row_names=names):
        assert len(values) == len(row_names), tag
        for name, value in zip(row_names, values):
            out[tag, name] = np.array(value)

    # (a) host lists, the same batch twice more with other values (the layout repeated, then replayed), a device matrix
    before, replayed = dev.replayed_pushes(), []
    for i, values in enumerate(sets):
        rows(f"a lists {i}", ev.evaluate_circuits(circuits, values))
        replayed.append(dev.replayed_pushes() - before)
    out["a replayed pushes", ""] = tuple(replayed)
    if h.matrix is not None:
        rows("a matrix", ev.evaluate_device_parameters(circuits, h.matrix))
    if "b" in letters:
        for name, c, cost in zip(names, circuits, ev.circuit_costs(circuits)):
            out["b route", name] = (cost["route"], cost["n_keys"], cost["n_passes"])
            out["b launch form", name] = tuple(sorted(dev.circuit_launch_form(c).items()))
    if "c" in letters:
        rows("c parameter shift", dev.gradients(h.grad_circuits, h.grad_params, h.wrt), h.grad_names)
        rows("c adjoint", dev.adjoint_gradients(h.grad_circuits, h.grad_params, h.wrt), h.grad_names)
        if h.n == 14 and h.dtype == "fp64":
            # the walked handle's plan was made at the first stop, under the first kind, and runs under the operator set now;
            # the reference device differentiates the same device matrix without a plan
            grads = torch.full((len(h.grad_circuits), h.out_width), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            width = int(h.grad_matrix.shape[1])
            if h.walked:
                if h.plan is None:
                    h.plan = dev.gradient_plan(h.grad_circuits, width, h.out_width, h.wrt)
                h.plan.run(h.grad_matrix.data_ptr(), 0, grads.data_ptr())
            else:
                dev.gradients_of_device_parameters(h.grad_circuits, h.grad_matrix.data_ptr(), width, 0, grads.data_ptr(), h.out_width, h.wrt)
            torch.cuda.synchronize()
            rows("c gradient plan", grads.cpu().numpy(), h.grad_names)
    if "d" in letters:
        rows("d observables", dev.observable_values(circuits, sets[0], h.observables))
        rows("d then a", ev.evaluate_circuits(circuits, sets[0]))
    if "e" in letters:
        values, variances = dev.variances(circuits, sets[0])
        rows("e values", values)
        rows("e variances", variances)
    if "f" in letters:
        calls = {"f exact cvar": lambda: (dev.exact_cvar_batch(circuits, sets[0], 0.3),),
                 "f samples": lambda: dev.sample_batch(circuits, sets[0], SHOTS, ow.SEED, with_values=True),
                 "f sampled cvar": lambda: (dev.sample_cvar_batch(circuits, sets[0], SHOTS, ow.SEED, 0.5),),
                 "f top states": lambda: dev.top_states(circuits, sets[0], TOP_K, with_values=True)}
        for tag, call in calls.items():
            # the refusals are where qsv_api.hip has them (the has_diag_part && diagonal checks), and nowhere else.  Every error
            # of the library is a CircuitEvaluatorException: only the refusal's own message makes one a refusal, anything
            # else -- a HIP error -- leaves the test here, before another call is made
            try:
                parts = call()
            except CircuitEvaluatorException as refusal:
                if diagonal or not REFUSAL.search(str(refusal)):
                    raise
                out[tag, ""] = REFUSED
                continue
            assert diagonal, (kind, tag, "answered under an operator without a table of D")
            out[tag, ""] = "answered"
            for part, values in enumerate(parts):
                rows(f"{tag} [{part}]", values)
        rows("f samples without values", dev.sample_batch(circuits, sets[0], SHOTS, ow.SEED)[0])
        rows("f then a", ev.evaluate_circuits(circuits, sets[0]))
    if "g" in letters:
        if h.kept is None:  # (once, at the handle's first stop)
            h.kept_states = ev.keep_states(h.fronts, [[] for _ in h.fronts])
            h.kept = [rest.continue_from(state) for rest, state in zip(h.rests, h.kept_states)]
        rows("g kept states", ev.evaluate_circuits(h.kept, h.kept_values), h.kept_names)
    return out


def _difference(got, want) -> str:
    if isinstance(got, (str, tuple)) or isinstance(want, (str, tuple)):
        return f"{got!r} | {want!r}"
    a, b = np.atleast_1d(got).ravel(), np.atleast_1d(want).ravel()
    if a.shape != b.shape:
        return f"shape {np.shape(got)} | shape {np.shape(want)}"
    differ = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(a, b)])
    if not len(differ):
        return f"dtype {a.dtype} | dtype {b.dtype}"
    i = int(differ[0])
    return f"{a[i]!r} | {b[i]!r} (entry {i}, {len(differ)} of {a.size} differ)"


def _compare(findings, stop, move, got, want, what="reference device"):
    """Rows for every entry of `want` that `got` does not have bit for bit."""
    for key, value in want.items():
        consumer, circuit = key
        if key not in got:
            findings.append((stop, move, consumer, circuit, "missing", what, ""))
        elif not ow.same_bits(got[key], value):
            route = got.get(("b route", circuit), ("",))[0]
            findings.append((stop, move, f"{consumer} vs {what}", circuit, *_difference(got[key], value).split(" | ", 1), route))


def _self_consistency(findings, stop, move, got, letters):
    """An observable set and the refusals leave the handle's operator in place: the next (a) call gives (a)'s bits."""
    for tag in [t for t, letter in (("d then a", "d"), ("f then a", "f")) if letter in letters]:
        for (consumer, circuit), value in got.items():
            if consumer == tag and not ow.same_bits(value, got["a lists 0", circuit]):
                findings.append((stop, move, f"{tag} vs a lists 0", circuit, repr(value), repr(got["a lists 0", circuit]), ""))


def _oracle(findings, h: _Handle, kind: str, got: dict, letters: str, c_oracle):
    """The reference device's numbers of one kind against the CPU oracles, each at the tolerance of the module that owns it."""
    n, op, fp32 = h.n, h.ops[kind], h.dtype == "fp32"
    scale = ow.spread(op)
    diagonal = kind in ow.DIAGONAL_KINDS
    table = c_oracle.diagonal_table(op) if diagonal else None
    move = f"first visit of {kind}"

    def check(consumer, circuit, value, want, bound):
        error = float(np.abs(np.asarray(value) - np.asarray(want)).max(initial=0.0))
        if not error < bound:
            findings.append(("oracle", move, consumer, circuit, f"error {error:.3e}", f"bound {bound:.3e}", got.get(("b route", circuit), ("",))[0]))

    scratch = np.zeros(2 << n)
    for name, c, p in zip(h.names, h.circuits, h.sets[0]):
        # (a): tests/test_gpu_operator_families.py's bound
        want = c_oracle.evaluate(c, p, op, table, scratch)
        check("a lists 0", name, got["a lists 0", name], want, FP32_REL * scale if fp32 else EXP_TOL * max(1.0, scale / 50.0))
        if "e" in letters:
            state = _state(n, name, c, p, c_oracle)
            check("e values", name, got["e values", name], want, FP32_REL * scale if fp32 else vr.TOL_VALUES)
            bound = TOL_FP32_REL * scale ** 2 if fp32 else vr.tol_fp64(op)
            if n <= 14:
                check("e variances", name, got["e variances", name], vr.reference(op, [state])[1][0], bound)
            elif diagonal:
                # (20 qubits: variance_reference.moments passes over the 2^20 state string by string -- 10 s per circuit under
                # the Ising operator, 4 s under "mixed".  Its quantity from the plain-C oracle's table of D instead ...
                check("e variances", name, got["e variances", name], ow.diagonal_moments(table, state)[1], bound)
            else:
                # ... and, for operators with x masks, with the strings grouped by x mask: one pass per group.
                # tests/test_operator_walk.py holds both forms to variance_reference.moments.)
                check("e variances", name, got["e variances", name], ow.grouped_moments(op, state)[1], bound)
        if "f" in letters and diagonal:
            # the exact CVaR as tests/test_gpu_differential.py _oracle_check holds it
            probs = np.abs(_state(n, name, c, p, c_oracle)) ** 2
            want = so.cvar_expectation(list(zip(range(1 << n), probs.tolist(), table.tolist())), 0.3)
            check("f exact cvar", name, got["f exact cvar [0]", name], want, FP32_REL * scale if fp32 else EXP_TOL)
    if "c" in letters:
        for name, c, p, wrt in zip(h.grad_names, h.grad_circuits, h.grad_params, h.wrt):
            want = adjoint_reference.gradient(c, p, op)[np.asarray(wrt)]
            assert float(np.abs(want).max()) > 1e-3  # (not a gradient of zeros)
            bound = GRADIENT_FP32_REL * scale if fp32 else GRADIENT_TOL
            check("c parameter shift", name, got["c parameter shift", name], want, bound)
            check("c adjoint", name, got["c adjoint", name], want, bound)
            if ("c gradient plan", name) in got:
                check("c gradient plan", name, got["c gradient plan", name][: len(wrt)], want, bound)
                assert not got["c gradient plan", name][len(wrt):].any()  # (zeros behind a circuit's entries)


def _table(findings) -> str:
    head = ("stop", "transition", "consumer", "circuit", "got", "want", "route")
    return "\n".join(" | ".join(str(x) for x in row) for row in [head] + findings[:60]) + (
        f"\n... and {len(findings) - 60} more" if len(findings) > 60 else "")


def _print_routes(n, dtype, routes):
    print(f"\nn = {n} {dtype}: route / keys / passes per circuit under each kind")
    for name in routes[ow.KINDS[0]]:
        print(f"   {name:16s} " + " | ".join(f"{kind}: {routes[kind][name][0]} / {routes[kind][name][1]} / {routes[kind][name][2]}" for kind in ow.KINDS))


@pytest.mark.parametrize("n,dtype", ARMS, ids=[f"{n}-{dtype}" for n, dtype in ARMS])
def test_every_consumer_at_every_stop_of_the_walk(n, dtype, c_oracle):
    started = time.perf_counter()
    letters, stops = CONSUMERS[n], ow.walk()
    findings: list = []
    references: dict = {}
    walked = _Handle(n, dtype, walked=True)
    try:
        walked.register(stops[0])  # (the population once, before the first stop, under the first kind)
        for stop, kind in enumerate(stops):
            move = f"{stops[stop - 1]} -> {kind}" if stop else f"-> {kind}"
            if kind not in references:
                reference = _Handle(n, dtype, walked=False)  # (sees this kind's operator and no other)
                try:
                    reference.register(kind)
                    references[kind] = _consume(reference, kind, letters)
                    _oracle(findings, reference, kind, references[kind], letters, c_oracle)
                finally:
                    reference.close()
            got = _consume(walked, kind, letters)
            _compare(findings, stop, move, got, references[kind])  # (a revisit against the same bits as the first visit)
            _self_consistency(findings, stop, move, got, letters)
    finally:
        walked.close()
    # an observable set does not use the handle's operator: the same bits under every kind
    if "d" in letters:
        for kind in ow.KINDS[1:]:
            want = {key: value for key, value in references[ow.KINDS[0]].items() if key[0] == "d observables"}
            _compare(findings, "-", f"{ow.KINDS[0]} / {kind}", references[kind], want, "the set under another kind")
    routes = {kind: {name: references[kind]["b route", name] for name in walked.names} for kind in ow.KINDS}
    _print_routes(n, dtype, routes)
    print(f"   replayed pushes over the three (a) calls: {({kind: references[kind]['a replayed pushes', ''] for kind in ow.KINDS})}")
    # every batch of these arms records its launches (no chain of a second stream, tests/test_gpu_replay.py): the first (a) call
    # lays out and records, the second and the third are replayed -- on the fresh reference device of every kind, the
    # quadratic ones at 14 qubits with their four-key circuit included, and so (compared above) at every stop of the walk
    for kind in ow.KINDS:
        assert references[kind]["a replayed pushes", ""] == (0, 1, 2), (kind, references[kind]["a replayed pushes", ""])
    # what the arm is there for, read off split_rule: up to kMaxSplitKeys keys on the factor path (a quadratic operator), three
    # otherwise -- the four-key circuit splits under "ising" and "fields" and goes through gate passes under the others
    for kind in ow.KINDS:
        quadratic = kind in ("ising", "fields")
        if n == 10:
            assert {r[0] for r in routes[kind].values()} == {"one tile"}, routes[kind]
        if n == 14:
            assert routes[kind][ow.FOUR_KEYS][:2] == (("split", 4) if quadratic else ("gate passes", 0)), (kind, routes[kind])
            assert routes[kind]["all_pairs"][0] == "gate passes" and routes[kind]["two_blocks 2"][:2] == ("split", 2), routes[kind]
        if n == 20:
            assert {r[0] for r in routes[kind].values()} == {"split, one launch" if quadratic else "split"}, routes[kind]
            assert max(r[1] for r in routes[kind].values()) == 2 and min(r[1] for r in routes[kind].values()) >= 1, routes[kind]
    if n == 20:  # (a reduced side: the launch form under the quadratic kinds is smaller than the circuit's split form)
        forms = {kind: dict(references[kind]["b launch form", "two_blocks 2"])["n_virtual"] for kind in ("ising", "cubic")}
        assert sum(forms["ising"]) < sum(forms["cubic"]), forms
    print(f"   {len(stops)} stops, consumers {letters}: {time.perf_counter() - started:.1f} s")
    assert not findings, f"{len(findings)} mismatches over the walk\n" + _table(findings)


# ---- circuits coming and going during the walk ----------------------------------------------------------------------------------


def test_circuits_come_and_go_during_the_walk():
    """The same walk at 14 qubits while every third stop registers one new circuit and drops the one registered three stops
    earlier (del, gc.collect(): the next call reaps it, and its id may be used again): the arena then holds plans uploaded under
    different operators.  (a), (b) and (e) on all live circuits at every stop: the bits of the per-kind reference devices, which
    register the same circuits when they first meet them."""
    started = time.perf_counter()
    n, dtype, letters = 14, "fp64", "abe"
    stops = ow.walk()
    findings: list = []
    handles = {"walked": _Handle(n, dtype, walked=True)}
    walked = handles["walked"]
    _, cases = ow.population(n)
    live = {-1 - i: case for i, case in enumerate(cases) if case[0] in ("individual 0", "two_blocks 2", ow.FOUR_KEYS, "all_pairs")}
    first: dict = {}
    high_water = 0

    def at_stop(h, kind):
        h.set_cases(list(live.values()), with_matrix=False)  # (the list dies with this call: no reference outlives the stop)
        try:
            return _consume(h, kind, letters)
        finally:
            h.names, h.circuits, h.sets = [], [], []
            h.dev.forget_last_batch()

    try:
        for stop, kind in enumerate(stops):
            move = f"{stops[stop - 1]} -> {kind}" if stop else f"-> {kind}"
            if stop % 3 == 0:
                made = cf.ladder(n, 1, seed=stop) if (stop // 3) % 2 == 0 else cf.two_blocks(n, 2, seed=stop)
                live[stop] = (f"{'ladder' if (stop // 3) % 2 == 0 else 'two_blocks'} of stop {stop}", made[0], list(made[1]))
                del made
                if stop - 3 in live:
                    del live[stop - 3]
                    gc.collect()
            if kind not in handles:
                handles[kind] = _Handle(n, dtype, walked=False)
            want = at_stop(handles[kind], kind)
            got = at_stop(walked, kind)
            _compare(findings, stop, move, got, want)
            # a circuit that was there at the kind's first visit: those bits (the perturbed parameter sets are drawn for the
            # whole list, so they change as circuits come and go)
            for key, value in got.items():
                if key[0] in ("a lists 1", "a lists 2", "a replayed pushes"):
                    continue
                if not ow.same_bits(first.setdefault((kind, *key), value), value):
                    findings.append((stop, move, f"{key[0]} vs first visit", key[1], repr(value), repr(first[(kind, *key)]), ""))
            high_water = max(high_water, len(walked.dev._watched))
        # seven circuits were registered on the way and six of them dropped: their ids were destroyed as the walk went on
        assert len(live) == 5 and high_water <= 4 + 2, (len(live), high_water)
    finally:
        for h in handles.values():
            h.close()
    print(f"\n{len(stops)} stops with circuits coming and going: {time.perf_counter() - started:.1f} s")
    assert not findings, f"{len(findings)} mismatches over the walk\n" + _table(findings)


# ---- many alternations: the arena fills with plans uploaded again and is rebuilt --------------------------------------------------

ALTERNATION = ("ising", "mixed", "cubic")
ALTERNATIONS = 48
ARENA_WORDS = 1 << 20  # (upload_plans: the arena's first allocation is max(2 * the first batch's words, 2^20) words)


def test_many_alternations_rebuild_the_plan_arena(c_oracle, monkeypatch, capfd):
    """qsv_set_operator marks every plan as not uploaded and gives no arena room back, so every change of operator appends the
    used plans again until upload_plans finds the arena full and rebuilds it.  Eight circuits of cf.staging's largest shape
    ("everything over": 3106 plan words each) are 24848 words per upload; the arena's first allocation is 2^20 words, so
    floor(2^20 / 24848) = 42 uploads fit and the 43rd -- the 42nd change of operator -- rebuilds it.  48 stops over "ising",
    "mixed", "cubic" are 47 changes: one rebuild, shown as tests/test_gpu_configs.py's arena test shows it (every value keeps
    its bits through it) and by the library's own arena log.  Between two changes an (a) call and the exact CVaR (diagonal
    kinds) or the variances ("mixed")."""
    started = time.perf_counter()
    n = 10
    n_fold, n_trig, n_params = cf.STAGING_SHAPES["everything over"]
    made = [cf.staging(n, n_fold, n_trig - n_fold, n_params, seed=seed) for seed in range(8)]
    circuits, params = [c for c, _ in made], [list(p) for _, p in made]
    words = sum(len(build_plan_words(c)) for c in circuits)
    fit = max(2 * words, ARENA_WORDS) // words  # uploads that fit the arena
    assert fit < ALTERNATIONS - 1, (words, fit)  # (the count above, from the plan sizes)
    monkeypatch.setenv("QSV_ARENA_DEBUG", "1")
    ops = ow.kinds(n)
    dev = StatevectorDevice(n)
    first: dict = {}
    findings: list = []
    try:
        evaluators = {kind: OperatorCircuitEvaluator(ops[kind], statevector_device=dev) for kind in ALTERNATION}
        capfd.readouterr()
        for stop in range(ALTERNATIONS):
            kind = ALTERNATION[stop % 3]
            got = {"a": np.asarray(evaluators[kind].evaluate_circuits(circuits, params))}
            if kind == "mixed":
                got["e values"], got["e variances"] = dev.variances(circuits, params)
            else:
                got["f exact cvar"] = np.asarray(dev.exact_cvar_batch(circuits, params, 0.3))
            if kind not in first:
                table = c_oracle.diagonal_table(ops[kind]) if kind != "mixed" else None
                want = [c_oracle.evaluate(c, p, ops[kind], table) for c, p in zip(circuits, params)]
                assert np.abs(got["a"] - want).max() < EXP_TOL * max(1.0, ow.spread(ops[kind]) / 50.0), (kind, got["a"], want)
            for key, value in got.items():
                if not ow.same_bits(first.setdefault((kind, key), value), value):
                    findings.append((stop, kind, key, "", *_difference(value, first[kind, key]).split(" | ", 1), ""))
    finally:
        dev.close()
    log = [line for line in capfd.readouterr().err.splitlines() if line.startswith("plan arena: rebuilt")]
    rebuilds = [line for line in log if "(grows)" not in line]
    print(f"\n{ALTERNATIONS} stops, {words} plan words per upload, {fit} uploads fit: {len(log)} arena logs, {len(rebuilds)} rebuilds without growth; "
          f"{time.perf_counter() - started:.1f} s")
    assert len(rebuilds) >= 1, log
    assert not findings, f"{len(findings)} mismatches\n" + _table(findings)
