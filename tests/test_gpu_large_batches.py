"""GPU tests of host-list batches in which ONE PUSH holds more evaluations than its lane has slots (csrc/qsv_api.hip,
eval_push: split evaluations take slot ``lane * SG + j % SG``, ordinary ones ``lane * G + j % G`` or the auxiliary stream's).

1. The call DESIGN.md 4.10 records: the 2170 shifted evaluations of the mixed-depth n = 17 population in one
   ``evaluate_circuits`` call over host lists, three times on a fresh evaluator -- in a fresh process and on a fresh handle --
   bit for bit the values of one call per circuit, and the ends of every circuit's block against the plain-C oracle.
2. The regime around it at the smallest shapes (tests/batch_shapes.py).

The bound is the project's standing promise: an evaluation's bits are a property of its circuit and its handle, never of its
batch.  Run on the MI355X box with -m gpu."""

from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import batch_shapes
import circuit_families as cf
import helpers
import test_gpu_gradients
from batch_shapes import ARMS, WAYS, bits
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe import EVQEPopulation
from test_gpu_gradients import ShiftedValues

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10
FP32_REL = 2e-6
CHILD = Path(__file__).resolve().parent / "large_batch_child.py"


# ---- 1. the documented call ------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def documented():
    """The documented call's inputs, and *want*: the values of one ``evaluate_circuits`` call per circuit (ShiftedValues)."""
    op, circuits, points = batch_shapes.documented_call()
    their_circuits, params = test_gpu_gradients._mixed(batch_shapes.DOCUMENTED_N)
    assert len(their_circuits) == len(circuits) == 6
    for mine, theirs, p in zip(circuits, their_circuits, params):  # (the population of test_gpu_gradients._mixed(17) itself)
        assert mine.bound_ops(p) == theirs.bound_ops(p)
    reference = OperatorCircuitEvaluator(op)
    shifted = ShiftedValues(reference, circuits, params)
    flat_c, flat_p, owner = batch_shapes.flatten(circuits, points)
    assert shifted.n_shifted == len(flat_c) == batch_shapes.DOCUMENTED_EVALUATIONS == 2170
    for pts, values in zip(points, shifted.values):
        assert len(pts) == len(values)
    want = np.concatenate(shifted.values)
    routes = [c["route"] for c in reference.circuit_costs(circuits)]
    # the pushes of the default helper path (two for a batch of this size, unless the environment says otherwise)
    pushes = int(os.environ.get("QSV_PUSHES", "0") or 0) or 2
    bounds = batch_shapes.helper_bounds(len(flat_c), pushes)
    return {"op": op, "circuits": circuits, "flat_c": flat_c, "flat_p": flat_p, "owner": owner, "want": want, "routes": routes,
            "bounds": bounds}


def _hold(documented, calls):
    want = documented["want"]
    if all(np.array_equal(bits(got), bits(want)) for got in calls.values()):
        return
    pytest.fail("one host-list call differs from one call per circuit\n"
                + batch_shapes.failure_table(calls, want, documented["owner"], documented["routes"], documented["bounds"]))


def test_the_documented_call_regime(documented):
    """Each of the two pushes holds about 1085 evaluations; a lane has 128 side-table slots and 128 state slots."""
    dev = OperatorCircuitEvaluator(documented["op"]).statevector_device
    sizes = np.diff(documented["bounds"])
    print(f"\nroutes {documented['routes']}, pushes of {sizes.tolist()}, group {dev._group}")
    assert dev._group == 256 and len(sizes) == 2 and sizes.min() > 4 * dev._group // 2
    assert len(set(documented["routes"])) >= 2, "split and gate-pass circuits in one call"


def test_the_documented_call_on_a_fresh_handle(documented):
    evaluator = OperatorCircuitEvaluator(documented["op"])
    calls = {}
    for call in range(3):
        calls[f"{call} (fresh handle)"] = np.asarray(evaluator.evaluate_circuits(documented["flat_c"], documented["flat_p"]))
    _hold(documented, calls)


def test_the_documented_call_in_a_fresh_process(documented):
    """One child, no retries: the child runs only the three calls and prints their bits."""
    done = subprocess.run([sys.executable, str(CHILD)], capture_output=True, text=True, timeout=240)
    assert done.returncode == 0, f"child exited with {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}"
    lines = [line for line in done.stdout.splitlines() if line.startswith("call ")]
    assert len(lines) == 3, done.stdout[-2000:]
    calls = {}
    for call, line in enumerate(lines):
        head, _, words = line.partition(": ")
        assert head == f"call {call}"
        got = batch_shapes.from_hex_line(words)
        assert got.size == 2170
        calls[f"{call} (fresh process)"] = got.view(np.float64)
    _hold(documented, calls)


def test_the_documented_call_against_the_oracle(documented, c_oracle):
    """The first and the last evaluation of every circuit's block, twelve in all, from one host-list call."""
    op, flat_c, flat_p, owner = documented["op"], documented["flat_c"], documented["flat_p"], np.asarray(documented["owner"])
    got = np.asarray(OperatorCircuitEvaluator(op).evaluate_circuits(flat_c, flat_p))
    table, scratch = c_oracle.diagonal_table(op), np.zeros(2 << batch_shapes.DOCUMENTED_N)
    anchors = sorted({int(np.nonzero(owner == e)[0][k]) for e in range(6) for k in (0, -1)})
    assert len(anchors) == 12
    for i in anchors:
        ref = c_oracle.evaluate(flat_c[i], flat_p[i], op, table, scratch)
        print(f"evaluation {i} (circuit {owner[i]}, {documented['routes'][owner[i]]}): got {got[i]!r}, oracle {ref!r}")
        assert abs(got[i] - ref) < EXP_TOL, (i, got[i], ref)


# ---- 2. the regime around it, at the smallest shapes -------------------------------------------------------------------------
# A case is (arm, mix, order, size) of tests/batch_shapes.py.  Every feed and every consumer runs on the arm's ONE device over
# the same evaluations and must return the bits of calls of one structure each.  Before every feed the same structures are
# evaluated at OTHER points: whatever a feed finds left in a buffer by the call before it is then a wrong value, not by chance
# the right one (the documented call repeated found the previous call's partial sums, and passed from the third call on).

_OPENED: dict = {}      # arm -> {"dev", "ev", "op", "group", "side_slots", "table"}
_STRUCTURES: dict = {}  # (arm, mix) -> structures
_REFERENCES: dict = {}  # (arm, mix, size) -> (evaluations per structure, points, other points, values of one-structure calls)


@pytest.fixture(scope="module", autouse=True)
def _close_the_arms():
    yield
    _REFERENCES.clear()
    _STRUCTURES.clear()  # (kept states go before their device)
    for arm in _OPENED.values():
        arm["dev"].close()
    _OPENED.clear()


def _open(name, monkeypatch):
    """The arm's device, created once under the arm's QSV_SIDE_SLOTS; the environment stays as the arm wants it for the test."""
    spec = ARMS[name]
    if spec["side_slots"]:
        monkeypatch.setenv("QSV_SIDE_SLOTS", str(spec["side_slots"]))
    else:
        monkeypatch.delenv("QSV_SIDE_SLOTS", raising=False)
    if name not in _OPENED:
        dev = StatevectorDevice(spec["n"], dtype=spec["dtype"], group=spec["group"])
        op = helpers.random_ising_operator(spec["n"], seed=spec["n"])
        _OPENED[name] = {"dev": dev, "ev": OperatorCircuitEvaluator(op, statevector_device=dev), "op": op, "group": dev._group,
                         "side_slots": spec["side_slots"] or batch_shapes.DEFAULT_SIDE_SLOTS, "table": None}
        assert spec["group"] in (0, dev._group)
    return _OPENED[name]


def _structures(name, mix, monkeypatch):
    """The mix's structures on the arm, picked by the route the arm's device gives them: dicts of label, circuit, the whole
    circuit the oracle runs, route, halves, kind ("split", "ordinary" or "kept")."""
    if (name, mix) in _STRUCTURES:
        return _STRUCTURES[name, mix]
    arm = _open(name, monkeypatch)
    dev, ev, n = arm["dev"], arm["ev"], ARMS[name]["n"]
    pool = batch_shapes.candidates(n)
    costs = ev.circuit_costs([c for _, c in pool])

    def pick(route, count, want=None):
        found = [(label, c, c) for (label, c), cost in zip(pool, costs) if cost["route"] == route and (want is None or want(c))]
        assert len(found) >= count, (name, mix, route, sorted({cost["route"] for cost in costs}))
        return found[:count]

    def halved(c):
        return dev.circuit_form(c)["halves"]

    if mix == "one tile":
        chosen = pick("one tile", 3)
    elif mix == "split":  # (only split circuits with launches of their own)
        chosen = pick("split", 3)
    elif mix == "split+passes":
        all_pairs, ladder = cf.all_pairs(n)[0], cf.ladder(n)[0]
        nine = next((label, c, c) for (label, c), cost in zip(pool, costs) if label.startswith("L9") and cost["route"] == "gate passes")
        chosen = pick("split", 2) + [("all_pairs", all_pairs, all_pairs), ("ladder", ladder, ladder), nine]
    elif mix == "kept":
        chosen = pick("split", 2) + pick("gate passes", 1)
        population = EVQEPopulation.random_population(n, 3, 2, True, 7)
        for i, ind in enumerate(population.individuals):
            front, rest = ind.get_layer_search_circuits(2)
            state = dev.keep_states([front], [[]])[0]
            chosen.append((f"kept#{i}", rest.continue_from(state), ind.get_partially_parameterized_quantum_circuit({2})))
    else:  # "strata": the one-launch route with and without half sides, four- and five-key circuits, gate passes
        assert mix == "strata"
        chosen = (pick("split, one launch", 2, lambda c: not halved(c)) + pick("split, one launch", 1, halved) + pick("split", 2)
                  + pick("gate passes", 1))
    structures = []
    for (label, circuit, whole), cost in zip(chosen, ev.circuit_costs([c for _, c, _ in chosen])):
        kind = "kept" if cost["on_kept_state"] else "split" if cost["route"].startswith("split") else "ordinary"
        form = dev.circuit_form(circuit) if kind == "split" else {"halves": False, "one_launch": False}
        assert whole.num_parameters == circuit.num_parameters
        structures.append({"label": label, "circuit": circuit, "whole": whole, "route": cost["route"], "n_keys": cost["n_keys"],
                           "halves": form["halves"], "kind": kind})
    # split structures first, then ordinary ones, then those on kept states: in blocks, the batch's later pushes then hold no
    # split evaluation of their own (the documented call's second push)
    structures.sort(key=lambda st: ("split", "ordinary", "kept").index(st["kind"]))
    _STRUCTURES[name, mix] = structures
    return structures


def _reference(name, mix, size, monkeypatch):
    """Evaluations per structure (every kind's number relative to ways * slots of the kind), their points, other points of
    the same shape, and *want*: ONE ``evaluate_circuits`` call per structure.  Computed once per (arm, mix, size)."""
    key = (name, mix, size)
    if key not in _REFERENCES:
        arm = _open(name, monkeypatch)
        structures = _structures(name, mix, monkeypatch)
        units = batch_shapes.units(arm["group"], arm["side_slots"])
        per = [0] * len(structures)
        for kind in ("split", "ordinary", "kept"):
            members = [s for s, st in enumerate(structures) if st["kind"] == kind]
            for j, s in enumerate(members):
                count = batch_shapes.count_for(units[kind], size)
                per[s] = count // len(members) + (1 if j < count % len(members) else 0)
        points = [batch_shapes.points_for(st["label"], st["circuit"], m) for st, m in zip(structures, per)]
        others = [batch_shapes.points_for(st["label"], st["circuit"], m, salt=1) for st, m in zip(structures, per)]
        want = [np.asarray(arm["ev"].evaluate_circuits([st["circuit"]] * m, pts)) for st, m, pts in zip(structures, per, points)]
        _REFERENCES[key] = (per, points, others, want)
    return _REFERENCES[key]


def _dealt(structures, per, order, *per_structure):
    """The case's evaluations in its order: circuits, the structure of each, then every per-structure list dealt alike."""
    pairs = batch_shapes.deal(per, order)
    return ([structures[s]["circuit"] for s, _ in pairs], [s for s, _ in pairs],
            *[[values[s][k] for s, k in pairs] for values in per_structure])


def _in_the_regime(arm, kinds, size):
    """The coverage guard: from the device's group, the QSV_SIDE_SLOTS the arm set and the push bounds the test chose."""
    n = len(kinds)
    slots = {"split": arm["side_slots"] // WAYS, "ordinary": arm["group"] // WAYS, "kept": arm["group"] // WAYS}
    present = [k for k in slots if k in kinds]
    assert present
    uneven = batch_shapes.plan_bounds(n, batch_shapes.uneven_plan(n, arm["side_slots"] // WAYS))
    for kind in present:
        assert kinds.count(kind) > slots[kind], f"one push of everything: {kinds.count(kind)} {kind} evaluations, {slots[kind]} slots"
    if size == "4.3 times":
        assert len(uneven) - 1 >= 3, uneven
        for bounds in (uneven, batch_shapes.helper_bounds(n, 2)):  # (the helper path makes two pushes of a batch of more than 128)
            for kind in present:
                assert max(push[kind] for push in batch_shapes.kinds_per_push(bounds, kinds)) > slots[kind], (bounds, kind)
    return uneven


@pytest.mark.parametrize("case", batch_shapes.CASES, ids=batch_shapes.case_id)
def test_every_feed_returns_the_bits_of_one_structure_calls(case, c_oracle, monkeypatch):
    import torch

    name, mix, order, size = case
    arm = _open(name, monkeypatch)
    dev, ev, op = arm["dev"], arm["ev"], arm["op"]
    structures = _structures(name, mix, monkeypatch)
    per, points, others, want = _reference(name, mix, size, monkeypatch)
    flat_c, owner, flat_p, flat_o, flat_w = _dealt(structures, per, order, points, others, want)
    kinds = [structures[s]["kind"] for s in owner]
    n = len(flat_c)
    uneven = _in_the_regime(arm, kinds, size)
    want_flat = np.asarray(flat_w)
    routes = [st["route"] for st in structures]
    print(f"\n{batch_shapes.case_id(case)}: {n} evaluations, {dict(zip((st['label'] for st in structures), per))}, "
          f"group {arm['group']}, side slots {arm['side_slots']}, uneven pushes {np.diff(uneven).tolist()}")

    def matrix_of(vectors):
        host = np.zeros((n, max(1, max(len(v) for v in vectors)) + 1))  # (an odd row length among them)
        for i, v in enumerate(vectors):
            host[i, : len(v)] = v
        tensor = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        return tensor

    def through_plan(plan):
        monkeypatch.setenv("QSV_PUSH_PLAN", ",".join(str(s) for s in plan))
        monkeypatch.setattr(dev, "_push_plan", list(plan))  # (what a device created under QSV_PUSH_PLAN holds: the ctypes path)
        try:
            return ev.evaluate_circuits(flat_c, flat_p)
        finally:
            monkeypatch.setattr(dev, "_push_plan", [])
            monkeypatch.delenv("QSV_PUSH_PLAN")

    def with_option(option, value, default):
        dev.set_option(option, value)
        try:
            return ev.evaluate_circuits(flat_c, flat_p)
        finally:
            dev.set_option(option, default)

    def to_device():
        out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert ev.evaluate_circuits_to_device(flat_c, flat_p, out.data_ptr())
        torch.cuda.synchronize()
        dev.results_seen()
        return out.cpu().numpy()

    feeds = {
        "host lists": (lambda: ev.evaluate_circuits(flat_c, flat_p), batch_shapes.helper_bounds(n, 2)),
        "uneven plan": (lambda: through_plan(batch_shapes.uneven_plan(n, arm["side_slots"] // WAYS)), uneven),
        "one push": (lambda: through_plan([n]), [0, n]),
        "device matrix": (lambda: ev.evaluate_device_parameters(flat_c, matrix_of(flat_p)), batch_shapes.helper_bounds(n, 2)),
        "to device": (to_device, batch_shapes.helper_bounds(n, 2)),
        "streams=1": (lambda: with_option("streams", 1, 2), batch_shapes.helper_bounds(n, 2)),
        "chain_stream=0": (lambda: with_option("chain_stream", 0, 1), batch_shapes.helper_bounds(n, 2)),
    }
    failed, first = [], None
    for feed, (run, bounds) in feeds.items():
        ev.evaluate_circuits(flat_c, flat_o)  # (the same structures at other points: nothing left behind is right by chance)
        got = np.asarray(run(), dtype=np.float64)
        first = got if first is None else first
        if not np.array_equal(bits(got), bits(want_flat)):
            failed.append(batch_shapes.failure_table({feed: got}, want_flat, owner, routes, bounds, limit=12))
    if failed:
        pytest.fail(f"{batch_shapes.case_id(case)}: a batch's value differs from the one-structure call's\n" + "\n".join(failed))
    # one evaluation per route against the C oracle (fp32: FP32_REL * sum |c_k|, also against fp64 on the n = 14 arm)
    spread = float(np.abs(op.coeffs).sum())
    tol = EXP_TOL if ARMS[name]["dtype"] == "fp64" else FP32_REL * spread
    if arm["table"] is None:
        arm["table"] = (c_oracle.diagonal_table(op), np.zeros(2 << ARMS[name]["n"]))
    seen = set()
    for i, s in enumerate(owner):
        st = structures[s]
        stratum = (st["route"], st["kind"], st["halves"])
        if stratum in seen:
            continue
        seen.add(stratum)
        ref = c_oracle.evaluate(st["whole"], flat_p[i], op, *arm["table"])
        assert abs(first[i] - ref) < tol, (st["label"], stratum, first[i], ref)
    assert len(seen) <= (8 if ARMS[name]["n"] == 20 else 24)
    if ARMS[name]["dtype"] == "fp32":
        fp64 = _open("n14", monkeypatch)["ev"]
        want64 = [np.asarray(fp64.evaluate_circuits([st["circuit"]] * m, pts)) for st, m, pts in zip(structures, per, points)]
        flat64 = np.asarray(_dealt(structures, per, order, want64)[2])
        assert np.abs(first - flat64).max() <= FP32_REL * spread


@pytest.mark.parametrize("case", batch_shapes.CLIENT_CASES, ids=batch_shapes.case_id)
def test_the_other_clients_of_the_batch_driver(case, monkeypatch):
    """exact_cvar_batch, sample_cvar_batch, variances and observable_values over the case's evaluations, each against calls of
    its own of one structure each.  A sampled evaluation's draws depend on its index in its batch: its one-structure call
    holds the structure at every index, the structure's points where the batch has them.  (The library evaluates circuits on
    kept states through qsv_eval_* alone -- expectation values and observables -- and refuses them to the sampler, the exact
    CVaR and the variance: the mix with kept states runs observable_values.)"""
    name, mix, order, size = case
    arm = _open(name, monkeypatch)
    dev, op = arm["dev"], arm["op"]
    structures = _structures(name, mix, monkeypatch)
    per, points, others, _ = _reference(name, mix, size, monkeypatch)
    flat_c, owner, flat_p, flat_o = _dealt(structures, per, order, points, others)
    _in_the_regime(arm, [structures[s]["kind"] for s in owner], size)
    owner = np.asarray(owner)
    n = len(flat_c)
    observables = [op, helpers.random_pauli_operator(ARMS[name]["n"], 12, seed=3)]
    clients = {"observable_values": lambda c, p: dev.observable_values(c, p, observables)}
    whole_only = not any(st["kind"] == "kept" for st in structures)
    if whole_only:
        clients["exact_cvar_batch"] = lambda c, p: np.asarray(dev.exact_cvar_batch(c, p, 0.5))
        clients["variances"] = lambda c, p: np.stack(dev.variances(c, p), axis=1)
    dev.set_operator(op)
    for client, call in clients.items():
        call(flat_c, flat_o)  # (other points first, as above)
        got = call(flat_c, flat_p)
        for s, st in enumerate(structures):
            alone = call([st["circuit"]] * per[s], points[s])
            mine = np.nonzero(owner == s)[0]
            same = (bits(got[mine]) == bits(alone)).reshape(len(mine), -1).all(axis=1)
            assert same.all(), f"{client}: {st['label']} ({st['route']}): {(~same).sum()} of {len(mine)} differ, first at {mine[~same][:8].tolist()}"
    if not whole_only:
        return
    dev.sample_cvar_batch(flat_c, flat_o, 256, 5, 0.5)
    got = np.asarray(dev.sample_cvar_batch(flat_c, flat_p, 256, 5, 0.5))
    for s, st in enumerate(structures):
        mine = np.nonzero(owner == s)[0]
        filled = [points[s][0]] * n
        for i in mine:
            filled[i] = flat_p[i]
        alone = np.asarray(dev.sample_cvar_batch([st["circuit"]] * n, filled, 256, 5, 0.5))
        assert np.array_equal(bits(got[mine]), bits(alone[mine])), f"sample_cvar_batch: {st['label']} ({st['route']})"


def test_the_compositions_reach_every_route_and_kind(monkeypatch):
    """Read from the devices, without evaluating: every route name, both kinds of split evaluation -- finished by the launch
    that runs their virtual circuits (the one-launch route, half sides among them) and with launches of their own --,
    ordinary evaluations and evaluations on kept states; and no case of the list is left out of the parametrisation."""
    reached = {}
    for name, spec in ARMS.items():
        for mix in spec["mixes"]:
            for st in _structures(name, mix, monkeypatch):
                reached.setdefault((st["route"], st["kind"], st["halves"]), f"{name} / {mix} / {st['label']}")
    for key, where in sorted(reached.items(), key=str):
        print(key, where)
    assert {route for route, _, _ in reached} == set(_lib.ROUTE_NAMES)
    assert ("split, one launch", "split", True) in reached and ("split, one launch", "split", False) in reached
    assert ("split", "split", False) in reached
    assert {kind for _, kind, _ in reached} == {"split", "ordinary", "kept"}
    assert len(batch_shapes.CASES) == sum(len(spec["mixes"]) for spec in ARMS.values()) * 8
    assert {(a, m) for a, m, _, _ in batch_shapes.CASES} == {(a, m) for a, spec in ARMS.items() for m in spec["mixes"]}
