"""A repeated batch queues the launches its kept layout's one push recorded (option "replay_launches", csrc/qsv_api.hip
replay_push) instead of deriving them again.  The launches are the same, so every value must be the SAME BITS as a second
handle with the option off returns -- on every kind of push, for host lists and for a device matrix, and whatever happens
between two calls -- and ``replayed_pushes`` must count exactly the pushes that were replayed."""

from __future__ import annotations

import threading

import numpy as np
import pytest

import circuit_families as cf
import helpers
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, OperatorSamplerCircuitEvaluator
from queasars_amd.ir import PauliOperator

pytestmark = pytest.mark.gpu

CALLS = 6


def _parameter_sets(params, seed, count=CALLS):
    rng = np.random.default_rng(seed)
    return [params] + [[[float(v + rng.normal(0.0, 0.3)) for v in p] for p in params] for _ in range(count - 1)]


def _matrix(params):
    import torch

    width = max(1, max(len(p) for p in params))
    host = np.zeros((len(params), width))
    for i, p in enumerate(params):
        host[i, : len(p)] = p
    matrix = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return matrix


def _split_case(n, count):
    """Split evaluations under a seeded Ising operator, one of them with two cut keys: at 14 qubits with launches of their own (the
    virtual circuits, then the Gram matrices and their combination), at 20 the one-launch route."""
    _, circuits, params = helpers.population_circuits(n, 3, count - 1, seed=n)
    c, p = cf.two_blocks(n, 2)
    return n, helpers.random_ising_operator(n, seed=2020), circuits + [c], params + [list(p)]


def _cases():
    yield ("split", *_split_case(14, 6), {}, 1)
    yield ("one launch", *_split_case(20, 4), {}, 1)
    n = 10
    _, circuits, params = helpers.population_circuits(n, 3, 5, seed=10)
    yield "one tile", n, helpers.random_ising_operator(n, seed=2020), circuits, params, {}, 1
    n = 14
    _, circuits, params = helpers.population_circuits(n, 3, 6, seed=14)
    yield "gate passes", n, helpers.random_ising_operator(n, seed=2020), circuits, params, {"split": 0}, 1
    # split evaluations on the push's lane, ordinary ones (no split form) beside them on the auxiliary stream
    _, circuits, params = helpers.population_circuits(n, 3, 3, seed=15)
    extra = [cf.two_blocks(n, 2), cf.all_pairs(n, 1), cf.ladder(n, 2)]
    yield ("mixed", n, helpers.random_ising_operator(n, seed=2020), circuits + [c for c, _ in extra],
           params + [list(p) for _, p in extra], {}, 1)
    # one-launch evaluations and a four-key circuit, whose launches of its own go to a second stream behind events: never replayed
    n = 20
    _, circuits, params = helpers.population_circuits(n, 3, 2, seed=21)
    extra = [cf.two_blocks(n, 2), cf.two_blocks(n, 4), cf.ladder(n, 2)]
    yield ("mixed with a chain", n, helpers.random_ising_operator(n, seed=2020), circuits + [c for c, _ in extra],
           params + [list(p) for _, p in extra], {}, 0)
    n = 12
    labels = ["ZZ" + "I" * (n - 2), "II" + "XX" + "I" * (n - 4), "I" * 6 + "Y" + "I" * (n - 8) + "Z"]
    _, circuits, params = helpers.population_circuits(n, 3, 5, seed=12)
    yield "general operator", n, PauliOperator(labels, [0.7, -0.4, 0.9]), circuits, params, {}, 1


CASES = {case[0]: case[1:] for case in _cases()}


def _pair(op, options):
    """(evaluator, reference evaluator with replay_launches off), both with ``options`` set."""
    made = []
    for replay in (1, 0):
        ev = OperatorCircuitEvaluator(op)
        for name, value in options.items():
            ev.statevector_device.set_option(name, value)
        ev.statevector_device.set_option("replay_launches", replay)
        made.append(ev)
    return made


@pytest.mark.parametrize("feed", ["lists", "matrix"])
@pytest.mark.parametrize("name", list(CASES))
def test_six_calls_replay_five_pushes_and_keep_every_bit(name, feed, c_oracle):
    n, op, circuits, params, options, replayable = CASES[name]
    ev, ref = _pair(op, options)
    try:
        dev = ev.statevector_device
        ev.circuit_costs(circuits)  # (registers them)
        forms = [dev.circuit_form(c) for c in circuits]
        routes = sorted({f["route"] for f in forms})
        if name == "split":
            assert routes == [_lib_route("SPLIT")] and max(f["n_keys"] for f in forms) >= 1, forms
        elif name == "one launch":
            assert routes == [_lib_route("SPLIT_ONE_LAUNCH")] and max(f["n_keys"] for f in forms) >= 1, forms
        elif name == "one tile":
            assert routes == [_lib_route("ONE_TILE")], forms
        elif name == "gate passes":
            assert routes == [_lib_route("PASSES")], forms
        elif name == "mixed":
            assert routes == [_lib_route("SPLIT"), _lib_route("PASSES")], forms
        elif name == "mixed with a chain":
            assert routes == [_lib_route("SPLIT_ONE_LAUNCH"), _lib_route("SPLIT")], forms
        sets = _parameter_sets(params, seed=n)
        for i, values in enumerate(sets):
            fed = _matrix(values) if feed == "matrix" else values
            got = np.asarray(ev.evaluate_circuits(circuits, fed))
            want = np.asarray(ref.evaluate_circuits(circuits, fed))
            assert np.array_equal(got, want), (name, feed, i, np.abs(got - want).max())
            if i:
                assert np.abs(got - first).max() > 1e-6  # (the new values were read)
            else:
                first = got
                table = None if op.x_mask.any() else c_oracle.diagonal_table(op)
                assert abs(got[-1] - c_oracle.evaluate(circuits[-1], values[-1], op, table)) < 1e-10
        print(f"\n{name}, {feed}: routes {routes}, replayed pushes {dev.replayed_pushes()} of {CALLS - 1}")
        assert dev.replayed_pushes() == (CALLS - 1) * replayable
        assert ref.statevector_device.replayed_pushes() == 0
    finally:
        ev.statevector_device.close()
        ref.statevector_device.close()


def _lib_route(name):
    return {"ONE_TILE": 0, "SPLIT_ONE_LAUNCH": 1, "SPLIT": 2, "PASSES": 3}[name]


def test_profiled_calls_are_not_replayed():
    n, op, circuits, params, options, _ = CASES["split"]
    ev, ref = _pair(op, options)
    try:
        dev = ev.statevector_device
        dev.set_profiling(True)
        for values in _parameter_sets(params, seed=3, count=3):
            assert np.array_equal(np.asarray(ev.evaluate_circuits(circuits, values)), np.asarray(ref.evaluate_circuits(circuits, values)))
        assert dev.profile()["kernel_launches"][0] >= 1
        assert dev.replayed_pushes() == 0
    finally:
        ev.statevector_device.close()
        ref.statevector_device.close()


# ---- what may come between two calls ---------------------------------------------------------------------------------------


def _register_another(ev, ctx):
    c, p = cf.ladder(ctx["n"], 1, seed=5)
    ev.circuit_costs([c])
    return True


def _set_an_option_and_set_it_back(ev, ctx):
    ev.statevector_device.set_option("fused_lds_table", 0)
    ev.statevector_device.set_option("fused_lds_table", 1)
    return True


def _another_operator_and_back(ev, ctx):
    other = OperatorCircuitEvaluator(helpers.random_ising_operator(ctx["n"], seed=7), statevector_device=ev.statevector_device)
    got = np.asarray(other.evaluate_circuits(ctx["circuits"], ctx["sets"][0]))
    assert np.abs(got - ctx["first"]).max() > 1e-6
    return True


def _a_different_batch(ev, ctx):
    got = np.asarray(ev.evaluate_circuits(ctx["circuits"][1:4], ctx["sets"][0][1:4]))
    assert np.array_equal(got, ctx["first"][1:4])
    return True


def _two_pieces(ev, ctx):
    dev = ev.statevector_device
    dev._push_evals = 3
    try:
        assert np.array_equal(np.asarray(ev.evaluate_circuits(ctx["circuits"], ctx["sets"][0])), ctx["first"])
    finally:
        dev._push_evals = 0
    return True


def _one_profiled_call(ev, ctx):
    dev = ev.statevector_device
    dev.set_profiling(True)
    try:
        assert np.array_equal(np.asarray(ev.evaluate_circuits(ctx["circuits"], ctx["sets"][0])), ctx["first"])
    finally:
        dev.set_profiling(False)
    return True


def _results_to_a_device_buffer(ev, ctx):
    import torch

    out = torch.zeros(len(ctx["circuits"]), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert ev.evaluate_circuits_to_device(ctx["circuits"], ctx["sets"][1], out.data_ptr())
    torch.cuda.synchronize()
    ev.statevector_device.results_seen()
    assert np.array_equal(out.cpu().numpy(), ctx["second"])
    return False  # (nothing the layout depends on has changed: the epoch stands)


def _a_masked_cvar_call(ev, ctx):
    import torch

    sampler = OperatorSamplerCircuitEvaluator(None, ctx["op"], alpha=0.5, statevector_device=ev.statevector_device)
    count = len(ctx["circuits"])
    out = torch.full((count,), -77.0, dtype=torch.float64, device="cuda")
    active = torch.tensor([i % 2 for i in range(count)], dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sampler.evaluate_device_to_device(ctx["circuits"], _matrix(ctx["sets"][0]), out, active=active)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[0::2] == -77.0).all() and (got[1::2] != -77.0).all()
    return True


BETWEEN = {"register another circuit": _register_another, "set an option and set it back": _set_an_option_and_set_it_back,
           "another operator and back": _another_operator_and_back, "a different batch": _a_different_batch,
           "the same batch in two pieces": _two_pieces, "one profiled call": _one_profiled_call,
           "results to a device buffer": _results_to_a_device_buffer, "a masked qsv_cvar_device call": _a_masked_cvar_call}

_REFERENCE: dict = {}  # the 14-qubit split case's values with replay_launches off: computed once, shared, never written to


def _reference():
    if not _REFERENCE:
        n, op, circuits, params, options, _ = CASES["split"]
        sets = _parameter_sets(params, seed=99, count=4)
        ref = OperatorCircuitEvaluator(op)
        try:
            ref.statevector_device.set_option("replay_launches", 0)
            values = [np.asarray(ref.evaluate_circuits(circuits, s)) for s in sets]
        finally:
            ref.statevector_device.close()
        for v in values:
            v.setflags(write=False)
        _REFERENCE.update(n=n, op=op, circuits=circuits, sets=sets, values=values, first=values[0], second=values[1])
    return _REFERENCE


@pytest.mark.parametrize("between", list(BETWEEN))
def test_what_comes_between_two_calls_drops_the_record_or_leaves_it_valid(between):
    ctx = _reference()
    ev = OperatorCircuitEvaluator(ctx["op"])
    try:
        dev = ev.statevector_device
        for i in (0, 1, 2):  # laid out, then repeated twice
            assert np.array_equal(np.asarray(ev.evaluate_circuits(ctx["circuits"], ctx["sets"][i])), ctx["values"][i])
        assert dev.replayed_pushes() == 2
        epoch_moved = BETWEEN[between](ev, ctx)
        after = dev.replayed_pushes()
        # (a call with a device output may itself be a replay, where the batch cycles over as many streams either way)
        assert after == 2 if epoch_moved else after in (2, 3)
        assert np.array_equal(np.asarray(ev.evaluate_circuits(ctx["circuits"], ctx["sets"][3])), ctx["values"][3])
        assert dev.replayed_pushes() == after + (0 if epoch_moved else 1)  # (laid out afresh where the epoch moved)
        assert np.array_equal(np.asarray(ev.evaluate_circuits(ctx["circuits"], ctx["sets"][1])), ctx["values"][1])
        assert dev.replayed_pushes() == after + (1 if epoch_moved else 2)
    finally:
        ev.statevector_device.close()


def test_the_switch_and_its_dependence_on_repeat_layout():
    ctx = _reference()
    ev = OperatorCircuitEvaluator(ctx["op"])
    try:
        dev = ev.statevector_device
        dev.set_option("repeat_layout", 0)  # (no kept layout: nothing to replay)
        for i in (0, 1, 2):
            assert np.array_equal(np.asarray(ev.evaluate_circuits(ctx["circuits"], ctx["sets"][i])), ctx["values"][i])
        assert dev.replayed_pushes() == 0
        dev.set_option("repeat_layout", 1)
        dev.set_option("replay_launches", 0)
        for i in (0, 1, 2):
            assert np.array_equal(np.asarray(ev.evaluate_circuits(ctx["circuits"], ctx["sets"][i])), ctx["values"][i])
        assert dev.replayed_pushes() == 0
        dev.set_option("replay_launches", 1)
        for i in (0, 1, 2):
            assert np.array_equal(np.asarray(ev.evaluate_circuits(ctx["circuits"], ctx["sets"][i])), ctx["values"][i])
        assert dev.replayed_pushes() == 2
        with pytest.raises(Exception):
            dev.set_option("replay_launch", 1)
    finally:
        dev.close()


def test_two_threads_alternating_two_batches_never_replay_each_other():
    ctx = _reference()
    circuits, sets, values = ctx["circuits"], ctx["sets"], ctx["values"]
    batches = [(circuits, lambda i: sets[i], lambda i: values[i]),
               (circuits[:4], lambda i: sets[i][:4], lambda i: values[i][:4])]
    ev = OperatorCircuitEvaluator(ctx["op"])
    turns = [threading.Semaphore(1), threading.Semaphore(0)]
    failures: list = []

    def work(me):
        cs, values_of, want_of = batches[me]
        for k in range(4):
            if not turns[me].acquire(timeout=60):
                failures.append((me, k, "turn"))
                return
            try:
                got = np.asarray(ev.evaluate_circuits(cs, values_of(k % len(sets))))
                if not np.array_equal(got, want_of(k % len(sets))):
                    failures.append((me, k, got))
            except Exception as exc:  # noqa: BLE001
                failures.append((me, k, exc))
            finally:
                turns[1 - me].release()

    try:
        threads = [threading.Thread(target=work, args=(me,)) for me in (0, 1)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not failures, failures
        assert ev.statevector_device.replayed_pushes() == 0
        # ... and one of them alone, afterwards: laid out, then replayed
        for i in (0, 1):
            assert np.array_equal(np.asarray(ev.evaluate_circuits(circuits, sets[i])), values[i])
        assert ev.statevector_device.replayed_pushes() == 1
    finally:
        ev.statevector_device.close()
