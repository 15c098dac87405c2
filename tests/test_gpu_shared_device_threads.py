"""One StatevectorDevice shared by evaluators of different operators, called from several threads on every consumer
(tests/shared_device_cases.py; the CPU half is tests/test_shared_device_host.py).

The reference calls its evaluators from population_size threads at once, one circuit per call.  Here the evaluators also share
the device, so a call is "install my operator if another one is there, then evaluate", under locks that differ from method to
method.  The reference of every comparison is the same call made alone on the same device before any thread starts: the project
promises the same bits in any batch and whatever came between, so under threads every result must have the serial run's bits --
nothing is compared by tolerance.  Every thread is a daemon and is joined with a time limit: a deadlock fails the test and names
the task each hanging thread was in."""

from __future__ import annotations

import gc
import threading
import time

import numpy as np
import pytest

import circuit_families as cf
import helpers
import shared_device_cases as sc
from queasars_amd.circuit_evaluation import (
    BitstringCircuitEvaluator,
    BitstringEvaluator,
    OperatorCircuitEvaluator,
    OperatorSamplerCircuitEvaluator,
    StatevectorDevice,
)
from queasars_amd.ir import CircuitIR

pytestmark = pytest.mark.gpu

THREADS = 8
ROUNDS = 3
ARMS = [(6, "fp64"), (14, "fp64"), (6, "fp32")]

_CASTS: dict = {}  # (n, dtype) -> (cast, its tasks, their serial results): made once, shared, the results never written to


def _cast(n, dtype="fp64"):
    if (n, dtype) not in _CASTS:
        cast = sc.Cast(n, dtype)
        tasks = cast.tasks()
        _CASTS[n, dtype] = (cast, tasks, sc.serial_reference(tasks))
    return _CASTS[n, dtype]


@pytest.fixture(scope="module", autouse=True)
def _close_the_casts():
    yield
    while _CASTS:
        _CASTS.popitem()[1][0].close()


# ---- 1. every consumer, many threads, its own bits --------------------------------------------------------------------------


@pytest.mark.parametrize("n,dtype", ARMS, ids=[f"{n}-{dtype}" for n, dtype in ARMS])
def test_every_consumer_from_eight_threads_returns_its_serial_bits(n, dtype):
    """Eight threads walk the task list for ROUNDS rounds.  In the first round the threads go in pairs -- one seeded order a
    pair, the two meeting before every task -- so every task is entered by two threads at once (four times over); after that
    every thread has a seeded order of its own.  In every order a task does not follow one that installs the same operator."""
    cast, tasks, expected = _cast(n, dtype)
    start = threading.Barrier(THREADS)
    meet = [threading.Barrier(2) for _ in range(THREADS // 2)]
    done = [0] * THREADS

    def body(worker, k):
        worker.doing = "the start"
        start.wait(sc.JOIN_S)
        for r in range(ROUNDS):
            for task in sc.order_of(tasks, seed=1000 * n + (k // 2 if r == 0 else 10 * r + k)):
                if r == 0:
                    worker.doing = f"meeting its partner before: {task.name}"
                    meet[k // 2].wait(sc.JOIN_S)
                got = worker.attempt(task.name, task.call)
                if got is not None and not sc.same(got, expected[task.name]):
                    worker.fail(f"round {r}: not the bits of the serial run")
                done[k] += 1

    sc.run_workers({f"thread {k}": (lambda worker, k=k: body(worker, k)) for k in range(THREADS)})
    assert done == [ROUNDS * len(tasks)] * THREADS
    # ... and the device is as good as before: every task alone once more
    for task in tasks:
        assert sc.same(task.call(), expected[task.name]), task.name


# ---- 2. fresh objects every call --------------------------------------------------------------------------------------------


def test_fresh_circuit_objects_every_call_beside_long_lived_lists_and_a_collector():
    """The reference's habit: new circuit objects of the same few structures at every call, dropped at once -- registered,
    watched, queued for destruction by their finalizers and reaped by whoever registers next -- while other threads evaluate
    lists that live on and one thread runs the garbage collector."""
    n, iterations = 6, 20
    started = time.perf_counter()
    dev = StatevectorDevice(n)
    try:
        ops = [helpers.random_ising_operator(n, seed=sc.SEED), helpers.random_pauli_operator(n, 12, seed=sc.SEED + 1),
               helpers.random_ising_operator(n, seed=sc.SEED + 2)]
        evaluators = [OperatorCircuitEvaluator(ops[0], statevector_device=dev),
                      OperatorCircuitEvaluator(ops[1], statevector_device=dev, gradient_method="adjoint"),
                      OperatorSamplerCircuitEvaluator(None, ops[2], alpha=0.5, statevector_device=dev)]
        builders = [lambda: cf.ladder(n, 2), lambda: cf.two_blocks(n, 2), lambda: cf.all_pairs(n, 1), lambda: cf.ladder(n, 1, seed=3)]

        def fresh(k, j):
            """Structure (k + j) % 4 as new objects, evaluated by evaluator j % 3, and gone when this returns."""
            circuit, params = builders[(k + j) % 4]()
            return evaluators[j % 3].evaluate_circuits([circuit], [list(params)])

        def kept_round_trip(k, j):
            front, front_params = builders[k % 4]()
            (state,) = evaluators[0].keep_states([front], [list(front_params)])
            try:
                rest, rest_params = builders[(k + j + 1) % 4]()
                return evaluators[j % 2].evaluate_circuits([rest.continue_from(state)], [list(rest_params)])
            finally:
                state.release()

        circuits, params = sc.population(n)
        long_lived = [lambda: evaluators[0].evaluate_circuits(circuits, params),
                      lambda: evaluators[1].evaluate_variances(circuits, params, with_values=True),
                      lambda: evaluators[2].evaluate_circuits(circuits, params)]
        want_long = [call() for call in long_lived]
        want_fresh = {(k, j): fresh(k, j) for k in range(4) for j in range(12)}  # (12: every structure with every evaluator)
        want_kept = {(k, j): kept_round_trip(k, j) for k in range(4) for j in range(12)}
        for ev in evaluators[:2]:
            ev.forget_circuits()
        for call in long_lived:
            call()
        gc.collect()
        assert dev.kept_state_count() == 0
        watched = len(dev._watched)
        assert watched == len(circuits)  # (the long-lived list and nothing else)

        # (the collector collects once per tick -- every fifth iteration of every other thread -- and ends with them: no clock)
        busy, busy_lock, idle, tick = [7], threading.Lock(), threading.Event(), threading.Semaphore(0)
        collections = [0]

        def counted(body):
            def run(worker):
                try:
                    body(worker)
                finally:
                    with busy_lock:
                        busy[0] -= 1
                        if busy[0] == 0:
                            idle.set()
                    tick.release()
            return run

        def fresh_body(k):
            def body(worker):
                for j in range(iterations):
                    if j % 5 == 0:
                        tick.release()
                    got = worker.attempt(f"fresh objects, structure {(k + j) % 4}, evaluator {j % 3}", lambda: fresh(k, j))
                    if got is not None and not sc.same(got, want_fresh[k, j % 12]):
                        worker.fail("not the bits of the serial run")
                    if j % 3 == 0:
                        got = worker.attempt(f"kept round trip, front {k % 4}", lambda: kept_round_trip(k, j))
                        if got is not None and not sc.same(got, want_kept[k, j % 12]):
                            worker.fail("not the bits of the serial run")
            return body

        def long_body(i):
            def body(worker):
                for j in range(iterations):
                    if j % 5 == 0:
                        tick.release()
                    got = worker.attempt(f"long-lived list {i}", long_lived[i])
                    if got is not None and not sc.same(got, want_long[i]):
                        worker.fail("not the bits of the serial run")
            return body

        def collector(worker):
            worker.doing = "gc.collect()"
            while not idle.is_set():
                if not tick.acquire(timeout=sc.JOIN_S):
                    raise AssertionError("no thread came by")
                # (a whole collection walks everything the test session has made so far: four of those, then the young generations)
                gc.collect() if collections[0] < 4 else gc.collect(1)
                collections[0] += 1

        bodies = {f"fresh {k}": counted(fresh_body(k)) for k in range(4)}
        bodies.update({f"long-lived {i}": counted(long_body(i)) for i in range(3)})
        bodies["collector"] = collector
        serial_s, started = time.perf_counter() - started, time.perf_counter()
        try:
            sc.run_workers(bodies)
        finally:
            idle.set()
            tick.release()
        print(f"\nfresh objects: serial references {serial_s:.2f} s, eight threads {time.perf_counter() - started:.2f} s, "
              f"{collections[0]} collections beside them")
        for ev in evaluators[:2]:
            ev.forget_circuits()
        gc.collect()
        assert dev.kept_state_count() == 0
        assert len(dev._watched) == watched  # (the long-lived list again, and nothing else)
        assert [sc.same(call(), want) for call, want in zip(long_lived, want_long)] == [True] * 3
    finally:
        dev.close()


# ---- 3. observable sets beyond the cache ------------------------------------------------------------------------------------

SET_SIZES = (1, 2, 16, 17, 64)
N_SETS = 24


def _observable_lists(n):
    """N_SETS distinct lists of observables, of SET_SIZES members in turn, each member three random strings."""
    return [[helpers.random_pauli_operator(n, 3, seed=1000 * k + m) for m in range(SET_SIZES[k % len(SET_SIZES)])] for k in range(N_SETS)]


def test_more_observable_sets_in_flight_than_the_device_caches():
    """24 distinct observable lists over eight threads, through evaluate_observables and evaluate_covariances of two evaluators
    of the shared device: a miss evicts the least recently used of 16 sets, which must never be one whose caller is on its way
    to the library.  List 0 is asked for by every thread at the start of every round: several misses of one key."""
    n = 6
    cast, _tasks, _expected = _cast(n)
    dev, circuits, params = cast.dev, cast.circuits, cast.params
    assert N_SETS > StatevectorDevice.MAX_OBSERVABLE_SETS == 16
    lists = _observable_lists(n)
    calls = {("values", k): (lambda k=k: cast.first.evaluate_observables(circuits, params, lists[k])) for k in range(N_SETS)}
    calls.update({("covariances", k): (lambda k=k: cast.general.evaluate_covariances(circuits, params, lists[k], with_values=True))
                  for k in range(N_SETS)})
    want = {key: call() for key, call in calls.items()}
    start = threading.Barrier(THREADS)

    def body(worker, t):
        worker.doing = "the start"
        start.wait(sc.JOIN_S)
        for r in range(ROUNDS):
            mine = [0] + list(range(t, N_SETS, THREADS))
            for k in mine if r % 2 == 0 else mine[::-1]:
                for kind in (("values", "covariances") if (t + r) % 2 == 0 else ("covariances", "values")):
                    got = worker.attempt(f"{kind} of list {k} ({len(lists[k])} observables)", calls[kind, k])
                    if got is not None and not sc.same(got, want[kind, k]):
                        worker.fail("not the bits of the serial run")

    sc.run_workers({f"thread {t}": (lambda worker, t=t: body(worker, t)) for t in range(THREADS)})
    assert len(dev._observable_sets) <= StatevectorDevice.MAX_OBSERVABLE_SETS
    for key in (("values", 0), ("covariances", N_SETS - 1), ("values", 7)):
        assert sc.same(calls[key](), want[key]), key
    assert len(dev._observable_sets) <= StatevectorDevice.MAX_OBSERVABLE_SETS


# ---- 4. a shared value cache ------------------------------------------------------------------------------------------------


def _basis_state_circuit(n, state):
    """|state> from |0..0>: u(pi, 0, pi) = X on every set bit, so every shot is that state whatever the seed."""
    circuit = CircuitIR(n)
    for q in range(n):
        if (state >> q) & 1:
            circuit.u(np.pi, 0.0, np.pi, q)
        else:
            circuit.id(q)
    return circuit


def test_a_value_cache_shared_by_eight_threads_one_circuit_a_call():
    """One BitstringCircuitEvaluator(device_value_cache=True) called from eight threads, one circuit a call -- the reference's
    pattern.  A lookup, its scoring and its finish are one step: every caller gets its own state's score, exactly (shots of one
    state, a dyadic score), and the scoring function is called once per distinct state over the whole test.  A value that went
    to another lookup's state would stay in the table: the serial pass afterwards reads every state again."""
    n, shots = 6, 64
    dev = StatevectorDevice(n)
    try:
        def score_of(state):
            return bin(state).count("1") + state / 64.0

        scored, scored_lock = [], threading.Lock()

        def score(bitstring):
            with scored_lock:
                scored.append(int(bitstring, 2))
            return score_of(int(bitstring, 2))

        ev = BitstringCircuitEvaluator(shots, BitstringEvaluator(n, score), alpha=0.5, seed=1, statevector_device=dev,
                                       device_value_cache=True)
        states = {t: [(5 * t + j) % 64 for j in range(8)] for t in range(THREADS)}  # (neighbours share three states)
        circuits = {s: _basis_state_circuit(n, s) for s in range(64)}
        start = threading.Barrier(THREADS)

        def body(worker, t):
            worker.doing = "the start"
            start.wait(sc.JOIN_S)
            for r in range(2):
                for s in states[t] if r == 0 else states[t][::-1]:
                    got = worker.attempt(f"state {s}", lambda: ev.evaluate_circuits([circuits[s]], [[]]))
                    if got is not None and got != [score_of(s)]:
                        worker.fail(f"{got} is not the score of state {s}, {score_of(s)}")

        sc.run_workers({f"thread {t}": (lambda worker, t=t: body(worker, t)) for t in range(THREADS)})
        distinct = sorted({s for mine in states.values() for s in mine})
        assert sorted(scored) == distinct  # (once each)
        assert ev.evaluate_circuits([circuits[s] for s in distinct], [[] for _ in distinct]) == [score_of(s) for s in distinct]
        assert sorted(scored) == distinct and ev.last_scored_bitstrings == 0
        assert ev.value_cache_stats["entries"] == len(distinct)
    finally:
        dev.close()


# ---- 5. device matrices from several torch streams --------------------------------------------------------------------------


def test_device_matrices_written_on_the_callers_own_torch_streams():
    """Every thread fills its parameter matrix with 1e300 on a torch stream of its own, queues passes over a large tensor on that
    stream, then the copy of the true values, and calls evaluate_circuits(circuits, matrix) at once: the handle's streams have to
    wait for THAT thread's stream.  (The passes only widen the window: nothing here depends on a time.)"""
    import torch

    cast, _tasks, expected = _cast(14)
    circuits = cast.circuits
    evaluators = [(cast.first, expected["evaluate_circuits, lists"]), (cast.general, expected["evaluate_circuits, lists, general operator"])]
    true_values = cast.matrix.clone()
    torch.cuda.synchronize()
    start = threading.Barrier(4)

    def body(worker, t):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            big = torch.ones(1 << 23, dtype=torch.float64, device=cast.where)
            matrix = torch.empty_like(true_values)
            stream.synchronize()
            worker.doing = "the start"
            start.wait(sc.JOIN_S)
            for r in range(ROUNDS):
                ev, want = evaluators[(t + r) % 2]
                matrix.fill_(1e300)
                for _ in range(8):
                    big.mul_(1.0000001)
                matrix.copy_(true_values)
                got = worker.attempt(f"round {r}, evaluate_circuits from the matrix of stream {t}", lambda: ev.evaluate_circuits(circuits, matrix))
                if got is not None and not sc.same(got, want):
                    worker.fail(f"not the host lists' values: {got} / {want}")
            stream.synchronize()

    sc.run_workers({f"thread {t}": (lambda worker, t=t: body(worker, t)) for t in range(4)})
    torch.cuda.synchronize()
