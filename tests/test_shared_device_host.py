"""A device shared by threads, without a device: the two places where a caller's second step used what another caller's first
step had taken away, made deterministic with a stand-in library and ``threading.Event``.

* ``StatevectorDevice._observable_set`` hands out the id of a cached observable set, and the library call that uses the id is a
  second step: a caller that misses meanwhile evicts -- destroys -- the least recently used set, which may be that one.
* ``BitstringCircuitEvaluator(device_value_cache=True)`` looks up, scores on the host and finishes: the library refuses a second
  lookup on a cache whose first waits for its finish (include/qsv.h, VALUE CACHES).

A thread is parked INSIDE the stand-in library (or inside the scoring function), the other thread is started, and the parked one
is released once the other has either finished or is waiting for a lock (``WatchedLock`` tells): no sleep decides anything."""

import ctypes as C
import threading
from collections import OrderedDict

import numpy as np

from queasars_amd import _lib
from queasars_amd.circuit_evaluation import BitstringCircuitEvaluator, BitstringEvaluator
from queasars_amd.circuit_evaluation.circuit_evaluation import DeviceValueCache, StatevectorDevice
from queasars_amd.ir import CircuitIR, PauliOperator

N_QUBITS = 3
JOIN_S = 60.0  # (a deadlock ends as a failed test)


class WatchedLock:
    """A lock that says when a thread has to wait for it."""

    def __init__(self, on_wait):
        self._lock, self._on_wait = threading.Lock(), on_wait

    def acquire(self, blocking=True, timeout=-1):
        if self._lock.acquire(False):
            return True
        self._on_wait()
        return self._lock.acquire(blocking, timeout)

    def release(self):
        self._lock.release()

    def __enter__(self):
        return self.acquire()

    def __exit__(self, *exc):
        self.release()


def run_threads(*threads):
    for t in threads:
        t.join(JOIN_S)
    alive = [t.name for t in threads if t.is_alive()]
    assert not alive, f"still running after {JOIN_S} s: {alive}"


def thread(name, target):
    t = threading.Thread(target=target, name=name, daemon=True)
    t.start()
    return t


# ---- observable sets ------------------------------------------------------------------------------------------------------


class ObservableLib:
    """``qsv_observables_create`` / ``_destroy`` / ``qsv_eval_observables`` / ``qsv_observables_covariance``: the ids that are
    alive, every use of one that is not, and a place to park the calling thread in (``park[name of the entry point]`` = (thread
    name, event set on arrival, event waited for))."""

    def __init__(self):
        self.live, self.dead_uses, self.uses, self.next_id = set(), [], [], 100
        self.park: dict = {}
        self._lock = threading.Lock()

    def _arrive(self, where):
        parked = self.park.get(where)
        if parked is not None and parked[0] == threading.current_thread().name:
            del self.park[where]
            parked[1].set()
            assert parked[2].wait(JOIN_S), f"{where}: never released"

    def qsv_observables_create(self, handle, n, offsets, x, z, cre, cim, out):
        with self._lock:
            self.next_id += 1
            new = self.next_id
            self.live.add(new)
        self._arrive("create")
        out._obj.value = new
        return _lib.QSV_OK

    def qsv_observables_destroy(self, handle, set_id):
        with self._lock:
            self.live.discard(set_id)
        return _lib.QSV_OK

    def _use(self, where, set_id):
        self._arrive(where)
        with self._lock:
            self.uses.append((where, set_id))
            if set_id not in self.live:
                self.dead_uses.append((threading.current_thread().name, where, set_id))
        return _lib.QSV_OK  # (the library would refuse a dead id with QSV_E_ARG: here it is written down instead)

    def qsv_eval_observables(self, handle, set_id, n, ids, offsets, flat, out):
        return self._use("values", set_id)

    def qsv_observables_covariance(self, handle, set_id, n, ids, offsets, flat, values, covariances):
        return self._use("covariances", set_id)


def observable_device(progress):
    """A ``StatevectorDevice`` without a handle: the fields its observable methods read, the stand-in library, and one
    evaluation's packed arguments whatever the circuits (nothing is registered)."""
    dev = object.__new__(StatevectorDevice)  # no GPU here: only the bookkeeping is exercised
    dev._n_qubits, dev._handle, dev._lib = N_QUBITS, 1, ObservableLib()
    dev._observable_sets = OrderedDict()
    dev._observable_lock = WatchedLock(progress.set)
    arguments = (np.zeros(1, dtype=np.int32), np.zeros(2, dtype=np.int64), np.zeros(1))
    dev._batch_arguments = lambda circuits, parameter_values: arguments
    return dev


def observables(k):
    """Observable list k: distinct content, so a cache key of its own."""
    return [PauliOperator(["ZII"], [1.0 + k]), PauliOperator(["IXI"], [0.5])]


CIRCUITS, VALUES = [CircuitIR(N_QUBITS).u(0.1, 0.2, 0.3, 0)], [[]]


def assert_sets_are_consistent(dev):
    lib = dev._lib
    assert not lib.dead_uses, f"a destroyed observable set was used: {lib.dead_uses}"
    assert lib.live == set(dev._observable_sets.values()), "a live set is not in the cache (leaked) or a cached one is dead"
    assert len(lib.live) <= StatevectorDevice.MAX_OBSERVABLE_SETS
    dev._handle = None  # keep __del__ from calling qsv_destroy on the stand-in


def test_a_set_is_not_destroyed_between_its_lookup_and_its_use():
    """A holds the id of its set and waits for the handle; B misses MAX_OBSERVABLE_SETS times, which makes A's the least
    recently used one."""
    progress = threading.Event()
    dev = observable_device(progress)
    lib = dev._lib
    arrived, go = threading.Event(), threading.Event()
    lib.park["values"] = ("A", arrived, go)
    failures = []

    def a():
        try:
            dev.observable_values(CIRCUITS, VALUES, observables(0))
        except BaseException as exc:  # noqa: BLE001
            failures.append(("A", exc))

    def b():
        try:
            for k in range(1, StatevectorDevice.MAX_OBSERVABLE_SETS + 1):
                if k % 2:
                    dev.observable_covariances(CIRCUITS, VALUES, observables(k))
                else:
                    dev.observable_values(CIRCUITS, VALUES, observables(k))
        except BaseException as exc:  # noqa: BLE001
            failures.append(("B", exc))
        finally:
            progress.set()

    ta = thread("A", a)
    assert arrived.wait(JOIN_S), "A never reached the library"
    tb = thread("B", b)
    assert progress.wait(JOIN_S), "B neither finished nor waited"  # (B is done, or waits for the lock A holds)
    go.set()
    run_threads(ta, tb)
    assert not failures, failures
    assert len(lib.uses) == 1 + StatevectorDevice.MAX_OBSERVABLE_SETS
    assert_sets_are_consistent(dev)
    # ... and A's list again, alone: found or created anew, and used alive
    dev._handle = 1
    dev.observable_values(CIRCUITS, VALUES, observables(0))
    assert_sets_are_consistent(dev)


def test_two_misses_of_one_key_leave_one_set_and_no_orphan():
    """C is inside ``qsv_observables_create`` for a list when D asks for the same list."""
    progress = threading.Event()
    dev = observable_device(progress)
    lib = dev._lib
    arrived, go = threading.Event(), threading.Event()
    lib.park["create"] = ("C", arrived, go)
    failures = []

    def call(name):
        try:
            dev.observable_values(CIRCUITS, VALUES, observables(7))
        except BaseException as exc:  # noqa: BLE001
            failures.append((name, exc))
        finally:
            if name == "D":
                progress.set()

    tc = thread("C", lambda: call("C"))
    assert arrived.wait(JOIN_S), "C never reached the library"
    td = thread("D", lambda: call("D"))
    assert progress.wait(JOIN_S), "D neither finished nor waited"
    go.set()
    run_threads(tc, td)
    assert not failures, failures
    assert len(lib.uses) == 2
    assert_sets_are_consistent(dev)


# ---- a shared value cache -------------------------------------------------------------------------------------------------


class CacheLib:
    """``qsv_value_cache_*`` and ``qsv_sample_lookup`` / ``_finish`` for circuits whose every shot is ONE basis state -- the one
    the evaluation's first parameter names.  As the header states, a second lookup before the finish is ``QSV_E_STATE``."""

    def __init__(self):
        self.table: dict = {}
        self.pending = None  # (states of the lookup's evaluations, its miss list)
        self.refused = 0
        self._keep = None

    def qsv_last_error(self, handle):
        return b"a lookup on this cache waits for its finish"

    def qsv_value_cache_create(self, handle, log2_slots, log2_max_slots, out):
        out._obj.value = 1
        return _lib.QSV_OK

    def qsv_value_cache_destroy(self, handle, cache_id):
        return _lib.QSV_OK

    def qsv_value_cache_clear(self, handle, cache_id):
        self.table.clear()
        self.pending = None
        return _lib.QSV_OK

    def qsv_sample_lookup(self, handle, cache_id, n, ids, offsets, flat, shots, seed, n_missing, states):
        if self.pending is not None:
            self.refused += 1
            return _lib.QSV_E_STATE
        offs = C.cast(offsets, C.POINTER(C.c_int64))
        values = C.cast(flat, C.POINTER(C.c_double))
        sampled = [int(values[offs[i]]) for i in range(n)]
        missing = sorted({s for s in sampled if s not in self.table}, reverse=True)  # ("in no particular order")
        self.pending = (sampled, missing)
        self._keep = (C.c_uint64 * max(1, len(missing)))(*missing)
        n_missing._obj.value = len(missing)
        states._obj.value = C.addressof(self._keep)
        return _lib.QSV_OK

    def qsv_sample_lookup_finish(self, handle, cache_id, n_given, given, alpha, out, out_values):
        if self.pending is None:
            return _lib.QSV_E_STATE
        sampled, missing = self.pending
        if n_given != len(missing):
            return _lib.QSV_E_ARG
        scores = C.cast(given, C.POINTER(C.c_double))
        for j, state in enumerate(missing):
            self.table[state] = scores[j]
        results = C.cast(out, C.POINTER(C.c_double))
        for i, state in enumerate(sampled):
            results[i] = self.table[state]  # (the CVaR of shots that all have this value)
        self.pending = None
        return _lib.QSV_OK


class CacheDevice:
    """What a ``DeviceValueCache`` and the evaluator ask of their device."""

    n_qubits = N_QUBITS
    _handle = 1

    def __init__(self):
        self._lib = CacheLib()
        self._kept = []

    def value_cache(self):
        return DeviceValueCache(self)

    def _batch_arguments(self, circuits, parameter_values):
        n = len(circuits)
        offsets = np.arange(n + 1, dtype=np.int64)
        flat = np.asarray([p[0] for p in parameter_values], dtype=np.float64)
        return np.zeros(n, dtype=np.int32), offsets, flat


def score_of(state: int) -> float:
    return 10.0 + state / 8


def test_two_threads_share_one_cached_evaluator_and_each_gets_its_own_values():
    """The first caller is inside the scoring function -- between its lookup and its finish -- when the second one calls."""
    progress, arrived, go = threading.Event(), threading.Event(), threading.Event()
    scored, scored_lock = [], threading.Lock()

    def score(bitstring: str) -> float:
        state = int(bitstring, 2)
        with scored_lock:
            scored.append(state)
        if threading.current_thread().name == "first" and not arrived.is_set():
            arrived.set()
            assert go.wait(JOIN_S), "the scoring function was never released"
        return score_of(state)

    device = CacheDevice()
    ev = BitstringCircuitEvaluator(4, BitstringEvaluator(N_QUBITS, score), alpha=0.5, seed=1, statevector_device=device,
                                   device_value_cache=True)
    ev._cache_lock = WatchedLock(progress.set)
    circuit = CircuitIR(N_QUBITS).u(0.1, 0.2, 0.3, 0)
    results, failures = {}, []

    def call(name, states):
        try:
            results[name] = ev.evaluate_circuits([circuit] * len(states), [[float(s)] for s in states])
        except BaseException as exc:  # noqa: BLE001
            failures.append((name, exc))
        finally:
            if name == "second":
                progress.set()

    first = thread("first", lambda: call("first", [5, 3]))
    assert arrived.wait(JOIN_S), "the first caller never scored"
    second = thread("second", lambda: call("second", [6, 5]))
    assert progress.wait(JOIN_S), "the second caller neither finished nor waited"
    go.set()
    run_threads(first, second)
    assert not failures, failures
    assert device._lib.refused == 0
    assert results == {"first": [score_of(5), score_of(3)], "second": [score_of(6), score_of(5)]}
    assert sorted(scored) == [3, 5, 6]  # (once per distinct state, over both calls)
    assert ev.evaluate_circuits([circuit] * 3, [[3.0], [5.0], [6.0]]) == [score_of(3), score_of(5), score_of(6)]
    assert sorted(scored) == [3, 5, 6] and ev.last_scored_bitstrings == 0


def test_a_cached_evaluator_pickles_without_its_cache_and_gets_a_lock_of_its_own():
    ev = BitstringCircuitEvaluator(4, BitstringEvaluator(N_QUBITS, len), statevector_device=CacheDevice(), device_value_cache=True)
    state = ev.__getstate__()
    assert state["_value_cache"] is None
    assert not any(isinstance(v, type(threading.Lock())) for v in state.values())  # (a lock does not pickle)
    restored = BitstringCircuitEvaluator.__new__(BitstringCircuitEvaluator)
    restored.__setstate__(state)
    assert restored._value_cache is None and restored._cache_lock is not ev._cache_lock
    with restored._cache_lock:
        pass


# ---- merged one-circuit callers on a device other evaluators use ------------------------------------------------------------


class WatchedCondition(threading.Condition):
    """A condition that says when a thread waits for it."""

    def __init__(self, on_wait):
        super().__init__(threading.Lock())
        self._on_wait = on_wait

    def wait(self, timeout=None):
        self._on_wait()
        return super().wait(timeout)


class OperatorLib:
    """``qsv_set_operator``: which installation came while a merged caller was inside the library."""

    def __init__(self):
        self.inside, self.changed_under_a_caller = 0, []

    def qsv_set_operator(self, handle, n_terms, x, z, cre, cim):
        if self.inside:
            self.changed_under_a_caller.append(threading.current_thread().name)
        return _lib.QSV_OK


def test_the_operator_stays_while_a_merged_one_circuit_caller_is_inside_the_library():
    """``CoalescingCircuitEvaluator``'s native path waits in ``qsv_eval_coalesced`` without ``operator_lock`` -- the callers are
    merged because they wait together --, so on a shared device another evaluator's ``set_operator`` has to wait for them: the
    merged batch is evaluated under the operator installed when it RUNS."""
    from queasars_amd.circuit_evaluation import CoalescingCircuitEvaluator, OperatorCircuitEvaluator

    progress, arrived, go = threading.Event(), threading.Event(), threading.Event()
    dev = object.__new__(StatevectorDevice)  # no GPU here: only the bookkeeping is exercised
    dev._n_qubits, dev._handle, dev._lib, dev._operator = N_QUBITS, 1, OperatorLib(), None
    dev.operator_lock = threading.RLock()
    dev._coalesced, dev._coalesced_callers = WatchedCondition(progress.set), 0
    lib = dev._lib
    seen = {}

    def coalesced(circuit, parameter_values, window_us=0.0):
        lib.inside += 1
        seen["on entry"] = dev._operator
        arrived.set()
        assert go.wait(JOIN_S), "the merged caller was never released"
        seen["on return"] = dev._operator
        lib.inside -= 1
        return 0.25

    dev.expectation_value_coalesced = coalesced
    dev.expectation_values = lambda circuits, parameter_values: np.full(len(circuits), 0.5)
    mine, other = PauliOperator(["ZZI"], [1.0]), PauliOperator(["IXX"], [1.0])
    merged = CoalescingCircuitEvaluator(OperatorCircuitEvaluator(mine, statevector_device=dev))
    rival = OperatorCircuitEvaluator(other, statevector_device=dev)
    merged._evaluator.evaluate_circuits(CIRCUITS, VALUES)  # (mine is installed)
    assert merged._native and dev._operator is mine
    results, failures = {}, []

    def call(name, evaluator):
        try:
            results[name] = evaluator.evaluate_circuits(CIRCUITS, VALUES)
        except BaseException as exc:  # noqa: BLE001
            failures.append((name, exc))
        finally:
            if name == "rival":
                progress.set()

    first = thread("merged", lambda: call("merged", merged))
    assert arrived.wait(JOIN_S), "the merged caller never reached the library"
    second = thread("rival", lambda: call("rival", rival))
    assert progress.wait(JOIN_S), "the rival neither finished nor waited"
    go.set()
    run_threads(first, second)
    dev._handle = None  # keep __del__ from calling qsv_destroy on the stand-in
    assert not failures, failures
    assert results == {"merged": [0.25], "rival": [0.5]}
    assert lib.changed_under_a_caller == [] and seen == {"on entry": mine, "on return": mine}
    assert dev._operator is other and dev._coalesced_callers == 0
    # with the rival's operator installed a one-circuit call goes through the merged batch, which installs its own
    assert merged.evaluate_circuits(CIRCUITS, VALUES) == [0.5] and dev._operator is mine
