"""Entry points called from the thread that has a batch open, and host pointers at the device-pointer sites, through the raw
C ABI (queasars_amd._lib).

Between qsv_eval_begin and qsv_eval_end the calling thread holds the handle's lock.  Every entry point that takes the handle goes
through one opening (qsv_api.hip: open_handle), which refuses such a call with QSV_E_STATE and "a batch is open on this handle
(<name> goes between batches)" instead of waiting for itself.  Two handles make the same calls in the same order (WALK); on the
second the batch between them is interrupted by one call of every entry point.  What is asserted, per entry point:

- inside the batch it returns QSV_E_STATE (the const getters return the code), and qsv_last_error names it;
- afterwards it returns what it returned before the batch (its outputs bit for bit; for a call without outputs its return code);
- everything it returned, ids and counters included, is what the uninterrupted handle returned: nothing half-done was left
  behind (no mask, no open lookup on the cache, no stale layout).

The interrupted batch returns the bits of the uninterrupted one.  Nothing here depends on size: 4 qubits, fp64, two genome
circuits, an Ising operator, a set of two observables, one value cache, one gradient plan, one kept state.  What is compared is
exact, except the two qsv_bench_* times (a measured duration: return code only) and qsv_get_profile's times (its integer
counters only).
"""

import ctypes as C

import numpy as np
import pytest

import helpers
from queasars_amd import _lib
from queasars_amd.ir import QSV_OP_DTYPE

pytestmark = pytest.mark.gpu

N = 4
SHOTS, SEED, ALPHA = 8, 5, 0.5


class Walk:
    """One handle with everything the calls need, and the calls themselves: each returns (stable, volatile) -- what must be the same
    before and after the batch, and what only has to match the other handle (ids, cumulative counters)."""

    def __init__(self):
        self.lib = lib = _lib.load()
        self.h = C.c_void_p()
        assert lib.qsv_create(N, _lib.QSV_F64, 0, None, C.byref(self.h)) == _lib.QSV_OK, _lib.last_error(lib, None)
        op = helpers.random_ising_operator(N, seed=4)
        self.op = [np.ascontiguousarray(a) for a in (op.x_mask, op.z_mask, op.coeffs.real, op.coeffs.imag)]
        self.ok(self.set_operator()[0][0])
        _, self.circuits, params = helpers.population_circuits(N, 2, 2, seed=0)
        self.ops = [np.ascontiguousarray(c.packed()) for c in self.circuits]
        self.n_params = np.asarray([c.num_parameters for c in self.circuits], dtype=np.int32)
        self.ids = np.zeros(2, dtype=np.int32)
        for i in range(2):
            cid = C.c_int()
            self.ok(lib.qsv_circuit_create(self.h, len(self.ops[i]), _lib.as_ptr(self.ops[i]), int(self.n_params[i]), C.byref(cid)))
            self.ids[i] = cid.value
        self.params = [np.asarray(p, dtype=np.float64) for p in params]
        self.flat = np.concatenate(self.params)
        self.offsets = np.asarray([0, len(self.params[0]), len(self.flat)], dtype=np.int64)
        self.counts = np.diff(self.offsets)
        self.all_ops = np.concatenate(self.ops)
        self.op_offsets = np.asarray([0, len(self.ops[0]), len(self.all_ops)], dtype=np.int64)
        # a bound one-gate circuit (qsv_bench_ops, circuits on the kept state)
        self.gate = np.zeros(1, dtype=QSV_OP_DTYPE)
        self.gate[0] = (1, 0, 255, 0, -1, -1, -1, 0.3, 0.2, 0.1)  # QSV_OP_U on qubit 0, literal angles
        self.gate_offsets = np.asarray([0, 1, 2], dtype=np.int64)
        # observables Z0 Z1 and 0.5 X0
        self.obs = [np.asarray(a) for a in ([0, 1, 2], np.asarray([0, 1], dtype=np.uint64), np.asarray([3, 0], dtype=np.uint64), [1.0, 0.5])]
        self.obs[0] = self.obs[0].astype(np.int64)
        self.obs[3] = self.obs[3].astype(np.float64)
        self.set_id = self.observables_create()[1][0]
        self.cache_id = self.value_cache_create()[1][0]
        self.prefix = np.zeros(1, dtype=np.int32)
        self.ok(lib.qsv_prefix_create(self.h, 1, _lib.as_ptr(self.ids), _lib.as_ptr(self.offsets), _lib.as_ptr(self.flat), _lib.as_ptr(self.prefix)))
        plan, shifted = C.c_int(), C.c_int64()
        width = int(self.counts.max())
        self.ok(lib.qsv_gradient_plan_create(self.h, 2, _lib.as_ptr(self.ids), width, None, None, width, C.byref(plan), C.byref(shifted)))
        self.plan_id = plan.value
        self.temp_circuits, self.temp_sets, self.temp_caches = [], [], []
        self.missing = np.zeros(0, dtype=np.uint64)

    def ok(self, rc):
        assert rc == _lib.QSV_OK, _lib.last_error(self.lib, self.h)

    def close(self):
        self.lib.qsv_destroy(self.h)

    def batch(self, between=None):
        """begin, `between`, one push, end: the expectation values."""
        out = np.zeros(2)
        self.ok(self.lib.qsv_eval_begin(self.h, 2, _lib.as_ptr(self.ids), _lib.as_ptr(self.counts)))
        if between:
            between()
        self.ok(self.lib.qsv_eval_push(self.h, 0, 2, _lib.as_ptr(self.flat)))
        self.ok(self.lib.qsv_eval_end(self.h, _lib.as_ptr(out)))
        return out.tobytes()

    # ---- the entry points, each with valid arguments ----------------------------------------------------------------------
    def _batch_args(self):
        return 2, _lib.as_ptr(self.ids), _lib.as_ptr(self.offsets), _lib.as_ptr(self.flat)

    def set_operator(self):
        x, z, cre, cim = self.op
        return (self.lib.qsv_set_operator(self.h, len(x), _lib.as_ptr(x), _lib.as_ptr(z), _lib.as_ptr(cre), _lib.as_ptr(cim)),), ()

    def set_option(self):
        return (self.lib.qsv_set_option(self.h, b"gradient_chunk", 0),), ()

    def set_profiling(self):
        return (self.lib.qsv_set_profiling(self.h, 0),), ()

    def eval_circuits(self):
        out = np.zeros(2)
        return (self.lib.qsv_eval_circuits(self.h, *self._batch_args(), _lib.as_ptr(out)), out.tobytes()), ()

    def eval_batch(self):
        out = np.zeros(2)
        rc = self.lib.qsv_eval_batch(self.h, 2, _lib.as_ptr(self.op_offsets), _lib.as_ptr(self.all_ops), _lib.as_ptr(self.offsets),
                                     _lib.as_ptr(self.flat), _lib.as_ptr(out))
        return (rc, out.tobytes()), ()

    def eval_coalesced(self):
        out = C.c_double()
        rc = self.lib.qsv_eval_coalesced(self.h, int(self.ids[0]), _lib.as_ptr(self.params[0]), len(self.params[0]), 1.0, C.byref(out))
        return (rc, out.value), ()

    def statevector(self):
        out = np.zeros(2 << N)
        return (self.lib.qsv_statevector(self.h, int(self.ids[0]), _lib.as_ptr(self.params[0]), len(self.params[0]), _lib.as_ptr(out)), out.tobytes()), ()

    def probabilities(self):
        out = np.zeros(1 << N)
        return (self.lib.qsv_probabilities(self.h, int(self.ids[1]), _lib.as_ptr(self.params[1]), len(self.params[1]), _lib.as_ptr(out)), out.tobytes()), ()

    def sample(self):
        out = np.zeros(SHOTS, dtype=np.uint64)
        rc = self.lib.qsv_sample(self.h, int(self.ids[0]), _lib.as_ptr(self.params[0]), len(self.params[0]), SHOTS, C.c_uint64(SEED), _lib.as_ptr(out))
        return (rc, out.tobytes()), ()

    def sample_batch(self):
        states, values = np.zeros(2 * SHOTS, dtype=np.uint64), np.zeros(2 * SHOTS)
        rc = self.lib.qsv_sample_batch(self.h, *self._batch_args(), SHOTS, C.c_uint64(SEED), _lib.as_ptr(states), _lib.as_ptr(values))
        return (rc, states.tobytes(), values.tobytes()), ()

    def sample_cvar_batch(self):
        out = np.zeros(2)
        return (self.lib.qsv_sample_cvar_batch(self.h, *self._batch_args(), SHOTS, C.c_uint64(SEED), ALPHA, _lib.as_ptr(out)), out.tobytes()), ()

    def exact_cvar_batch(self):
        out = np.zeros(2)
        return (self.lib.qsv_exact_cvar_batch(self.h, *self._batch_args(), ALPHA, _lib.as_ptr(out)), out.tobytes()), ()

    def top_states(self):
        states, probs, values = np.zeros(4, dtype=np.uint64), np.zeros(4), np.zeros(4)
        rc = self.lib.qsv_top_states(self.h, *self._batch_args(), 2, _lib.as_ptr(states), _lib.as_ptr(probs), _lib.as_ptr(values))
        return (rc, states.tobytes(), probs.tobytes(), values.tobytes()), ()

    def value_cache_clear(self):  # (in front of the lookup: every state is missing again, so the lookup repeats itself)
        return (self.lib.qsv_value_cache_clear(self.h, self.cache_id),), ()

    def sample_lookup(self):
        n_missing, states = C.c_int64(), C.POINTER(C.c_uint64)()
        rc = self.lib.qsv_sample_lookup(self.h, self.cache_id, *self._batch_args(), SHOTS, C.c_uint64(SEED), C.byref(n_missing), C.byref(states))
        if rc:
            return (rc,), ()
        self.missing = np.asarray([states[i] for i in range(n_missing.value)], dtype=np.uint64)
        return (rc, tuple(sorted(self.missing.tolist()))), ()  # (the missing states arrive in any order)

    def sample_lookup_finish(self):
        scores = self.missing.astype(np.float64)  # (a state's score: a function of the state)
        cvar, values = np.zeros(2), np.zeros(2 * SHOTS)
        rc = self.lib.qsv_sample_lookup_finish(self.h, self.cache_id, len(scores), _lib.as_ptr(scores), ALPHA, _lib.as_ptr(cvar), _lib.as_ptr(values))
        return (rc, cvar.tobytes(), values.tobytes()), ()

    def value_cache_create(self):
        cid = C.c_int()
        rc = self.lib.qsv_value_cache_create(self.h, 4, 10, C.byref(cid))
        if rc == _lib.QSV_OK and hasattr(self, "temp_caches"):
            self.temp_caches.append(cid.value)
        return (rc,), (cid.value,)

    def value_cache_destroy(self):  # (what value_cache_create just made; inside the batch, where it made nothing, the cache in use)
        cid = self.temp_caches.pop() if self.temp_caches else self.cache_id
        return (self.lib.qsv_value_cache_destroy(self.h, cid),), ()

    def value_cache_stats(self):
        out = _lib.QsvValueCacheStats()
        return (self.lib.qsv_value_cache_stats(self.h, self.cache_id, C.byref(out)),), (bytes(out),)

    def observables_create(self):
        offsets, x, z, c = self.obs
        sid = C.c_int()
        rc = self.lib.qsv_observables_create(self.h, 2, _lib.as_ptr(offsets), _lib.as_ptr(x), _lib.as_ptr(z), _lib.as_ptr(c), None, C.byref(sid))
        if rc == _lib.QSV_OK and hasattr(self, "temp_sets"):
            self.temp_sets.append(sid.value)
        return (rc,), (sid.value,)

    def observables_destroy(self):
        sid = self.temp_sets.pop() if self.temp_sets else self.set_id
        return (self.lib.qsv_observables_destroy(self.h, sid),), ()

    def eval_observables(self):
        out = np.zeros(4)
        return (self.lib.qsv_eval_observables(self.h, self.set_id, *self._batch_args(), _lib.as_ptr(out)), out.tobytes()), ()

    def _created(self, rc, ids):
        if rc == _lib.QSV_OK:
            self.temp_circuits.extend(int(i) for i in ids)
        return (rc,), tuple(int(i) for i in ids)

    def circuit_create(self):
        cid = C.c_int()
        rc = self.lib.qsv_circuit_create(self.h, len(self.ops[0]), _lib.as_ptr(self.ops[0]), int(self.n_params[0]), C.byref(cid))
        return self._created(rc, [cid.value])

    def circuits_create(self):
        ids = np.zeros(2, dtype=np.int32)
        rc = self.lib.qsv_circuits_create(self.h, 2, _lib.as_ptr(self.op_offsets), _lib.as_ptr(self.all_ops), _lib.as_ptr(self.n_params), _lib.as_ptr(ids))
        return self._created(rc, ids)

    def circuit_create_on_prefix(self):
        cid = C.c_int()
        rc = self.lib.qsv_circuit_create_on_prefix(self.h, int(self.prefix[0]), 1, _lib.as_ptr(self.gate), 0, C.byref(cid))
        return self._created(rc, [cid.value])

    def circuits_create_on_prefixes(self):
        ids, zero = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        gates, prefixes = np.concatenate([self.gate, self.gate]), np.repeat(self.prefix, 2)
        rc = self.lib.qsv_circuits_create_on_prefixes(self.h, 2, _lib.as_ptr(self.gate_offsets), _lib.as_ptr(gates), _lib.as_ptr(zero),
                                                      _lib.as_ptr(prefixes), _lib.as_ptr(ids))
        return self._created(rc, ids)

    def circuit_destroy(self):  # (every circuit the four calls above made; inside the batch, where they made none, one in use)
        doomed, self.temp_circuits = self.temp_circuits or [int(self.ids[0])], []
        return tuple(self.lib.qsv_circuit_destroy(self.h, cid) for cid in doomed), ()

    def prefix_count(self):
        return (self.lib.qsv_prefix_count(self.h),), ()

    def circuit_cost(self):
        out = _lib.QsvCircuitCost()
        return (self.lib.qsv_circuit_cost(self.h, int(self.ids[0]), C.byref(out)), bytes(out)), ()

    def circuit_form(self):
        out = _lib.QsvCircuitForm()
        return (self.lib.qsv_circuit_form(self.h, int(self.ids[0]), C.byref(out)), bytes(out)), ()

    def circuit_launch_form(self):
        out = _lib.QsvCircuitForm()
        return (self.lib.qsv_circuit_launch_form(self.h, int(self.ids[1]), C.byref(out)), bytes(out)), ()

    def get_profile(self):
        out = _lib.QsvProfile()
        rc = self.lib.qsv_get_profile(self.h, C.byref(out))
        return (rc,), (out.n_evals, out.n_pass_launches, out.n_state_passes, out.n_gates, tuple(out.kernel_launches))

    def replayed_pushes(self):
        value = self.lib.qsv_replayed_pushes(self.h)
        return (min(value, 0),), (value,)  # (a count, or a negative code)

    def gradient_stats(self):
        out = _lib.QsvGradientStats()
        return (self.lib.qsv_gradient_stats(self.h, C.byref(out)),), (bytes(out),)

    def adjoint_stats(self):
        out = _lib.QsvAdjointStats()
        return (self.lib.qsv_adjoint_stats(self.h, C.byref(out)),), (bytes(out),)

    def gradient_plan_stats(self):
        out = _lib.QsvGradientPlanStats()
        return (self.lib.qsv_gradient_plan_stats(self.h, self.plan_id, C.byref(out)),), (bytes(out),)

    def bench_ops(self):
        ms, passes = C.c_double(), C.c_int()
        return (self.lib.qsv_bench_ops(self.h, 1, _lib.as_ptr(self.gate), 1, C.byref(ms), C.byref(passes)), passes.value), ()

    def bench_gate(self):
        ms = C.c_double()
        return (self.lib.qsv_bench_gate(self.h, 0, -1, 0.3, 0.2, 0.1, 1, C.byref(ms)),), ()


# in the order they are called (a create in front of its destroy, the cache's clear, lookup and finish in that order)
ENTRY_POINTS = [
    "eval_circuits", "eval_batch", "eval_coalesced", "statevector", "probabilities", "sample", "sample_batch", "sample_cvar_batch",
    "exact_cvar_batch", "top_states", "value_cache_clear", "sample_lookup", "sample_lookup_finish", "value_cache_create",
    "value_cache_destroy", "value_cache_stats", "observables_create", "observables_destroy", "eval_observables", "circuit_create",
    "circuits_create", "circuit_create_on_prefix", "circuits_create_on_prefixes", "circuit_destroy", "prefix_count", "circuit_cost",
    "circuit_form", "circuit_launch_form", "set_operator", "set_option", "set_profiling", "get_profile", "replayed_pushes",
    "gradient_stats", "adjoint_stats", "gradient_plan_stats", "bench_ops", "bench_gate",
]  # fmt: skip


def run_walk(interrupted: bool) -> dict:
    walk = Walk()
    try:
        record = {"before": {}, "inside": {}, "after": {}}

        def call_all(phase):
            for name in ENTRY_POINTS:
                result = getattr(walk, name)()
                record[phase][name] = (result, _lib.last_error(walk.lib, walk.h))

        call_all("before")
        record["plain batch"] = walk.batch()
        record["batch"] = walk.batch((lambda: call_all("inside")) if interrupted else None)
        call_all("after")
        return record
    finally:
        walk.close()


@pytest.fixture(scope="module")
def walks():
    return run_walk(False), run_walk(True)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_refused_inside_an_open_batch_and_unchanged_after_it(walks, name):
    plain, interrupted = walks
    for phase in ("before", "after"):
        (stable, _), error = interrupted[phase][name]
        codes = stable if name == "circuit_destroy" else stable[:1]
        assert all(code == _lib.QSV_OK for code in codes) or name == "prefix_count", (phase, stable, error)
    assert interrupted["before"]["prefix_count"][0][0] == (1,)
    (stable, _), error = interrupted["inside"][name]
    assert stable[0] == _lib.QSV_E_STATE, (stable, error)
    assert f"(qsv_{name} goes between batches)" in error and error.startswith("a batch is open on this handle"), error
    # what it returned before the batch, and what the handle whose batch nobody interrupted returned
    assert interrupted["after"][name][0][0] == interrupted["before"][name][0][0]
    for phase in ("before", "after"):
        assert interrupted[phase][name][0] == plain[phase][name][0], phase


def test_the_interrupted_batch_returns_the_bits_of_a_plain_one(walks):
    plain, interrupted = walks
    assert interrupted["batch"] == interrupted["plain batch"] == plain["batch"] == plain["plain batch"]
    assert not plain["inside"]
    # ... which are the expectation values (the oracle: 1e-10, the suite's fp64 bound)
    walk = Walk()
    try:
        got = np.frombuffer(interrupted["batch"])
        ref = [helpers.oracle_expectation(c, p, helpers.random_ising_operator(N, seed=4)) for c, p in zip(walk.circuits, walk.params)]
        assert np.abs(got - np.asarray(ref)).max() < 1e-10
    finally:
        walk.close()


# ---- a host pointer at each of the five device-pointer sites -------------------------------------------------------------------

POINTER_SITES = [
    ("qsv_cvar_device", "device_values"), ("qsv_cvar_device", "device_out"), ("qsv_cvar_device", "device_active"),
    ("qsv_gradient_device", "device_values"), ("qsv_gradient_device", "device_out"),
    ("qsv_adjoint_gradient_device", "device_values"), ("qsv_adjoint_gradient_device", "device_out"),
    ("qsv_adjoint_gradient_device", "device_out_values"),
    ("qsv_gradient_plan_run", "device_values"), ("qsv_gradient_plan_run", "device_out"),
    ("qsv_eval_push_device", "device_values"),
]  # fmt: skip


@pytest.fixture(scope="module")
def pointer_walk():
    walk = Walk()
    yield walk
    walk.close()


@pytest.mark.parametrize("site,argument", POINTER_SITES)
def test_a_host_pointer_is_refused_by_name(pointer_walk, site, argument):
    import torch

    walk, lib = pointer_walk, pointer_walk.lib
    width = int(walk.counts.max())
    host = np.zeros(2 * width + 2)  # (large enough for any of the arguments)
    device = {
        "device_values": torch.zeros(2 * width, dtype=torch.float64, device="cuda"),
        "device_out": torch.zeros(2 * width, dtype=torch.float64, device="cuda"),
        "device_out_values": torch.zeros(2, dtype=torch.float64, device="cuda"),
        "device_active": torch.ones(2, dtype=torch.uint8, device="cuda"),
    }
    torch.cuda.synchronize()
    arg = {key: C.c_void_p(host.ctypes.data if key == argument else tensor.data_ptr()) for key, tensor in device.items()}
    ids = _lib.as_ptr(walk.ids)
    if site == "qsv_cvar_device":
        rc = lib.qsv_cvar_device(walk.h, 2, ids, width, arg["device_values"], None, SHOTS, C.c_uint64(SEED), ALPHA, arg["device_active"], 1,
                                 arg["device_out"])
    elif site == "qsv_gradient_device":
        rc = lib.qsv_gradient_device(walk.h, 2, ids, width, arg["device_values"], None, None, None, width, arg["device_out"], None)
    elif site == "qsv_adjoint_gradient_device":
        rc = lib.qsv_adjoint_gradient_device(walk.h, 2, ids, width, arg["device_values"], None, None, None, width, arg["device_out"],
                                             arg["device_out_values"])
    elif site == "qsv_gradient_plan_run":
        rc = lib.qsv_gradient_plan_run(walk.h, walk.plan_id, arg["device_values"], None, arg["device_out"])
    else:
        counts = np.full(2, width, dtype=np.int64)
        walk.ok(lib.qsv_eval_begin(walk.h, 2, ids, _lib.as_ptr(counts)))
        rc = lib.qsv_eval_push_device(walk.h, 0, 2, arg["device_values"], None)
        error = _lib.last_error(lib, walk.h)
        assert lib.qsv_eval_end(walk.h, None) != _lib.QSV_OK  # (nothing was pushed, and there is no output: the batch is closed)
        assert rc == _lib.QSV_E_ARG and error == "device_values is not memory of this handle's device"
        return
    assert rc == _lib.QSV_E_ARG
    assert _lib.last_error(lib, walk.h) == f"{argument} is not memory of this handle's device"
    torch.cuda.synchronize()
