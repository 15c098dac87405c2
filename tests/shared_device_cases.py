"""One ``StatevectorDevice`` shared by evaluators of different operators and called from several threads (test helpers, no tests;
tests/test_gpu_shared_device_threads.py).

``Cast`` is the device with its evaluators, ``tasks()`` one call of every public consumer, each tagged with the operator it
installs (None: it reads none).  The reference of a task is the task itself, run alone: the project promises the same bits in
any batch and whatever came between, so a result under threads must be ``same`` as the serial one.  ``run_workers`` starts
daemon threads and turns a thread that does not come back into a failed test that names where it was.
"""

from __future__ import annotations

import threading
import time
from typing import Callable, NamedTuple, Optional

import numpy as np
import pytest

import circuit_families as cf
import helpers
import operator_families as of
from queasars_amd.circuit_evaluation import (
    CoalescingCircuitEvaluator,
    DeflatedOperatorCircuitEvaluator,
    ExactCVaRCircuitEvaluator,
    OperatorCircuitEvaluator,
    OperatorSamplerCircuitEvaluator,
    StatevectorDevice,
)

JOIN_S = 90.0  # (tests of seconds: a thread that has not come back by then never will)
SEED, SHOTS, TOP_K = 2020, 256, 4


class Task(NamedTuple):
    name: str
    operator: Optional[str]  # which of the cast's operators the call installs on the shared device
    call: Callable[[], object]


def population(n: int):
    """(circuits, parameters).  14 qubits: tests/test_gpu_replay.py's "split" case (genome circuits that split without a key and
    a two-key circuit) and all pairs of qubits, which never split -- ordinary gate passes beside the split forms on the auxiliary
    stream.  6 qubits: four genome circuits and a ladder, the one-tile route."""
    if n == 14:
        from test_gpu_replay import CASES

        _n, _op, circuits, params, _options, _replayable = CASES["split"]
        extra = [cf.all_pairs(n, 1)]
    else:
        _, circuits, params = helpers.population_circuits(n, 2, 4, seed=n)
        extra = [cf.ladder(n, 2)]
    return list(circuits) + [c for c, _ in extra], [list(p) for p in params] + [list(p) for _, p in extra]


def device_matrix(params):
    """The parameter vectors as rows of a device matrix, complete."""
    import torch

    width = max(1, max(len(p) for p in params))
    host = np.zeros((len(params), width))
    for i, p in enumerate(params):
        host[i, : len(p)] = p
    matrix = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return matrix


def same(got, want) -> bool:
    """Bit for bit, through tuples and lists: the same structure, and every leaf the same dtype, shape and bytes."""
    if isinstance(want, (tuple, list)) and any(isinstance(w, (tuple, list, np.ndarray)) or w is None for w in want):
        return type(got) is type(want) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if want is None or got is None:
        return got is want
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Cast:
    """The shared device of one size and number format, the evaluators that all take it, and what their calls need."""

    def __init__(self, n: int, dtype: str = "fp64"):
        import torch

        self.n, self.dtype = n, dtype
        self.dev = dev = StatevectorDevice(n, dtype=dtype)
        self.circuits, self.params = population(n)
        self.operators = {
            "ising": helpers.random_ising_operator(n, seed=SEED),
            "pauli": helpers.random_pauli_operator(n, 12, seed=SEED + 1),
            "sampler": helpers.random_ising_operator(n, seed=SEED + 2),
            "cvar": helpers.random_ising_operator(n, seed=SEED + 3),
            "deflated": of.heisenberg(n),
        }
        ops = self.operators
        self.first = OperatorCircuitEvaluator(ops["ising"], statevector_device=dev, gradient_method="auto")
        self.general = OperatorCircuitEvaluator(ops["pauli"], statevector_device=dev, gradient_method="adjoint")
        self.sampler = OperatorSamplerCircuitEvaluator(None, ops["sampler"], alpha=0.5, statevector_device=dev)
        self.cvar = ExactCVaRCircuitEvaluator(ops["cvar"], 0.25, statevector_device=dev)
        self.kept = dev.keep_states(self.circuits[:3], self.params[:3])
        self.deflated = DeflatedOperatorCircuitEvaluator(ops["deflated"], self.kept, statevector_device=dev)
        self.merged = CoalescingCircuitEvaluator(self.first)
        assert self.merged._native
        self.observables = [of.unweighted_cut(n, 3), of.transverse_ising(n), of.one_group(n, 24)]
        self.diagonal_observables = [of.unweighted_cut(n, 3), helpers.random_ising_operator(n, seed=SEED + 4)]
        self.wrt = [list(range(0, c.num_parameters, 7)) for c in self.circuits]  # (every seventh: all three slots, u and cu3)
        self.out_width = max(len(w) for w in self.wrt) + 3
        self.subsets = [[0], [n - 1, 1], [2, 0, n - 2]]
        self.matrix = device_matrix(self.params)
        self.where = torch.device("cuda", dev.device_index)
        self.plan = self.first.gradient_plan(self.circuits, self.matrix, self._gradient_rows(), self.wrt)

    def close(self):
        self.plan.close()
        for state in self.kept:
            state.release()
        self.dev.close()

    # -- pieces of the tasks ------------------------------------------------------------------------------------------------
    def _gradient_rows(self):
        """A fresh output matrix for a device-to-device gradient call, complete (NaN: every entry has to be written)."""
        import torch

        out = torch.full((len(self.circuits), self.out_width), float("nan"), dtype=torch.float64, device=self.where)
        torch.cuda.synchronize()
        return out

    def _device_gradients(self, queue) -> np.ndarray:
        import torch

        out = self._gradient_rows()
        queue(out)  # (queued on the handle's stream and not waited for)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def _kept_round_trip(self):
        """keep_states + continue_from + evaluate + release, with objects of this call alone."""
        states = self.first.keep_states(self.circuits[:2], self.params[:2])
        try:
            rests = [cf.ladder(self.n, 1, seed=5) for _ in states]
            continued = [rest.continue_from(state) for (rest, _), state in zip(rests, states)]
            return self.first.evaluate_circuits(continued, [list(p) for _, p in rests])
        finally:
            for state in states:
                state.release()

    def _under(self, operator: str, call):
        with self.dev.with_operator(self.operators[operator]):
            return call()

    def tasks(self) -> list[Task]:
        """One call of every public consumer.  Neighbours install different operators (or none)."""
        c, p, dev = self.circuits, self.params, self.dev
        first, general, sampler, cvar, deflated, merged = self.first, self.general, self.sampler, self.cvar, self.deflated, self.merged
        made = [
            Task("evaluate_circuits, lists", "ising", lambda: first.evaluate_circuits(c, p)),
            Task("evaluate_circuits, lists, general operator", "pauli", lambda: general.evaluate_circuits(c, p)),
            Task("evaluate_circuits, device matrix", "ising", lambda: first.evaluate_circuits(c, self.matrix)),
            Task("exact distribution, alpha 0.5", "sampler", lambda: sampler.evaluate_circuits(c, p)),
            Task("evaluate_gradients, auto", "ising", lambda: first.evaluate_gradients(c, p, self.wrt)),
            Task("evaluate_gradients, adjoint", "pauli", lambda: general.evaluate_gradients(c, p, self.wrt)),
            Task("evaluate_gradients_device_to_device, auto", "ising", lambda: self._device_gradients(
                lambda out: first.evaluate_gradients_device_to_device(c, self.matrix, out, self.wrt))),
            Task("evaluate_gradients_device_to_device, adjoint", "pauli", lambda: self._device_gradients(
                lambda out: general.evaluate_gradients_device_to_device(c, self.matrix, out, self.wrt))),
            Task("gradient plan run", "ising", lambda: self._device_gradients(lambda out: self.plan.run(self.matrix, out))),
            Task("CVaR values", "cvar", lambda: cvar.evaluate_circuits(c, p)),
            Task("evaluate_variances", "ising", lambda: first.evaluate_variances(c, p, with_values=True)),
            Task("evaluate_variances, general operator", "pauli", lambda: general.evaluate_variances(c, p, with_values=True)),
            Task("evaluate_observables", None, lambda: first.evaluate_observables(c, p, self.observables)),
            Task("CVaR gradients", "cvar", lambda: cvar.evaluate_gradients(c, p, self.wrt)),
            Task("evaluate_covariances", None, lambda: general.evaluate_covariances(c, p, self.observables, with_values=True)),
            Task("deflated cost", "deflated", lambda: deflated.evaluate_circuits(c, p)),
            Task("evaluate_overlaps", None, lambda: first.evaluate_overlaps(c, p, self.kept)),
            Task("evaluate_overlaps, with the operator", "pauli", lambda: general.evaluate_overlaps(c, p, self.kept, with_operator=True)),
            Task("deflated gradients", "deflated", lambda: deflated.evaluate_gradients(c, p, self.wrt)),
            Task("evaluate_subspace_matrices", "pauli", lambda: general.evaluate_subspace_matrices(c[:3], p[:3])),
            Task("reduced_density_matrices", None, lambda: first.reduced_density_matrices(c, p, self.subsets)),
            Task("deflation terms", "deflated", lambda: deflated.evaluate_deflation_terms(c, p)),
            Task("operator_density_matrices", "pauli", lambda: general.operator_density_matrices(c, p, self.subsets, with_values=True)),
            Task("metric_tensors", None, lambda: first.metric_tensors(c, p, self.wrt)),
            Task("top_states, diagonal operator", "sampler", lambda: sampler.top_states(c, p, TOP_K)),
            Task("top_states, general operator", None, lambda: general.top_states(c, p, TOP_K)),
            Task("CVaR values and gradients", "cvar", lambda: cvar.evaluate_values_and_gradients(c, p, self.wrt)),
            Task("sampler evaluate_observables", "sampler", lambda: sampler.evaluate_observables(c, p, self.diagonal_observables)),
            Task("CVaR thresholds", "cvar", lambda: cvar.evaluate_thresholds(c, p)),
            Task("keep, continue, evaluate, release", "ising", self._kept_round_trip),
            Task("statevector", None, lambda: dev.statevector(c[-1], p[-1])),
            Task("device sample_cvar_batch", "sampler", lambda: self._under(
                "sampler", lambda: dev.sample_cvar_batch(c, p, SHOTS, SEED, 0.5))),
            Task("device exact_cvar_batch", "cvar", lambda: self._under("cvar", lambda: dev.exact_cvar_batch(c, p, 0.3))),
            Task("merged one-circuit call", "ising", lambda: merged.evaluate_circuits(c[1:2], p[1:2])),
            Task("deflated cost, again", "deflated", lambda: deflated.evaluate_circuits(c[::-1], p[::-1])),
            Task("merged two-circuit call", "ising", lambda: merged.evaluate_circuits(c[:2], p[:2])),
        ]
        for before, after in zip(made[:-1], made[1:]):
            assert before.operator is None or before.operator != after.operator, (before.name, after.name)
        return made


def serial_reference(tasks: list[Task]) -> dict:
    """{name: result} of every task run alone, twice: the second run must give the first one's bits -- the premise of every
    comparison under threads.  A task that is not stable serially is a finding of its own."""
    first = {task.name: task.call() for task in tasks}
    unstable = [task.name for task in tasks if not same(task.call(), first[task.name])]
    assert not unstable, f"not the same bits in two serial runs: {unstable}"
    return first


def order_of(tasks: list[Task], seed: int) -> list[Task]:
    """A seeded order of ``tasks`` in which a task does not follow one that installs the same operator, wherever another
    task is left to take."""
    rng = np.random.default_rng(seed)
    left = [tasks[i] for i in rng.permutation(len(tasks))]
    out: list[Task] = []
    while left:
        last = out[-1].operator if out else None
        pick = next((i for i, task in enumerate(left) if last is None or task.operator != last), 0)
        out.append(left.pop(pick))
    return out


class Worker:
    """A daemon thread that notes what it is doing and every failure with the name of what it was doing."""

    def __init__(self, name: str, body: Callable[["Worker"], None], failures: list):
        self.name, self.doing, self._failures = name, "starting", failures
        self._thread = threading.Thread(target=self._run, args=(body,), name=name, daemon=True)

    def _run(self, body):
        try:
            body(self)
        except BaseException as exc:  # noqa: BLE001
            self.fail(exc)

    def fail(self, what):
        self._failures.append(f"{self.name}, {self.doing}: {what!r}")

    def attempt(self, what: str, call):
        """``call()``; an exception is written down under ``what`` and None returned: the thread goes on."""
        self.doing = what
        try:
            return call()
        except Exception as exc:  # noqa: BLE001
            self.fail(exc)
            return None


def run_workers(bodies: dict) -> None:
    """Start one daemon thread per ``{name: body(worker)}``, join them within JOIN_S and fail with every failure written down --
    a thread that is still alive names the task it was in."""
    failures: list = []
    workers = [Worker(name, body, failures) for name, body in bodies.items()]
    for w in workers:
        w._thread.start()
    deadline = time.monotonic() + JOIN_S
    for w in workers:
        w._thread.join(max(0.0, deadline - time.monotonic()))
    stuck = [f"{w.name} never came back from: {w.doing}" for w in workers if w._thread.is_alive()]
    if stuck:
        pytest.fail("a thread hangs (the others may wait for what it holds)\n" + "\n".join(stuck + failures))
    assert not failures, f"{len(failures)} failures\n" + "\n".join(failures[:40])
