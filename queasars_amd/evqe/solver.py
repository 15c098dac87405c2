"""EVQE driver over a circuit evaluator.

Restates the control flow of the reference's solver so that the evaluator can be exercised end to end
(BASELINE config 4), without Qiskit, Dask or a thread pool:

* operator order and seeding chain: queasars/minimum_eigensolvers/evqe/evqe.py:188-229;
* generation loop, callbacks, termination: queasars/minimum_eigensolvers/base/evolving_ansatz_minimum_eigensolver.py:331-433;
* mutation: queasars/minimum_eigensolvers/evqe/evolutionary_algorithm/mutation.py:28-132 (layer optimisation),
  :194-235 (who is mutated, with which seed), :328-334 / :347-353 / :383-395 (the four mutation operators);
* speciation: .../speciation.py:34-90;  selection: .../selection.py:64-175;
* termination criterion: queasars/minimum_eigensolvers/base/termination_criteria.py:90-144;
* SPSA stopping rule: queasars/utility/spsa_termination.py:48-96.

The optimiser itself lives in qiskit-algorithms (absent here); :class:`SPSA` restates its published first-order
algorithm for the settings the reference's examples use (constant learning rate and perturbation, Bernoulli +-1
directions from ``numpy.random.default_rng(seed)``, one resampling, optional trust region, ``last_avg=1``).

MI355X-first difference: the reference farms one optimiser run per individual to a thread pool and lets a
"batching mutex" glue their two-circuit requests together inside a 0.1 s window
(queasars/circuit_evaluation/mutex_primitives.py:67-199).  Here all runs advance in lock-step and every SPSA
iteration of the whole population is ONE ``evaluate_circuits`` call.  Each run still sees exactly the sequence of
function values an independent run with its seed would see.
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from random import Random
from statistics import mean, median
from typing import Any, Callable, Optional, Sequence, Union

import numpy as np

from queasars_amd.evqe import device_search
from queasars_amd.evqe.device_search import _full_point, _PackedRuns, _positions  # (the run layout is stated there)
from queasars_amd.evqe.genome import EVQECircuitLayer, EVQEIndividual, EVQEPopulation, new_random_seed


# ---- optimiser ------------------------------------------------------------------------------------------------


class SPSATerminationChecker:
    """Stop when |f_k - f_{k-1}| / f_{k-1} stayed below ``minimum_relative_change`` for
    ``allowed_consecutive_violations + 1`` consecutive accepted iterations, or when ``maxfev`` evaluations are reached
    (reference: queasars/utility/spsa_termination.py:9-134; held to sequences the reference's class itself answered,
    tests/golden/spsa_termination_reference.json).  One object may serve one optimisation after another: a call after it has
    said "stop", or with fewer evaluations than the call before, starts a new history."""

    def __init__(self, minimum_relative_change: float, allowed_consecutive_violations: int, maxfev: Optional[int] = None):
        self.minimum_relative_change = minimum_relative_change
        self.allowed_consecutive_violations = allowed_consecutive_violations
        self.maxfev = maxfev
        self._start_over()

    def _start_over(self) -> None:
        self.function_value_history: list[float] = []
        self.n_function_evaluation_history: list[int] = []
        self._changes: list[float] = []
        self.n_function_evaluations = 0
        self.best_function_value = float("inf")
        self._best_parameter_values = None
        self._done = False

    @property
    def best_parameter_values(self):
        if self._best_parameter_values is None:
            raise ValueError("The termination checker has stored no parameter values (no accepted step since its history began)!")
        return self._best_parameter_values

    def fresh(self) -> "SPSATerminationChecker":
        return SPSATerminationChecker(self.minimum_relative_change, self.allowed_consecutive_violations, self.maxfev)

    def termination_check(self, n_function_evaluations: int, parameter_values, function_value: float, step_size: float, accepted: bool) -> bool:
        if self._done or n_function_evaluations < self.n_function_evaluations:
            self._start_over()
        self.n_function_evaluations = n_function_evaluations
        if self.maxfev is not None and n_function_evaluations >= self.maxfev:
            return True
        if not accepted:
            return False
        self.function_value_history.append(function_value)
        self.n_function_evaluation_history.append(n_function_evaluations)
        if function_value < self.best_function_value:
            self.best_function_value = function_value
            self._best_parameter_values = parameter_values
        if len(self.function_value_history) < 2:
            return False
        previous = self.function_value_history[-2]
        self._changes.append(abs(function_value - previous) / previous)
        window = self.allowed_consecutive_violations + 1
        if len(self._changes) < window:
            return False
        if max(self._changes[-window:]) < self.minimum_relative_change:
            self._done = True
            return True
        return False


@dataclass
class SPSA:
    """First-order SPSA with constant gains (the configuration of examples/evqe_jssp_optimization.ipynb)."""

    maxiter: int = 33
    learning_rate: float = 0.43
    perturbation: float = 0.35
    trust_region: bool = True
    termination_checker: Optional[SPSATerminationChecker] = None

    @property
    def n_circuit_evaluations(self) -> int:
        return 2 * self.maxiter

    def new_run(self, x0: Sequence[float], seed: Optional[int]) -> "_SPSARun":
        return _SPSARun(self, x0, seed)


class _SPSARun:
    """State of one SPSA minimisation; the driver advances many of them in lock-step."""

    def __init__(self, config: SPSA, x0: Sequence[float], seed: Optional[int]):
        self.config = config
        self.x = np.asarray(x0, dtype=np.float64).copy()
        self.rng = np.random.default_rng(seed)
        self.checker = config.termination_checker.fresh() if config.termination_checker else None
        self.nfev = 0
        self.iteration = 0
        self.done = self.x.size == 0 or config.maxiter <= 0
        self._delta = None
        # (base vector, positions): the run's variables are entries `positions` of a longer parameter vector whose other
        # entries stay at `base` -- a layer of an individual inside the individual's fully parameterised circuit
        self.embed = None

    def propose(self) -> list[np.ndarray]:
        """The two points the next iteration evaluates."""
        self._delta = 1 - 2 * self.rng.binomial(1, 0.5, size=self.x.size)
        eps = self.config.perturbation
        return [self.x + eps * self._delta, self.x - eps * self._delta]

    def accept(self, f_plus: float, f_minus: float) -> None:
        cfg = self.config
        self.nfev += 2
        self.iteration += 1
        update = (f_plus - f_minus) / (2 * cfg.perturbation) * self._delta
        if cfg.trust_region:
            norm = float(np.linalg.norm(update))
            if norm > 1:
                update = update / norm
        update = update * cfg.learning_rate
        self.x = self.x - update
        stop = self.iteration >= cfg.maxiter
        if self.checker is not None and self.checker.termination_check(
            self.nfev, self.x, 0.5 * (f_plus + f_minus), float(np.linalg.norm(update)), True
        ):
            stop = True
        self.done = stop


@dataclass
class NFT:
    """Nakanishi-Fujii-Todo sequential minimisation (Phys. Rev. Research 2, 043158): with every other angle fixed, the
    expectation value is a sinusoid of period 2 pi in one gate angle, f(t) = c + a cos(t - b), so three values --
    f(t0), f(t0 + pi/2), f(t0 - pi/2) -- determine it and the parameter jumps to the exact minimiser t = b + pi.
    Parameters are visited cyclically; the fitted minimum c - a is reused as the next f(t0) and re-evaluated every
    ``reset_interval`` iterations.  This is the optimiser of the reference's own test harness
    (test/minimum_eigensolvers/evqe/solver.py:28-36: ``NFT(maxfev=40)``); restated from the paper, the reference takes
    it from qiskit-algorithms."""

    maxfev: int = 40
    maxiter: Optional[int] = None
    reset_interval: int = 32

    @property
    def n_circuit_evaluations(self) -> int:
        return self.maxfev

    def new_run(self, x0: Sequence[float], seed: Optional[int]) -> "_NFTRun":
        return _NFTRun(self, x0)


class _NFTRun:
    """State of one NFT minimisation, advanced in lock-step with the others like :class:`_SPSARun`."""

    def __init__(self, config: NFT, x0: Sequence[float]):
        self.config = config
        self.x = np.asarray(x0, dtype=np.float64).copy()
        self.nfev = 0
        self.iteration = 0
        self.done = self.x.size == 0 or config.maxfev <= 0
        self._recycled: Optional[float] = None
        self._needs_base = True
        self.embed = None  # (as _SPSARun.embed)

    def propose(self) -> list[np.ndarray]:
        cfg = self.config
        j = self.iteration % self.x.size
        if cfg.reset_interval > 0 and self.iteration % cfg.reset_interval == 0:
            self._recycled = None
        self._needs_base = self._recycled is None
        plus, minus = self.x.copy(), self.x.copy()
        plus[j] += 0.5 * math.pi
        minus[j] -= 0.5 * math.pi
        return ([self.x.copy()] if self._needs_base else []) + [plus, minus]

    def accept(self, *values: float) -> None:
        cfg = self.config
        self.nfev += len(values)
        z0 = values[0] if self._needs_base else self._recycled
        z1, z3 = values[-2], values[-1]
        j = self.iteration % self.x.size
        # f(t) = c + a cos(t - b):  z0 - c = a cos(t0 - b),  (z3 - z1) / 2 = a sin(t0 - b)
        c = 0.5 * (z1 + z3)
        cos_part, sin_part = z0 - c, 0.5 * (z3 - z1)
        a = math.hypot(cos_part, sin_part)
        if a > 0.0:
            self.x[j] = self.x[j] - math.atan2(sin_part, cos_part) + math.pi
        self._recycled = c - a
        self.iteration += 1
        self.done = self.nfev >= cfg.maxfev or (cfg.maxiter is not None and self.iteration >= cfg.maxiter)


@dataclass
class Adam:
    """Adam (Kingma and Ba, "Adam: A Method for Stochastic Optimization", ICLR 2015, algorithm 1) on the evaluator's analytic
    gradients (``evaluate_gradients``: parameter shift on the device).  Restated from the paper, in its notation: ``lr`` is
    alpha.  A run stops after ``maxiter`` iterations, or when the norm of an update falls below ``tol``.  Deterministic: the
    seed of ``new_run`` is not used.  An iteration costs the shifted evaluations of the run's free parameters (two per
    angle, four for theta of a cu3), which is what ``nfev`` and the solver's accounting count."""

    maxiter: int = 33
    lr: float = 0.1
    beta_1: float = 0.9
    beta_2: float = 0.999
    eps: float = 1e-8
    tol: float = 0.0

    #: a driver must hand these runs to ``evaluate_gradients`` (_minimize_batched)
    needs_gradients = True

    @property
    def n_circuit_evaluations(self) -> int:
        """Evaluations of one run when every free parameter takes two (the count depends on the searched layer:
        :meth:`n_circuit_evaluations_for`)."""
        return 2 * self.maxiter

    def n_circuit_evaluations_for(self, n_qubits: int) -> int:
        """Most evaluations of one layer search on ``n_qubits`` qubits, for the solver's budget: a layer has at most a rotation
        per qubit (three angles, two evaluations each) and a controlled rotation per pair of qubits (4 + 2 + 2)."""
        return self.maxiter * (6 * n_qubits + 8 * (n_qubits // 2))

    def new_run(self, x0: Sequence[float], seed: Optional[int]) -> "_AdamRun":
        return _AdamRun(self, x0)


class _AdamRun:
    """State of one Adam minimisation; the driver advances many of them in lock-step (:func:`_minimize_adam`)."""

    def __init__(self, config: Adam, x0: Sequence[float]):
        self.config = config
        self.x = np.asarray(x0, dtype=np.float64).copy()
        self.m = np.zeros_like(self.x)
        self.v = np.zeros_like(self.x)
        self.nfev = 0
        self.iteration = 0
        self.done = self.x.size == 0 or config.maxiter <= 0
        self.embed = None  # (as _SPSARun.embed)

    def accept_gradient(self, gradient: np.ndarray, n_evaluations: int) -> None:
        cfg = self.config
        g = np.asarray(gradient, dtype=np.float64)
        self.nfev += int(n_evaluations)
        self.iteration += 1
        t = self.iteration
        self.m = cfg.beta_1 * self.m + (1 - cfg.beta_1) * g
        self.v = cfg.beta_2 * self.v + (1 - cfg.beta_2) * (g * g)
        m_hat = self.m / (1 - cfg.beta_1**t)
        v_hat = self.v / (1 - cfg.beta_2**t)
        update = cfg.lr * m_hat / (np.sqrt(v_hat) + cfg.eps)
        self.x = self.x - update
        self.done = t >= cfg.maxiter or float(np.linalg.norm(update)) < cfg.tol


@dataclass
class NaturalGradient:
    """Quantum natural gradient descent (Stokes, Izaac, Killoran and Carleo, "Quantum Natural Gradient", Quantum 4, 269, 2020):
    ``x <- x - learning_rate * solve(G + regularization * I, g)`` with g the evaluator's analytic gradient
    (``evaluate_gradients``) and G the Fubini-Study metric of the run's free parameters (``metric_tensors``).
    ``regularization`` must be positive: G is singular wherever an angle does nothing to the state (lambda of a ``u`` on
    |0>).  A run stops after ``maxiter`` iterations, or when the norm of an update falls below ``tol``.  Deterministic: the
    seed of ``new_run`` is not used.  ``nfev`` counts what the gradient cost, as :class:`Adam`'s does; the metric call of an
    iteration is one more sweep per run and is not counted."""

    maxiter: int = 33
    learning_rate: float = 0.1
    regularization: float = 1e-3
    tol: float = 0.0

    #: a driver must hand these runs to ``evaluate_gradients`` and ``metric_tensors`` (_minimize_batched)
    needs_gradients = True
    needs_metric = True

    def __post_init__(self):
        if not self.regularization > 0:
            raise ValueError("regularization must be positive: the metric is singular wherever an angle does nothing")

    @property
    def n_circuit_evaluations(self) -> int:
        """As :attr:`Adam.n_circuit_evaluations`."""
        return 2 * self.maxiter

    def n_circuit_evaluations_for(self, n_qubits: int) -> int:
        """As :meth:`Adam.n_circuit_evaluations_for`: the gradient's shifted evaluations of the largest layer."""
        return self.maxiter * (6 * n_qubits + 8 * (n_qubits // 2))

    def new_run(self, x0: Sequence[float], seed: Optional[int]) -> "_NaturalGradientRun":
        return _NaturalGradientRun(self, x0)


class _NaturalGradientRun:
    """State of one natural-gradient minimisation; the driver advances many of them in lock-step
    (:func:`_minimize_natural_gradient`)."""

    def __init__(self, config: NaturalGradient, x0: Sequence[float]):
        self.config = config
        self.x = np.asarray(x0, dtype=np.float64).copy()
        self.nfev = 0
        self.iteration = 0
        self.done = self.x.size == 0 or config.maxiter <= 0
        self.embed = None  # (as _SPSARun.embed)

    def accept_gradient_and_metric(self, gradient: np.ndarray, metric: np.ndarray, n_evaluations: int) -> None:
        cfg = self.config
        g = np.asarray(gradient, dtype=np.float64)
        m = np.asarray(metric, dtype=np.float64)
        self.nfev += int(n_evaluations)
        self.iteration += 1
        update = cfg.learning_rate * np.linalg.solve(m + cfg.regularization * np.eye(g.size), g)
        self.x = self.x - update
        self.done = self.iteration >= cfg.maxiter or float(np.linalg.norm(update)) < cfg.tol


def _require_gradients(evaluator, optimizer) -> None:
    """An optimiser that needs gradients (:class:`Adam`) with an evaluator that has none: said before anything runs; likewise
    one that needs the metric (:class:`NaturalGradient`)."""
    if getattr(optimizer, "needs_gradients", False) and not callable(getattr(evaluator, "evaluate_gradients", None)):
        raise ValueError(f"{type(optimizer).__name__} needs an evaluator with evaluate_gradients (OperatorCircuitEvaluator); "
                         f"{type(evaluator).__name__} has none")
    if getattr(optimizer, "needs_metric", False) and not callable(getattr(evaluator, "metric_tensors", None)):
        raise ValueError(f"{type(optimizer).__name__} needs an evaluator with metric_tensors (a device evaluator); "
                         f"{type(evaluator).__name__} has none")


def _minimize_adam(evaluator, jobs: list) -> None:
    """:func:`_minimize_batched` for Adam runs: ONE ``evaluate_gradients`` call per iteration for all runs, each run
    differentiated by its free parameters only (the searched layer of an embedded run).  A run's ``nfev`` counts its shifted
    evaluations, by the circuit's shift plan; their sum is checked against what the evaluator reports.  An evaluator whose
    ``gradient_method`` is not "parameter_shift" reports each circuit's count itself (one for a circuit differentiated by the
    adjoint sweep)."""
    _require_gradients(evaluator, jobs[0][1].config)
    wrt, cost = {}, {}
    for circuit, run in jobs:
        positions = _positions(run).tolist()
        terms = circuit.gradient_terms()
        wrt[id(run)] = positions
        cost[id(run)] = sum(max(0, terms[p]) for p in positions)
    active = [job for job in jobs if not job[1].done]
    while active:
        circuits = [circuit for circuit, _ in active]
        params = [_full_point(run, run.x).tolist() for _, run in active]
        gradients = evaluator.evaluate_gradients(circuits, params, [wrt[id(run)] for _, run in active])
        if getattr(evaluator, "gradient_method", "parameter_shift") != "parameter_shift":
            # (the adjoint sweep, for all circuits or for those the evaluator chose: it says what each circuit's gradient cost)
            for (_, run), gradient, spent in zip(active, gradients, evaluator.last_gradient_evaluation_counts):
                run.accept_gradient(gradient, spent)
            active = [job for job in active if not job[1].done]
            continue
        counted = sum(cost[id(run)] for _, run in active)
        reported = getattr(evaluator, "last_gradient_evaluations", counted)
        if reported != counted:
            raise RuntimeError(f"the evaluator ran {reported} shifted evaluations, the shift plans say {counted}")
        for (_, run), gradient in zip(active, gradients):
            run.accept_gradient(gradient, cost[id(run)])
        active = [job for job in active if not job[1].done]


def _minimize_natural_gradient(evaluator, jobs: list) -> None:
    """:func:`_minimize_batched` for :class:`NaturalGradient` runs: ONE ``evaluate_gradients`` and ONE ``metric_tensors`` call
    per iteration for all running jobs, each run differentiated by its free parameters only.  ``nfev`` as in
    :func:`_minimize_adam`: the shift plans' counts, or what an evaluator with another ``gradient_method`` reports."""
    _require_gradients(evaluator, jobs[0][1].config)
    wrt, cost = {}, {}
    for circuit, run in jobs:
        positions = _positions(run).tolist()
        terms = circuit.gradient_terms()
        wrt[id(run)] = positions
        cost[id(run)] = sum(max(0, terms[p]) for p in positions)
    active = [job for job in jobs if not job[1].done]
    while active:
        circuits = [circuit for circuit, _ in active]
        params = [_full_point(run, run.x).tolist() for _, run in active]
        requested = [wrt[id(run)] for _, run in active]
        gradients = evaluator.evaluate_gradients(circuits, params, requested)
        if getattr(evaluator, "gradient_method", "parameter_shift") != "parameter_shift":
            spent = list(evaluator.last_gradient_evaluation_counts)
        else:
            spent = [cost[id(run)] for _, run in active]
        metrics = evaluator.metric_tensors(circuits, params, requested)
        for (_, run), gradient, metric, n in zip(active, gradients, metrics, spent):
            run.accept_gradient_and_metric(gradient, metric, n)
        active = [job for job in active if not job[1].done]


def _minimize_spsa_vectorised(evaluator, jobs: list) -> None:
    """:func:`_minimize_batched` for SPSA runs of one configuration, with the arithmetic of all runs in whole-array NumPy
    operations: as written per run (propose / accept of :class:`_SPSARun`: a binomial draw, two array expressions and two
    ``tolist`` per proposal, a dozen small NumPy calls per acceptance) an iteration of 64 runs costs 0.9 ms of Python around
    0.1 ms of GPU work.  Here every run's sign vectors are drawn once (the same draws, in the same order, as one call per
    iteration makes), the iterates live in one zero-padded matrix, and the evaluator receives rows of it (NumPy views: the
    packer copies them as buffers).  Every run still gets exactly the iterates its own ``propose`` / ``accept`` would have
    produced -- bit for bit: the same expressions element by element, the norm of an update taken over the run's own length
    (``tests/test_evqe_solver.py``)."""
    runs = [run for _, run in jobs]
    cfg = runs[0].config
    eps, lr = cfg.perturbation, cfg.learning_rate
    sizes = np.array([run.x.size for run in runs])
    width = int(sizes.max())
    n_runs = len(runs)
    x = np.zeros((n_runs, width))
    signs = np.zeros((n_runs, cfg.maxiter, width))
    for i, run in enumerate(runs):
        x[i, : sizes[i]] = run.x
        left = cfg.maxiter - run.iteration
        if left > 0 and sizes[i] > 0:  # (what propose() would draw call by call: one draw of the lot gives the same numbers)
            signs[i, run.iteration :, : sizes[i]] = 1 - 2 * run.rng.binomial(1, 0.5, size=(left, int(sizes[i])))
    iteration = np.array([run.iteration for run in runs])
    nfev = np.array([run.nfev for run in runs])
    any_checker = any(run.checker is not None for run in runs)
    active = np.array([i for i, run in enumerate(runs) if not run.done], dtype=np.int64)
    embedded = any(run.embed is not None for run in runs)
    if embedded:
        # (every run's variables are entries of a longer vector: the rows the evaluator gets are the runs' full vectors -- the
        # shared layout of device_search.py -- with the points scattered over the variables' own entries)
        packed = _PackedRuns(runs)
        full, full_sizes = packed.x_host, packed.lengths
    circuits_of = {}
    while active.size:
        key = active.tobytes()
        cached = circuits_of.get(key)
        if cached is None:  # (the same list object while the same runs are active: the evaluator's caches key on it)
            scatter = None
            if embedded:
                rows, cols, src = [], [], []
                for a, i in enumerate(active):
                    positions = packed.where[i]
                    rows.append(np.full(positions.size, 2 * a))
                    cols.append(positions)
                    src.append(np.arange(positions.size))
                scatter = (np.concatenate(rows), np.concatenate(cols), np.concatenate(src))
            lengths = full_sizes if embedded else sizes
            cached = circuits_of[key] = ([jobs[i][0] for i in active for _ in (0, 1)],
                                         [slice(0, int(lengths[i])) for i in active for _ in (0, 1)], scatter)
        circuits, cuts, scatter = cached
        delta = signs[active, iteration[active]]
        points = np.empty((2 * active.size, width))
        points[0::2] = x[active] + eps * delta
        points[1::2] = x[active] - eps * delta
        if embedded:
            rows, cols, src = scatter
            sent = np.repeat(full[active], 2, axis=0)
            sent[rows, cols] = points[rows, src]
            sent[rows + 1, cols] = points[rows + 1, src]
        else:
            sent = points
        values = np.asarray(evaluator.evaluate_circuits(circuits, [row[cut] for row, cut in zip(sent, cuts)]), dtype=np.float64)
        f_plus, f_minus = values[0::2], values[1::2]
        update = ((f_plus - f_minus) / (2 * eps))[:, None] * delta
        if cfg.trust_region:
            # (the exact norm -- the run's own sum, in its own order -- only where the update can be longer than 1 at all)
            for a in np.nonzero(np.einsum("ij,ij->i", update, update) > 0.999)[0]:
                row = update[a, : sizes[active[a]]]
                norm = math.sqrt(row.dot(row))  # (= numpy.linalg.norm of a real vector)
                if norm > 1:
                    update[a] = update[a] / norm
        update = update * lr
        x[active] = x[active] - update
        iteration[active] += 1
        nfev[active] += 2
        stop = iteration[active] >= cfg.maxiter
        if any_checker:
            for a, i in enumerate(active):
                run = runs[i]
                if run.checker is not None:
                    row = update[a, : sizes[i]]
                    if run.checker.termination_check(int(nfev[i]), x[i, : sizes[i]].copy(), 0.5 * (f_plus[a] + f_minus[a]),
                                                     float(math.sqrt(row.dot(row))), True):
                        stop[a] = True
        for i in active[stop]:
            runs[i].done = True
        active = active[~stop]
    for i, run in enumerate(runs):
        run.x = x[i, : sizes[i]].copy()
        run.iteration = int(iteration[i])
        run.nfev = int(nfev[i])


def _device_search_asked_for(evaluator, n_runs: int, flag: Optional[bool], opt_in: bool = False) -> bool:
    """What the configuration's ``device_resident_search`` (``flag``) and ``QSV_DEVICE_SEARCH`` say about a search of ``n_runs``
    runs, before anyone asks whether it can be done.  ``None`` is "where it pays" -- searches of at least
    ``_DEVICE_SEARCH_MIN_RUNS`` runs -- for an evaluator whose ``device_resident_search_by_default`` is true (the exact
    estimator), and the host driver for every other one (a sampling evaluator: the device search is opt-in there, so that runs
    configured before it existed keep their numbers).  ``opt_in``: ``None`` is the host driver whatever the evaluator (NFT
    searches, for the same reason).  The one place that resolves the default: ``_device_search_wanted``,
    which also decides whether layer searches embed their runs, and ``_minimize_batched`` both ask here."""
    env = os.environ.get("QSV_DEVICE_SEARCH")
    if env == "0":
        return False
    if flag is None:
        flag = (not opt_in and bool(getattr(evaluator, "device_resident_search_by_default", False))
                and n_runs >= _DEVICE_SEARCH_MIN_RUNS)
    return bool(flag) or env == "1"


# What can keep its state on the device (evqe/device_search.py), by run class: the optimiser's class; is ``None`` of the
# configuration's ``device_resident_search`` the host driver whatever the evaluator (opt-in: _device_search_asked_for)?; and the
# names in device_search of the rule before the runs exist, the rule over the runs, and the driver -- looked up when they are
# called (tests and measurements replace them).
_DEVICE_SEARCHES = {
    _SPSARun: (SPSA, False, "possible", "supported", "minimize_spsa_on_device"),
    _NFTRun: (NFT, True, "possible_nft", "supported_nft", "minimize_nft_on_device"),
    _AdamRun: (Adam, True, "possible_adam", "supported_adam", "minimize_adam_on_device"),
}


def _device_search_wanted(evaluator, n_runs: int, flag: Optional[bool], optimizer) -> bool:
    """Will a search of ``n_runs`` fresh runs of ``optimizer`` keep its state on the device?  What ``_minimize_batched`` will find,
    said before the runs exist: asked for, and possible by the device search's own rule."""
    for optimizer_class, opt_in, possible, _, _ in _DEVICE_SEARCHES.values():
        if isinstance(optimizer, optimizer_class):
            if optimizer_class is SPSA and os.environ.get("QSV_SCALAR_SPSA"):
                return False
            return (_device_search_asked_for(evaluator, n_runs, flag, opt_in)
                    and getattr(device_search, possible)(evaluator, optimizer, n_runs))
    return False


_DEVICE_SEARCH_MIN_RUNS = 16  # (config 4 on one MI355X: searches of 25 - 64 runs 1.5 x faster end to end, of 10 runs no faster)


def _searched_on_device(evaluator, waiting: list, on_device: Optional[bool]) -> bool:
    """Hand the unfinished jobs to their optimiser's device search, if there are several, all of one run class and one
    configuration, it is asked for and the search says it can take them; says whether that happened."""
    if len(waiting) < 2:
        return False
    first = waiting[0][1]
    entry = _DEVICE_SEARCHES.get(type(first))
    if entry is None or not all(type(job[1]) is type(first) and job[1].config is first.config for job in waiting):
        return False
    _, opt_in, _, supported, minimize = entry
    if not _device_search_asked_for(evaluator, len(waiting), on_device, opt_in):
        return False
    if not getattr(device_search, supported)(evaluator, waiting):
        return False
    getattr(device_search, minimize)(evaluator, waiting)
    return True


def _minimize_batched(evaluator, jobs: list, on_device: Optional[bool] = False) -> None:
    """Advance every (circuit, run) pair to completion; one evaluate_circuits call per optimiser iteration of the whole
    set (SPSA proposes two points per run and iteration, NFT two or three).  ``on_device``: SPSA runs whose evaluator can
    read points from and leave values in device memory keep their whole state there (evqe/device_search.py); fresh NFT runs of
    one configuration likewise, but only where asked for (``True`` or ``QSV_DEVICE_SEARCH=1``; ``None`` is the loop below), and
    so do fresh Adam runs of one configuration with an evaluator that has gradient plans (``None`` is :func:`_minimize_adam`)."""
    active = [job for job in jobs if not job[1].done]
    spsa = [] if os.environ.get("QSV_SCALAR_SPSA") else [job for job in active if isinstance(job[1], _SPSARun)]
    if len(spsa) > 1 and len(spsa) == len(active) and all(job[1].config is spsa[0][1].config for job in spsa):
        if not _searched_on_device(evaluator, spsa, on_device):
            _minimize_spsa_vectorised(evaluator, spsa)
        return
    if jobs and all(isinstance(job[1], _AdamRun) for job in jobs):
        if not _searched_on_device(evaluator, active, on_device):
            _minimize_adam(evaluator, jobs)
        return
    if jobs and all(isinstance(job[1], _NaturalGradientRun) for job in jobs):
        _minimize_natural_gradient(evaluator, jobs)  # (on the host: a device-resident form is not built)
        return
    if any(isinstance(job[1], (_AdamRun, _NaturalGradientRun)) for job in jobs):
        raise ValueError("Adam and NaturalGradient runs cannot share a search with runs of another optimiser")
    if active and isinstance(active[0][1], _NFTRun) and _searched_on_device(evaluator, active, on_device):
        return
    while active:
        circuits, params, counts = [], [], []
        for circuit, run in active:
            points = run.propose()
            counts.append(len(points))
            circuits += [circuit] * len(points)
            params += [_full_point(run, p).tolist() for p in points]
        values = evaluator.evaluate_circuits(circuits, params)
        cur = 0
        for (_, run), k in zip(active, counts):
            run.accept(*values[cur : cur + k])
            cur += k
        active = [job for job in active if not job[1].done]


# ---- configuration / result -----------------------------------------------------------------------------------


class BestIndividualRelativeChangeTolerance:
    def __init__(self, minimum_relative_change: float, allowed_consecutive_violations: int = 0):
        if minimum_relative_change <= 0 or minimum_relative_change > 1:
            raise ValueError("The minimum relative improvement parameter must not exceed the range )0,1)!")
        if allowed_consecutive_violations < 0:
            raise ValueError("allowed_consecutive_violations must be at least 0!")
        self._threshold = minimum_relative_change
        self._window = allowed_consecutive_violations + 1
        self.reset_state()

    def reset_state(self) -> None:
        self._previous: Optional[float] = None
        self._history: list[float] = []

    def check_termination(self, best_expectation_value_of_generation: float) -> bool:
        if self._previous is None:
            self._previous = best_expectation_value_of_generation
            return False
        self._history.append(abs(self._previous - best_expectation_value_of_generation) / abs(self._previous))
        self._previous = best_expectation_value_of_generation
        if len(self._history) < self._window:
            return False
        return max(self._history[-self._window :]) < self._threshold


@dataclass
class EVQEMinimumEigensolverConfiguration:
    """The solver knobs of queasars/minimum_eigensolvers/evqe/evqe.py:34-177 that do not concern primitives/executors."""

    optimizer: object  # SPSA, NFT or Adam: anything with new_run(x0, seed) and n_circuit_evaluations
    population_size: int
    max_generations: Optional[int] = None
    max_circuit_evaluations: Optional[int] = None
    termination_criterion: Optional[BestIndividualRelativeChangeTolerance] = None
    random_seed: Optional[int] = None
    n_initial_layers: int = 1
    randomize_initial_population_parameters: bool = False
    speciation_genetic_distance_threshold: int = 2
    use_tournament_selection: bool = False
    tournament_size: Optional[int] = None
    selection_alpha_penalty: float = 0.1
    selection_beta_penalty: float = 0.1
    parameter_search_probability: float = 0.24
    topological_search_probability: float = 0.2
    layer_removal_probability: float = 0.05
    # SPSA searches keep iterates, points and values in device memory and never wait for the GPU inside a search
    # (evqe/device_search.py; iterates agree with the host driver's to the last bits, not bit for bit; the same stopping
    # iterations).  None: where the evaluator can do it and a search has at least 16 runs -- for an evaluator that does not
    # sample (``device_resident_search_by_default``: the exact estimator); a sampler evaluator's searches stay with the host
    # driver under None, as before the device search could take them, and go to the device with True (or QSV_DEVICE_SEARCH=1).
    # False: never; True: whenever it can.
    # NFT searches have a device form too (qsv_nft_step: the whole schedule is known ahead, the host never looks at the device
    # inside a search) and are opt-in with EVERY evaluator: None keeps them on the host driver and their numbers as they were,
    # True (or QSV_DEVICE_SEARCH=1) sends them to the device.  Their accepts call the device's hypot / atan2, which in the flat
    # directions these searches are full of can turn an angle by pi without changing a value.
    device_resident_search: Optional[bool] = None
    # Layer searches of individuals whose circuits have no split form on the device (deep individuals: every evaluation is a few
    # passes over the 2^n state) keep the state in front of the searched layer on the device and evaluate from there
    # (mutation.py:57-59: only that layer's angles change) -- where the evaluator can (``keep_states``) and the circuit costs
    # say it pays.  None: yes; False: never (QSV_KEPT_STATES=0 / 1 overrides).
    kept_state_search: Optional[bool] = None
    # Layers drawn per individual that the topological search grows (evqe/growth.py): with k > 1 the layer whose
    # parameters have the largest gradient norm at zero angles is kept -- exact first-order numbers from ONE
    # ``evaluator.operator_density_matrices`` call per generation over all chosen parents; no candidate circuit is run and no
    # circuit evaluation is counted.  Candidate 0 is the layer that is drawn with 1, and the solver's random streams are consumed
    # as with 1.  1: every draw, circuit and result as without the option.
    growth_candidates: int = 1

    def __post_init__(self):
        if self.population_size < 1:
            raise ValueError("population_size must be at least 1!")
        if self.growth_candidates < 1:
            raise ValueError("growth_candidates must be at least 1!")
        if self.max_generations is None and self.max_circuit_evaluations is None and self.termination_criterion is None:
            raise ValueError("At least one of max_generations, max_circuit_evaluations or termination_criterion is needed!")
        if self.use_tournament_selection and (self.tournament_size is None or self.tournament_size < 1):
            raise ValueError("tournament_size cannot be None, if tournament selection should be used!")
        for name in ("parameter_search_probability", "topological_search_probability", "layer_removal_probability"):
            if not 0 <= getattr(self, name) <= 1:
                raise ValueError(f"{name} must be in the range [0, 1]!")


@dataclass
class EVQEResult:
    eigenvalue: float
    best_individual: EVQEIndividual
    generations: int
    circuit_evaluations: list[int]
    best_expectation_values: list[float] = field(default_factory=list)
    median_expectation_values: list[float] = field(default_factory=list)
    mean_expectation_values: list[float] = field(default_factory=list)
    # the aux operators' values at the best individual, a list or dict as they were given (None: none were given)
    aux_operators_evaluated: Optional[Union[list[float], dict[Any, float]]] = None
    # the most probable basis states of the best individual, bitstring (qubit 0 last) -> exact probability, most probable
    # first (None: not asked for), and -- under a diagonal operator -- bitstring -> the operator's value on it
    eigenstate: Optional[dict[str, float]] = None
    eigenstate_values: Optional[dict[str, float]] = None
    # <H^2> - <H>^2 of the evaluator's operator at the best individual: zero on an eigenstate (None: not asked for)
    eigenvalue_variance: Optional[float] = None
    # the aux operators' covariance matrix at the best individual, C_ab = <{O_a, O_b}> / 2 - <O_a><O_b>, an (M, M) array in the aux
    # operators' order (a dict's in list(aux_operators) order), and its diagonal, the variances, in the shape of
    # aux_operators_evaluated (None: not asked for)
    aux_operators_covariance: Optional[np.ndarray] = None
    aux_operators_variance: Optional[Union[list[float], dict[Any, float]]] = None
    # the subspace refinement over the best individual and the last scored generation (None: not asked for): the lowest
    # generalised eigenvalue of (H, S) over the picked states, its coefficients over them (c^H S c = 1), the number of
    # directions of S that were kept, and S itself, the picked states' overlap matrix as the device returned it, best individual first
    subspace_eigenvalue: Optional[float] = None
    subspace_coefficients: Optional[np.ndarray] = None
    subspace_rank: Optional[int] = None
    subspace_overlaps: Optional[np.ndarray] = None
    # the best individual's single-qubit entanglement entropies, (n_qubits,), and the mutual information between every two
    # qubits, (n_qubits, n_qubits), symmetric with a zero diagonal, both in bits (None: not asked for)
    qubit_entropies: Optional[np.ndarray] = None
    mutual_information: Optional[np.ndarray] = None
    # the Fubini-Study metric of ALL the best individual's parameters at its point, (P, P) in circuit order, and the number of its
    # eigenvalues above 1e-10 (fp64) or 1e-5 (fp32): how many directions of parameter space move the state (None: not asked for)
    parameter_metric: Optional[np.ndarray] = None
    parameter_metric_rank: Optional[int] = None
    # set by evqe.deflation.compute_eigenvalues (None from compute_minimum_eigenvalue itself): the deflated cost the run
    # minimised, E + sum_k beta_k |<phi_k|psi>|^2 at the best individual -- `eigenvalue` is then E alone --, and the best
    # individual's overlaps <phi_k|psi> with the states kept by the runs before it, complex, (number of runs before,)
    deflated_value: Optional[float] = None
    overlaps_with_previous: Optional[np.ndarray] = None
    # ... and, with keep=True, the best individual's state as it stays kept on the evaluator's device (a KeptState)
    kept_state: Optional[Any] = None


# ---- the solver -----------------------------------------------------------------------------------------------


class EVQEMinimumEigensolver:
    def __init__(self, configuration: EVQEMinimumEigensolverConfiguration, log: Optional[Callable[[str], None]] = None,
                 on_generation: Optional[Callable[[dict], None]] = None, shard: bool = False, process_group=None):
        """``on_generation``: called when a generation has been scored, with {"generation", "population", "values",
        "circuit_evaluations" (so far)}.  ``shard``: one process per GPU (torch.distributed initialised), every rank running
        this same solver with the same seed: the individuals' optimiser runs and the fitness evaluations are dealt to the ranks
        (the reference hands each to a worker of its pool, mutation.py:194-235, selection.py:75-85) and ONE all-gather per
        search / per scoring gives every rank all results, so that the evolution is the same everywhere."""
        self.configuration = configuration
        self._log = log or (lambda message: None)
        self._on_generation = on_generation
        self.shard = bool(shard)
        self.process_group = process_group
        # (QSV_SHARE_CIRCUITS=0: a circuit per individual and search, the other layers' values bound into it, as the reference has it)
        self.share_circuits = os.environ.get("QSV_SHARE_CIRCUITS", "1") != "0"
        rng = Random(configuration.random_seed)
        # one seed per consumer, drawn in the reference's order (evqe.py:188-229)
        self._population_seed = new_random_seed(rng)
        self._rng_last_layer = Random(new_random_seed(rng))
        self._rng_speciation = Random(new_random_seed(rng))
        self._rng_selection = Random(new_random_seed(rng))
        self._rng_parameter_search = Random(new_random_seed(rng))
        self._rng_topological = Random(new_random_seed(rng))
        self._rng_layer_removal = Random(new_random_seed(rng))
        # per grown individual of the last topological search with growth_candidates > 1: (kept candidate, every candidate's norm)
        self.last_growth_scores: list = []

    # -- mutation helpers -----------------------------------------------------------------------------------
    @staticmethod
    def _chosen(population: EVQEPopulation, rng: Random, probability: float) -> dict[int, int]:
        """index -> seed of the individuals an operator mutates (mutation.py:206-216)."""
        chosen = {}
        for i in range(len(population.individuals)):
            if rng.random() <= probability:
                chosen[i] = new_random_seed(rng)
        return chosen

    def _optimize_layers(self, evaluator, individuals: list[EVQEIndividual], layer_ids: list[int], seeds: list[int]):
        """optimize_layer_of_individual (mutation.py:28-89) for many individuals at once."""
        # The reference binds every other layer's values into the circuit (a new circuit per individual, layer and search:
        # get_partially_parameterized_quantum_circuit).  Here the search runs on the individual's FULLY parameterised circuit --
        # one shared object per structure, registered once --, the other layers' values travelling as parameter values that
        # do not move: the same matrices, gate for gate, hence the same numbers (tests hold the two forms to equality).
        # (Where the points are packed on the host -- small searches, evaluators that sample -- the wider rows cost more than the
        # registrations they save, measured on config 4's sampler branch: there the circuits are bound as the reference binds them.)
        embed = self.share_circuits and _device_search_wanted(evaluator, len(individuals), self.configuration.device_resident_search,
                                                              self.configuration.optimizer)
        if os.environ.get("QSV_SHARE_CIRCUITS") == "2":  # (measurements, tests: embedded also where the host packs the points)
            embed = True
        jobs = []
        for k, (individual, layer_id, seed) in enumerate(zip(individuals, layer_ids, seeds)):
            run = self.configuration.optimizer.new_run(individual.get_layer_parameter_values(layer_id), seed)
            if embed:
                circuit = individual.get_parameterized_quantum_circuit(shared=True)
                # (positions and the other layers' values in the CIRCUIT's parameter order -- name-sorted blocks, which is
                # the layer order only up to ten layers: layer10_ sorts before layer2_)
                layer = layer_id % len(individual.layers)
                start = individual.circuit_parameter_offsets[layer]
                positions = np.arange(start, start + individual.layers[layer].n_parameters, dtype=np.int64)
                run.embed = (np.asarray(individual.parameter_values_in_circuit_order(), dtype=np.float64), positions)
            else:
                circuit = individual.get_partially_parameterized_quantum_circuit({layer_id})
            jobs.append((circuit, run))
        # several ranks: each runs the searches of ITS individuals (dealt by what their circuits cost), one all-gather at the end
        mine = None
        if self.shard:
            from queasars_amd import distributed

            mine = distributed.shard_searches(evaluator, jobs, self.process_group)
        own = list(range(len(jobs))) if mine is None else list(mine)
        # deep individuals of this rank: from a kept state (the searched layer and what follows it: the layer's own parameters)
        kept = self._kept_state_circuits(evaluator, [individuals[j] for j in own], [layer_ids[j] for j in own])
        for position, circuit in kept.items():
            j = own[position]
            jobs[j][1].embed = None
            jobs[j] = (circuit, jobs[j][1])
        _minimize_batched(evaluator, [jobs[j] for j in own], on_device=self.configuration.device_resident_search)
        if kept:  # (nothing may hold the search's circuits any longer: their kept states are a 2^n-amplitude buffer each)
            evaluator.forget_circuits()
        if mine is not None:
            distributed.gather_search_results(jobs, mine, self.process_group)  # (the share itself: it knows the longest one's length)
        out, nfev = [], 0
        for individual, layer_id, (_, run) in zip(individuals, layer_ids, jobs):
            out.append(EVQEIndividual.change_layer_parameter_values(individual, layer_id, tuple(run.x.tolist())))
            nfev += run.nfev
        return out, nfev

    def _kept_state_circuits(self, evaluator, individuals: list[EVQEIndividual], layer_ids: list[int]) -> dict:
        """position -> the circuit a layer search evaluates from a KEPT state: for individuals whose whole circuit takes gate
        passes over the 2^n state on the evaluator's device (no split form: deep individuals), the state in front of the
        searched layer is computed once, kept resident, and every evaluation of the search applies only the searched layer and
        what follows it (reference: the layers in front are bound and never change, mutation.py:57-59).  Taken where the
        evaluator reports fewer, cheaper passes for it (last-layer searches of deep individuals: 1.5 - 1.8 x at 20 / 24
        qubits and eight layers, profiles/r04_prefix_reuse.txt); a search in the middle of a deep circuit keeps its whole
        circuit (the same number of passes either way).  The values agree with the whole circuit's to rounding (1e-14), not
        bit for bit."""
        flag = self.configuration.kept_state_search
        env = os.environ.get("QSV_KEPT_STATES")
        if env == "0" or (flag is False and env != "1") or not hasattr(evaluator, "keep_states") or not hasattr(evaluator, "circuit_costs"):
            return {}
        force = env == "1" or flag is True  # (asked for: taken wherever the rest of the circuit is cheaper than the whole)
        candidates = [k for k, (ind, layer) in enumerate(zip(individuals, layer_ids)) if layer % len(ind.layers) > 0]
        if not candidates:
            return {}
        whole = [individuals[k].get_parameterized_quantum_circuit(shared=True) for k in candidates]
        first = evaluator.circuit_costs(whole[:1])[0]
        if first["route"] == "one tile":  # (a register of one tile: nothing to save)
            return {}
        costs = [first] + evaluator.circuit_costs(whole[1:])
        # Worth it?  A kept state costs about one and a half whole evaluations (the circuit in front run once, its state copied)
        # plus the registration of the rest; every evaluation of the search then saves (whole - rest) microseconds.  A search
        # makes at most n_circuit_evaluations of them -- about a third of that where a termination checker ends runs early
        # (measured on the benchmark's trajectory: 22 of 66).  The rest's cost is estimated from its layers: the passes of the
        # whole circuit scale with its depth, a single last layer takes two.
        optimizer = self.configuration.optimizer
        expected = float(optimizer.n_circuit_evaluations)
        if getattr(optimizer, "termination_checker", None) is not None:
            expected /= 3.0
        deep = []
        for k, c in zip(candidates, costs):
            if c["route"] != "gate passes":
                continue
            n_layers = len(individuals[k].layers)
            rest_layers = n_layers - layer_ids[k] % n_layers
            rest_passes = max(2.0, c["n_passes"] * rest_layers / n_layers + 1.0)
            per_pass = c["microseconds"] / max(1, c["n_passes"])
            saving = c["microseconds"] - 1.1 * per_pass * rest_passes
            if force or saving * expected > 1.5 * c["microseconds"] + 60.0:
                deep.append((k, c))
        if not deep:
            return {}
        fronts = [individuals[k].get_layer_search_state_circuit(layer_ids[k]) for k, _ in deep]
        states = evaluator.keep_states([circuit for circuit, _ in fronts], [list(values) for _, values in fronts])
        circuits = [individuals[k].get_layer_search_circuits(layer_ids[k])[1].continue_from(state) for (k, _), state in zip(deep, states)]
        out = {}
        for (k, cost), circuit, kept_cost in zip(deep, circuits, evaluator.circuit_costs(circuits)):
            if kept_cost["microseconds"] < 0.9 * cost["microseconds"]:
                out[k] = circuit
        return out

    def _last_layer_search(self, evaluator, population: EVQEPopulation) -> tuple[EVQEPopulation, int]:
        chosen = self._chosen(population, self._rng_last_layer, 1.0)
        idx = sorted(chosen)
        new, nfev = self._optimize_layers(evaluator, [population.individuals[i] for i in idx], [-1] * len(idx), [chosen[i] for i in idx])
        individuals = list(population.individuals)
        for i, ind in zip(idx, new):
            individuals[i] = ind
        return EVQEPopulation(tuple(individuals), population.species_representatives, None, None), nfev

    def _parameter_search(self, evaluator, population: EVQEPopulation) -> tuple[EVQEPopulation, int]:
        """optimize_all_parameters_of_individual (mutation.py:92-132): layers in a random order, one at a time; the
        j-th layer of every chosen individual is optimised in the same batch."""
        chosen = self._chosen(population, self._rng_parameter_search, self.configuration.parameter_search_probability)
        state = {}
        for i, seed in chosen.items():
            randomizer = Random(seed)
            state[i] = [population.individuals[i], list(range(len(population.individuals[i].layers))), randomizer]
        total = 0
        while any(todo for _, todo, _ in state.values()):
            batch = [i for i, (_, todo, _) in state.items() if todo]
            layers, seeds = [], []
            for i in batch:
                _, todo, randomizer = state[i]
                layer = randomizer.choice(todo)
                todo.remove(layer)
                layers.append(layer)
                seeds.append(new_random_seed(randomizer))
            new, nfev = self._optimize_layers(evaluator, [state[i][0] for i in batch], layers, seeds)
            total += nfev
            for i, ind in zip(batch, new):
                state[i][0] = ind
        individuals = list(population.individuals)
        for i, (ind, _, _) in state.items():
            individuals[i] = ind
        return EVQEPopulation(tuple(individuals), population.species_representatives, None, None), total

    def _topological_search(self, population: EVQEPopulation, evaluator=None) -> EVQEPopulation:
        chosen = self._chosen(population, self._rng_topological, self.configuration.topological_search_probability)
        individuals = list(population.individuals)
        candidates = self.configuration.growth_candidates
        if candidates > 1 and not callable(getattr(evaluator, "operator_density_matrices", None)):
            raise ValueError("growth_candidates > 1 needs an evaluator with operator_density_matrices (an operator evaluator)")
        if candidates > 1 and chosen:
            grown = self._grow_by_gradient(evaluator, [individuals[i] for i in chosen], list(chosen.values()), candidates)
            for i, individual in zip(chosen, grown):
                individuals[i] = individual
        else:
            for i, seed in chosen.items():
                individuals[i] = EVQEIndividual.add_random_layers(individuals[i], 1, False, random_seed=seed)
        return EVQEPopulation(tuple(individuals), population.species_representatives, None, None)

    def _grow_by_gradient(self, evaluator, parents: list[EVQEIndividual], seeds: list[int], candidates: int) -> list[EVQEIndividual]:
        """One new layer per parent, at zero angles: of `candidates` layers drawn against the parent's last layer, the one whose
        parameters have the largest gradient norm at identity (evqe/growth.py); the lowest index wins a tie, candidate 0 --
        the layer ``add_random_layers`` draws from the same seed -- when all norms are zero.  One device call for all parents."""
        from queasars_amd.evqe.growth import appended_gate_gradients, layer_gradient

        circuits = [parent.get_parameterized_quantum_circuit(shared=self.share_circuits) for parent in parents]
        u, cu3 = appended_gate_gradients(evaluator, circuits, [list(parent.parameter_values) for parent in parents])
        grown, self.last_growth_scores = [], []
        for e, (parent, seed) in enumerate(zip(parents, seeds)):
            local = Random(seed)  # (its first draw is add_random_layers' own)
            layers = [EVQECircuitLayer.random_layer(n_qubits=parent.n_qubits, random_seed=new_random_seed(local), previous_layer=parent.layers[-1])
                      for _ in range(candidates)]
            norms = [float(np.linalg.norm(layer_gradient(layer, u[e], cu3[e]))) for layer in layers]
            best = max(range(candidates), key=lambda c: (norms[c], -c))
            self.last_growth_scores.append((best, norms))
            layer = layers[best]
            grown.append(EVQEIndividual(parent.n_qubits, (*parent.layers, layer), (*parent.parameter_values, *((0,) * layer.n_parameters))))
        return grown

    def _layer_removal(self, population: EVQEPopulation) -> EVQEPopulation:
        chosen = self._chosen(population, self._rng_layer_removal, self.configuration.layer_removal_probability)
        individuals = list(population.individuals)
        for i, seed in chosen.items():
            ind = individuals[i]
            if len(ind.layers) > 1:
                individuals[i] = EVQEIndividual.remove_layers(ind, Random(seed).randrange(1, len(ind.layers)))
        return EVQEPopulation(tuple(individuals), population.species_representatives, None, None)

    # -- speciation / selection -----------------------------------------------------------------------------
    def _speciation(self, population: EVQEPopulation) -> EVQEPopulation:
        threshold = self.configuration.speciation_genetic_distance_threshold
        representatives = list(population.species_representatives or [])
        members: dict[EVQEIndividual, list[int]] = {rep: [] for rep in representatives}
        if 0 < threshold <= 1:
            # A genetic distance below one is zero: the same number of layers and every layer equal (individual.py:217-237), and
            # an equal individual has equal layers too -- the first representative with the individual's layers, found by
            # hashing instead of by comparing with every representative in turn (36 k distance calls per run of the
            # benchmark's trajectory, a sixth of the driver's time; the notebooks' threshold is 1).
            first = {}
            for rep in representatives:
                first.setdefault(rep.layers, rep)
            for i, individual in enumerate(population.individuals):
                rep = first.get(individual.layers)
                if rep is None:
                    representatives.append(individual)
                    members[individual] = [i]
                    first[individual.layers] = individual
                else:
                    members[rep].append(i)
        else:
            for i, individual in enumerate(population.individuals):
                for rep in representatives:
                    if EVQEIndividual.get_genetic_distance(individual, rep) < threshold or individual == rep:
                        members[rep].append(i)
                        break
                else:
                    representatives.append(individual)
                    members[individual] = [i]
        new_members: dict[EVQEIndividual, list[int]] = {}
        for group in members.values():
            if not group:
                continue
            representative = population.individuals[self._rng_speciation.choice(group)]
            new_members.setdefault(representative, []).extend(group)
        membership = {i: rep for rep, group in new_members.items() for i in group}
        return EVQEPopulation(population.individuals, list(new_members), new_members, membership)

    def _selection(self, population: EVQEPopulation, values: list[float]) -> EVQEPopulation:
        cfg = self.configuration
        rng = self._rng_selection
        n = len(population.individuals)
        species_size = [float(len(population.species_members[population.species_membership[i]])) for i in range(n)]
        penalties = [
            cfg.selection_alpha_penalty * len(ind.layers) + cfg.selection_beta_penalty * ind.get_n_controlled_gates()
            for ind in population.individuals
        ]
        if not cfg.use_tournament_selection:
            best = min(values)
            offset = -best + 1 if best <= 0 else 0
            fitness = [(values[i] + offset + penalties[i]) * species_size[i] for i in range(n)]
            selected = rng.choices(population.individuals, weights=[1 / (f + offset) for f in fitness], k=n)
        else:
            fitness = [(values[i] + penalties[i]) * species_size[i] for i in range(n)]
            selected = []
            while len(selected) < n:
                contenders = rng.choices(range(n), k=cfg.tournament_size)
                winner = min(contenders, key=lambda j: (fitness[j], contenders.index(j)))
                selected.append(population.individuals[winner])
        return EVQEPopulation(tuple(selected), population.species_representatives, None, None)

    # -- main loop ------------------------------------------------------------------------------------------
    def compute_minimum_eigenvalue(self, evaluator, search_evaluator=None, aux_operators=None,
                                   eigenstate_states: Optional[int] = None, eigenvalue_variance: bool = False,
                                   aux_operators_covariance: bool = False, subspace_states: Optional[int] = None,
                                   subspace_rcond: Optional[float] = None, qubit_correlations: bool = False,
                                   parameter_metric: bool = False) -> EVQEResult:
        """``search_evaluator``: a second evaluator of the SAME operator for the parameter searches alone -- a single-precision
        handle: the points a search compares differ by far more than 1e-6 (the reference's own tests run their searches on an
        estimator with precision 0.05, test/minimum_eigensolvers/evqe/solver.py:20-27), a layer search on kept states is bound
        by the bytes of the state, and fp32 halves them (bench.py layer_search: 227 k against 160 k evaluations per second at
        seven layers, 170 k against 107 k at eight).  Every individual's FITNESS, what selection and the result see, comes from
        ``evaluator``.

        ``aux_operators``: a list or dict of PauliOperator, evaluated once after the run at the best individual by
        ``evaluator.evaluate_observables`` (reference: evolving_ansatz_minimum_eigensolver.py:177-199, :461-476); the values go
        to ``result.aux_operators_evaluated`` in the same shape.  They use no random stream of the solver and are not counted
        in ``circuit_evaluations``.  (A sampling evaluator draws its samples with its own generator, after the run, as the
        reference's aux sampler evaluators do.)  In a sharded run every rank evaluates them itself.

        ``eigenstate_states``: how many of the best individual's most probable basis states to read out after the run, in one
        ``top_states`` call on the evaluator's ``statevector_device`` -- exact probabilities, selected on the device
        (reference: the distribution measured for ``result.eigenstate``, evolving_ansatz_minimum_eigensolver.py:442-454, of
        which users decode the most probable states).  They go to ``result.eigenstate`` (bitstring -> probability, most
        probable first) and, when the evaluator's operator is diagonal, their values to ``result.eigenstate_values``.  Like the
        aux operators the call uses no random stream of the solver, is not counted in ``circuit_evaluations`` and is made by
        every rank of a sharded run itself.  ``None``: no call, both stay ``None``.

        ``eigenvalue_variance``: after the run, one ``evaluator.evaluate_variances`` call at the best individual; the operator's
        variance there, ``<H^2> - <H>^2`` (zero on an eigenstate; for a diagonal cost the spread over the individual's
        distribution), goes to ``result.eigenvalue_variance``.  The same rules: no random stream of the solver, not counted in
        ``circuit_evaluations``, made by every rank of a sharded run itself.  ``False``: no call, the field stays ``None``.

        ``aux_operators_covariance``: after the run, one ``evaluator.evaluate_covariances`` call at the best individual with the
        aux operators; their covariance matrix there goes to ``result.aux_operators_covariance`` (an (M, M) array in the aux
        operators' order, a dict's in ``list(aux_operators)`` order) and its diagonal, the variances, to
        ``result.aux_operators_variance`` in the shape of ``aux_operators_evaluated``.  With the cost's parts as aux operators
        ``w @ C @ w`` is the variance of any re-weighting of them.  The same rules as ``eigenvalue_variance``.  ``False``: no
        call, both fields stay ``None``.

        ``subspace_states``: after the run, diagonalise the operator in the span of up to that many (at most 64) states the run
        already has -- the best individual first, then the individuals of the last scored generation in ascending value, one
        that repeats an earlier pick's structure and parameter values skipped -- from one
        ``evaluator.evaluate_subspace_matrices`` call: S_ij = <psi_i|psi_j> and H_ij = <psi_i|H|psi_j> on the device (DESIGN.md
        4.15).  The lowest generalised eigenvalue of (H, S) (``evqe.subspace.lowest_subspace_eigenvalue``) goes to
        ``result.subspace_eigenvalue``: a variational upper bound that is never above ``result.eigenvalue`` beyond rounding,
        for no new circuit and no optimiser step.  Its coefficients over the picked states, the number of directions of S that
        were kept and S itself go to ``result.subspace_coefficients``, ``subspace_rank`` and ``subspace_overlaps``.
        ``subspace_rcond``: directions of S with eigenvalues below that times the largest are dropped; ``None`` means 1e-8 on
        an fp64 evaluator (entries of S carry up to 1e-11, so eigenvalues of a 64 x 64 S below about 6e-10 are noise: ten times
        that) and 1e-4 on an fp32 one (entries to about 2e-6, by the same argument).  The eigenvalue's error grows as (entry
        error) * sum_k|c_k| / s_min_kept, c_k the operator's coefficients and s_min_kept the smallest kept eigenvalue of S.  The
        same rules as ``eigenvalue_variance``: no random stream of the solver, not counted in ``circuit_evaluations``, made by
        every rank of a sharded run itself.  ``None``: no call, the four fields stay ``None``.

        ``qubit_correlations``: after the run, one ``evaluator.reduced_density_matrices`` call at the best individual over all
        single qubits and pairs; every qubit's entanglement entropy with the rest goes to
        ``result.qubit_entropies`` and the mutual information between every two qubits to ``result.mutual_information``, both
        in bits (``queasars_amd.entanglement``): where the evolved entanglers act, and whether the state is a basis state.
        The same rules as ``eigenvalue_variance``.  ``False``: no call, both fields stay ``None``.

        ``parameter_metric``: after the run, one ``evaluator.metric_tensors`` call at the best individual; the
        Fubini-Study metric of all its parameters, in the circuit's parameter order, goes to ``result.parameter_metric`` and
        the number of its eigenvalues above 1e-10 (1e-5 on an fp32 evaluator) to ``result.parameter_metric_rank``: how many
        directions of the individual's parameter space change the state at all.  The same rules as ``eigenvalue_variance``.
        ``False``: no call, both fields stay ``None``."""
        cfg = self.configuration
        if cfg is not None and cfg.growth_candidates > 1 and not callable(getattr(evaluator, "operator_density_matrices", None)):
            raise ValueError("growth_candidates > 1 needs an evaluator with operator_density_matrices (an operator evaluator)")
        searcher = evaluator if search_evaluator is None else search_evaluator
        if searcher.n_qubits != evaluator.n_qubits:
            raise ValueError("the search evaluator must be over the same register")
        if aux_operators is not None:
            if not callable(getattr(evaluator, "evaluate_observables", None)):
                raise ValueError("aux_operators need an evaluator with evaluate_observables (an operator evaluator)")
            for op in (aux_operators.values() if isinstance(aux_operators, dict) else aux_operators):
                if op.num_qubits != evaluator.n_qubits:
                    raise ValueError(f"an aux operator acts on {op.num_qubits} qubits, the evaluator on {evaluator.n_qubits}")
        if eigenstate_states is not None and getattr(evaluator, "statevector_device", None) is None:
            raise ValueError("eigenstate_states needs an evaluator with a statevector_device (a device evaluator)")
        if eigenvalue_variance and not callable(getattr(evaluator, "evaluate_variances", None)):
            raise ValueError("eigenvalue_variance needs an evaluator with evaluate_variances (an operator evaluator)")
        if aux_operators_covariance:
            if aux_operators is None or len(aux_operators) == 0:
                raise ValueError("aux_operators_covariance needs aux_operators")
            if not callable(getattr(evaluator, "evaluate_covariances", None)):
                raise ValueError("aux_operators_covariance needs an evaluator with evaluate_covariances (an operator evaluator)")
        if qubit_correlations and not callable(getattr(evaluator, "reduced_density_matrices", None)):
            raise ValueError("qubit_correlations needs an evaluator with reduced_density_matrices (an operator evaluator)")
        if parameter_metric and not callable(getattr(evaluator, "metric_tensors", None)):
            raise ValueError("parameter_metric needs an evaluator with metric_tensors (a device evaluator)")
        if subspace_states is not None:
            if not 1 <= int(subspace_states) <= 64:
                raise ValueError("subspace_states must be between 1 and 64")
            if not callable(getattr(evaluator, "evaluate_subspace_matrices", None)):
                raise ValueError("subspace_states needs an evaluator with evaluate_subspace_matrices (an operator evaluator)")
            if subspace_rcond is not None and not subspace_rcond > 0:
                raise ValueError("subspace_rcond must be positive")
        elif subspace_rcond is not None:
            raise ValueError("subspace_rcond needs subspace_states")
        last_scored: Optional[tuple] = None  # (individuals, values) of the last scored generation
        if cfg.termination_criterion is not None:
            cfg.termination_criterion.reset_state()
        population = EVQEPopulation.random_population(
            evaluator.n_qubits, cfg.n_initial_layers, cfg.population_size, cfg.randomize_initial_population_parameters,
            random_seed=self._population_seed,
        )
        evaluations: list[int] = [0]
        result = EVQEResult(eigenvalue=math.inf, best_individual=population.individuals[0], generations=0, circuit_evaluations=evaluations)
        _require_gradients(searcher, cfg.optimizer)
        n_opt = cfg.optimizer.n_circuit_evaluations
        if hasattr(cfg.optimizer, "n_circuit_evaluations_for"):  # (an optimiser whose cost depends on the register: Adam)
            n_opt = cfg.optimizer.n_circuit_evaluations_for(evaluator.n_qubits)

        def budget_left(expected: int) -> bool:
            if cfg.max_circuit_evaluations is None:
                return True
            used = sum(evaluations)
            return used < cfg.max_circuit_evaluations and used + expected < cfg.max_circuit_evaluations

        while True:
            if cfg.max_generations is not None and result.generations >= cfg.max_generations:
                break
            # 1. last-layer parameter search on everyone
            if not budget_left(len(population.individuals) * n_opt):
                break
            population, nfev = self._last_layer_search(searcher, population)
            evaluations[-1] += nfev
            # 2. speciation, 3. selection (this is where a generation is scored)
            population = self._speciation(population)
            if not budget_left(len(population.individuals)):
                break
            circuits = [ind.get_parameterized_quantum_circuit(shared=self.share_circuits) for ind in population.individuals]
            if self.shard:
                from queasars_amd.distributed import evaluate_population_sharded

                values = evaluate_population_sharded(evaluator, circuits, [list(ind.parameter_values) for ind in population.individuals],
                                                     group=self.process_group)
            else:
                values = evaluator.evaluate_circuits(circuits, [list(ind.parameter_values) for ind in population.individuals])
            evaluations[-1] += len(values)
            if subspace_states is not None:
                last_scored = (tuple(population.individuals), [float(v) for v in values])
            best = int(np.argmin(values))
            if values[best] < result.eigenvalue:
                result.eigenvalue, result.best_individual = values[best], population.individuals[best]
            result.best_expectation_values.append(values[best])
            result.median_expectation_values.append(median(values))
            result.mean_expectation_values.append(mean(values))
            self._log(f"generation {result.generations}: best {values[best]:.6f} median {median(values):.6f} mean {mean(values):.6f}")
            if self._on_generation is not None:
                self._on_generation({"generation": result.generations, "population": population, "values": list(values),
                                     "circuit_evaluations": sum(evaluations)})
            result.generations += 1
            evaluations.append(0)
            terminate = cfg.termination_criterion is not None and cfg.termination_criterion.check_termination(values[best])
            population = self._selection(population, values)
            if terminate or (cfg.max_generations is not None and result.generations >= cfg.max_generations):
                break
            # 4. full parameter search, 5. growth, 6. pruning
            expected = math.ceil(cfg.parameter_search_probability * sum(len(i.layers) for i in population.individuals) * n_opt)
            if not budget_left(expected):
                break
            population, nfev = self._parameter_search(searcher, population)
            evaluations[-1] += nfev
            population = self._topological_search(population, evaluator)
            population = self._layer_removal(population)
        if evaluations and evaluations[-1] == 0 and len(evaluations) > 1:
            evaluations.pop()
        if aux_operators is not None:
            result.aux_operators_evaluated = self._evaluate_aux_operators(evaluator, result.best_individual, aux_operators)
        if eigenstate_states is not None:
            result.eigenstate, result.eigenstate_values = self._read_eigenstate(evaluator, result.best_individual, eigenstate_states)
        if eigenvalue_variance:
            best = result.best_individual
            circuit = best.get_parameterized_quantum_circuit(shared=self.share_circuits)
            result.eigenvalue_variance = float(evaluator.evaluate_variances([circuit], [list(best.parameter_values)])[0])
        if aux_operators_covariance:
            best = result.best_individual
            names = list(aux_operators) if isinstance(aux_operators, dict) else None
            operators = [aux_operators[k] for k in names] if names is not None else list(aux_operators)
            circuit = best.get_parameterized_quantum_circuit(shared=self.share_circuits)
            matrix = np.array(evaluator.evaluate_covariances([circuit], [list(best.parameter_values)], operators)[0], dtype=np.float64)
            variances = [float(v) for v in np.diagonal(matrix)]
            result.aux_operators_covariance = matrix
            result.aux_operators_variance = dict(zip(names, variances)) if names is not None else variances
        if subspace_states is not None:
            self._refine_in_subspace(evaluator, result, last_scored, int(subspace_states), subspace_rcond)
        if qubit_correlations:
            from queasars_amd.entanglement import mutual_information

            best = result.best_individual
            circuit = best.get_parameterized_quantum_circuit(shared=self.share_circuits)
            entropies, information = mutual_information(evaluator, [circuit], [list(best.parameter_values)], with_entropies=True)
            result.qubit_entropies, result.mutual_information = entropies[0], information[0]
        if parameter_metric:
            best = result.best_individual
            circuit = best.get_parameterized_quantum_circuit(shared=self.share_circuits)
            metric = np.array(evaluator.metric_tensors([circuit], [list(best.parameter_values)])[0], dtype=np.float64)
            device = getattr(evaluator, "statevector_device", None)
            floor = 1e-5 if getattr(device, "dtype", "fp64") == "fp32" else 1e-10
            result.parameter_metric = metric
            result.parameter_metric_rank = int((np.linalg.eigvalsh(metric) > floor).sum()) if metric.size else 0
        return result

    def _refine_in_subspace(self, evaluator, result: EVQEResult, last_scored, k: int, rcond: Optional[float]) -> None:
        """The subspace fields of ``result``: picks the states, one ``evaluate_subspace_matrices`` call, the host's
        diagonalisation."""
        from queasars_amd.evqe.subspace import lowest_subspace_eigenvalue

        picks = [result.best_individual]
        if last_scored is not None:
            individuals, values = last_scored
            picks += [individuals[i] for i in sorted(range(len(values)), key=lambda i: (values[i], i))]
        chosen: list[EVQEIndividual] = []
        seen = set()
        for individual in picks:
            key = (individual.layers, tuple(float(v) for v in individual.parameter_values))
            if key in seen:
                continue
            seen.add(key)
            chosen.append(individual)
            if len(chosen) == k:
                break
        if rcond is None:
            device = getattr(evaluator, "statevector_device", None)
            rcond = 1e-4 if getattr(device, "dtype", "fp64") == "fp32" else 1e-8
        circuits = [ind.get_parameterized_quantum_circuit(shared=self.share_circuits) for ind in chosen]
        overlaps, elements = evaluator.evaluate_subspace_matrices(circuits, [list(ind.parameter_values) for ind in chosen])
        overlaps = np.asarray(overlaps, dtype=np.complex128)
        eigenvalue, coefficients, rank, _ = lowest_subspace_eigenvalue(overlaps, elements, rcond)
        result.subspace_eigenvalue = eigenvalue
        result.subspace_coefficients = coefficients
        result.subspace_rank = rank
        result.subspace_overlaps = overlaps

    def _read_eigenstate(self, evaluator, individual: EVQEIndividual, k: int):
        """The ``k`` most probable basis states of ``individual`` and, where the evaluator knows them, their values: one
        ``top_states`` call -- the evaluator's own (behind its initial state, with its operator's values) where it has one,
        else its device's."""
        circuit = individual.get_parameterized_quantum_circuit(shared=self.share_circuits)
        read = getattr(evaluator, "top_states", None)
        if not callable(read):
            read = evaluator.statevector_device.top_states
        states, probabilities, values = read([circuit], [list(individual.parameter_values)], int(k))
        names = [format(int(s), f"0{evaluator.n_qubits}b") for s in states[0]]
        eigenstate = {name: float(p) for name, p in zip(names, probabilities[0])}
        return eigenstate, None if values is None else {name: float(v) for name, v in zip(names, values[0])}

    def _evaluate_aux_operators(self, evaluator, individual: EVQEIndividual, aux_operators):
        """The aux operators' values at ``individual``, one call of ``evaluator.evaluate_observables``."""
        names = list(aux_operators) if isinstance(aux_operators, dict) else None
        operators = [aux_operators[k] for k in names] if names is not None else list(aux_operators)
        if not operators:
            return {} if names is not None else []
        circuit = individual.get_parameterized_quantum_circuit(shared=self.share_circuits)
        values = [float(v) for v in evaluator.evaluate_observables([circuit], [list(individual.parameter_values)], operators)[0]]
        return dict(zip(names, values)) if names is not None else values
