"""Lock-step parameter searches of a population with their state ON THE DEVICE: SPSA, NFT and Adam.

The host drivers (``solver._minimize_batched``, ``_minimize_spsa_vectorised``, ``_minimize_adam``) keep every run's iterate in
host memory: an iteration builds the points in NumPy, hands them to the evaluator (packing, PCIe), waits for the values and
updates the iterates -- and the GPU idles while the host does its share (SPSA: 8.0 ms per search of 64 individuals at 20 qubits,
of which the device is busy for 3).  Here iterates, points and values are tensors in device memory, the evaluator reads the
points where they are and leaves its results where the optimiser's step reads them, and everything of an iteration is queued on
ONE HIP stream without the host waiting for any of it.  What the three drivers share is written once:

* the LAYOUT (:class:`_PackedRuns`, :func:`_full_point`): one row per run, the run's whole parameter vector -- its own ``x``, or
  (``run.embed``: a layer inside the individual's fully parameterised circuit) the base vector with ``x`` at the layer's
  positions --, zero-padded to the widest; ``columns`` says where in its row each run's variables are;
* the STREAM (:func:`_on_search_stream`): the one the evaluator's handle launches on, ordered after the caller's on entry and
  before it on exit -- or, for a library that works in host memory (the host tests' emulations), no stream at all;
* the RULE that sends a search here, in two parts: what ``(evaluator, configuration, number of runs)`` decide
  (:func:`possible`, :func:`possible_nft`, :func:`possible_adam` -- ``solver._device_search_wanted`` asks these before the runs
  exist, to decide whether layer searches embed their runs) and what only the runs can say (fresh runs of one configuration
  object: :func:`supported`, :func:`supported_nft`, :func:`supported_adam`, which ask both).

SPSA (:func:`minimize_spsa_on_device`, ``qsv_spsa_step``).  Arithmetic: element by element the expressions of
``_SPSARun.propose`` / ``accept`` (reference: qiskit_algorithms' SPSA with constant gains as the notebook configures it,
mutation.py:63-75 for the batched callback), in the same order; the one difference is the trust region's norm, summed by the
device in its own order, so an iterate can differ from the host driver's in the last bits (tests hold the two to 1e-9 and to the
same stopping iterations).  The termination rule is the reference's ``SPSATerminationChecker``
(queasars/utility/spsa_termination.py:46-94) as array operations; the runs' host-side checker objects are not fed (nothing reads
them afterwards).  The host looks at the device every few iterations only to see whether every run has stopped.  Runs that have
stopped stay in the batch with their updates masked -- taking them out would mean waiting for the device --, and are not
counted: ``nfev`` is two per iteration a run was active, as on the host.  An evaluator whose ``evaluate_device_to_device`` takes
a mask (the sampler evaluator) is handed the runs' ``active`` flags, so that the two evaluations of a stopped run cost a dispatch
and nothing else.  With a sampling evaluator (``sampler_shots`` given) every iteration draws one seed from the evaluator's
generator, as an ``evaluate_circuits`` call of the host driver does -- also the up to ``look_every - 1`` iterations queued after
the last run has stopped and before the host has looked: the generator then stands further on than after the same search on the
host.

NFT (:func:`minimize_nft_on_device`, ``qsv_nft_step``) is simpler: fresh runs of one configuration move in perfect lock-step,
the host knows every iteration's form and the last iteration before it starts (:func:`nft_schedule`), and it never looks at the
device inside a search.

Adam (:func:`minimize_adam_on_device`, ``qsv_adam_step``) differentiates instead of evaluating: one gradient plan per search
(``OperatorCircuitEvaluator.gradient_plan``; include/qsv.h, GRADIENT PLANS), whose runs follow each other on the stream with one
step launch between them.  The step's arithmetic is ``_AdamRun.accept_gradient``'s, bit for bit.
"""

from __future__ import annotations

import contextlib

import numpy as np


_MAX_SIGN_BYTES = 256 << 20


# ---- the layout ---------------------------------------------------------------------------------------------------------------


def _positions(run) -> np.ndarray:
    """Where in its parameter vector (:func:`_full_point`) a run's variables are."""
    return np.arange(run.x.size) if run.embed is None else run.embed[1]


def _row_length(run) -> int:
    return run.x.size if run.embed is None else run.embed[0].size


def _full_point(run, point: np.ndarray) -> np.ndarray:
    """The parameter vector the evaluator gets for a run's point: the point itself, or (``run.embed = (base, positions)``: the
    run's variables are entries of a longer vector whose other entries do not move) the base vector with the point at the
    positions."""
    if run.embed is None:
        return point
    base, positions = run.embed
    full = base.copy()
    full[positions] = point
    return full


class _PackedRuns:
    """Runs laid out as one zero-padded matrix: row i of ``x_host`` (``n_runs`` x ``width``) is ``_full_point(run, run.x)``, of
    which ``lengths[i]`` entries are the run's and ``sizes[i]`` are searched, at the columns ``where[i]`` -- which are also the
    first ``sizes[i]`` entries of row i of ``columns_host`` (``n_runs`` x ``stride``, int32: what the step kernels index with).
    Entries of a row that are not searched travel into every point untouched."""

    def __init__(self, runs):
        self.runs = runs
        self.where = [_positions(run) for run in runs]
        self.lengths = np.array([_row_length(run) for run in runs])
        self.sizes = np.array([run.x.size for run in runs], dtype=np.int32)
        self.n_runs, self.width, self.stride = len(runs), int(self.lengths.max()), int(self.sizes.max())
        self.x_host = np.zeros((self.n_runs, self.width))
        self.columns_host = np.zeros((self.n_runs, self.stride), dtype=np.int32)
        for i, run in enumerate(runs):
            self.x_host[i, : self.lengths[i]] = _full_point(run, run.x)
            self.columns_host[i, : self.sizes[i]] = self.where[i]

    def draw_signs(self, n_iter: int) -> np.ndarray:
        """Every run's SPSA sign vectors of the next ``n_iter`` iterations from the run's own generator -- what ``propose()``
        would draw call by call: one draw of the lot gives the same numbers --, zero where a row is not searched (x +- eps * 0
        leaves those entries where they are, the update is zero there and the norm does not see them).  As bytes,
        ``(n_iter, n_runs, width)``: an eighth of the transfer, which was a tenth of a short search."""
        signs = np.zeros((n_iter, self.n_runs, self.width), dtype=np.int8)
        for i, run in enumerate(self.runs):
            signs[:, i, self.where[i]] = 1 - 2 * run.rng.binomial(1, 0.5, size=(n_iter, run.x.size))
        return signs

    def write_back(self, x_final: np.ndarray) -> None:
        """The inverse: every run's ``x`` from its row of ``x_final``."""
        for i, run in enumerate(self.runs):
            run.x = x_final[i, self.where[i]].copy()


# ---- the stream ---------------------------------------------------------------------------------------------------------------


@contextlib.contextmanager
def _on_search_stream(evaluator):
    """Inside: torch's current stream is the one the evaluator's handle launches on, which has been told to wait for the
    caller's; on the way out -- also when the body raises -- the caller's stream is told to wait for it.  Yields the torch
    device to allocate on.  Nothing here waits on the host.  A statevector device without ``device_index`` is a library that
    works in host memory -- the NumPy emulations of the step contracts that the host tests drive the searches with: the same
    tensors, pointers and calls, on the CPU and without a stream."""
    import torch

    index = evaluator.statevector_device.device_index
    if index is None:
        yield torch.device("cpu")
        return
    from queasars_amd.distributed import _chain_state

    device = torch.device("cuda", index)
    stream = _chain_state(evaluator, device)["stream"]
    caller = torch.cuda.current_stream(device)
    stream.wait_stream(caller)
    try:
        with torch.cuda.stream(stream):
            yield device
    finally:
        caller.wait_stream(stream)


# ---- the rule -----------------------------------------------------------------------------------------------------------------


def _evaluator_can(evaluator, n_runs: int, method: str) -> bool:
    """At least two runs, and an evaluator that has ``method`` and says its device can hold a search."""
    return n_runs >= 2 and callable(getattr(evaluator, method, None)) and bool(evaluator.device_resident_search_possible())


def possible(evaluator, config, n_runs: int) -> bool:
    """Could :func:`minimize_spsa_on_device` take ``n_runs`` fresh runs of ``config``, as far as anyone can say before they exist?
    An evaluator that reads points from and leaves values in device memory (the exact estimator; the sampler evaluator with the
    exact distribution or up to 4096 shots) on a GPU, something to do, and no termination rule or the one the device implements.
    (The one thing :func:`supported` may still refuse such runs for is the size of their sign vectors.)"""
    checker = config.termination_checker
    # (by name: solver.py imports this module, and a class object from there would close the circle)
    return (_evaluator_can(evaluator, n_runs, "evaluate_device_to_device") and config.maxiter > 0
            and (checker is None or type(checker).__name__ == "SPSATerminationChecker"))


def possible_nft(evaluator, config, n_runs: int) -> bool:
    """:func:`possible` for :func:`minimize_nft_on_device`: the same evaluators, a schedule that is not empty."""
    return _evaluator_can(evaluator, n_runs, "evaluate_device_to_device") and len(nft_schedule(config)[0]) > 0


def possible_adam(evaluator, config, n_runs: int) -> bool:
    """:func:`possible` for :func:`minimize_adam_on_device`: an evaluator with gradient plans, on a GPU, whose gradients are
    parameter shift (a gradient plan is a parameter-shift plan: an evaluator told to differentiate by the adjoint sweep, or to
    choose per circuit, runs the host driver)."""
    if getattr(evaluator, "gradient_method", "parameter_shift") != "parameter_shift":
        return False
    return _evaluator_can(evaluator, n_runs, "gradient_plan") and int(config.maxiter) > 0


def _in_lock_step(runs, run_class) -> bool:
    """What only the runs can say: every one a ``run_class`` of ONE configuration object with something to search, unfinished and
    at the same iteration as the others."""
    if not runs or not all(isinstance(run, run_class) for run in runs):
        return False
    cfg, first = runs[0].config, runs[0].iteration
    return not any(run.config is not cfg or run.iteration != first or run.done or run.x.size < 1 for run in runs)


def supported(evaluator, jobs) -> bool:
    """Can :func:`minimize_spsa_on_device` take these jobs?  :func:`possible`, and fresh SPSA runs of one configuration."""
    from queasars_amd.evqe.solver import _SPSARun

    runs = [run for _, run in jobs]
    if not _in_lock_step(runs, _SPSARun) or any(run.iteration != 0 or run.nfev != 0 for run in runs):
        return False
    cfg = runs[0].config
    # (the sign vectors of every iteration are drawn ahead, as float64 rows of the widest run's width -- on the host and again on
    # the device: long optimisations of many deep individuals with embedded parameter vectors would be hundreds of megabytes;
    # beyond a quarter of a gigabyte the host driver, which draws them iteration by iteration, takes the search)
    width = max(_row_length(run) for run in runs)
    if int(cfg.maxiter) * len(runs) * width * 8 > _MAX_SIGN_BYTES:  # (as doubles on the device; bytes on the host)
        return False
    return possible(evaluator, cfg, len(runs))


def minimize_spsa_on_device(evaluator, jobs, look_every: int = 8) -> None:
    """One launch per iteration for the optimiser's share (``qsv_spsa_step``: accept iteration k, propose iteration k + 1) and
    one chain for the evaluation, which is all this function asks of the evaluator (``evaluate_device_to_device``; where that
    method takes ``active`` it gets the runs' flags, two evaluations per entry).  The iterations queued between the last run's
    stop and the host's next look (``look_every``) also advance a sampling evaluator's generator.  ``QSV_DEVICE_SEARCH_TORCH=1``: the same arithmetic as a few dozen torch operations per
    iteration (:func:`_minimize_with_torch_operations`; the tests hold the two against each other)."""
    import ctypes as C
    import os

    import torch

    from queasars_amd import _lib

    if os.environ.get("QSV_DEVICE_SEARCH_TORCH") == "1":
        return _minimize_with_torch_operations(evaluator, jobs, look_every)
    pack = _PackedRuns([run for _, run in jobs])
    cfg = pack.runs[0].config
    n_iter, n_runs, width = int(cfg.maxiter), pack.n_runs, pack.width
    signs_host = pack.draw_signs(n_iter)
    circuits = [circuit for circuit, _ in jobs for _ in (0, 1)]
    checker = cfg.termination_checker
    window = checker.allowed_consecutive_violations + 1 if checker is not None else 0

    dev = evaluator.statevector_device
    lib, handle = dev._lib, dev._handle
    takes_mask = _takes_mask(evaluator)
    with _on_search_stream(evaluator) as device:
        x = torch.from_numpy(pack.x_host).to(device)
        signs = torch.from_numpy(signs_host).to(device).to(torch.float64)  # (bytes on the way, doubles on the device)
        points = torch.empty((2 * n_runs, width), dtype=torch.float64, device=device)
        values = torch.empty(2 * n_runs, dtype=torch.float64, device=device)
        active = torch.ones(n_runs, dtype=torch.uint8, device=device)
        iterations = torch.zeros(n_runs, dtype=torch.int64, device=device)
        previous = torch.zeros(n_runs, dtype=torch.float64, device=device)
        n_values = torch.zeros(n_runs, dtype=torch.int64, device=device)
        changes = torch.full((n_runs, max(window, 1)), float("inf"), dtype=torch.float64, device=device)
        args = _lib.QsvSpsaStepArgs(
            n_runs=n_runs, width=width, x=x.data_ptr(), active=active.data_ptr(), iterations=iterations.data_ptr(),
            delta_accept=None, values=None, delta_propose=None, points=points.data_ptr(), eps=cfg.perturbation,
            lr=cfg.learning_rate, trust_region=int(bool(cfg.trust_region)), maxiter=n_iter, window=window, reserved=0,
            min_rel=checker.minimum_relative_change if checker is not None else 0.0,
            maxfev=checker.maxfev if checker is not None and checker.maxfev is not None else -1,
            previous=previous.data_ptr(), n_values=n_values.data_ptr(), changes=changes.data_ptr())
        base, stride = signs.data_ptr(), n_runs * width * 8
        for k in range(n_iter + 1):
            # accept iteration k - 1 (its values are in `values`), propose iteration k
            args.delta_accept = base + (k - 1) * stride if k > 0 else None
            args.values = values.data_ptr() if k > 0 else None
            args.delta_propose = base + k * stride if k < n_iter else None
            dev._check(lib.qsv_spsa_step(handle, C.byref(args)))
            if k == n_iter:
                break
            if k > 0 and k % look_every == 0 and not bool(active.any()):
                break
            if takes_mask:
                evaluator.evaluate_device_to_device(circuits, points, values, active=active, active_stride=2)
            else:
                evaluator.evaluate_device_to_device(circuits, points, values)
        x_final = x.cpu().numpy()
        done_iterations = iterations.cpu().numpy()
    _spsa_write_back(pack, x_final, done_iterations)


def _spsa_write_back(pack: _PackedRuns, x_final, done_iterations) -> None:
    pack.write_back(x_final)
    for i, run in enumerate(pack.runs):
        run.iteration = int(done_iterations[i])
        run.nfev = 2 * int(done_iterations[i])
        run.done = True


def nft_schedule(config) -> tuple[list[bool], int]:
    """What fresh NFT runs of ``config`` will do, known before any value is: per iteration whether the base point is evaluated
    (three values per run) or the fitted minimum of the iteration before stands in for it (two), and the evaluations one run
    has made when it stops.  ``_NFTRun.propose`` / ``accept`` restated without a run: the base at iteration 0 and at every
    multiple of a positive ``reset_interval``; the stopping rule -- ``nfev >= maxfev`` or ``iteration >= maxiter`` -- is looked
    at after an accept, so ``NFT(maxfev=40)`` runs 20 iterations and 41 evaluations.  No function value enters: every fresh
    run of one configuration has this schedule, whatever its size.  Needs no device."""
    flags: list[bool] = []
    nfev = 0
    if config.maxfev <= 0:
        return flags, nfev
    while True:
        iteration = len(flags)
        with_base = iteration == 0 or (config.reset_interval > 0 and iteration % config.reset_interval == 0)
        flags.append(with_base)
        nfev += 3 if with_base else 2
        if nfev >= config.maxfev or (config.maxiter is not None and iteration + 1 >= config.maxiter):
            return flags, nfev


def supported_nft(evaluator, jobs) -> bool:
    """Can :func:`minimize_nft_on_device` take these jobs?  An evaluator that reads points from and leaves values in device
    memory, on a GPU; at least two runs, every one a fresh NFT run of one configuration object with something to search."""
    from queasars_amd.evqe.solver import _NFTRun

    runs = [run for _, run in jobs]
    if not _in_lock_step(runs, _NFTRun) or any(run.iteration != 0 or run.nfev != 0 for run in runs):
        return False
    return possible_nft(evaluator, runs[0].config, len(runs))


def minimize_nft_on_device(evaluator, jobs, state: dict | None = None) -> None:
    """The lock-step NFT search of fresh runs of one configuration with its whole state in device memory: iterates, the
    fitted minima that stand in for base values, points and function values are tensors on the stream of the evaluator's
    handle.  The host knows the whole schedule ahead (:func:`nft_schedule`), so it queues, per iteration, one ``qsv_nft_step``
    launch (accept iteration k - 1, propose iteration k) and one ``evaluate_device_to_device`` -- of the three-per-run circuit
    list where the base is evaluated, of the two-per-run list and the first 2 R rows otherwise, the same two list objects
    throughout -- and looks at the device once, at the end, for ``x`` and the fitted minima.  Nothing in the loop waits (the
    library does where it lays a batch out afresh: when the list changes).

    Given the same ``x`` and values, a proposal is bit for bit ``_NFTRun.propose``'s; an accept calls the device's ``hypot``
    and ``atan2``, so an updated coordinate and the fitted minimum can differ from the host's in the last bits -- and in a flat
    direction, where the fitted amplitude is rounding noise, a last bit decides an angle: whole searches are not comparable
    with the host driver's iterate by iterate.

    With a sampling evaluator every iteration draws exactly one seed from the evaluator's generator, as one
    ``evaluate_circuits`` call of the host driver does, and nothing is queued beyond the schedule: after the search the
    generator stands exactly where the host driver leaves it.

    ``state``: a dictionary that receives the search's tensors (``x``, ``recycled``, ``points``, ``values``) before the first
    iteration is queued -- for tests and measurements that look at an iteration from inside the evaluator."""
    import ctypes as C

    import torch

    from queasars_amd import _lib

    pack = _PackedRuns([run for _, run in jobs])
    with_base, nfev = nft_schedule(pack.runs[0].config)
    n_iter, n_runs, width = len(with_base), pack.n_runs, pack.width
    # (the same two list objects call after call: the evaluators key their caches on identity)
    three = [circuit for circuit, _ in jobs for _ in (0, 1, 2)]
    two = [circuit for circuit, _ in jobs for _ in (0, 1)]

    dev = evaluator.statevector_device
    lib, handle = dev._lib, dev._handle
    with _on_search_stream(evaluator) as device:
        x = torch.from_numpy(pack.x_host).to(device)
        sizes = torch.from_numpy(pack.sizes).to(device)
        columns = torch.from_numpy(pack.columns_host).to(device)
        recycled = torch.zeros(n_runs, dtype=torch.float64, device=device)
        points = torch.empty((3 * n_runs, width), dtype=torch.float64, device=device)
        values = torch.empty(3 * n_runs, dtype=torch.float64, device=device)
        points_two, values_two = points[: 2 * n_runs], values[: 2 * n_runs]
        if state is not None:
            state.update(x=x, recycled=recycled, points=points, values=values)
        args = _lib.QsvNftStepArgs(
            n_runs=n_runs, width=width, columns_stride=pack.stride, reserved=0, x=x.data_ptr(), sizes=sizes.data_ptr(),
            columns=columns.data_ptr(), recycled=recycled.data_ptr(), values=values.data_ptr(), points=points.data_ptr())
        for k in range(n_iter + 1):
            # accept iteration k - 1 (its values are in `values`), propose iteration k
            args.accept, args.accept_iteration, args.accept_with_base = int(k > 0), max(k - 1, 0), int(k > 0 and with_base[k - 1])
            args.propose, args.propose_iteration, args.propose_with_base = int(k < n_iter), k, int(k < n_iter and with_base[k])
            dev._check(lib.qsv_nft_step(handle, C.byref(args)))
            if k == n_iter:
                break
            if with_base[k]:
                evaluator.evaluate_device_to_device(three, points, values)
            else:
                evaluator.evaluate_device_to_device(two, points_two, values_two)
        x_final = x.cpu().numpy()
        recycled_final = recycled.cpu().numpy()
    pack.write_back(x_final)
    for i, run in enumerate(pack.runs):
        run.iteration = n_iter
        run.nfev = nfev
        run._recycled = float(recycled_final[i])
        run._needs_base = with_base[-1]
        run.done = True


def supported_adam(evaluator, jobs) -> bool:
    """Can :func:`minimize_adam_on_device` take these jobs?  An evaluator with gradient plans, on a GPU; at least two runs, every
    one an Adam run of one configuration object that has something to search, stands at the same iteration as the others and
    has not moved yet (``m`` and ``v`` zero: the device starts its moments there)."""
    from queasars_amd.evqe.solver import _AdamRun

    runs = [run for _, run in jobs]
    if not _in_lock_step(runs, _AdamRun) or any(np.any(run.m) or np.any(run.v) for run in runs):
        return False
    cfg = runs[0].config
    return int(cfg.maxiter) > runs[0].iteration and possible_adam(evaluator, cfg, len(runs))


def minimize_adam_on_device(evaluator, jobs, look_every: int = 8, state: dict | None = None) -> None:
    """The lock-step Adam search of fresh runs of one configuration with its whole state in device memory: iterates, moments,
    gradients, iteration counts and ``active`` flags are tensors on the stream of the evaluator's handle.  ONE gradient plan
    for the search -- every run differentiated by its free parameters only, ``run.embed``'s positions or all of them --, and
    per iteration one run of the plan and one ``qsv_adam_step`` launch, neither of which waits: with ``tol == 0`` every run
    makes ``maxiter`` iterations, so all of them are queued at once and the host looks at the device once, for ``x``, the
    moments and the counts.  With ``tol > 0`` it queues ``look_every`` iterations, reads ``active`` and goes on while a run is
    left.  A run that has stopped keeps its bits -- the step leaves it alone -- but is STILL DIFFERENTIATED until the search
    ends (taking it out of the plan would mean a new plan and a wait); its ``nfev`` counts the iterations it was active for.

    Afterwards every run's ``x``, ``m``, ``v``, ``iteration``, ``done`` and ``nfev`` are what ``solver._minimize_adam`` leaves,
    bit for bit: the gradients are the same (plans against ``qsv_gradient_device``), and the step rounds every product,
    quotient, square root and sum as NumPy does.  The one number formed differently is the norm of the update behind ``tol``
    (summed in ascending order; NumPy's ``dot`` has its own): a run whose norm lies within rounding of ``tol`` may stop an
    iteration apart.  The shifted evaluations one run of the plan queues are checked against the circuits' shift plans, as
    ``_minimize_adam`` checks what the evaluator reports.

    ``state``: a dictionary that receives the search's tensors and the plan before the first iteration is queued."""
    import ctypes as C

    import torch

    from queasars_amd import _lib

    pack = _PackedRuns([run for _, run in jobs])
    runs, n_runs, stride = pack.runs, pack.n_runs, pack.stride
    cfg = runs[0].config
    first = int(runs[0].iteration)
    n_iter = int(cfg.maxiter) - first
    circuits = [circuit for circuit, _ in jobs]
    wrt = [[int(p) for p in positions] for positions in pack.where]  # (the gradient is taken by exactly the searched entries)
    cost = []
    for circuit, positions in zip(circuits, wrt):
        terms = circuit.gradient_terms()
        cost.append(sum(max(0, terms[p]) for p in positions))

    dev = evaluator.statevector_device
    lib, handle = dev._lib, dev._handle
    with _on_search_stream(evaluator) as device:
        x = torch.from_numpy(pack.x_host).to(device)
        sizes = torch.from_numpy(pack.sizes).to(device)
        columns = torch.from_numpy(pack.columns_host).to(device)
        m = torch.zeros((n_runs, stride), dtype=torch.float64, device=device)
        v = torch.zeros((n_runs, stride), dtype=torch.float64, device=device)
        gradient = torch.zeros((n_runs, stride), dtype=torch.float64, device=device)
        active = torch.ones(n_runs, dtype=torch.uint8, device=device)
        iterations = torch.full((n_runs,), first, dtype=torch.int64, device=device)
        plan = evaluator.gradient_plan(circuits, x, gradient, wrt)
        try:
            if plan.n_shifted != sum(cost):
                raise RuntimeError(f"the gradient plan runs {plan.n_shifted} shifted evaluations, the shift plans say {sum(cost)}")
            if state is not None:
                state.update(x=x, m=m, v=v, gradient=gradient, active=active, iterations=iterations, plan=plan)
            args = _lib.QsvAdamStepArgs(
                n_runs=n_runs, width=pack.width, columns_stride=stride, grad_width=stride, x=x.data_ptr(), sizes=sizes.data_ptr(),
                columns=columns.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), gradient=gradient.data_ptr(), active=active.data_ptr(),
                iterations=iterations.data_ptr(), lr=cfg.lr, beta_1=cfg.beta_1, beta_2=cfg.beta_2,
                one_minus_beta_1=1 - cfg.beta_1, one_minus_beta_2=1 - cfg.beta_2, eps=cfg.eps, tol=cfg.tol, maxiter=int(cfg.maxiter))
            for k in range(n_iter):
                t = first + k + 1
                plan.run(x, gradient)
                args.bias_1, args.bias_2 = 1 - cfg.beta_1**t, 1 - cfg.beta_2**t
                dev._check(lib.qsv_adam_step(handle, C.byref(args)))
                if cfg.tol > 0 and (k + 1) % look_every == 0 and k + 1 < n_iter and not bool(active.any()):
                    break
            x_final, m_final, v_final = x.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
            done_iterations = iterations.cpu().numpy()
        finally:
            plan.close()
    pack.write_back(x_final)
    for i, run in enumerate(runs):
        size = int(pack.sizes[i])
        run.m = m_final[i, :size].copy()
        run.v = v_final[i, :size].copy()
        run.nfev += (int(done_iterations[i]) - first) * cost[i]
        run.iteration = int(done_iterations[i])
        run.done = True


def _takes_mask(evaluator) -> bool:
    """Does the evaluator's ``evaluate_device_to_device`` accept the runs' ``active`` flags?  (``QSV_DEVICE_SEARCH_MASK=0``: do
    not hand them over -- the measurement of what the mask saves.)"""
    import inspect
    import os

    if os.environ.get("QSV_DEVICE_SEARCH_MASK") == "0":
        return False
    try:
        return "active" in inspect.signature(evaluator.evaluate_device_to_device).parameters
    except (TypeError, ValueError):
        return False


def _minimize_with_torch_operations(evaluator, jobs, look_every: int = 8) -> None:
    import torch

    pack = _PackedRuns([run for _, run in jobs])
    cfg = pack.runs[0].config
    eps, lr, n_iter = cfg.perturbation, cfg.learning_rate, int(cfg.maxiter)
    n_runs, width = pack.n_runs, pack.width
    signs_host = pack.draw_signs(n_iter)
    circuits = [circuit for circuit, _ in jobs for _ in (0, 1)]
    checker = cfg.termination_checker
    window = checker.allowed_consecutive_violations + 1 if checker is not None else 0

    with _on_search_stream(evaluator) as device:
        x = torch.from_numpy(pack.x_host).to(device)
        signs = torch.from_numpy(signs_host).to(device).to(torch.float64)
        points = torch.empty((2 * n_runs, width), dtype=torch.float64, device=device)
        values = torch.empty(2 * n_runs, dtype=torch.float64, device=device)
        active = torch.ones(n_runs, dtype=torch.bool, device=device)
        iterations = torch.zeros(n_runs, dtype=torch.int64, device=device)
        one = torch.ones(n_runs, dtype=torch.float64, device=device)
        if checker is not None:
            previous = torch.zeros(n_runs, dtype=torch.float64, device=device)
            n_values = torch.zeros(n_runs, dtype=torch.int64, device=device)
            # the last `window` relative changes of every run, oldest first; +inf = not there yet
            changes = torch.full((n_runs, window), float("inf"), dtype=torch.float64, device=device)
        for k in range(n_iter):
            delta = signs[k]
            shift = delta * eps
            torch.add(x, shift, out=points[0::2])
            torch.sub(x, shift, out=points[1::2])
            evaluator.evaluate_device_to_device(circuits, points, values)
            f_plus, f_minus = values[0::2], values[1::2]
            update = ((f_plus - f_minus) / (2 * eps))[:, None] * delta
            if cfg.trust_region:
                norm = torch.sqrt((update * update).sum(dim=1))
                update = update / torch.where(norm > 1, norm, one)[:, None]
            update = update * lr
            x = x - update * active[:, None]
            iterations = iterations + active
            stop = iterations >= n_iter
            if checker is not None:
                # SPSATerminationChecker.termination_check with accepted = True, for every active run at once
                nfev = 2 * iterations
                if checker.maxfev is not None:
                    over = nfev >= checker.maxfev
                    stop = stop | over
                    fed = active & ~over  # (the reference returns before it stores anything)
                else:
                    fed = active
                value = 0.5 * (f_plus + f_minus)
                has_previous = fed & (n_values >= 1)
                change = (value - previous).abs() / previous
                shifted = torch.cat([changes[:, 1:], change[:, None]], dim=1)
                changes = torch.where(has_previous[:, None], shifted, changes)
                previous = torch.where(fed, value, previous)
                n_values = n_values + fed
                converged = has_previous & (changes.max(dim=1).values < checker.minimum_relative_change)
                stop = stop | converged
            active = active & ~stop
            if (k + 1) % look_every == 0 and k + 1 < n_iter and not bool(active.any()):
                break
        x_final = x.cpu().numpy()
        done_iterations = iterations.cpu().numpy()
    _spsa_write_back(pack, x_final, done_iterations)
