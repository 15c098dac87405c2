"""Gradient plans and the Adam search with its state on the device: ``qsv_adam_step`` by hand against ``_AdamRun``, plans against
``qsv_gradient_device``, runs of a plan that follow each other without the host, and whole searches
(``device_search.minimize_adam_on_device``) against ``solver._minimize_adam`` on an identically built evaluator.

Everything is compared with ``numpy.array_equal``: a plan queues the work ``qsv_gradient_device`` queues, and the step rounds every
product, quotient, square root and sum on its own, as NumPy does (fp64 division and square root are correctly rounded on the
device).  The one number formed differently is the norm behind ``tol`` -- the device adds the squares in ascending order, NumPy's
``dot`` in its own --, so every case with ``tol > 0`` first asserts, on the host reference alone, that no update norm lies within
1e-6 (relative) of ``tol``: seven orders above what two summation orders of at most 300 squares can differ by."""

import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import helpers
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe import EVQEPopulation, device_search
from queasars_amd.evqe import solver as S
from queasars_amd.ir import CircuitIR, ParamRef

pytestmark = pytest.mark.gpu

P = ParamRef
MARGIN = 1e-6


def _update_norm(run) -> float:
    """The norm ``accept_gradient`` has just compared with ``tol``: the update once more, by its own expressions (the same bits)."""
    cfg, t = run.config, run.iteration
    update = cfg.lr * (run.m / (1 - cfg.beta_1**t)) / (np.sqrt(run.v / (1 - cfg.beta_2**t)) + cfg.eps)
    return float(np.linalg.norm(update))


def _tol_between(norms: list) -> float:
    """A ``tol`` that stops exactly one of the host reference's runs early: between the smallest and the second smallest of the
    runs' least norms before their last iteration (``norms[r][k]``: run r, iteration k, of a search without ``tol``)."""
    least = sorted(min(run[:-1]) for run in norms)
    assert least[0] < least[1]
    return float(np.sqrt(least[0] * least[1]))


def _assert_margin(norms: list, tol: float) -> None:
    flat = np.array([v for run in norms for v in run])
    assert np.all(np.abs(flat - tol) > MARGIN * tol), "a norm of the host reference lies within the margin of tol"


# ---- 1. the entry point by hand ----------------------------------------------------------------------------------------------


def _by_hand(n_runs, width, stride, sizes, columns, with_tol):
    import torch

    dev = StatevectorDevice(6)
    lib, handle = dev._lib, dev._handle
    rng = np.random.default_rng(17)
    n_calls, maxiter = 6, 5
    x0 = rng.normal(size=(n_runs, width)) * 2.0
    gradients = rng.normal(size=(n_calls, n_runs, stride))
    gradients[1, :, ::3] = 0.0  # (entries without a gradient: the moments decay, nothing divides by zero)
    columns_host = np.zeros((n_runs, stride), dtype=np.int32)
    for r in range(n_runs):
        columns_host[r, : sizes[r]] = columns[r]

    def reference(tol):
        """``_AdamRun`` fed the same gradients: per call (x, m, v, iteration, done) of every run, and every norm."""
        cfg = S.Adam(maxiter=maxiter, lr=0.1, tol=tol)
        runs = [cfg.new_run(x0[r, columns[r]], seed=None) for r in range(n_runs)]
        history, norms = [], [[] for _ in runs]
        for k in range(n_calls):
            for r, run in enumerate(runs):
                if not run.done:
                    run.accept_gradient(gradients[k, r, : sizes[r]], 0)
                    norms[r].append(_update_norm(run))
            history.append([(run.x.copy(), run.m.copy(), run.v.copy(), run.iteration, run.done) for run in runs])
        return cfg, history, norms

    tol = 0.0
    if with_tol:
        _, _, free = reference(0.0)
        tol = _tol_between(free)
    cfg, history, norms = reference(tol)
    if with_tol:
        _assert_margin(norms, tol)
        stops = [h[3] for h in history[-1]]
        assert min(stops) < maxiter and max(stops) == maxiter  # (one run stops early, another does not)

    x = torch.from_numpy(x0.copy()).cuda()
    sizes_dev = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    columns_dev = torch.from_numpy(columns_host).cuda()
    m = torch.zeros((n_runs, stride), dtype=torch.float64, device="cuda")
    v = torch.zeros((n_runs, stride), dtype=torch.float64, device="cuda")
    gradient = torch.zeros((n_runs, stride), dtype=torch.float64, device="cuda")
    active = torch.ones(n_runs, dtype=torch.uint8, device="cuda")
    iterations = torch.zeros(n_runs, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def args(t=1, **kw):
        a = _lib.QsvAdamStepArgs(
            n_runs=n_runs, width=width, columns_stride=stride, grad_width=stride, x=x.data_ptr(), sizes=sizes_dev.data_ptr(),
            columns=columns_dev.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), gradient=gradient.data_ptr(), active=active.data_ptr(),
            iterations=iterations.data_ptr(), lr=cfg.lr, beta_1=cfg.beta_1, beta_2=cfg.beta_2, one_minus_beta_1=1 - cfg.beta_1,
            one_minus_beta_2=1 - cfg.beta_2, eps=cfg.eps, tol=cfg.tol, bias_1=1 - cfg.beta_1**t, bias_2=1 - cfg.beta_2**t,
            maxiter=maxiter)
        for k, value in kw.items():
            setattr(a, k, value)
        return a

    def step(t=1, **kw):
        code = lib.qsv_adam_step(handle, C.byref(args(t, **kw)))
        torch.cuda.synchronize()
        return code

    def state():
        return x.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), iterations.cpu().numpy(), active.cpu().numpy()

    try:
        # every refusal comes before any launch; an empty call launches nothing
        assert lib.qsv_adam_step(handle, None) == _lib.QSV_E_ARG
        for name in ("x", "sizes", "columns", "m", "v", "gradient", "active", "iterations"):
            assert step(**{name: None}) == _lib.QSV_E_ARG, name
        for name in ("n_runs", "width", "grad_width"):
            assert step(**{name: -1}) == _lib.QSV_E_ARG, name
        assert step(columns_stride=0) == _lib.QSV_E_ARG
        assert step(grad_width=stride - 1) == _lib.QSV_E_ARG  # (smaller than a run's size may be)
        assert step(n_runs=0) == _lib.QSV_OK and step(width=0) == _lib.QSV_OK
        got = state()
        assert np.array_equal(got[0], x0) and not got[1].any() and not got[2].any() and not got[3].any() and got[4].all()

        for k in range(n_calls):
            before = state()
            gradient.copy_(torch.from_numpy(gradients[k]))
            assert step(t=k + 1) == _lib.QSV_OK
            got_x, got_m, got_v, got_iterations, got_active = state()
            for r in range(n_runs):
                want_x, want_m, want_v, want_iteration, want_done = history[k][r]
                size = sizes[r]
                assert np.array_equal(got_x[r, columns[r]], want_x), (k, r)
                untouched = np.ones(width, dtype=bool)
                untouched[columns[r]] = False
                assert np.array_equal(got_x[r, untouched], x0[r, untouched]), (k, r)
                assert np.array_equal(got_m[r, :size], want_m) and np.array_equal(got_v[r, :size], want_v), (k, r)
                assert not got_m[r, size:].any() and not got_v[r, size:].any(), (k, r)
                assert got_iterations[r] == want_iteration and bool(got_active[r]) == (not want_done), (k, r)
            if k == n_calls - 1:  # (maxiter = 5: the sixth call finds every run stopped and changes nothing)
                assert not before[4].any()
                for a, b in zip(before, (got_x, got_m, got_v, got_iterations, got_active)):
                    assert np.array_equal(a, b)
    finally:
        dev.close()


SMALL = (3, 5, 5, [1, 3, 5], [np.array([3]), np.array([4, 0, 2]), np.array([2, 4, 1, 0, 3])])


def _large():
    rng = np.random.default_rng(5)
    sizes = [1, 300, 2, 299, 64, 65, 128] + rng.integers(1, 301, size=63).tolist()
    columns = [np.sort(rng.permutation(300)[:s]) if r % 2 else rng.permutation(300)[:s] for r, s in enumerate(sizes)]
    return 70, 300, 300, sizes, columns


@pytest.mark.parametrize("with_tol", [False, True], ids=["tol=0", "tol>0"])
def test_adam_step_by_hand_small_odd_width(with_tol):
    """R = 3, width 5 (odd), sizes 1 / 3 / 5 with scattered, non-monotone columns: a run narrower than its row, whose other
    entries must keep their bits.  Six calls with ``maxiter = 5``; the sixth changes nothing."""
    _by_hand(*SMALL, with_tol)


@pytest.mark.parametrize("with_tol", [False, True], ids=["tol=0", "tol>0"])
def test_adam_step_by_hand_more_runs_than_lanes_more_columns_than_threads(with_tol):
    """R = 70, ``grad_width`` 300, sizes from 1 to 300 (64, 65 and 128 among them): more runs than a wave has lanes, more
    columns than a workgroup has threads, several rounds of the norm's lane-by-lane sum."""
    _by_hand(*_large(), with_tol)


# ---- 2. plans are the existing entry point ------------------------------------------------------------------------------------


def _population_n6():
    from queasars_amd.evqe.serialization import population_from_dict

    data = json.loads((Path(__file__).resolve().parent / "golden" / "population_n6.json").read_text())
    return 6, population_from_dict(data["population"])


def _population_n13():
    return 13, EVQEPopulation.random_population(13, 3, 6, True, 0)


def _last_layer(individual):
    layer = len(individual.layers) - 1
    start = individual.circuit_parameter_offsets[layer]
    return list(range(start, start + individual.layers[layer].n_parameters))


def _operator(kind, n):
    return helpers.random_ising_operator(n, seed=12) if kind == "ising" else helpers.random_pauli_operator(n, 40, seed=6)


def _points(circuits, params, extra=1):
    """The points as a padded device matrix (an odd row length among the populations: rows need not be aligned)."""
    import torch

    width = max(len(p) for p in params) + extra
    matrix = torch.zeros((len(circuits), width), dtype=torch.float64, device="cuda")
    for e, p in enumerate(params):
        matrix[e, : len(p)] = torch.tensor(p, dtype=torch.float64)
    return matrix


def _by_the_entry_point(evaluator, circuits, matrix, wrt, out_width):
    """``qsv_gradient_device`` at the points, read back after a synchronise: the reference every plan is held to."""
    import torch

    out = torch.full((len(circuits), out_width), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    evaluator.evaluate_gradients_device_to_device(circuits, matrix.clone(), out, wrt)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("which", ["full", "layer"])
@pytest.mark.parametrize("kind", ["ising", "general"])
@pytest.mark.parametrize("population", [_population_n6, _population_n13], ids=["n6", "n13"])
def test_a_plan_writes_what_the_entry_point_writes(population, kind, which):
    import torch

    n, pop = population()
    circuits = [ind.get_parameterized_quantum_circuit() for ind in pop.individuals]
    params = [list(ind.parameter_values) for ind in pop.individuals]
    wrt = None if which == "full" else [_last_layer(ind) for ind in pop.individuals]
    evaluator = OperatorCircuitEvaluator(_operator(kind, n))
    dev = evaluator.statevector_device
    matrix = _points(circuits, params)
    out_width = max(c.num_parameters for c in circuits) + 2
    want = _by_the_entry_point(evaluator, circuits, matrix, wrt, out_width)
    n_shifted = evaluator.last_gradient_evaluations
    assert n_shifted > 0 and np.abs(want).max() > 1e-3 and not np.isnan(want).any()

    def through(plan):
        out = torch.full((len(circuits), out_width), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert plan.run(matrix, out) == n_shifted == evaluator.last_gradient_evaluations
        torch.cuda.synchronize()
        return out.cpu().numpy()

    plan = evaluator.gradient_plan(circuits, matrix, torch.empty((len(circuits), out_width), dtype=torch.float64, device="cuda"), wrt)
    chunked = None
    try:
        assert plan.n_shifted == n_shifted
        assert np.array_equal(through(plan), want)
        stats = plan.stats()
        assert stats["n_shifted"] == n_shifted and stats["n_chunks"] == 1 and stats["n_runs"] == 1 and stats["table_bytes"] > 0
        # chunks of seven, in force when a second plan is made: the same bits; the first plan keeps its one chunk
        dev.set_option("gradient_chunk", 7)
        chunked = evaluator.gradient_plan(circuits, matrix, torch.empty((len(circuits), out_width), dtype=torch.float64, device="cuda"), wrt)
        dev.set_option("gradient_chunk", 0)
        assert chunked.stats()["n_chunks"] == -(-n_shifted // 7) > 1
        assert np.array_equal(through(chunked), want)
        assert np.array_equal(through(plan), want) and plan.stats()["n_chunks"] == 1
        # another operator between runs is allowed: the tables depend on the circuits alone
        other = OperatorCircuitEvaluator(_operator("general" if kind == "ising" else "ising", n), statevector_device=dev)
        want_other = _by_the_entry_point(other, circuits, matrix, wrt, out_width)
        assert not np.array_equal(want_other, want)
        with dev.operator_lock:
            dev.set_operator(other._operator)
            out = torch.full((len(circuits), out_width), float("nan"), dtype=torch.float64, device="cuda")
            plan._plan.run(matrix.data_ptr(), 0, out.data_ptr())
            torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want_other)
        assert np.array_equal(through(plan), want)  # (and the evaluator's own operator again)
    finally:
        dev.set_option("gradient_chunk", 0)
        plan.close()
        if chunked is not None:
            chunked.close()
    plan.close()  # (idempotent)
    with pytest.raises(RuntimeError, match="closed"):
        plan.stats()


def test_plan_errors():
    import torch

    n = 13
    _, circuits, params = helpers.population_circuits(n, 2, 3, seed=1)
    evaluator = OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=1))
    dev = evaluator.statevector_device
    matrix = _points(circuits, params)
    width = matrix.shape[1]
    out = torch.zeros((3, width), dtype=torch.float64, device="cuda")
    # a parameter that two angle slots read: refused as qsv_gradient_device refuses it
    repeated = CircuitIR(n).u(P(0), 0.3, P(1), 0).cu3(P(2), P(1), 0.1, 0, 1)
    with pytest.raises(ValueError, match="parameter 1 "):
        dev.gradient_plan([circuits[0], repeated], width, width)
    ids, _need, _total = dev._batch_metadata([circuits[0], repeated])
    plan_id, n_shifted = C.c_int(-1), C.c_int64(-1)
    rc = dev._lib.qsv_gradient_plan_create(dev._handle, 2, _lib.as_ptr(ids), width, None, None, width, C.byref(plan_id), C.byref(n_shifted))
    assert rc == _lib.QSV_E_UNSUPPORTED and "more than one angle slot" in _lib.last_error(dev._lib, dev._handle)
    assert dev.gradient_plan([repeated], width, width, [[0, 2]]).n_shifted == 6  # (its other parameters have rules: 2 + 4)
    # the other refusals, with their codes
    with pytest.raises(ValueError, match="wrt index"):
        dev.gradient_plan(circuits[:1], width, width, [[circuits[0].num_parameters]])
    with pytest.raises(ValueError, match="out_width"):
        dev.gradient_plan(circuits, width, 5)
    with pytest.raises(ValueError, match="parameter values"):
        dev.gradient_plan(circuits, 3, width)
    with pytest.raises(ValueError, match="estimator_precision"):
        OperatorCircuitEvaluator(evaluator._operator, estimator_precision=0.1, statevector_device=dev).gradient_plan(circuits, matrix, out)
    for bad in (torch.zeros((3, width), dtype=torch.float32, device="cuda"), torch.zeros((3, width), dtype=torch.float64),
                torch.zeros((2, width), dtype=torch.float64, device="cuda"), torch.zeros((3, 5), dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError):
            evaluator.gradient_plan(circuits, matrix, bad)
    bare = StatevectorDevice(n)
    ids3, _need, _total = bare._batch_metadata(circuits)
    rc = bare._lib.qsv_gradient_plan_create(bare._handle, 3, _lib.as_ptr(ids3), width, None, None, width, C.byref(plan_id), C.byref(n_shifted))
    assert rc == _lib.QSV_E_STATE  # (no operator set)
    stats = _lib.QsvGradientPlanStats()
    assert dev._lib.qsv_gradient_plan_run(dev._handle, 12345, C.c_void_p(matrix.data_ptr()), None, C.c_void_p(out.data_ptr())) == _lib.QSV_E_ARG
    assert dev._lib.qsv_gradient_plan_destroy(dev._handle, 12345) == _lib.QSV_E_ARG
    assert dev._lib.qsv_gradient_plan_stats(dev._handle, 12345, C.byref(stats)) == _lib.QSV_E_ARG
    # a plan whose circuit is destroyed fails cleanly, run after run, and the handle goes on working
    plan = evaluator.gradient_plan(circuits, matrix, out)
    want = _by_the_entry_point(evaluator, circuits[:2], matrix[:2].contiguous(), None, width)
    plan.run(matrix, out)
    torch.cuda.synchronize()
    assert dev._lib.qsv_circuit_destroy(dev._handle, dev.circuit_id(circuits[2])) == _lib.QSV_OK
    for _ in range(2):
        with pytest.raises(ValueError, match="unknown circuit id"):
            plan.run(matrix, out)
    assert plan.stats()["n_runs"] == 1
    plan.close()
    assert np.array_equal(_by_the_entry_point(evaluator, circuits[:2], matrix[:2].contiguous(), None, width), want)
    # a plan that outlives its device: closing it is harmless
    left = dev.gradient_plan(circuits[:2], width, width)
    dev.close()
    left.close()


# ---- 3. runs follow each other without the host -------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["ising", "general"])
def test_runs_of_a_one_chunk_plan_follow_each_other_without_the_host(kind):
    import torch

    from queasars_amd.distributed import _chain_state

    n, pop = _population_n13()
    circuits = [ind.get_parameterized_quantum_circuit(shared=True) for ind in pop.individuals]
    params = [list(ind.parameter_values_in_circuit_order()) for ind in pop.individuals]
    wrt = [_last_layer(ind) for ind in pop.individuals]
    evaluator = OperatorCircuitEvaluator(_operator(kind, n))
    dev = evaluator.statevector_device
    device = torch.device("cuda", dev.device_index)
    stream = _chain_state(evaluator, device)["stream"]  # (the stream the evaluator's handle launches on)
    out_width = max(len(w) for w in wrt)
    rng = np.random.default_rng(2)
    x0 = _points(circuits, params, extra=0)
    delta = torch.from_numpy(0.05 * rng.normal(size=tuple(x0.shape))).cuda()
    outs = [torch.full((len(circuits), out_width), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    x = x0.clone()
    torch.cuda.synchronize()
    plan = evaluator.gradient_plan(circuits, x, outs[0], wrt)
    try:
        assert plan.stats()["n_chunks"] == 1
        with torch.cuda.stream(stream):
            plan.run(x, outs[0])
            first = plan.stats()
            allocations = dev.gradient_stats()["n_allocations"]
            for out in outs[1:]:
                x.add_(delta)  # (the optimiser's share, on the stream, in place: the next run reads it where it is)
                plan.run(x, out)
        after = plan.stats()
        assert after["n_runs"] == 3 and first["n_runs"] == 1
        assert after["n_host_waits"] == first["n_host_waits"], "a run behind a run of the same plan made the host wait"
        assert dev.gradient_stats()["n_allocations"] == allocations
        stream.synchronize()  # (the one wait)
        got = [out.cpu().numpy() for out in outs]
    finally:
        plan.close()
    at = x0.clone()
    for k in range(3):
        if k:
            at.add_(delta)
        want = _by_the_entry_point(evaluator, circuits, at, wrt, out_width)
        assert np.array_equal(got[k], want), k
        assert k == 0 or not np.array_equal(got[k], got[k - 1])
    assert np.array_equal(x.cpu().numpy(), at.cpu().numpy())


# ---- 4. a whole search ----------------------------------------------------------------------------------------------------------


def _search_jobs(pop, cfg, embedded):
    jobs = []
    for ind in pop.individuals:
        run = cfg.new_run(ind.get_layer_parameter_values(-1), seed=None)
        if embedded:  # (the last layer's angles inside the individual's fully parameterised circuit, as the solver shares circuits)
            run.embed = (np.asarray(ind.parameter_values_in_circuit_order(), dtype=np.float64), np.asarray(_last_layer(ind), dtype=np.int64))
            jobs.append((ind.get_parameterized_quantum_circuit(shared=True), run))
        else:
            jobs.append((ind.get_partially_parameterized_quantum_circuit({-1}), run))
    return jobs


@pytest.mark.parametrize("with_tol", [False, True], ids=["tol=0", "tol>0"])
@pytest.mark.parametrize("kind", ["ising", "general"])
@pytest.mark.parametrize("embedded", [False, True], ids=["own", "embedded"])
def test_a_search_on_the_device_leaves_what_the_host_driver_leaves(embedded, kind, with_tol, monkeypatch):
    n, maxiter = 10, 4
    pop = EVQEPopulation.random_population(n, 3, 5, True, 3)
    op = _operator(kind, n)
    tol = 0.0
    if with_tol:
        # the host driver without a tolerance, every update's norm noted: tol goes between two runs' least norms
        norms = {}
        inner = S._AdamRun.accept_gradient

        def noting(run, gradient, n_evaluations):
            inner(run, gradient, n_evaluations)
            norms.setdefault(id(run), []).append(_update_norm(run))

        free = _search_jobs(pop, S.Adam(maxiter=maxiter, lr=0.1), embedded)
        monkeypatch.setattr(S._AdamRun, "accept_gradient", noting)
        S._minimize_adam(OperatorCircuitEvaluator(op), free)
        monkeypatch.setattr(S._AdamRun, "accept_gradient", inner)
        noted = [norms[id(run)] for _, run in free]
        tol = _tol_between(noted)
        print(f"update norms of the host reference: {noted}; tol = {tol}")
        _assert_margin(noted, tol)
    cfg = S.Adam(maxiter=maxiter, lr=0.1, tol=tol)
    host, device = _search_jobs(pop, cfg, embedded), _search_jobs(pop, cfg, embedded)
    S._minimize_adam(OperatorCircuitEvaluator(op), host)
    stops = [run.iteration for _, run in host]
    if with_tol:
        assert min(stops) < maxiter and max(stops) == maxiter  # (one run stops early, another does not)
    else:
        assert stops == [maxiter] * len(host)
    evaluator = OperatorCircuitEvaluator(op)
    assert device_search.supported_adam(evaluator, device)
    state = {}
    device_search.minimize_adam_on_device(evaluator, device, look_every=2, state=state)
    for r, ((_, a), (_, b)) in enumerate(zip(host, device)):
        assert np.array_equal(a.x, b.x), r
        assert np.array_equal(a.m, b.m) and np.array_equal(a.v, b.v), r
        assert (a.iteration, a.nfev, a.done) == (b.iteration, b.nfev, b.done) and b.done and b.nfev > 0, r
    assert any(np.abs(a.x - ind.get_layer_parameter_values(-1)).max() > 1e-3 for (_, a), ind in zip(host, pop.individuals))


def test_the_solver_takes_the_device_search_only_when_asked_to(monkeypatch):
    """The solver's last-layer search with ``Adam``: on the host with ``None`` (and with ``QSV_DEVICE_SEARCH=0`` whatever the
    configuration says), on the device with ``True`` -- where it leaves the parameter values the host driver leaves when that
    searches the same shared circuits (``QSV_SHARE_CIRCUITS=2``), and makes the same number of evaluations."""
    n = 10
    op = helpers.random_ising_operator(n, seed=12)
    ev = OperatorCircuitEvaluator(op)
    population = EVQEPopulation.random_population(n, 2, 8, True, 0)
    calls = []
    inner = device_search.minimize_adam_on_device

    def spy(evaluator, jobs, *args, **kwargs):
        calls.append(len(jobs))
        return inner(evaluator, jobs, *args, **kwargs)

    monkeypatch.setattr(device_search, "minimize_adam_on_device", spy)

    def solver(flag):
        return S.EVQEMinimumEigensolver(S.EVQEMinimumEigensolverConfiguration(
            optimizer=S.Adam(maxiter=4, lr=0.1), population_size=8, max_generations=1, random_seed=0, n_initial_layers=2,
            randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2, use_tournament_selection=True,
            tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1, parameter_search_probability=0.3,
            topological_search_probability=0.4, layer_removal_probability=0.05, device_resident_search=flag,
        ))

    def values(pop):
        return [list(ind.parameter_values) for ind in pop.individuals]

    monkeypatch.setenv("QSV_SHARE_CIRCUITS", "2")
    on_host, host_nfev = solver(None)._last_layer_search(ev, population)
    assert calls == [] and host_nfev > 0 and values(on_host) != values(population)
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "0")
    refused, nfev = solver(True)._last_layer_search(ev, population)
    assert calls == [] and nfev == host_nfev and values(refused) == values(on_host)
    monkeypatch.delenv("QSV_DEVICE_SEARCH")
    monkeypatch.delenv("QSV_SHARE_CIRCUITS")
    searched, nfev = solver(True)._last_layer_search(ev, population)
    assert calls == [8]
    assert nfev == host_nfev
    assert values(searched) == values(on_host)
    solver(False)._last_layer_search(ev, population)
    assert calls == [8]
