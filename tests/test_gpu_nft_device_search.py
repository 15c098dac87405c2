"""The NFT search with its state on the device: ``qsv_nft_step`` by hand, every iteration of real searches
(``device_search.minimize_nft_on_device``) replayed on the host from the DEVICE's own inputs, and the solver end to end.

Whole searches are not held against the host driver's: these searches are full of flat directions (lambda of a ``u`` acting on
|0>, phi and lambda under a diagonal operator), where the fitted amplitude is rounding noise and the last bit of ``hypot`` /
``atan2`` decides an angle.  Step by step the inputs are bit-identical, and then only those two library calls differ:

* proposals and every entry of ``x`` an accept does not touch: ``==``;
* the updated entry: ``|dx| <= 64 * spacing(max(1, |x|, pi))``;
* the fitted minimum: ``|d| <= 64 * spacing(max(1, |c|, a))``

-- 64 ulp is an order of magnitude over what ``hypot`` / ``atan2`` of two libraries can differ by and nine orders under a wrong
sign, column or value.
"""

import ctypes as C
import math

import numpy as np
import pytest

import helpers
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, OperatorSamplerCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe import EVQEPopulation, device_search
from queasars_amd.evqe import solver as S

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10
ULPS = 64


def _x_tolerance(x):
    return ULPS * np.spacing(max(1.0, abs(x), np.pi))


def _recycled_tolerance(c, a):
    return ULPS * np.spacing(max(1.0, abs(c), a))


def _fit(z0, z1, z3):
    c = 0.5 * (z1 + z3)
    return c, math.hypot(z0 - c, 0.5 * (z3 - z1))


def _host_accept(cfg, x_row, columns, iteration, with_base, recycled, values):
    """A host run put where the device's run stands, fed the same values: (its x, its fitted minimum, c, a)."""
    run = cfg.new_run(x_row[columns], seed=None)
    run.iteration, run._needs_base, run._recycled = iteration, with_base, None if with_base else float(recycled)
    run.accept(*[float(v) for v in values])
    z0 = float(values[0]) if with_base else float(recycled)
    return run.x, run._recycled, *_fit(z0, float(values[-2]), float(values[-1]))


def _host_points(cfg, x_row, columns, iteration, with_base):
    """The rows a host run at the device's x proposes, scattered into the device's row as the host driver scatters them."""
    run = cfg.new_run(x_row[columns], seed=None)
    run.iteration, run._recycled = iteration, None if with_base else 0.0
    proposed = run.propose()
    assert len(proposed) == (3 if with_base else 2)
    rows = np.repeat(x_row[None, :], len(proposed), axis=0)
    rows[:, columns] = np.asarray(proposed)
    return rows


class _Worst:
    def __init__(self):
        self.x = self.recycled = 0.0

    def check(self, got_row, x_before, columns, iteration, host_x, got_recycled, host_recycled, c, a, label):
        j = iteration % len(columns)
        col = columns[j]
        untouched = np.ones(got_row.size, dtype=bool)
        untouched[col] = False
        assert np.array_equal(got_row[untouched], x_before[untouched]), label
        others = np.arange(len(columns)) != j
        assert np.array_equal(host_x[others], x_before[columns][others]), label
        dx, dr = abs(got_row[col] - host_x[j]), abs(got_recycled - host_recycled)
        self.x = max(self.x, dx / np.spacing(max(1.0, abs(host_x[j]), np.pi)))
        self.recycled = max(self.recycled, dr / np.spacing(max(1.0, abs(c), a)))
        assert dx <= _x_tolerance(host_x[j]), (label, dx)
        assert dr <= _recycled_tolerance(c, a), (label, dr)
        if a == 0.0:
            assert got_row[col] == x_before[col] and got_recycled == c, label


# ---- 1. the entry point by hand ----------------------------------------------------------------------------------------------


def _sinusoid_values(points, per_run, columns, sizes, iteration, curves, constant_run):
    """f_r at the proposed points: c + A cos(t - b) in the one coordinate the iteration visits; a constant for one run."""
    out = np.empty(points.shape[0])
    for r, (c, amp, b) in enumerate(curves):
        col = columns[r][iteration % sizes[r]]
        for i in range(per_run):
            t = points[per_run * r + i, col]
            out[per_run * r + i] = 0.7 if r == constant_run else c + amp * math.cos(t - b)
    return out


def _by_hand(n_runs, width, sizes, columns, first_iteration, constant_run):
    import torch

    dev = StatevectorDevice(6)
    lib, handle = dev._lib, dev._handle
    cfg = S.NFT(maxfev=10**6, reset_interval=0)  # (a host run takes the base exactly when it has nothing recycled)
    rng = np.random.default_rng(11)
    stride = max(sizes)
    x0 = rng.normal(size=(n_runs, width)) * 2.0
    columns_host = np.zeros((n_runs, stride), dtype=np.int32)
    for r in range(n_runs):
        columns_host[r, : sizes[r]] = columns[r]
    curves = [(rng.normal(), abs(rng.normal()) + 0.1, rng.uniform(-3, 3)) for _ in range(n_runs)]
    x = torch.from_numpy(x0.copy()).cuda()
    sizes_dev = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    columns_dev = torch.from_numpy(columns_host).cuda()
    recycled = torch.full((n_runs,), -77.0, dtype=torch.float64, device="cuda")
    points = torch.full((3 * n_runs, width), -55.0, dtype=torch.float64, device="cuda")
    values = torch.zeros(3 * n_runs, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def args(**kw):
        a = _lib.QsvNftStepArgs(n_runs=n_runs, width=width, columns_stride=stride, reserved=0, x=x.data_ptr(), sizes=sizes_dev.data_ptr(),
                                columns=columns_dev.data_ptr(), recycled=recycled.data_ptr(), accept=0, accept_with_base=0,
                                accept_iteration=0, propose=0, propose_with_base=0, propose_iteration=0, values=values.data_ptr(),
                                points=points.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def step(**kw):
        code = lib.qsv_nft_step(handle, C.byref(args(**kw)))
        torch.cuda.synchronize()
        return code

    worst = _Worst()
    try:
        # every refusal comes before any launch
        assert lib.qsv_nft_step(handle, None) == _lib.QSV_E_ARG
        for name in ("x", "sizes", "columns", "recycled"):
            assert step(propose=1, **{name: None}) == _lib.QSV_E_ARG, name
        assert step(propose=1, n_runs=-1) == _lib.QSV_E_ARG and step(propose=1, width=-1) == _lib.QSV_E_ARG
        assert step(propose=1, columns_stride=0) == _lib.QSV_E_ARG
        assert step(accept=1, values=None) == _lib.QSV_E_ARG and step(propose=1, points=None) == _lib.QSV_E_ARG
        assert step(accept=1, accept_iteration=-1) == _lib.QSV_E_ARG and step(propose=1, propose_iteration=-1) == _lib.QSV_E_ARG
        assert step(propose=1, n_runs=0) == 0 and step(propose=1, width=0) == 0
        assert step() == 0  # (neither half: nothing moves)
        assert np.array_equal(x.cpu().numpy(), x0) and np.all(points.cpu().numpy() == -55.0) and np.all(recycled.cpu().numpy() == -77.0)

        # propose only, three-wide (the number on the half that is not asked for is not looked at)
        it = first_iteration
        assert step(propose=1, propose_with_base=1, propose_iteration=it, accept_iteration=-1, values=None) == 0
        got = points.cpu().numpy()
        for r in range(n_runs):
            assert np.array_equal(got[3 * r : 3 * r + 3], _host_points(cfg, x0[r], columns[r], it, True)), r
        assert np.array_equal(x.cpu().numpy(), x0)

        # accept it (base values came) and propose the next, two-wide, in one call
        f = _sinusoid_values(got, 3, columns, sizes, it, curves, constant_run)
        values.copy_(torch.from_numpy(f))
        assert step(accept=1, accept_with_base=1, accept_iteration=it, propose=1, propose_with_base=0, propose_iteration=it + 1) == 0
        three_wide = got
        x1, rec1, got = x.cpu().numpy(), recycled.cpu().numpy(), points.cpu().numpy()
        for r in range(n_runs):
            host_x, host_rec, c, a = _host_accept(cfg, x0[r], columns[r], it, True, None, f[3 * r : 3 * r + 3])
            worst.check(x1[r], x0[r], columns[r], it, host_x, rec1[r], host_rec, c, a, ("three", r))
            assert np.array_equal(got[2 * r : 2 * r + 2], _host_points(cfg, x1[r], columns[r], it + 1, False)), r
        assert (_fit(*f[3 * constant_run : 3 * constant_run + 3])[1] == 0.0) and rec1[constant_run] == 0.7
        assert np.array_equal(got[2 * n_runs :], three_wide[2 * n_runs :])  # (a two-wide proposal writes 2 R rows and no more)

        # accept only, two-wide: the fitted minimum of the step before stands in for the base value
        f = _sinusoid_values(got[: 2 * n_runs], 2, columns, sizes, it + 1, curves, -1)
        values[: 2 * n_runs].copy_(torch.from_numpy(f))
        before = points.clone()
        assert step(accept=1, accept_with_base=0, accept_iteration=it + 1, points=None, propose_iteration=-1) == 0
        x2, rec2 = x.cpu().numpy(), recycled.cpu().numpy()
        for r in range(n_runs):
            host_x, host_rec, c, a = _host_accept(cfg, x1[r], columns[r], it + 1, False, rec1[r], f[2 * r : 2 * r + 2])
            worst.check(x2[r], x1[r], columns[r], it + 1, host_x, rec2[r], host_rec, c, a, ("two", r))
        assert torch.equal(points, before)

        # propose only, two-wide
        assert step(propose=1, propose_with_base=0, propose_iteration=it + 2) == 0
        got = points.cpu().numpy()
        for r in range(n_runs):
            assert np.array_equal(got[2 * r : 2 * r + 2], _host_points(cfg, x2[r], columns[r], it + 2, False)), r
        print(f"R={n_runs} width={width}: largest |dx| = {worst.x:.2f} ulp, largest |d recycled| = {worst.recycled:.2f} ulp")
    finally:
        dev.close()


def test_entry_point_by_hand_small_odd_width():
    """R = 3, width 5 (odd: odd rows sit on 8-byte alignment only), sizes 1 / 3 / 5, columns (4, 0, 2) for the run in the
    middle -- the entries 1 and 3 of its row must come through untouched --, iteration 4 >= size for two of the runs, both forms,
    accept only / propose only / both, and one run whose three values are equal (a == 0: x as it was, recycled == c)."""
    _by_hand(3, 5, [1, 3, 5], [np.array([0]), np.array([4, 0, 2]), np.arange(5)], first_iteration=4, constant_run=0)


def test_entry_point_by_hand_more_runs_than_lanes_more_columns_than_threads():
    """R = 70, width 257: more runs than a wave has lanes, more columns than a workgroup has threads, an odd width again;
    sizes from 1 to 257, columns a permutation's head, the iteration number past most sizes."""
    rng = np.random.default_rng(5)
    sizes = [1, 257, 2, 256] + rng.integers(1, 258, size=66).tolist()
    columns = [np.sort(rng.permutation(257)[:s]) if r % 2 else rng.permutation(257)[:s] for r, s in enumerate(sizes)]
    _by_hand(70, 257, sizes, columns, first_iteration=131, constant_run=7)


# ---- 2. real searches, replayed iteration by iteration from the device's own inputs -----------------------------------------


def _search_jobs(pop, cfg, embedded):
    jobs = []
    for ind in pop.individuals:
        run = cfg.new_run(ind.get_layer_parameter_values(-1), seed=None)
        if embedded:  # (the last layer's angles inside the individual's fully parameterised circuit, as the solver shares circuits)
            layer = len(ind.layers) - 1
            start = ind.circuit_parameter_offsets[layer]
            run.embed = (np.asarray(ind.parameter_values_in_circuit_order(), dtype=np.float64),
                         np.arange(start, start + ind.layers[layer].n_parameters, dtype=np.int64))
            jobs.append((ind.get_parameterized_quantum_circuit(shared=True), run))
        else:
            jobs.append((ind.get_partially_parameterized_quantum_circuit({-1}), run))
    return jobs


def _evaluator(kind, op, seed=3):
    if kind == "fp64" or kind == "fp32":
        return OperatorCircuitEvaluator(op, dtype=kind)
    if kind == "exact":
        return OperatorSamplerCircuitEvaluator(None, op, alpha=0.5, seed=seed)
    return OperatorSamplerCircuitEvaluator(64, op, alpha=0.5, seed=seed)


CASES = [
    ("fp64", dict(maxfev=23, reset_interval=4), True),
    ("fp64", dict(maxfev=40), False),
    ("fp32", dict(maxfev=23, reset_interval=4), False),
    ("fp32", dict(maxfev=40), True),
    ("exact", dict(maxfev=23, reset_interval=4), True),
    ("exact", dict(maxfev=40), False),
    ("shots", dict(maxfev=23, reset_interval=4), False),
    ("shots", dict(maxfev=40), True),
]


@pytest.mark.parametrize("kind,nft,embedded", CASES, ids=[f"{k}-{n['maxfev']}-{'embedded' if e else 'own'}" for k, n, e in CASES])
def test_every_iteration_of_a_search_is_the_hosts_step_on_the_devices_inputs(kind, nft, embedded, monkeypatch):
    n = 6
    pop = EVQEPopulation.random_population(n, 2, 8, True, 0)
    op = helpers.random_ising_operator(n, seed=12)
    cfg = S.NFT(**nft)
    flags, nfev = device_search.nft_schedule(cfg)
    ev = _evaluator(kind, op)
    jobs = _search_jobs(pop, cfg, embedded)
    assert device_search.supported_nft(ev, jobs)
    state, records = {}, []
    inner = ev.evaluate_device_to_device

    def recording(circuits, matrix, out, **kwargs):
        assert not kwargs  # (lock-step runs: no mask)
        before = (state["points"].clone(), state["x"].clone(), state["recycled"].clone())
        inner(circuits, matrix, out)
        records.append((circuits, matrix.shape[0], *before, state["values"].clone()))

    monkeypatch.setattr(ev, "evaluate_device_to_device", recording)
    device_search.minimize_nft_on_device(ev, jobs, state=state)
    assert len(records) == len(flags)
    n_runs = len(jobs)
    where = [run.embed[1] if run.embed is not None else np.arange(run.x.size) for _, run in jobs]
    lists = {3: records[0][0]}
    x_after = [rec[3].cpu().numpy() for rec in records[1:]] + [state["x"].cpu().numpy()]
    recycled_after = [rec[4].cpu().numpy() for rec in records[1:]] + [state["recycled"].cpu().numpy()]
    worst = _Worst()
    for k, (circuits, n_rows, points, x, recycled, values) in enumerate(records):
        per_run = 3 if flags[k] else 2
        assert n_rows == per_run * n_runs == len(circuits)
        assert lists.setdefault(per_run, circuits) is circuits  # (the same list object for every iteration of its kind)
        assert [c for c in circuits] == [job[0] for job in jobs for _ in range(per_run)]
        points, x, recycled, values = points.cpu().numpy(), x.cpu().numpy(), recycled.cpu().numpy(), values.cpu().numpy()
        for r in range(n_runs):
            rows = slice(per_run * r, per_run * r + per_run)
            assert np.array_equal(points[rows], _host_points(cfg, x[r], where[r], k, flags[k])), (k, r)
            host_x, host_rec, c, a = _host_accept(cfg, x[r], where[r], k, flags[k], recycled[r], values[rows])
            worst.check(x_after[k][r], x[r], where[r], k, host_x, recycled_after[k][r], host_rec, c, a, (k, r))
    print(f"{kind} {nft} embedded={embedded}: largest |dx| = {worst.x:.2f} ulp, largest |d recycled| = {worst.recycled:.2f} ulp")
    for r, (_, run) in enumerate(jobs):
        assert run.done and run.iteration == len(flags) and run.nfev == nfev
        assert np.array_equal(run.x, x_after[-1][r][where[r]]) and run._recycled == recycled_after[-1][r]
    if kind == "shots":
        # one seed per iteration, none beyond the schedule: the generator stands where the host driver leaves a twin's
        twin = _evaluator(kind, op)
        host_jobs = _search_jobs(pop, cfg, embedded)
        S._minimize_batched(twin, host_jobs)
        assert all(run.iteration == len(flags) and run.nfev == nfev for _, run in host_jobs)
        assert ev._rng.bit_generator.state == twin._rng.bit_generator.state


# ---- 3. the solver end to end -------------------------------------------------------------------------------------------------


def test_the_solver_takes_the_device_search_only_when_asked_to(monkeypatch):
    """The configuration of ``test_nft_last_layer_search_on_the_device`` (n = 10, 8 individuals, ``NFT(maxfev=40)``) with
    ``device_resident_search=True``: the last-layer search runs on the device, the sum of expectation values decreases, every
    run makes the host driver's 41 evaluations, and an individual's value is the oracle's.  With ``None`` the search stays on
    the host."""
    n = 10
    op = helpers.random_ising_operator(n, seed=12)
    ev = OperatorCircuitEvaluator(op)
    population = EVQEPopulation.random_population(n, 2, 8, False, 0)
    calls = []
    inner = device_search.minimize_nft_on_device

    def spy(evaluator, jobs, *args, **kwargs):
        calls.append(len(jobs))
        return inner(evaluator, jobs, *args, **kwargs)

    monkeypatch.setattr(device_search, "minimize_nft_on_device", spy)

    def solver(flag):
        return S.EVQEMinimumEigensolver(S.EVQEMinimumEigensolverConfiguration(
            optimizer=S.NFT(maxfev=40), population_size=8, max_generations=1, random_seed=0, n_initial_layers=2,
            randomize_initial_population_parameters=False, speciation_genetic_distance_threshold=2, use_tournament_selection=True,
            tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1, parameter_search_probability=0.3,
            topological_search_probability=0.4, layer_removal_probability=0.05, device_resident_search=flag,
        ))

    def total(pop):
        cs = [i.get_parameterized_quantum_circuit() for i in pop.individuals]
        return sum(ev.evaluate_circuits(cs, [list(i.parameter_values) for i in pop.individuals]))

    before = total(population)
    on_host, host_nfev = solver(None)._last_layer_search(ev, population)
    assert calls == [] and host_nfev == 8 * 41 and total(on_host) < before
    searched, nfev = solver(True)._last_layer_search(ev, population)
    assert calls == [8]
    assert nfev == 8 * 41 == host_nfev
    assert total(searched) < before
    ind = searched.individuals[3]
    got = ev.evaluate_circuits([ind.get_parameterized_quantum_circuit()], [list(ind.parameter_values)])[0]
    assert abs(got - helpers.oracle_expectation(ind.get_parameterized_quantum_circuit(), list(ind.parameter_values), op)) < EXP_TOL
