"""The sampler (CVaR) branch with parameter values read from and results left in device memory (``qsv_cvar_device``,
``OperatorSamplerCircuitEvaluator.evaluate_device_to_device``), its mask of switched-off evaluations, and the lock-step SPSA
search of evqe/device_search.py on top of it.

The population mixes routes (asserted through ``circuit_costs`` / ``circuit_form``): circuits the sampler draws from their two
side tables and circuits that run gate passes into probabilities, shuffled, parameter rows padded to one width.
"""

import ctypes as C

import numpy as np
import pytest

import helpers
from oracle import statevector_oracle as so
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, OperatorSamplerCircuitEvaluator, StatevectorDevice
from queasars_amd.circuit_evaluation.circuit_evaluation import CircuitEvaluatorException
from queasars_amd.ir import PauliOperator
from sampler_draws import DELTA_FP64, DrawCheck, plain_order, shot_uniform, split_order

pytestmark = pytest.mark.gpu

N = 14
SENTINEL = -12345.678


def _population(n=N, blocks=((3, 8, 41), (4, 6, 42), (9, 4, 43)), shuffle_seed=5):
    circuits, params = [], []
    for layers, count, seed in blocks:
        _, c, p = helpers.population_circuits(n, layers, count, seed=seed)
        circuits += c
        params += p
    perm = np.random.default_rng(shuffle_seed).permutation(len(circuits))
    return [circuits[i] for i in perm], [list(params[i]) for i in perm]


def _matrix(params, width=None):
    import torch

    width = width or max(len(p) for p in params)
    rows = np.zeros((len(params), width))
    for i, p in enumerate(params):
        rows[i, : len(p)] = p
    return torch.from_numpy(rows).cuda()


def _routes(dev, op, circuits):
    """(cost route name, circuit_form) of every circuit under ``op``; the population must mix split-sampled circuits with
    circuits that run one-tile or gate passes."""
    costs = OperatorCircuitEvaluator(op, statevector_device=dev).circuit_costs(circuits)
    forms = [dev.circuit_form(c) for c in circuits]
    routes = {c["route"] for c in costs}
    assert len(routes) >= 2, routes
    assert any(f["split_sampled"] for f in forms) and any(not f["split_sampled"] for f in forms), forms
    assert routes & {"one tile", "gate passes"} and routes & {"split", "split, one launch"}, routes
    return costs, forms


def _sampler(op, shots, alpha, dev, seed=7):
    return OperatorSamplerCircuitEvaluator(shots, op, alpha=alpha, seed=seed, statevector_device=dev)


def _to_device(ev, circuits, matrix, active=None, stride=1, fill=SENTINEL):
    import torch

    out = torch.full((len(circuits),), fill, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ev.evaluate_device_to_device(circuits, matrix, out, active=active, active_stride=stride)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("many_groups", [False, True])
def test_entry_point_equals_the_host_forms_bit_for_bit(many_groups, monkeypatch):
    """``evaluate_device_to_device`` into a device tensor == ``sample_cvar_batch`` / ``exact_cvar_batch`` of the same points,
    in the caller's order; also when the batch spans many launch groups of both kinds (three state slots, eight side-table
    slots)."""
    circuits, params = _population()
    if many_groups:
        circuits, params = circuits + circuits[::-1], params + [list(p) for p in params[::-1]]
        monkeypatch.setenv("QSV_SIDE_SLOTS", "8")
    op = helpers.random_ising_operator(N, seed=N)
    dev = StatevectorDevice(N, group=3 if many_groups else 0)
    try:
        costs, forms = _routes(dev, op, circuits)
        if many_groups:
            assert sum(f["split_sampled"] for f in forms) > 8 and sum(not f["split_sampled"] for f in forms) > 3
        dev.set_operator(op)
        matrix = _matrix(params)
        for shots in (1, 300, 1024, 4096):
            for alpha in (0.1, 0.5, 1.0):
                ev, twin = _sampler(op, shots, alpha, dev), _sampler(op, shots, alpha, dev)
                for _ in range(2):  # (call after call: the two generators stay in step)
                    got = _to_device(ev, circuits, matrix)
                    want = np.asarray(twin.evaluate_circuits(circuits, params))
                    assert np.array_equal(got, want), (shots, alpha)
        for alpha in (0.1, 0.5, 1.0):
            got = _to_device(_sampler(op, None, alpha, dev), circuits, matrix)
            want = dev.exact_cvar_batch(circuits, params, alpha)
            assert np.array_equal(got, np.asarray(want)), alpha
        # rows padded further than any circuit needs: the same bits
        wide = _matrix(params, width=max(len(p) for p in params) + 9)
        assert np.array_equal(_to_device(_sampler(op, None, 0.5, dev), circuits, wide), np.asarray(dev.exact_cvar_batch(circuits, params, 0.5)))
    finally:
        dev.close()


def test_against_the_oracle():
    """Independent of the code under test.  Exact CVaR: within 1e-10 of the oracle's restatement of the reference's loop over
    the oracle state's probabilities (the bound qsv_exact_cvar_batch is held to).  With shots: every draw of
    ``sample_batch`` is accepted by ``DrawCheck`` against the oracle's probabilities, its value is D[state], and the CVaR
    recomputed on the host from those values is what the device call left (to the rounding of a sum of ``shots`` values:
    2 shots eps sum|c|)."""
    circuits, params = _population(blocks=((3, 3, 41), (4, 2, 42), (9, 2, 43)))
    op = helpers.random_ising_operator(N, seed=N)
    spread = float(np.abs(op.coeffs).sum())
    dev = StatevectorDevice(N)
    try:
        _, forms = _routes(dev, op, circuits)
        dev.set_operator(op)
        matrix = _matrix(params)
        table = so.diagonal_values(N, op.z_mask.tolist(), op.coeffs.real.tolist())
        probs = [so.probabilities(helpers.oracle_state(c, p)) for c, p in zip(circuits, params)]
        for alpha in (0.3, 0.05):
            got = _to_device(_sampler(op, None, alpha, dev), circuits, matrix)
            for i, p in enumerate(probs):
                want = so.cvar_expectation([(s, float(p[s]), float(table[s])) for s in range(p.size)], alpha)
                print(f"exact alpha={alpha} circuit {i}: |device - oracle| = {abs(got[i] - want):.3e}")
                assert abs(got[i] - want) < 1e-10, (alpha, i)
        import torch

        for shots, alpha, seed in ((300, 0.5, 11), (4096, 0.1, 12), (1000, 1.0, 13)):
            states, values = dev.sample_batch(circuits, params, shots, seed, with_values=True)
            out = torch.zeros(len(circuits), dtype=torch.float64, device="cuda")
            dev.cvar_of_device_parameters(circuits, matrix.data_ptr(), matrix.shape[1], 0, shots, seed, alpha, out.data_ptr())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for i, form in enumerate(forms):
                order = split_order(form["mask_x"], form["mask_y"]) if form["split_sampled"] else plain_order(N)
                check = DrawCheck(probs[i], order, DELTA_FP64)
                u = shot_uniform(seed, i, np.arange(shots))
                assert check.accepted(u, states[i]).all(), check.report(u, states[i])
                assert np.abs(values[i] - table[states[i].astype(np.int64)]).max() <= 1e-12 * spread
                ordered = np.sort(values[i])
                mass = alpha * shots
                whole = min(shots, int(np.floor(mass + 1e-12)))
                want = float(ordered[:whole].sum())
                if whole < shots and mass - whole > 1e-12:
                    want += (mass - whole) * float(ordered[whole])
                want /= mass
                print(f"shots={shots} alpha={alpha} circuit {i}: |device - host| = {abs(got[i] - want):.3e}")
                assert abs(got[i] - want) <= 2 * shots * np.finfo(float).eps * spread, (shots, alpha, i)
    finally:
        dev.close()


def test_it_does_not_wait_and_does_not_disturb():
    """Values queued on the handle's stream before the call are seen, a torch operation queued after it reads the results,
    a second call of another shape right behind the first -- no synchronisation between them -- is right too, and an
    estimator on the same device returns the same bits before and after."""
    import torch

    from queasars_amd.distributed import _chain_state

    circuits, params = _population()
    more, more_params = _population(blocks=((3, 10, 51), (5, 6, 52), (8, 5, 53)), shuffle_seed=9)
    more, more_params = circuits + more, params + more_params
    op = helpers.random_ising_operator(N, seed=N)
    dev = StatevectorDevice(N)
    try:
        _routes(dev, op, circuits)
        estimator = OperatorCircuitEvaluator(op, statevector_device=dev)
        before = estimator.evaluate_circuits(circuits, params)
        ev, twin = _sampler(op, 512, 0.4, dev), _sampler(op, 512, 0.4, dev)
        ev2, twin2 = _sampler(op, 2048, 0.25, dev, seed=8), _sampler(op, 2048, 0.25, dev, seed=8)
        want = np.asarray(twin.evaluate_circuits(circuits, params))
        want2 = np.asarray(twin2.evaluate_circuits(more, more_params))
        stream = _chain_state(ev, torch.device("cuda", dev.device_index))["stream"]
        host_rows, host_rows2 = _matrix(params).cpu().pin_memory(), _matrix(more_params).cpu().pin_memory()
        matrix = torch.zeros(host_rows.shape, dtype=torch.float64, device="cuda")
        matrix2 = torch.zeros(host_rows2.shape, dtype=torch.float64, device="cuda")
        out = torch.zeros(len(circuits), dtype=torch.float64, device="cuda")
        out2 = torch.zeros(len(more), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            # (a long-running operation in front, so that the fills below are still queued when the calls are made)
            busy = torch.randn(4096, 4096, device="cuda")
            for _ in range(20):
                busy = busy @ busy * 1e-3
            matrix.copy_(host_rows, non_blocking=True)
            matrix2.copy_(host_rows2, non_blocking=True)
            ev.evaluate_device_to_device(circuits, matrix, out)
            ev2.evaluate_device_to_device(more, matrix2, out2)
            doubled = out * 2.0
            doubled2 = out2 * 2.0
        stream.synchronize()
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(doubled.cpu().numpy(), 2.0 * want)
        assert np.array_equal(out2.cpu().numpy(), want2) and np.array_equal(doubled2.cpu().numpy(), 2.0 * want2)
        assert estimator.evaluate_circuits(circuits, params) == before
        # the same batch again and again without a wait in between (the layout of the first call is reused)
        ev3, twin3 = _sampler(op, None, 0.3, dev), _sampler(op, None, 0.3, dev)
        want3 = np.asarray(twin3.evaluate_circuits(circuits, params))
        outs = [torch.zeros(len(circuits), dtype=torch.float64, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for o in outs:
                ev3.evaluate_device_to_device(circuits, matrix, o)
        stream.synchronize()
        for o in outs:
            assert np.array_equal(o.cpu().numpy(), want3)
        assert estimator.evaluate_circuits(circuits, params) == before
    finally:
        dev.close()


@pytest.mark.parametrize("shots", [None, 700])
def test_the_mask(shots):
    """Every third plus / minus pair switched off -- split circuits and others among them: ``out`` keeps its sentinel there,
    every other entry equals the unmasked call bit for bit; all off and none off both work; a mask written on the handle's
    stream just before the call is the one the kernels see; and other entry points return what they returned before."""
    import torch

    from queasars_amd.distributed import _chain_state

    base, base_params = _population()
    op = helpers.random_ising_operator(N, seed=N)
    dev = StatevectorDevice(N)
    # (every third pair is switched off below: ordered so that those are split-sampled circuits and others in turn)
    sampled = [dev.circuit_form(c)["split_sampled"] for c in base]
    pools = {True: [i for i, f in enumerate(sampled) if f], False: [i for i, f in enumerate(sampled) if not f]}
    order, want = [], True
    for position in range(len(base)):
        kind = want if position % 3 == 0 and pools[want] else bool(len(pools[True]) >= len(pools[False]))
        kind = kind if pools[kind] else not kind
        order.append(pools[kind].pop(0))
        if position % 3 == 0:
            want = not want
    base, base_params = [base[i] for i in order], [base_params[i] for i in order]
    circuits = [c for c in base for _ in (0, 1)]  # (pairs, as a search's plus / minus points)
    rng = np.random.default_rng(3)
    params = [list(np.asarray(p) + s * 0.35 * rng.choice([-1.0, 1.0], size=len(p))) for p in base_params for s in (1, -1)]
    try:
        _, forms = _routes(dev, op, circuits)
        matrix = _matrix(params)
        n_pairs = len(base)
        flags = np.ones(n_pairs, dtype=np.uint8)
        flags[::3] = 0
        off = [2 * r for r in range(n_pairs) if not flags[r]]
        assert any(forms[i]["split_sampled"] for i in off) and any(not forms[i]["split_sampled"] for i in off)
        halves = [i for i, f in enumerate(forms) if f["halves"]]
        if halves:  # (none at this size on the devices seen so far: asserted, not assumed)
            flags[halves[0] // 2] = 0
        estimator = OperatorCircuitEvaluator(op, statevector_device=dev)
        before = estimator.evaluate_circuits(circuits, params)
        alpha = 0.3
        seeds = dict(seed=21)
        full = _to_device(_sampler(op, shots, alpha, dev, **seeds), circuits, matrix)
        assert not np.any(full == SENTINEL)
        keep = np.repeat(flags.astype(bool), 2)
        active = torch.from_numpy(flags).cuda()
        got = _to_device(_sampler(op, shots, alpha, dev, **seeds), circuits, matrix, active=active, stride=2)
        assert np.array_equal(got[keep], full[keep]) and np.all(got[~keep] == SENTINEL)
        # none switched off, all switched off, one entry per evaluation
        ones, zeros = torch.ones_like(active), torch.zeros_like(active)
        assert np.array_equal(_to_device(_sampler(op, shots, alpha, dev, **seeds), circuits, matrix, active=ones, stride=2), full)
        assert np.all(_to_device(_sampler(op, shots, alpha, dev, **seeds), circuits, matrix, active=zeros, stride=2) == SENTINEL)
        each = torch.from_numpy(np.repeat(flags, 2)).cuda()
        assert np.array_equal(_to_device(_sampler(op, shots, alpha, dev, **seeds), circuits, matrix, active=each, stride=1), got)
        # written on the handle's stream right before the call
        ev = _sampler(op, shots, alpha, dev, **seeds)
        stream = _chain_state(ev, torch.device("cuda", dev.device_index))["stream"]
        late = torch.ones_like(active)
        out = torch.full((len(circuits),), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            busy = torch.randn(2048, 2048, device="cuda")
            for _ in range(10):
                busy = busy @ busy * 1e-3
            late.copy_(active, non_blocking=True)
            ev.evaluate_device_to_device(circuits, matrix, out, active=late, active_stride=2)
        stream.synchronize()
        assert np.array_equal(out.cpu().numpy(), got)
        # the mode bit does not leak: the same evaluator and an estimator on the same device afterwards
        plain = _sampler(op, shots, alpha, dev, **seeds)
        assert np.array_equal(np.asarray(plain.evaluate_circuits(circuits, params)), full)
        assert estimator.evaluate_circuits(circuits, params) == before
        # alpha = 1 on the exact distribution is the expectation value; the mask withholds results there too
        if shots is None:
            exact_one = _to_device(_sampler(op, None, 1.0, dev), circuits, matrix, active=active, stride=2)
            assert np.array_equal(exact_one[keep], np.asarray(before)[keep]) and np.all(exact_one[~keep] == SENTINEL)
    finally:
        dev.close()


def test_refusals():
    """Kept-state circuit, non-diagonal operator, 4097 shots, a host pointer: each the documented error, and the handle
    serves the next call."""
    import torch

    from queasars_amd.evqe import EVQEPopulation

    n = 13
    op = helpers.random_ising_operator(n, seed=13)
    dev = StatevectorDevice(n)
    try:
        dev.set_operator(op)
        _, circuits, params = helpers.population_circuits(n, 3, 4, seed=1)
        matrix = _matrix(params)
        out = torch.zeros(4, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ids, _, _ = dev._batch_metadata(circuits)

        def call(ids=ids, n=4, matrix_ptr=matrix.data_ptr(), shots=16, alpha=0.5, out_ptr=out.data_ptr(), active=None, stride=1):
            return dev._lib.qsv_cvar_device(dev._handle, n, _lib.as_ptr(ids), matrix.shape[1], C.c_void_p(matrix_ptr), None, shots,
                                            C.c_uint64(3), alpha, active, stride, C.c_void_p(out_ptr))

        def works():
            assert call() == _lib.QSV_OK
            torch.cuda.synchronize()
            assert out.cpu().tolist() == dev.sample_cvar_batch(circuits, params, 16, 3, 0.5)

        works()
        assert call(shots=4097) == _lib.QSV_E_ARG and "4096" in _lib.last_error(dev._lib, dev._handle)
        works()
        assert call(alpha=0.0) == _lib.QSV_E_ARG and call(alpha=1.5) == _lib.QSV_E_ARG
        host = np.zeros((4, matrix.shape[1]))
        assert call(matrix_ptr=host.ctypes.data) == _lib.QSV_E_ARG and "device_values" in _lib.last_error(dev._lib, dev._handle)
        host_out = np.zeros(4)
        assert call(out_ptr=host_out.ctypes.data) == _lib.QSV_E_ARG and "device_out" in _lib.last_error(dev._lib, dev._handle)
        works()
        with pytest.raises(ValueError):
            dev.cvar_of_device_parameters(circuits, matrix.data_ptr(), matrix.shape[1], 0, 4097, 3, 0.5, out.data_ptr())
        # a circuit on a kept state
        population = EVQEPopulation.random_population(n, 3, 2, True, 2)
        pairs = [ind.get_layer_search_circuits(2) for ind in population.individuals]
        values = [list(ind.get_layer_parameter_values(2)) for ind in population.individuals]
        states = dev.keep_states([front for front, _ in pairs], [[] for _ in pairs])
        kept = [rest.continue_from(state) for (_, rest), state in zip(pairs, states)]
        kept_matrix = _matrix(values)
        for shots in (0, 16):
            with pytest.raises(CircuitEvaluatorException, match="kept states are not sampled"):
                dev.cvar_of_device_parameters(kept, kept_matrix.data_ptr(), kept_matrix.shape[1], 0, shots, 3, 0.5, out.data_ptr())
        works()
        # a non-diagonal operator
        dev.set_operator(helpers.random_pauli_operator(n, 6, seed=4))
        assert call() == _lib.QSV_E_STATE and call(shots=0) == _lib.QSV_E_STATE
        dev.set_operator(op)
        works()
    finally:
        dev.close()


def _search_jobs(pop, cfg, embedded):
    jobs = []
    for k, ind in enumerate(pop.individuals):
        if embedded:  # (the last layer's angles inside the individual's fully parameterised circuit, as the solver shares circuits)
            layer = len(ind.layers) - 1
            start = ind.circuit_parameter_offsets[layer]
            run = cfg.new_run(ind.get_layer_parameter_values(-1), seed=k)
            run.embed = (np.asarray(ind.parameter_values_in_circuit_order(), dtype=np.float64),
                         np.arange(start, start + ind.layers[layer].n_parameters, dtype=np.int64))
            jobs.append((ind.get_parameterized_quantum_circuit(shared=True), run))
        else:
            jobs.append((ind.get_partially_parameterized_quantum_circuit({-1}), cfg.new_run(ind.get_layer_parameter_values(-1), seed=k)))
    return jobs


@pytest.mark.parametrize("with_checker,trust_region,embedded", [(False, True, False), (True, True, False), (True, False, False),
                                                                (True, True, True)])
def test_search_on_the_exact_distribution_against_the_host_driver(with_checker, trust_region, embedded, monkeypatch):
    """``sampler_shots=None``, alpha 0.3: the device search against the host driver on copies of the same jobs -- the same
    stopping iterations and ``nfev``, iterates within 1e-9 (the exact CVaR is Lipschitz in the angles, so last-bit differences
    of the trust region's norm cannot move it by more), twice, and the same with the mask not handed through."""
    from queasars_amd.evqe import EVQEPopulation
    from queasars_amd.evqe import solver as S

    n = 14
    pop = EVQEPopulation.random_population(n, 3, 24, True, 5)
    # (the reference's termination rule divides a change by the previous value, so below zero it is met at once: an identity
    # term lifts the CVaR of this Ising operator above zero, and the runs stop anywhere between 3 and 20 iterations)
    ising = helpers.random_ising_operator(n, seed=2020)
    op = PauliOperator(list(ising.labels) + ["I" * n], list(ising.coeffs) + [0.3 * float(np.abs(ising.coeffs).sum())])
    ev = OperatorSamplerCircuitEvaluator(None, op, alpha=0.3)
    checker = S.SPSATerminationChecker(0.02, 1) if with_checker else None
    cfg = S.SPSA(maxiter=20, trust_region=trust_region, termination_checker=checker)
    host = _search_jobs(pop, cfg, embedded)
    S._minimize_batched(ev, host)
    for masked in (True, True, False):  # (twice: the second search finds the stream, the buffers and the layouts of the first)
        if not masked:
            monkeypatch.setenv("QSV_DEVICE_SEARCH_MASK", "0")
        device = _search_jobs(pop, cfg, embedded)
        S._minimize_batched(ev, device, on_device=True)
        assert [run.iteration for _, run in device] == [run.iteration for _, run in host]
        assert [run.nfev for _, run in device] == [run.nfev for _, run in host]
        assert all(run.done for _, run in device)
        worst = max(np.abs(a.x - b.x).max() for (_, a), (_, b) in zip(device, host))
        print(f"checker={with_checker} trust_region={trust_region} embedded={embedded} masked={masked}: max |dx| = {worst:.3e}")
        assert worst < 1e-9
    if with_checker:
        print("stopping iterations:", sorted({run.iteration for _, run in host}))
        assert len({run.iteration for _, run in host}) > 3  # (the runs did stop at different iterations)


def test_search_with_shots_uses_the_values_of_its_own_points(monkeypatch):
    """With shots a last-bit difference of an iterate can move a draw, and one moved draw moves the CVaR by a whole sample
    value: the device search cannot be held to the host driver's iterates.  Instead: no termination checker, a few iterations,
    and every iteration's points replayed through ``sample_cvar_batch`` with the seeds a same-seeded evaluator draws -- the
    values the search used are those, bit for bit."""
    import torch

    from queasars_amd.evqe import EVQEPopulation
    from queasars_amd.evqe import device_search
    from queasars_amd.evqe import solver as S

    n, shots, alpha = 14, 400, 0.5
    pop = EVQEPopulation.random_population(n, 3, 18, True, 6)
    op = helpers.random_ising_operator(n, seed=77)
    ev = OperatorSamplerCircuitEvaluator(shots, op, alpha=alpha, seed=99)
    twin_rng = np.random.default_rng(99)
    cfg = S.SPSA(maxiter=4, trust_region=True, termination_checker=None)
    jobs = _search_jobs(pop, cfg, False)
    assert device_search.supported(ev, jobs)
    seen = []
    inner = ev.evaluate_device_to_device

    def recording(circuits, matrix, out, active=None, active_stride=1):
        inner(circuits, matrix, out, active=active, active_stride=active_stride)
        torch.cuda.current_stream().synchronize()
        seen.append((list(circuits), matrix.cpu().numpy().copy(), out.cpu().numpy().copy()))

    monkeypatch.setattr(ev, "evaluate_device_to_device", recording)
    device_search.minimize_spsa_on_device(ev, jobs)
    assert len(seen) == 4 and all(run.iteration == 4 and run.nfev == 8 for _, run in jobs)
    dev = ev.statevector_device
    for circuits, points, values in seen:
        seed = int(twin_rng.integers(0, 2**63 - 1))
        rows = [points[i, : c.num_parameters].tolist() for i, c in enumerate(circuits)]
        assert np.array_equal(values, np.asarray(dev.sample_cvar_batch(circuits, rows, shots, seed, alpha)))


def test_solver_default_stays_on_the_host_and_true_takes_the_device_search(monkeypatch):
    """EVQE on a small JSSP instance with a sampler evaluator and a population of 16 (so that the default rule decides):
    ``device_resident_search=None`` reproduces the run with ``False`` number for number and never enters the device search;
    ``True`` enters it and ends on a valid schedule."""
    import jssp_instances as inst
    from queasars_amd.evqe import device_search
    from queasars_amd.evqe.solver import (
        SPSA, BestIndividualRelativeChangeTolerance, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration, SPSATerminationChecker,
    )
    from queasars_amd.job_shop_scheduling import JSSPDomainWallHamiltonianEncoder

    enc = JSSPDomainWallHamiltonianEncoder(inst.notebook_2x3(), makespan_limit=6, **inst.NOTEBOOK_PENALTIES)
    assert enc.n_qubits == 12
    op = enc.get_problem_hamiltonian()
    calls = []
    inner = device_search.minimize_spsa_on_device

    def counting(evaluator, jobs, *args, **kwargs):
        calls.append(len(jobs))
        return inner(evaluator, jobs, *args, **kwargs)

    monkeypatch.setattr(device_search, "minimize_spsa_on_device", counting)

    def run(flag, generations):
        evaluator = OperatorSamplerCircuitEvaluator(512, op, alpha=0.5, seed=0)
        cfg = EVQEMinimumEigensolverConfiguration(
            optimizer=SPSA(maxiter=33, perturbation=0.35, learning_rate=0.43, trust_region=True,
                           termination_checker=SPSATerminationChecker(0.01, 2)),
            population_size=16, max_generations=generations, termination_criterion=BestIndividualRelativeChangeTolerance(0.01, 1),
            random_seed=0, n_initial_layers=2, randomize_initial_population_parameters=True,
            speciation_genetic_distance_threshold=1, use_tournament_selection=True, tournament_size=2,
            selection_alpha_penalty=0.15, selection_beta_penalty=0.02, parameter_search_probability=0.39,
            topological_search_probability=0.79, layer_removal_probability=0.02, device_resident_search=flag,
        )
        result = EVQEMinimumEigensolver(cfg).compute_minimum_eigenvalue(evaluator)
        return result, evaluator

    by_default, _ = run(None, 3)
    assert calls == []
    never, _ = run(False, 3)
    assert calls == []
    assert by_default.eigenvalue == never.eigenvalue
    assert list(by_default.best_individual.parameter_values) == list(never.best_individual.parameter_values)
    on_device, evaluator = run(True, 8)
    assert calls and max(calls) >= 16
    best = on_device.best_individual
    probs = evaluator.statevector_device.probabilities(best.get_parameterized_quantum_circuit(), list(best.parameter_values))
    schedule = enc.translate_result_bitstring(format(int(np.argmax(probs)), f"0{enc.n_qubits}b"))
    assert schedule.is_valid
