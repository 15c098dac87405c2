"""Several observables per evaluation on the device (qsv_eval_observables, StatevectorDevice.observable_values and the layers
above it): per-string values against the oracle on every route, columns against the one-operator evaluator, bitwise
determinism, no effect on the handle's own operator, GpuEstimator array pubs, aux operators of the solver, argument errors."""

import ctypes as C

import numpy as np
import pytest

import helpers
from oracle import statevector_oracle as so
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, OperatorSamplerCircuitEvaluator
from queasars_amd.circuit_evaluation.circuit_evaluation import StatevectorDevice
from queasars_amd.evqe import EVQEPopulation
from queasars_amd.ir import PauliOperator
from queasars_amd.primitives import GpuEstimator

pytestmark = pytest.mark.gpu

ROUTE_ONE_TILE, ROUTE_SPLIT_ONE_LAUNCH, ROUTE_SPLIT, ROUTE_PASSES = 0, 1, 2, 3


def random_strings(n, extra, seed):
    """One Pauli string of every weight 0 .. n (random qubits, random X / Y / Z factors), `extra` random strings of any
    weight, and a few repeated: each as an operator of its own with coefficient 1."""
    rng = np.random.default_rng(seed)
    strings = []
    for weight in list(range(n + 1)) + [int(w) for w in rng.integers(0, n + 1, size=extra)]:
        qubits = sorted(rng.choice(n, size=weight, replace=False).tolist())
        kinds = "".join(rng.choice(list("XYZ"), size=weight))
        strings.append(PauliOperator(["I" * n], [1.0]) if weight == 0 else PauliOperator.from_sparse_list([(kinds, qubits, 1.0)], n))
    strings += [strings[3], strings[-1], strings[0]]  # duplicates across observables (and the identity twice)
    return strings


def oracle_terms(circuit, params, operators):
    state = helpers.oracle_state(circuit, params)
    return [so.pauli_term_expectation(state, int(op.x_mask[0]), int(op.z_mask[0])).real for op in operators]


def kept_state_circuits(dev, n, seed):
    """A layer search's circuits on kept states (as smoke() builds them) and the whole circuits they stand for."""
    population = EVQEPopulation.random_population(n, 3, 4, True, seed)
    whole = [ind.get_partially_parameterized_quantum_circuit({2}) for ind in population.individuals]
    values = [list(ind.get_layer_parameter_values(2)) for ind in population.individuals]
    pairs = [ind.get_layer_search_circuits(2) for ind in population.individuals]
    states = dev.keep_states([front for front, _ in pairs], [[] for _ in pairs])
    kept = [rest.continue_from(state) for (_, rest), state in zip(pairs, states)]
    return kept, whole, values, states


def pick_by_form(dev, circuits, params, want_keys, per_key=2):
    """Up to per_key circuits of each split form with n_keys in want_keys (and the forms of all)."""
    chosen, seen = [], {}
    for c, p in zip(circuits, params):
        f = dev.circuit_form(c)
        key = f["n_keys"] if f["route"] in (ROUTE_SPLIT_ONE_LAUNCH, ROUTE_SPLIT) else None
        if key in want_keys and seen.get(key, 0) < per_key:
            seen[key] = seen.get(key, 0) + 1
            chosen.append((c, p))
    return chosen, seen


@pytest.mark.parametrize("n", [6, 10, 13, 16, 20])
def test_per_string_values_against_the_oracle_on_every_route(n):
    strings = random_strings(n, 24, seed=n)
    dev = StatevectorDevice(n)
    cases = []  # (circuit run on the device, circuit for the oracle, parameters)
    routes = set()
    _, shallow, p_shallow = helpers.population_circuits(n, 3, 3, seed=n)
    _, deep, p_deep = helpers.population_circuits(n, 8, 3, seed=n + 1)
    cases += [(c, c, p) for c, p in zip(shallow + deep, p_shallow + p_deep)]
    if n == 20:
        # split forms of zero to three keys (the benchmark population), and of four and five keys under a quadratic operator
        _, pop, pp = helpers.population_circuits(20, 4, 64, seed=0)
        _, pop2, pp2 = helpers.population_circuits(20, 5, 32, seed=1)
        chosen, seen = pick_by_form(dev, pop + pop2, pp + pp2, {0, 1, 2, 3})
        assert set(seen) == {0, 1, 2, 3}, seen
        cases += [(c, c, p) for c, p in chosen]
        dev.set_operator(helpers.random_ising_operator(20, seed=3))
        _, wide, pw = helpers.population_circuits(20, 6, 32, seed=0)
        _, wide2, pw2 = helpers.population_circuits(20, 5, 8, seed=0)
        chosen, seen = pick_by_form(dev, wide + wide2, pw + pw2, {4, 5}, per_key=1)
        assert set(seen) == {4, 5}, seen
        cases += [(c, c, p) for c, p in chosen]
    if n == 13:
        kept, whole, values, _states = kept_state_circuits(dev, n, seed=2)
        cases += list(zip(kept, whole, values))
        assert all(dev.circuit_cost(c)["on_kept_state"] for c in kept)
    for c, _, _ in cases:
        routes.add(dev.circuit_form(c)["route"])
    got = dev.observable_values([c for c, _, _ in cases], [p for _, _, p in cases], strings)
    assert got.shape == (len(cases), len(strings))
    for row, (_, ref_circuit, p) in zip(got, cases):
        np.testing.assert_allclose(row, oracle_terms(ref_circuit, p, strings), rtol=0, atol=1e-12)
    if n <= 10:
        assert routes == {ROUTE_ONE_TILE}
    else:
        assert ROUTE_PASSES in routes
    if n == 20:
        assert ROUTE_SPLIT_ONE_LAUNCH in routes or ROUTE_SPLIT in routes
    dev.close()


def qubo_like(n, seed):
    rng = np.random.default_rng(seed)
    terms = [("I", [0], 3.5)] + [("Z", [q], float(rng.normal())) for q in range(n)]
    terms += [("ZZ", [a, b], float(rng.normal())) for a in range(n) for b in range(a + 1, n) if rng.random() < 0.3]
    return PauliOperator.from_sparse_list(terms, n)


def test_columns_equal_the_one_operator_evaluator():
    n = 20
    _, circuits, params = helpers.population_circuits(n, 4, 64, seed=0)
    ops = [helpers.random_ising_operator(n, seed=11), qubo_like(n, seed=12), helpers.random_pauli_operator(n, 500, seed=13)]
    dev = StatevectorDevice(n)
    got = dev.observable_values(circuits, params, ops)
    for m, op in enumerate(ops):
        want = np.asarray(OperatorCircuitEvaluator(op, statevector_device=dev).evaluate_circuits(circuits, params))
        np.testing.assert_allclose(got[:, m], want, rtol=0, atol=1e-12)
    dev.close()


def test_values_do_not_depend_on_the_batch():
    n = 20
    _, circuits, params = helpers.population_circuits(n, 4, 64, seed=0)
    _, deep, p_deep = helpers.population_circuits(n, 8, 8, seed=5)
    ops = [helpers.random_ising_operator(n, seed=11), helpers.random_pauli_operator(n, 60, seed=14)] + random_strings(n, 8, seed=2)
    dev = StatevectorDevice(n)
    batch = dev.observable_values(circuits, params, ops)
    reverse = dev.observable_values(circuits[::-1], params[::-1], ops)[::-1]
    assert np.array_equal(batch, reverse)
    mixed = dev.observable_values(deep + circuits[:16] + deep, p_deep + params[:16] + p_deep, ops)
    assert np.array_equal(mixed[8:24], batch[:16])
    for i in (0, 8, 41, 63):
        assert np.array_equal(dev.observable_values([circuits[i]], [params[i]], ops)[0], batch[i])
    assert np.array_equal(mixed[:8], mixed[24:])
    single = StatevectorDevice(n, dtype="fp32")
    low = single.observable_values(circuits, params, ops)
    scale = np.asarray([np.abs(op.coeffs).sum() for op in ops])
    assert np.all(np.abs(low - batch) <= 2e-6 * scale)
    single.close()
    dev.close()


def test_no_effect_on_the_handles_operator():
    n = 20
    _, circuits, params = helpers.population_circuits(n, 4, 64, seed=0)
    _, deep, p_deep = helpers.population_circuits(n, 8, 8, seed=5)
    for op in (helpers.random_ising_operator(n, seed=21), helpers.random_pauli_operator(n, 40, seed=22)):
        dev = StatevectorDevice(n)
        ev = OperatorCircuitEvaluator(op, statevector_device=dev)
        population = circuits + deep
        values = params + p_deep
        before = np.asarray(ev.evaluate_circuits(population, values))
        repeated = np.asarray(ev.evaluate_circuits(population, values))  # (a repeated batch: repeat_layout keeps its layout)
        dev.observable_values(deep[:3] + circuits[:5], p_deep[:3] + params[:5], [qubo_like(n, 1), op])
        after = np.asarray(ev.evaluate_circuits(population, values))
        again = np.asarray(ev.evaluate_circuits(population, values))
        assert np.array_equal(before, repeated) and np.array_equal(before, after) and np.array_equal(before, again)
        dev.close()


def test_estimator_array_pub():
    n = 10
    _, circuits, _ = helpers.population_circuits(n, 3, 1, seed=4)
    circuit = circuits[0]
    rng = np.random.default_rng(0)
    matrix = rng.uniform(-np.pi, np.pi, size=(4, circuit.num_parameters))
    ops = [helpers.random_ising_operator(n, seed=1), helpers.random_pauli_operator(n, 30, seed=2), helpers.random_ising_operator(n, seed=1)]
    est = GpuEstimator()
    results = est.run([(circuit, [[ops[0]], [ops[1]], [ops[2]]], matrix), (circuit, ops[1], matrix[0])]).result()
    evs = results[0].data.evs
    assert evs.shape == (3, 4)
    for m in range(3):
        for b in range(4):
            assert abs(evs[m, b] - helpers.oracle_expectation(circuit, list(matrix[b]), ops[m])) < 1e-12
    assert np.ndim(results[1].data.evs) == 0
    assert abs(float(results[1].data.evs) - helpers.oracle_expectation(circuit, list(matrix[0]), ops[1])) < 1e-12
    # an array of observables on a circuit without parameters: no values, or an empty vector
    bound = helpers.bound_copy(circuit, list(matrix[1]))
    want = [helpers.oracle_expectation(bound, [], op) for op in ops[:2]]
    for pub in ((bound, ops[:2]), (bound, ops[:2], []), (bound, np.asarray(ops[:2], dtype=object), None)):
        evs = est.run([pub]).result()[0].data.evs
        assert evs.shape == (2,)
        np.testing.assert_allclose(evs, want, rtol=0, atol=1e-12)


def _solver_config():
    from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolverConfiguration

    return EVQEMinimumEigensolverConfiguration(
        optimizer=SPSA(maxiter=8, perturbation=0.35, learning_rate=0.43), population_size=6, max_generations=2, random_seed=0,
        n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=1,
        use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.15, selection_beta_penalty=0.02,
        parameter_search_probability=0.39, topological_search_probability=0.79, layer_removal_probability=0.02,
    )


def test_solver_aux_operators_on_the_device():
    import jssp_instances as inst
    from queasars_amd.evqe.solver import EVQEMinimumEigensolver
    from queasars_amd.job_shop_scheduling import JSSPDomainWallHamiltonianEncoder

    enc = JSSPDomainWallHamiltonianEncoder(inst.notebook_2x3(), makespan_limit=6, **inst.NOTEBOOK_PENALTIES)
    op = enc.get_problem_hamiltonian()
    n = op.num_qubits
    aux = [PauliOperator.from_sparse_list([("ZZ", [0, 5], 1.0), ("Z", [3], -0.5)], n), PauliOperator.from_sparse_list([("Z", [n - 1], 2.0)], n)]

    def best_state(result):
        ind = result.best_individual
        return helpers.oracle_state(ind.get_parameterized_quantum_circuit(), list(ind.parameter_values))

    result = EVQEMinimumEigensolver(_solver_config()).compute_minimum_eigenvalue(OperatorCircuitEvaluator(op), aux_operators=aux)
    state = best_state(result)
    want = [so.pauli_expectation(state, a.x_mask.tolist(), a.z_mask.tolist(), a.coeffs.tolist()).real for a in aux]
    np.testing.assert_allclose(result.aux_operators_evaluated, want, rtol=0, atol=1e-12)

    sampler = OperatorSamplerCircuitEvaluator(None, op, alpha=0.5)
    named = {"a": aux[0], "b": aux[1]}
    result = EVQEMinimumEigensolver(_solver_config()).compute_minimum_eigenvalue(sampler, aux_operators=named)
    assert list(result.aux_operators_evaluated) == ["a", "b"]
    probs = so.probabilities(best_state(result))
    for name, a in named.items():
        values = so.diagonal_values(n, a.z_mask.tolist(), a.coeffs.real.tolist())
        want = so.cvar_expectation([(i, float(probs[i]), float(values[i])) for i in range(1 << n)], 0.5)
        assert abs(result.aux_operators_evaluated[name] - want) < 1e-10
    assert sampler.statevector_device._operator is op  # (the device's operator is left as it was)


def test_sampled_aux_values_are_the_cvar_of_the_same_samples():
    """With shots, evaluate_observables values ONE draw of samples per circuit for every operator: each column equals what a
    sampler evaluator of that operator alone returns for the same seed (the same samples, its CVaR taken on the device)."""
    n = 12
    _, circuits, params = helpers.population_circuits(n, 3, 6, seed=3)
    main = helpers.random_ising_operator(n, seed=1)
    aux = [helpers.random_ising_operator(n, seed=2), PauliOperator.from_sparse_list([("Z", [0], 1.0), ("ZZ", [3, 7], -0.5)], n)]
    for alpha in (1.0, 0.3):
        evaluator = OperatorSamplerCircuitEvaluator(1024, main, alpha=alpha, seed=9)
        got = np.asarray(evaluator.evaluate_observables(circuits, params, aux))
        assert got.shape == (len(circuits), len(aux))
        for m, op in enumerate(aux):
            want = OperatorSamplerCircuitEvaluator(1024, op, alpha=alpha, seed=9).evaluate_circuits(circuits, params)
            np.testing.assert_allclose(got[:, m], want, rtol=0, atol=1e-10)
        assert evaluator.statevector_device._operator is main
    with pytest.raises(ValueError):
        OperatorSamplerCircuitEvaluator(64, main).evaluate_observables(circuits, params, [helpers.random_pauli_operator(n, 4, seed=1)])


def test_argument_errors_on_a_device():
    dev = StatevectorDevice(6)
    lib, h = dev._lib, dev._handle
    one = np.asarray([0, 1], dtype=np.int64)
    x, z, c = np.zeros(1, np.uint64), np.ones(1, np.uint64), np.ones(1)
    out = C.c_int(0)
    ok = lib.qsv_observables_create(h, 1, _lib.as_ptr(one), _lib.as_ptr(x), _lib.as_ptr(z), _lib.as_ptr(c), _lib.as_ptr(c), C.byref(out))
    assert ok == _lib.QSV_OK
    good = out.value
    far = np.asarray([1 << 6], dtype=np.uint64)
    assert lib.qsv_observables_create(h, 1, _lib.as_ptr(one), _lib.as_ptr(far), _lib.as_ptr(z), _lib.as_ptr(c), None,
                                      C.byref(out)) == _lib.QSV_E_ARG
    assert lib.qsv_observables_create(h, 0, _lib.as_ptr(one), _lib.as_ptr(x), _lib.as_ptr(z), _lib.as_ptr(c), None,
                                      C.byref(out)) == _lib.QSV_E_ARG
    too_many = np.zeros((1 << 16) + 2, dtype=np.int64)
    assert lib.qsv_observables_create(h, (1 << 16) + 1, _lib.as_ptr(too_many), _lib.as_ptr(x), _lib.as_ptr(z), _lib.as_ptr(c), None,
                                      C.byref(out)) == _lib.QSV_E_ARG
    # every one of the 4096 Pauli strings of six qubits, one per observable, and a 4097th observable without terms (= 0)
    big = np.arange(4098, dtype=np.int64)
    big[-1] = 4096
    xs = np.asarray([k % 64 for k in range(4096)], dtype=np.uint64)
    zs = np.asarray([k // 64 for k in range(4096)], dtype=np.uint64)
    ones = np.ones(4096)
    assert lib.qsv_observables_create(h, 4097, _lib.as_ptr(big), _lib.as_ptr(xs), _lib.as_ptr(zs), _lib.as_ptr(ones), None,
                                      C.byref(out)) == _lib.QSV_OK
    big_id = out.value
    _, circuits, params = helpers.population_circuits(6, 2, 1, seed=0)
    cid = np.asarray([dev.circuit_id(circuits[0])], dtype=np.int32)
    offsets = np.asarray([0, len(params[0])], dtype=np.int64)
    values = np.asarray(params[0], dtype=np.float64)
    res = np.zeros(4097)
    assert lib.qsv_eval_observables(h, big_id, 1, _lib.as_ptr(cid), _lib.as_ptr(offsets), _lib.as_ptr(values), _lib.as_ptr(res)) == _lib.QSV_OK
    assert res[-1] == 0.0
    assert abs(res[0] - 1.0) < 1e-12  # (x = 0, z = 0: the identity)
    state = helpers.oracle_state(circuits[0], params[0])
    want = [so.pauli_term_expectation(state, int(x), int(z)).real for x, z in zip(xs, zs)]
    np.testing.assert_allclose(res[:4096], want, rtol=0, atol=1e-12)
    assert lib.qsv_eval_observables(h, 987654, 1, _lib.as_ptr(cid), _lib.as_ptr(offsets), _lib.as_ptr(values), _lib.as_ptr(res)) == _lib.QSV_E_ARG
    bad = np.asarray([987654], dtype=np.int32)
    assert lib.qsv_eval_observables(h, good, 1, _lib.as_ptr(bad), _lib.as_ptr(offsets), _lib.as_ptr(values), _lib.as_ptr(res)) == _lib.QSV_E_ARG
    assert lib.qsv_observables_destroy(h, good) == _lib.QSV_OK
    assert lib.qsv_observables_destroy(h, good) == _lib.QSV_E_ARG
    assert lib.qsv_eval_observables(h, good, 1, _lib.as_ptr(cid), _lib.as_ptr(offsets), _lib.as_ptr(values), _lib.as_ptr(res)) == _lib.QSV_E_ARG
    dev.close()
