"""GPU tests of the parameter-shift gradients (include/qsv.h: qsv_gradient_circuits, qsv_gradient_device).

The defining property is bitwise: a gradient entry is the documented combination (tests/shift_rules.py restates it in NumPy) of
what ``evaluate_circuits`` returns at the documented shifted points -- for any batch, any ``wrt``, any chunk size and either
entry point.  Against the plain-C oracle: fp64 within 1e-10 (the project's fp64 tolerance; the combination's coefficients sum
to at most 1 in absolute value), fp32 within 2e-6 * sum |c_k|.  Run on the MI355X box with -m gpu."""

import ctypes as C

import numpy as np
import pytest

import helpers
import shift_rules
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import CircuitEvaluatorException, OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe import EVQEPopulation
from queasars_amd.evqe.solver import SPSA, Adam, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration
from queasars_amd.ir import CircuitIR, ParamRef, PauliOperator

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10
FP32_REL = 2e-6
P = ParamRef


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def assert_same_bits(got, want, what=""):
    assert len(got) == len(want), what
    for e, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), f"{what}: circuit {e}"


class ShiftedValues:
    """``evaluate_circuits`` at every shifted point of the FULL gradient of a population, computed once and shared: any
    ``wrt`` selects its values from these (an evaluation's value does not depend on its batch).  One ``evaluate_circuits``
    call per circuit: a few hundred evaluations of ONE structure, a reference that shares no batch with what it is compared
    to.  (One call over all of them holds the same bits: tests/test_gpu_large_batches.py compares that call with these.)"""

    def __init__(self, evaluator, circuits, params):
        self.circuits, self.params = circuits, params
        self.terms = [c.gradient_terms() for c in circuits]
        self.values = []
        for c, t, p in zip(circuits, self.terms, params):
            assert min(t, default=0) >= 0, "no circuit of these populations may be refused"
            points = shift_rules.shifted_points(t, p)
            values = evaluator.evaluate_circuits([c] * len(points), points) if points else []
            self.values.append(np.asarray(values, dtype=np.float64))
        self.n_shifted = sum(len(v) for v in self.values)

    def expected(self, wrt=None) -> list[np.ndarray]:
        """The NumPy combination for ``wrt`` (None, one list for all, or one list per circuit)."""
        out = []
        for e, (t, v) in enumerate(zip(self.terms, self.values)):
            if wrt is None:
                out.append(shift_rules.combine(t, v))
                continue
            w = wrt if np.ndim(wrt[0]) == 0 else wrt[e]
            starts = np.concatenate([[0], np.cumsum(t)])
            picked = np.concatenate([v[starts[p]: starts[p] + t[p]] for p in w]) if len(w) else np.zeros(0)
            out.append(shift_rules.combine(t, picked, w))
        return out

    def count(self, wrt=None) -> int:
        if wrt is None:
            return self.n_shifted
        return sum(sum(t[p] for p in (wrt if np.ndim(wrt[0]) == 0 else wrt[e])) for e, t in enumerate(self.terms))


def device_gradients(evaluator, circuits, params, wrt=None, out_width=None, stream=None):
    """The device entry point: points in a padded matrix, gradients (and padding) read back after ONE stream synchronise."""
    import torch

    width = max(len(p) for p in params) + 1  # (an odd row length among them: rows need not be aligned)
    matrix = torch.zeros((len(circuits), width), dtype=torch.float64, device="cuda")
    for e, p in enumerate(params):
        matrix[e, : len(p)] = torch.tensor(p, dtype=torch.float64)
    counts = [c.num_parameters if wrt is None else len(wrt if np.ndim(wrt[0]) == 0 else wrt[e]) for e, c in enumerate(circuits)]
    out_width = out_width or max(counts) + 3
    out = torch.full((len(circuits), out_width), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    evaluator.evaluate_gradients_device_to_device(circuits, matrix, out, wrt)
    (stream or torch.cuda).synchronize()
    if stream is None:
        torch.cuda.synchronize()
    host = out.cpu().numpy()
    for e, k in enumerate(counts):
        assert np.array_equal(bits(host[e, k:]), np.zeros(out_width - k, dtype=np.uint64)), f"padding of row {e}"
    return [host[e, :k].copy() for e, k in enumerate(counts)]


# ---- the bitwise definition ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def headline():
    """n = 20, L = 4, P = 64 (seed 0) under the 210-term Ising operator: the benchmark's population."""
    population, circuits, params = helpers.population_circuits(20, 4, 64, seed=0)
    op = helpers.random_ising_operator(20, seed=0)
    assert len(op) == 210
    evaluator = OperatorCircuitEvaluator(op)
    return population, evaluator, ShiftedValues(evaluator, circuits, params)


def _layer_positions(individual, layer):
    start = individual.circuit_parameter_offsets[layer]
    return list(range(start, start + individual.layers[layer].n_parameters))


def _wrt_cases(population, circuits):
    layer = [_layer_positions(ind, 2) for ind in population.individuals]
    rng = np.random.default_rng(5)
    ragged = [rng.permutation(c.num_parameters)[: 1 + e % 9].tolist() for e, c in enumerate(circuits)]
    ragged[3] = []  # (a circuit nothing is asked of)
    return {"full": None, "layer": layer, "ragged": ragged}


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("which", ["full", "layer", "ragged"])
def test_headline_gradients_are_the_combination_of_evaluate_circuits(headline, which, entry):
    population, evaluator, shifted = headline
    wrt = _wrt_cases(population, shifted.circuits)[which]
    want = shifted.expected(wrt)
    if entry == "host":
        got = evaluator.evaluate_gradients(shifted.circuits, shifted.params, wrt)
    else:
        got = device_gradients(evaluator, shifted.circuits, shifted.params, wrt)
    assert evaluator.last_gradient_evaluations == shifted.count(wrt)
    assert_same_bits(got, want, f"{which} / {entry}")
    assert max(np.abs(g).max(initial=0.0) for g in got) > 1e-3  # (not a gradient of zeros)


@pytest.mark.parametrize("which,chunk", [("full", 1000), ("layer", 7), ("ragged", 3)])
def test_a_chunk_boundary_changes_no_bit(headline, which, chunk):
    """Chunks far smaller than a circuit's terms (about 700 for the full gradient, 130 for a layer): boundaries fall inside
    circuits and inside a parameter's two or four evaluations."""
    population, evaluator, shifted = headline
    wrt = _wrt_cases(population, shifted.circuits)[which]
    dev = evaluator.statevector_device
    dev.set_option("gradient_chunk", chunk)
    try:
        got = evaluator.evaluate_gradients(shifted.circuits, shifted.params, wrt)
        stats = dev.gradient_stats()
        assert stats["n_shifted"] == shifted.count(wrt) and stats["n_chunks"] == -(-shifted.count(wrt) // chunk) > 1
        assert_same_bits(got, shifted.expected(wrt), f"{which} / host / chunks of {chunk}")
        if which != "full":
            assert_same_bits(device_gradients(evaluator, shifted.circuits, shifted.params, wrt), shifted.expected(wrt),
                             f"{which} / device / chunks of {chunk}")
    finally:
        dev.set_option("gradient_chunk", 0)


def _mixed(n, seed=0):
    circuits, params = [], []
    for layers, count in ((2, 2), (4, 2), (6, 1), (9, 1)):
        _, c, p = helpers.population_circuits(n, layers, count, seed=seed + layers)
        circuits += c
        params += p
    return circuits, params


@pytest.mark.parametrize("n", range(13, 21))
def test_mixed_depths_are_the_combination_of_evaluate_circuits(n):
    circuits, params = _mixed(n)
    evaluator = OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=n))
    shifted = ShiftedValues(evaluator, circuits, params)
    print(f"n = {n}: routes {sorted({c['route'] for c in evaluator.circuit_costs(circuits)})}, {shifted.n_shifted} shifted evaluations")
    assert_same_bits(evaluator.evaluate_gradients(circuits, params), shifted.expected(), f"n = {n} / host")
    assert evaluator.last_gradient_evaluations == shifted.n_shifted
    rng = np.random.default_rng(n)
    ragged = [rng.permutation(c.num_parameters)[: 2 + e].tolist() for e, c in enumerate(circuits)]
    assert_same_bits(device_gradients(evaluator, circuits, params, ragged), shifted.expected(ragged), f"n = {n} / device")
    evaluator.statevector_device.set_option("gradient_chunk", 5)
    assert_same_bits(evaluator.evaluate_gradients(circuits, params, ragged), shifted.expected(ragged), f"n = {n} / chunks of 5")


# ---- against the oracle ------------------------------------------------------------------------------------------------


def _strata_population():
    """n = 20 circuits of every route: four layers (one launch, with and without half sides), six (split with launches of its
    own: four and five keys), nine (gate passes over the state)."""
    circuits, params = [], []
    for layers, count, seed in ((4, 64, 0), (6, 12, 0), (9, 2, 8)):
        _, c, p = helpers.population_circuits(20, layers, count, seed=seed)
        circuits += c
        params += p
    return circuits, params


def _stratum(form) -> str:
    route = _lib.ROUTE_NAMES[form["route"]]
    if route == "split, one launch":
        return "half-sided" if form["halves"] else "one-launch"
    return {"split": "through-state", "gate passes": "multi-pass"}.get(route, route)


def _two_and_four(circuit):
    """A few parameters of both rules: the first two-term and the first two four-term ones, and the last parameter."""
    terms = circuit.gradient_terms()
    two = [p for p, t in enumerate(terms) if t == 2][:1]
    four = [p for p, t in enumerate(terms) if t == 4][:2]
    assert two and four
    return sorted(set(two + four + [len(terms) - 1]))


@pytest.fixture(scope="module")
def strata(c_oracle):
    """One circuit of each route (read through circuit_form) with its oracle gradient entries.  The names: ``one-launch`` and
    ``half-sided`` are the one-launch split route without / with half sides, ``through-state`` the split route whose sides go
    through their state tables to launches of their own, ``multi-pass`` the gate passes over the 2^n state."""
    circuits, params = _strata_population()
    op = helpers.random_ising_operator(20, seed=0)
    evaluator = OperatorCircuitEvaluator(op)
    evaluator.circuit_costs(circuits)  # (registers them under the operator)
    dev = evaluator.statevector_device
    chosen = {}
    for c, p in zip(circuits, params):
        chosen.setdefault(_stratum(dev.circuit_form(c)), (c, p))
    assert set(chosen) >= {"one-launch", "half-sided", "through-state", "multi-pass"}, sorted(chosen)
    table, scratch = c_oracle.diagonal_table(op), np.zeros(2 << 20)
    cases = {}
    for name in ("one-launch", "half-sided", "through-state", "multi-pass"):
        c, p = chosen[name]
        wrt = _two_and_four(c)
        terms = c.gradient_terms()
        values = [c_oracle.evaluate(c, point, op, table, scratch) for point in shift_rules.shifted_points(terms, p, wrt)]
        cases[name] = (c, p, wrt, shift_rules.combine(terms, values, wrt))
    return op, evaluator, cases


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_every_route_against_the_oracle(strata, dtype):
    op, evaluator, cases = strata
    if dtype == "fp32":
        evaluator = OperatorCircuitEvaluator(op, dtype="fp32")
    tol = EXP_TOL if dtype == "fp64" else FP32_REL * float(np.abs(op.coeffs).sum())
    names = list(cases)
    got = evaluator.evaluate_gradients([cases[k][0] for k in names], [cases[k][1] for k in names], [cases[k][2] for k in names])
    for name, g in zip(names, got):
        deviation = float(np.abs(g - cases[name][3]).max())
        print(f"{dtype} {name}: largest deviation {deviation:.3e} (bound {tol:.3e})")
        assert deviation < tol, (dtype, name)


def test_general_operator_against_the_oracle(c_oracle):
    """n = 20 under 500 Pauli strings: both entry points are the combination of evaluate_circuits, and the oracle's within 1e-10."""
    _, circuits, params = helpers.population_circuits(20, 4, 3, seed=0)
    op = helpers.random_pauli_operator(20, 500, seed=6)
    assert len(op) == 500 and not op.is_diagonal()
    evaluator = OperatorCircuitEvaluator(op)
    wrt = [_two_and_four(c)[:2] for c in circuits]
    owners, points = [], []
    for c, p, w in zip(circuits, params, wrt):
        own = shift_rules.shifted_points(c.gradient_terms(), p, w)
        owners += [c] * len(own)
        points += own
    values = np.asarray(evaluator.evaluate_circuits(owners, points))
    want, cur = [], 0
    for c, w in zip(circuits, wrt):
        k = sum(c.gradient_terms()[p] for p in w)
        want.append(shift_rules.combine(c.gradient_terms(), values[cur: cur + k], w))
        cur += k
    got = evaluator.evaluate_gradients(circuits, params, wrt)
    assert_same_bits(got, want, "general / host")
    assert_same_bits(device_gradients(evaluator, circuits, params, wrt), want, "general / device")
    scratch = np.zeros(2 << 20)
    c, p, w = circuits[0], params[0], wrt[0]
    oracle = [c_oracle.evaluate(c, point, op, None, scratch) for point in shift_rules.shifted_points(c.gradient_terms(), p, w)]
    deviation = float(np.abs(got[0] - shift_rules.combine(c.gradient_terms(), oracle, w)).max())
    print(f"general operator: largest deviation {deviation:.3e}")
    assert deviation < EXP_TOL


# ---- kept states ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,layers", [(16, 5), (20, 5)])
def test_circuits_on_kept_states(n, layers):
    """The gradient by the searched (last) layer of a circuit that continues a kept state is that of the whole circuit from
    |0..0> with the layers in front bound (1e-10), and does not depend on the batch it is computed in."""
    population = EVQEPopulation.random_population(n, layers, 4, True, 3)
    evaluator = OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=n))
    whole, fronts, rests, values = [], [], [], []
    for ind in population.individuals:
        front, rest = ind.get_layer_search_circuits(layers - 1)
        whole.append(ind.get_partially_parameterized_quantum_circuit({layers - 1}))
        fronts.append(front)
        rests.append(rest)
        values.append(list(ind.get_layer_parameter_values(layers - 1)))
    states = evaluator.keep_states(fronts, [[] for _ in fronts])
    kept = [rest.continue_from(state) for rest, state in zip(rests, states)]
    assert all(c["on_kept_state"] for c in evaluator.circuit_costs(kept))
    from_zero = evaluator.evaluate_gradients(whole, values)
    on_kept = evaluator.evaluate_gradients(kept, values)
    for a, b in zip(on_kept, from_zero):
        assert a.shape == b.shape and np.abs(a - b).max() < EXP_TOL
    # the combination of evaluate_circuits on the kept circuits themselves, bit for bit
    assert_same_bits(on_kept, ShiftedValues(evaluator, kept, values).expected(), "kept states")
    # company: alone, reversed, and mixed with the whole circuits
    assert_same_bits([evaluator.evaluate_gradients([c], [v])[0] for c, v in zip(kept, values)], on_kept, "alone")
    assert_same_bits(evaluator.evaluate_gradients(kept[::-1], values[::-1])[::-1], on_kept, "reversed")
    mixed = evaluator.evaluate_gradients(whole[:2] + kept + whole[2:], values[:2] + values + values[2:])
    assert_same_bits(mixed[2:-2], on_kept, "mixed")
    assert_same_bits(mixed[:2] + mixed[-2:], from_zero, "mixed, whole circuits")


# ---- independence ---------------------------------------------------------------------------------------------------------


def test_results_do_not_depend_on_order_company_or_calls_in_between():
    n = 18
    circuits, params = _mixed(n, seed=40)
    evaluator = OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=2))
    values_before = evaluator.evaluate_circuits(circuits, params)
    wrt = [list(range(0, c.num_parameters, 7)) for c in circuits]
    base = evaluator.evaluate_gradients(circuits, params, wrt)
    order = np.random.default_rng(1).permutation(len(circuits)).tolist()
    shuffled = evaluator.evaluate_gradients([circuits[i] for i in order], [params[i] for i in order], [wrt[i] for i in order])
    assert_same_bits(shuffled, [base[i] for i in order], "shuffled")
    for i in (0, 3, 5):
        assert_same_bits(evaluator.evaluate_gradients([circuits[i]], [params[i]], [wrt[i]]), [base[i]], "alone")
    assert evaluator.evaluate_circuits(circuits, params) == values_before  # (bitwise: lists of floats)
    assert_same_bits(evaluator.evaluate_gradients(circuits, params, wrt), base, "after evaluate_circuits")
    assert_same_bits(device_gradients(evaluator, circuits, params, wrt), base, "device entry")
    assert evaluator.evaluate_circuits(circuits[::-1], params[::-1])[::-1] == values_before
    # a fresh evaluator that never computed a gradient returns the same values
    fresh = OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=2))
    assert fresh.evaluate_circuits(circuits, params) == values_before


# ---- errors ----------------------------------------------------------------------------------------------------------------


def test_errors():
    import torch

    n = 13
    _, circuits, params = helpers.population_circuits(n, 2, 2, seed=1)
    op = helpers.random_ising_operator(n, seed=1)
    evaluator = OperatorCircuitEvaluator(op)
    repeated = CircuitIR(n).u(P(0), 0.3, P(1), 0).cu3(P(2), P(1), 0.1, 0, 1)
    with pytest.raises(ValueError, match="parameter 1 "):
        evaluator.evaluate_gradients([circuits[0], repeated], [params[0], [0.1, 0.2, 0.3]])
    got = evaluator.evaluate_gradients([repeated], [[0.1, 0.2, 0.3]], [[0, 2]])  # (its other parameters have rules)
    assert got[0].shape == (2,)
    with pytest.raises(ValueError, match="wrt index"):
        evaluator.evaluate_gradients(circuits[:1], params[:1], [[circuits[0].num_parameters]])
    with pytest.raises(ValueError, match="estimator_precision"):
        OperatorCircuitEvaluator(op, estimator_precision=0.1, statevector_device=evaluator.statevector_device).evaluate_gradients(circuits, params)
    # no operator set: QSV_E_STATE from both entry points
    bare = StatevectorDevice(n)
    ids, offsets, flat = bare._batch_arguments(circuits, params)
    out, n_shifted = np.zeros(sum(c.num_parameters for c in circuits)), C.c_int64(-1)
    rc = bare._lib.qsv_gradient_circuits(bare._handle, 2, _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(flat), None, None,
                                         _lib.as_ptr(out), C.byref(n_shifted))
    assert rc == _lib.QSV_E_STATE
    with pytest.raises(CircuitEvaluatorException, match="no operator"):
        bare.gradients(circuits, params)
    width = max(c.num_parameters for c in circuits) + 1
    matrix = torch.zeros((2, width), dtype=torch.float64, device="cuda")
    good = torch.zeros((2, width), dtype=torch.float64, device="cuda")
    rc = bare._lib.qsv_gradient_device(bare._handle, 2, _lib.as_ptr(ids), width, C.c_void_p(matrix.data_ptr()), None, None, None, width,
                                       C.c_void_p(good.data_ptr()), None)
    assert rc == _lib.QSV_E_STATE
    # the output tensor
    for bad in (torch.zeros((2, width), dtype=torch.float32, device="cuda"), torch.zeros((2, width), dtype=torch.float64),
                torch.zeros((1, width), dtype=torch.float64, device="cuda"), torch.zeros((2, 5), dtype=torch.float64, device="cuda"),
                torch.zeros(2 * width, dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError):
            evaluator.evaluate_gradients_device_to_device(circuits, matrix, bad)
    # out_width too small at the C boundary: QSV_E_ARG
    dev = evaluator.statevector_device
    ids, _, _ = dev._batch_arguments(circuits, params)
    rc = dev._lib.qsv_gradient_device(dev._handle, 2, _lib.as_ptr(ids), width, C.c_void_p(matrix.data_ptr()), None, None, None, 5,
                                      C.c_void_p(good.data_ptr()), None)
    assert rc == _lib.QSV_E_ARG and "out_width" in _lib.last_error(dev._lib, dev._handle)
    evaluator.evaluate_gradients_device_to_device(circuits, matrix, good)  # (and the handle still works)
    torch.cuda.synchronize()


# ---- the device form --------------------------------------------------------------------------------------------------------


def test_device_form_is_complete_after_one_stream_synchronise_and_reuses_its_scratch():
    import torch

    n = 16
    _, circuits, params = helpers.population_circuits(n, 3, 8, seed=2)
    evaluator = OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=4))
    dev = evaluator.statevector_device
    want = evaluator.evaluate_gradients(circuits, params)
    stream = torch.cuda.Stream()
    dev.set_stream(stream.cuda_stream)
    try:
        got = device_gradients(evaluator, circuits, params, stream=stream)  # (waits for `stream` alone)
        assert_same_bits(got, want, "first call")
        first = dev.gradient_stats()
        assert first["n_allocations"] > 0 and first["scratch_bytes"] > 0 and first["n_chunks"] == 1
        for _ in range(3):
            assert_same_bits(device_gradients(evaluator, circuits, params, stream=stream), want, "a following call")
        # a smaller call and the host form of the same size reuse it as well
        device_gradients(evaluator, circuits[:3], params[:3], [[0, 1]] * 3, stream=stream)
        again = dev.gradient_stats()
        assert again["n_allocations"] == first["n_allocations"] and again["scratch_bytes"] == first["scratch_bytes"]
        # ... and a larger one grows it
        device_gradients(evaluator, circuits + circuits, params + params, stream=stream)
        grown = dev.gradient_stats()
        assert grown["n_allocations"] > first["n_allocations"] and grown["scratch_bytes"] > first["scratch_bytes"]
    finally:
        dev.set_stream(0)


# ---- the solver ---------------------------------------------------------------------------------------------------------------


def xy_hamiltonian(n_bits: int) -> PauliOperator:
    """min x^2 - y^2 over two registers of ``n_bits`` qubits (test_evqe_solver.py's model at n_bits = 2): x = sum 2^i q_i,
    q = (1 - Z) / 2; the minimum -(2^n_bits - 1)^2 at x = 0, y = 2^n_bits - 1."""
    terms = []
    for sign, base in ((1.0, 0), (-1.0, n_bits)):
        for i in range(n_bits):
            field = -(4.0**i) / 2 - sum(2.0 ** (i + j + 1) / 4 for j in range(n_bits) if j != i)
            terms.append(("Z", [base + i], sign * field))
            for j in range(i + 1, n_bits):
                terms.append(("ZZ", [base + i, base + j], sign * 2.0 ** (i + j + 1) / 4))
    return PauliOperator.from_sparse_list(terms, 2 * n_bits)


class Counting:
    """An evaluator's calls forwarded and counted."""

    def __init__(self, inner):
        self.inner, self.values, self.shifted = inner, 0, 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def evaluate_circuits(self, circuits, parameter_values):
        self.values += len(circuits)
        return self.inner.evaluate_circuits(circuits, parameter_values)

    def evaluate_gradients(self, circuits, parameter_values, wrt=None):
        out = self.inner.evaluate_gradients(circuits, parameter_values, wrt)
        self.shifted += self.inner.last_gradient_evaluations
        return out


SOLVER_BUDGET = 30000


def _solve(optimizer, evaluator):
    cfg = EVQEMinimumEigensolverConfiguration(
        optimizer=optimizer, population_size=8, max_generations=None, max_circuit_evaluations=SOLVER_BUDGET, random_seed=0,
        n_initial_layers=2, randomize_initial_population_parameters=True, use_tournament_selection=True, tournament_size=2,
        parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
        device_resident_search=False)
    return EVQEMinimumEigensolver(cfg).compute_minimum_eigenvalue(evaluator)


def test_adam_in_the_solver():
    op = xy_hamiltonian(4)
    assert op.num_qubits == 8
    spsa = _solve(SPSA(maxiter=25, learning_rate=0.4, perturbation=0.3), Counting(OperatorCircuitEvaluator(op)))
    counting = Counting(OperatorCircuitEvaluator(op))
    adam = _solve(Adam(maxiter=6, lr=0.3), counting)
    print(f"SPSA {spsa.eigenvalue:.6f} in {sum(spsa.circuit_evaluations)} evaluations, "
          f"Adam {adam.eigenvalue:.6f} in {sum(adam.circuit_evaluations)}")
    assert counting.shifted > 0
    assert sum(adam.circuit_evaluations) == counting.shifted + counting.values <= SOLVER_BUDGET
    assert sum(spsa.circuit_evaluations) <= SOLVER_BUDGET
    assert adam.eigenvalue <= spsa.eigenvalue
