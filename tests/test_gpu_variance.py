"""The operator's variance on the device (``qsv_variance_circuits``) against tests/variance_reference.py: the
dense Hermitian part up to eight qubits, the matrix-free strings above, both on the NumPy oracle's state -- operators with and
without a diagonal part and x-mask groups, closed forms, more rows than threads, circuits the expectation route would split,
the determinism and no-disturbance contracts, fp32 handles, the refusals, the EVQE result and GpuEstimator(shots=N)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import helpers
import operator_families as fam
import variance_reference as vr
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.ir import CircuitIR, PauliOperator
from queasars_amd.primitives import GpuEstimator, pub_broadcast

pytestmark = pytest.mark.gpu

H = (np.pi / 2, 0.0, np.pi)  # U(pi/2, 0, pi): the Hadamard gate
X = (np.pi, 0.0, np.pi)

# fp32 handles: the variance is allowed (sum |c_k|)^2 * max(FP32_FLOOR, 4 * E1_FP32), where E1_FP32 is the largest
# |E_32 - E_ref| / sum |c_k| of evaluate_circuits over the cases of the parity test, measured on an MI355X: 2.2e-8 (so the floor
# of 2e-6 decides).  dVar = d<H^2> - 2 E dE, each part bounded by sum |c_k| times the same state error, with a factor two of
# room.  The largest variance error seen over those cases: 1.9e-8 (sum |c_k|)^2.
E1_FP32 = 2.2e-8
TOL_FP32_REL = max(vr.FP32_FLOOR, 4.0 * E1_FP32)

PARITY_SIZES = (6, 11, 13)
STRINGS = {6: 33, 11: 40, 13: 48}


def xy_operator(n: int, identity: bool) -> PauliOperator:
    """X and Y strings only (every z mask inside its x mask, no x = 0 term): no diagonal part; `identity` adds a multiple of
    the identity, which shifts E and leaves the variance alone."""
    rng = np.random.default_rng(900 + n)
    terms = []
    for _ in range(12):
        x = int(rng.integers(1, 1 << n))
        terms.append((x, x & int(rng.integers(0, 1 << n)), float(rng.uniform(-1.0, 1.0))))
    if identity:
        terms.append((0, 0, 0.625))
    return fam.from_masks(n, terms)


@functools.lru_cache(maxsize=None)
def parity_operators(n: int) -> dict:
    return {
        "ising": helpers.random_ising_operator(n, seed=2020),
        "pauli": helpers.random_pauli_operator(n, STRINGS[n], seed=1234),
        "one group": fam.one_group(n, 24),
        "xy": xy_operator(n, False),
        "xy + identity": xy_operator(n, True),
    }


def _check(op, circuits, params, states, dtype="fp64", tol=None, keep=None):
    """evaluate_variances against the reference; returns (largest variance error, largest value error)."""
    evaluator = OperatorCircuitEvaluator(op, dtype=dtype)
    values, variances = evaluator.evaluate_variances(circuits, params, with_values=True)
    assert len(values) == len(variances) == len(circuits)
    ref_values, ref_variances = vr.reference(op, states)
    tol = vr.tol_fp64(op) if tol is None else tol
    err_var = float(np.abs(np.asarray(variances) - ref_variances).max())
    err_val = float(np.abs(np.asarray(values) - ref_values).max())
    print(f"n={op.num_qubits} dtype={dtype} terms={len(op)} spread={vr.spread(op):.3f} |dVar|={err_var:.3e} |dE|={err_val:.3e} tol={tol:.3e}")
    assert err_var <= tol, (err_var, tol)
    if dtype == "fp64":
        assert err_val <= vr.TOL_VALUES
        plain = np.asarray(evaluator.evaluate_circuits(circuits, params))
        assert np.abs(plain - np.asarray(values)).max() <= vr.TOL_VALUES
    if keep is not None:
        keep.append((evaluator, values, variances))
    return err_var, err_val


# ---- 1. parity ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", PARITY_SIZES)
def test_parity_with_the_reference(n):
    circuits, params, states = vr.population(n, 3, 4, 0)
    ops = parity_operators(n)
    assert ops["ising"].is_diagonal() and not (ops["xy"].x_mask == 0).any() and len(set(ops["one group"].x_mask.tolist())) == 1
    kept = []
    for name, op in ops.items():
        _check(op, circuits, params, states, keep=kept)
    # the identity term moves every value by its coefficient and no variance
    (_, plain_values, plain_variances), (_, shifted_values, shifted_variances) = kept[3], kept[4]
    tol = vr.tol_fp64(ops["xy + identity"])
    assert np.abs(np.asarray(shifted_variances) - np.asarray(plain_variances)).max() <= tol
    assert np.abs(np.asarray(shifted_values) - np.asarray(plain_values) - 0.625).max() <= vr.TOL_VALUES


# ---- 2. closed forms ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [3, 9])
def test_a_basis_state_has_no_variance_under_a_diagonal_operator(n):
    op = helpers.random_ising_operator(n, seed=5)
    circuit = CircuitIR(n)
    for q in range(0, n, 2):
        circuit.u(*X, q)
    values, variances = OperatorCircuitEvaluator(op).evaluate_variances([circuit], [[]], with_values=True)
    state = np.zeros(1 << n, dtype=np.complex128)
    state[sum(1 << q for q in range(0, n, 2))] = 1.0
    assert abs(variances[0]) <= vr.tol_fp64(op)
    assert abs(values[0] - vr.moments(op, state)[0]) <= vr.TOL_VALUES


@pytest.mark.parametrize("n", [2, 7, 10])
def test_the_plus_state_is_an_eigenstate_of_the_sum_of_x(n):
    """E = n, Var = 0: n x-mask groups whose rows must be summed before they are squared (squared one by one they give n)."""
    op = fam.from_masks(n, [(1 << q, 0, 1.0) for q in range(n)])
    circuit = CircuitIR(n)
    for q in range(n):
        circuit.u(*H, q)
    values, variances = OperatorCircuitEvaluator(op).evaluate_variances([circuit], [[]], with_values=True)
    assert abs(values[0] - n) <= vr.TOL_VALUES
    assert abs(variances[0]) <= vr.tol_fp64(op)


@pytest.mark.parametrize("n", [4, 10])
def test_the_zero_state_under_a_weighted_x_field(n):
    weights = np.random.default_rng(n).uniform(-1.5, 1.5, size=n)
    op = fam.from_masks(n, [(1 << q, 0, float(a)) for q, a in enumerate(weights)])
    circuit = CircuitIR(n).u(0.0, 0.0, 0.0, 0)  # (the identity: the state stays |0..0>)
    values, variances = OperatorCircuitEvaluator(op).evaluate_variances([circuit], [[]], with_values=True)
    assert abs(values[0]) <= vr.TOL_VALUES
    assert abs(variances[0] - float((weights ** 2).sum())) <= vr.tol_fp64(op)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_x_plus_y_on_the_plus_state(n):
    """|+> on qubit 0 under X_0 + Y_0: E = 1, <H^2> = 2, Var = 1 (the odd-Y phase)."""
    op = fam.from_masks(n, [(1, 0, 1.0), (1, 1, 1.0)])
    circuit = CircuitIR(n).u(*H, 0)
    values, variances = OperatorCircuitEvaluator(op).evaluate_variances([circuit], [[]], with_values=True)
    assert abs(values[0] - 1.0) <= vr.TOL_VALUES
    assert abs(variances[0] - 1.0) <= vr.tol_fp64(op)


# ---- 3. more rows than threads -----------------------------------------------------------------------------------------


def test_more_than_one_row_per_thread():
    """n = 17: 2^17 rows on 256 workgroups of 256 threads, two rows each."""
    n = 17
    circuits, params, states = vr.population(n, 3, 2, 3)
    _check(helpers.random_pauli_operator(n, 40, seed=17), circuits, params, states)


# ---- 4. circuits the expectation route would split ---------------------------------------------------------------------


def test_circuits_that_evaluate_circuits_splits():
    n = 16
    circuits, params, states = vr.population(n, 4, 8, 1)
    op = helpers.random_ising_operator(n, seed=16)
    kept = []
    _check(op, circuits, params, states, keep=kept)
    evaluator = kept[0][0]
    routes = {evaluator.statevector_device.circuit_form(c)["route"] for c in circuits}
    assert routes & {1, 2}, routes  # (QSV_ROUTE_SPLIT_ONE_LAUNCH / QSV_ROUTE_SPLIT: some circuit does take a split route there)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------


def test_an_evaluations_numbers_are_the_same_bits_wherever_it_stands():
    n = 6
    op = helpers.random_pauli_operator(n, 33, seed=1234)
    evaluator = OperatorCircuitEvaluator(op)
    dev = evaluator.statevector_device
    count = int(dev._lib.qsv_group_size(dev._handle)) + 3
    base_circuits, base_params, _ = vr.population(n, 3, 4, 0)
    rng = np.random.default_rng(8)
    circuits = [base_circuits[i % 4] for i in range(count)]
    params = [[float(v + rng.normal(0.0, 0.4)) for v in base_params[i % 4]] for i in range(count)]

    def run(order):
        values, variances = evaluator.evaluate_variances([circuits[i] for i in order], [params[i] for i in order], with_values=True)
        return {i: (np.float64(values[k]).tobytes(), np.float64(variances[k]).tobytes()) for k, i in enumerate(order)}

    whole = run(list(range(count)))
    probe = 5
    alone = run([probe])
    first = run([probe] + [i for i in range(count) if i != probe])
    last = run([i for i in range(count) if i != probe] + [probe])
    shuffled = run([int(i) for i in rng.permutation(count)])
    again = run(list(range(count)))
    assert alone[probe] == first[probe] == last[probe] == whole[probe]
    assert shuffled == whole and again == whole
    assert len({pair for pair in whole.values()}) > count // 2  # (the evaluations do differ)


# ---- 6. no disturbance -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["ising", "general"])
def test_a_variance_call_leaves_a_replayed_batch_and_the_adjoint_sweep_their_bits(kind):
    n = 10
    circuits, params, _ = vr.population(n, 3, 5, 10)
    op = helpers.random_ising_operator(n, seed=2020) if kind == "ising" else helpers.random_pauli_operator(n, 20, seed=1234)
    evaluator = OperatorCircuitEvaluator(op, gradient_method="adjoint")
    dev = evaluator.statevector_device
    before = evaluator.evaluate_circuits(circuits, params)
    replays = dev.replayed_pushes()
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert dev.replayed_pushes() == replays + 1  # (the second call did replay)
    variances = evaluator.evaluate_variances(circuits, params)
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert evaluator.evaluate_circuits(circuits, params) == before
    gradients = evaluator.evaluate_gradients(circuits, params)
    assert evaluator.evaluate_variances(circuits, params) == variances
    again = evaluator.evaluate_gradients(circuits, params)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gradients, again))
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert evaluator.evaluate_variances(circuits, params) == variances


# ---- 7. fp32 handles ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", PARITY_SIZES)
def test_fp32_handles(n):
    circuits, params, states = vr.population(n, 3, 4, 0)
    for name, op in parity_operators(n).items():
        spread = vr.spread(op)
        single = OperatorCircuitEvaluator(op, dtype="fp32")
        ref_values, _ = vr.reference(op, states)
        e1 = float(np.abs(np.asarray(single.evaluate_circuits(circuits, params)) - ref_values).max()) / spread
        print(f"n={n} {name}: e1 = {e1:.3e}")
        err_var, _ = _check(op, circuits, params, states, dtype="fp32", tol=spread ** 2 * TOL_FP32_REL)
        print(f"n={n} {name}: |dVar| / spread^2 = {err_var / spread ** 2:.3e}")


# ---- 8. errors ---------------------------------------------------------------------------------------------------------


def _raw(dev, circuits, params, n_evals=None, with_variances=True, with_values=True):
    """qsv_variance_circuits as the C ABI returns it: (return code, variances, values)."""
    n = len(circuits)
    ids, offsets, flat = dev._batch_arguments(circuits, params) if n else (np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1))
    variances, values = np.full(max(1, n), np.nan), np.full(max(1, n), np.nan)
    rc = dev._lib.qsv_variance_circuits(dev._handle, n if n_evals is None else n_evals, _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(flat),
                                        _lib.as_ptr(variances) if with_variances else None, _lib.as_ptr(values) if with_values else None)
    return rc, variances, values


def test_refusals_leave_the_handle_working():
    n = 10
    circuits, params, states = vr.population(n, 3, 4, 0)
    op = helpers.random_pauli_operator(n, 20, seed=1234)
    _, ref = vr.reference(op, states)
    dev = StatevectorDevice(n)

    def works():
        rc, variances, values = _raw(dev, circuits, params)
        assert rc == _lib.QSV_OK and np.abs(variances - ref).max() <= vr.tol_fp64(op)
        rc, only, _ = _raw(dev, circuits, params, with_values=False)  # (out_values may be NULL)
        assert rc == _lib.QSV_OK and only.tobytes() == variances.tobytes()

    assert _raw(dev, circuits, params)[0] == _lib.QSV_E_STATE  # no operator set
    assert _raw(dev, [], [], n_evals=0)[0] == _lib.QSV_OK
    dev.set_operator(op)
    works()
    assert _raw(dev, circuits, params, with_variances=False)[0] == _lib.QSV_E_ARG
    works()
    assert _raw(dev, circuits, params, n_evals=-1)[0] == _lib.QSV_E_ARG
    assert _raw(dev, [], [], n_evals=0)[0] == _lib.QSV_OK
    assert _raw(dev, [], [], n_evals=0, with_variances=False)[0] == _lib.QSV_OK
    front = CircuitIR(n).u(0.3, 0.2, 0.1, 0).cu3(0.5, 0.1, 0.2, 0, 1)
    state = dev.keep_states([front], [[]])[0]
    kept = CircuitIR(n).u(0.4, 0.0, 0.0, 2).continue_from(state)
    assert _raw(dev, [kept], [[]])[0] == _lib.QSV_E_UNSUPPORTED
    with pytest.raises(ValueError, match="kept state"):
        dev.variances([kept], [[]])
    works()
    with pytest.raises(ValueError):
        dev.variances(circuits, params[:-1])
    values, variances = dev.variances([], [])
    assert values.shape == variances.shape == (0,) and values.dtype == variances.dtype == np.float64


# ---- 9. the solver -----------------------------------------------------------------------------------------------------


def test_the_solver_reports_the_variance_at_its_best_individual():
    from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    def config():
        return EVQEMinimumEigensolverConfiguration(
            optimizer=SPSA(maxiter=10, learning_rate=0.4, perturbation=0.3), population_size=6, max_generations=3, random_seed=5,
            n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
            use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
            parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
        )

    n = 6
    op = helpers.random_ising_operator(n, seed=6)
    plain = EVQEMinimumEigensolver(config()).compute_minimum_eigenvalue(OperatorCircuitEvaluator(op))
    evaluator = OperatorCircuitEvaluator(op)
    asked = EVQEMinimumEigensolver(config()).compute_minimum_eigenvalue(evaluator, eigenvalue_variance=True)
    assert plain.eigenvalue_variance is None
    for name in ("eigenvalue", "best_individual", "generations", "circuit_evaluations", "best_expectation_values",
                 "median_expectation_values", "mean_expectation_values", "aux_operators_evaluated", "eigenstate", "eigenstate_values"):
        assert getattr(plain, name) == getattr(asked, name), name
    best = asked.best_individual
    circuit, values = best.get_parameterized_quantum_circuit(), list(best.parameter_values)
    assert asked.eigenvalue_variance == evaluator.evaluate_variances([circuit], [values])[0]
    assert abs(asked.eigenvalue_variance - vr.dense_moments(op, helpers.oracle_state(circuit, values))[1]) <= vr.tol_fp64(op)


# ---- 10. the estimator -------------------------------------------------------------------------------------------------


def test_the_estimators_shot_noise_on_the_device():
    n, shots = 6, 1024
    circuits, params, _ = vr.population(n, 3, 4, 0)
    circuit = circuits[0]
    op_a, op_b = helpers.random_pauli_operator(n, 33, seed=1234), helpers.random_ising_operator(n, seed=2020)
    bindings = np.asarray([params[0], [v + 0.25 for v in params[0]], [v - 0.5 for v in params[0]]])
    estimator = GpuEstimator(shots=shots, seed=7)
    single, array = estimator.run([(circuit, op_a, bindings[0]), (circuit, [[op_a], [op_b]], bindings)], precision=0.3).result()

    def sigma(op, binding):
        variance = vr.dense_moments(op, helpers.oracle_state(circuit, list(binding)))[1]
        return np.sqrt(variance / shots), vr.tol_fp64(op)

    def check(stds, expected, tolerances):
        # d sigma = d Var / (2 sigma shots)
        assert np.all(np.abs(stds - expected) <= tolerances / (2.0 * expected * shots)), (stds, expected)

    assert single.data.evs.shape == single.data.stds.shape == ()
    check(single.data.stds, *sigma(op_a, bindings[0]))
    assert array.data.evs.shape == array.data.stds.shape == pub_broadcast((2, 1), bindings.shape) == (2, 3)
    expected = np.asarray([[sigma(op, b) for b in bindings] for op in (op_a, op_b)])
    check(array.data.stds, expected[..., 0], expected[..., 1])
    assert single.metadata["shots"] == array.metadata["shots"] == shots
    # the draws: the generator's standard normals in the pubs' order, scaled entry by entry
    draws = np.random.default_rng(7)
    exact_single = OperatorCircuitEvaluator(op_a).evaluate_circuits([circuit], [list(bindings[0])])[0]
    assert abs((float(single.data.evs) - exact_single) / float(single.data.stds) - draws.standard_normal()) <= 1e-6
