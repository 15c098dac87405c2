"""The covariance matrix of an observable set on the device (``qsv_observables_covariance``) against
tests/covariance_reference.py -- the dense Hermitian parts up to eight qubits, the matrix-free strings above, both on the NumPy
oracle's state -- and against the device's own variance call: the block edges of the 16-observable tiles, sets with empty,
repeated, identical and opposite observables, closed forms, the determinism and no-disturbance contracts, fp32 handles, the
refusals, the EVQE result and GpuEstimator(shots=N, joint_moments=True)."""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import covariance_reference as cr
import helpers
import operator_families as fam
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.ir import CircuitIR
from queasars_amd.primitives import GpuEstimator

pytestmark = pytest.mark.gpu

H = (np.pi / 2, 0.0, np.pi)  # U(pi/2, 0, pi): the Hadamard gate
X = (np.pi, 0.0, np.pi)

SIZES = (4, 8, 11, 13)  # fewer amplitudes than a wave | the four chunks of 64 | several workgroups
SET_SIZES = (1, 2, 15, 16, 17, 33, 64)  # the edges of the 16-observable blocks: 1, 2, 3 and 4 blocks (1, 3, 6 and 10 block pairs)

# fp32 handles: an entry is allowed S_a S_b * max(FP32_FLOOR, 4 * E1_FP32), where E1_FP32 is the largest |E_32 - E_ref| / sum |c_k|
# of evaluate_circuits over the observables of the fp32 test (DESIGN.md 4.13 defines it so), measured on an MI355X: see the
# test's output and DESIGN.md 4.14.  dC_ab = d Re<lambda_a|lambda_b> - E_a dE_b - E_b dE_a, each part bounded by S_a S_b times the
# same state error, with a factor two of room.  Measured: e1 = 1.3e-7 (n = 13; 9.1e-8 at n = 8; 33 observables each), so the floor of
# 2e-6 decides; the largest covariance error seen over those cases: 1.7e-7 S_a S_b.
E1_FP32 = 1.3e-7
TOL_FP32_REL = max(cr.FP32_FLOOR, 4.0 * E1_FP32)


def _random_observable(n: int, rng, kind: str) -> list[tuple[int, int, float]]:
    """[(x, z, c)] of one to five strings: `diagonal` (x = 0), `xy` (z inside x: X and Y only) or `mixed`."""
    terms = []
    for _ in range(int(rng.integers(1, 6))):
        x = 0 if kind == "diagonal" else int(rng.integers(1, 1 << n))
        z = int(rng.integers(0 if kind != "diagonal" else 1, 1 << n))
        if kind == "xy":
            z &= x
        terms.append((x, z, float(rng.uniform(-1.0, 1.0))))
    return terms


@functools.lru_cache(maxsize=None)
def observable_set(n: int, m: int) -> tuple:
    """M observables on n qubits that hold what the kernel can get wrong: diagonal-only observables next to X/Y ones, a string
    whose x mask has the top qubit, strings with an odd and with an even number of Y, the same string in two observables and twice
    in one, two identical observables, and one observable the negative of another."""
    rng = np.random.default_rng(1000 * n + m)
    top = 1 << (n - 1)
    special = [
        [(top | 1, 1, 0.75), (0, 3, -0.5)],                    # Y on qubit 0 (odd), X on the top qubit; a diagonal string
        [(3, 3, 0.5), (3, 0, 0.25), (3, 3, 0.125)],            # YY (even), XX, and YY again: twice in one observable
        [(top | 1, 1, -0.3), (0, top, 1.0)],                   # the first string again, in another observable
        [(7 if n > 2 else 3, 7 if n > 2 else 3, 0.6)],         # YYY (odd, floor(3 / 2) = 1: the folded sign)
    ]
    kinds = ("diagonal", "xy", "mixed")
    terms = [special[k] if k < len(special) else _random_observable(n, rng, kinds[k % 3]) for k in range(m)]
    if m >= 15:
        terms[9] = list(terms[5])                               # two identical observables
        terms[m - 1] = [(x, z, -c) for x, z, c in terms[6]]     # O_b = -O_a, in the last block
    return tuple(fam.from_masks(n, t) for t in terms)


def _compare(ops, values, covariances, states, tol=None, value_tol=cr.TOL_VALUES):
    """The device's numbers against the reference; returns (largest |dC| / (S_a S_b), largest |dE|)."""
    ref_values, ref_cov = cr.reference(ops, states)
    tol = cr.tol_fp64(ops) if tol is None else tol
    s = np.maximum(1.0, cr.spreads(ops))
    err = np.abs(covariances - ref_cov)
    err_val = float(np.abs(values - ref_values).max())
    rel = float((err / np.outer(s, s)).max())
    print(f"n={ops[0].num_qubits} M={len(ops)} |dC|/(S_a S_b)={rel:.3e} |dE|={err_val:.3e}")
    assert np.all(err <= tol), (float(err.max()), float(np.min(tol)))
    if value_tol is not None:
        assert err_val <= value_tol
    return rel, err_val


def _assert_symmetric(covariances):
    assert covariances.tobytes() == np.ascontiguousarray(np.swapaxes(covariances, -1, -2)).tobytes()


# ---- 1. parity with the reference: every n, every block edge ---------------------------------------------------------------


@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_reference(n):
    circuits, params, states = cr.population(n, 3, 3, 0)
    dev = StatevectorDevice(n)
    for m in SET_SIZES:
        ops = observable_set(n, m)
        values, covariances = dev.observable_covariances(circuits, params, ops)
        assert values.shape == (3, m) and covariances.shape == (3, m, m) and values.dtype == covariances.dtype == np.float64
        _compare(ops, values, covariances, states)
        _assert_symmetric(covariances)
        assert np.abs(values - dev.observable_values(circuits, params, ops)).max() <= cr.TOL_VALUES
        if m >= 15:
            tol = cr.tol_fp64(ops)
            assert np.all(np.abs(covariances[:, 5, 9] - covariances[:, 5, 5]) <= tol[5, 5])
            assert np.all(np.abs(covariances[:, 9, 9] - covariances[:, 5, 5]) <= tol[5, 5])
            assert np.all(np.abs(covariances[:, 6, m - 1] + covariances[:, 6, 6]) <= tol[6, 6])
    dev.close()


def test_a_workgroup_walks_more_than_one_stride():
    """n = 17: 2048 chunks of 64 amplitudes on at most 1024 workgroups; 17 observables, so an off-diagonal block pair too."""
    n = 17
    circuits, params, states = cr.population(n, 3, 1, 3)
    ops = observable_set(n, 17)
    dev = StatevectorDevice(n)
    values, covariances = dev.observable_covariances(circuits, params, ops)
    _compare(ops, values, covariances, states)
    _assert_symmetric(covariances)
    dev.close()


def test_an_observable_without_terms_has_a_zero_row_and_column():
    n = 8
    circuits, params, states = cr.population(n, 3, 1, 0)
    ops = observable_set(n, 17)
    dev = StatevectorDevice(n)
    lib, h = dev._lib, dev._handle
    # observables 0 .. 2, one without terms, observables 3 .. 16, one without terms: 19 in all
    sizes = [len(op) for op in ops[:3]] + [0] + [len(op) for op in ops[3:]] + [0]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = np.concatenate([np.asarray(op.x_mask, dtype=np.uint64) for op in ops])
    z = np.concatenate([np.asarray(op.z_mask, dtype=np.uint64) for op in ops])
    c = np.ascontiguousarray(np.concatenate([op.coeffs.real for op in ops]), dtype=np.float64)
    out = C.c_int(0)
    assert lib.qsv_observables_create(h, 19, _lib.as_ptr(offsets), _lib.as_ptr(x), _lib.as_ptr(z), _lib.as_ptr(c), None, C.byref(out)) == _lib.QSV_OK
    ids, poffsets, flat = dev._batch_arguments(circuits, params)
    values, cov = np.full((1, 19), np.nan), np.full((1, 19, 19), np.nan)
    assert lib.qsv_observables_covariance(h, out.value, 1, _lib.as_ptr(ids), _lib.as_ptr(poffsets), _lib.as_ptr(flat), _lib.as_ptr(values),
                                          _lib.as_ptr(cov)) == _lib.QSV_OK
    assert values[0, 3] == 0.0 and values[0, 18] == 0.0
    for empty in (3, 18):
        assert not cov[0, empty, :].any() and not cov[0, :, empty].any()
    keep = [k for k in range(19) if k not in (3, 18)]
    _compare(ops, values[:, keep], cov[:, keep][:, :, keep], states)
    dev.close()


# ---- 2. known answers at n = 4 -------------------------------------------------------------------------------------------------


def _single(n, kind, qubits):
    x, z = fam._string(qubits, kind * len(qubits))
    return fam.from_masks(n, [(x, z, 1.0)])


def test_known_answers():
    n = 4
    dev = StatevectorDevice(n)
    zero = CircuitIR(n)
    plus = CircuitIR(n)
    for q in range(n):
        zero.id(q)
        plus.u(*H, q)
    bell = CircuitIR(n).u(*H, 0).cu3(*X, 0, 1)
    z_strings = [_single(n, "Z", [q]) for q in range(n)] + [_single(n, "Z", [0, 1]), _single(n, "Z", [0, 1, 2, 3])]
    x_strings = [_single(n, "X", [q]) for q in range(n)]
    tol = 1e-11
    values, cov = dev.observable_covariances([zero], [[]], z_strings)
    assert np.abs(values - 1.0).max() <= cr.TOL_VALUES and np.abs(cov).max() <= tol
    values, cov = dev.observable_covariances([plus], [[]], x_strings)
    assert np.abs(values - 1.0).max() <= cr.TOL_VALUES and np.abs(cov).max() <= tol
    values, cov = dev.observable_covariances([plus], [[]], z_strings[:n])
    assert np.abs(values).max() <= cr.TOL_VALUES and np.abs(cov[0] - np.eye(n)).max() <= tol
    values, cov = dev.observable_covariances([bell], [[]], [z_strings[0], z_strings[1], z_strings[4]])
    assert np.abs(values[0] - [0.0, 0.0, 1.0]).max() <= cr.TOL_VALUES
    assert abs(cov[0, 0, 1] - 1.0) <= tol and abs(cov[0, 0, 0] - 1.0) <= tol and abs(cov[0, 1, 1] - 1.0) <= tol
    assert np.abs(cov[0, 2, :]).max() <= tol and np.abs(cov[0, :, 2]).max() <= tol
    dev.close()


# ---- 3. against the device's own variance call ---------------------------------------------------------------------------------


@pytest.mark.parametrize("n,m", [(8, 17), (11, 5)])
def test_the_diagonal_and_weighted_sums_agree_with_the_variance_call(n, m):
    circuits, params, _ = cr.population(n, 3, 3, 0)
    ops = observable_set(n, m)
    dev = StatevectorDevice(n)
    values, cov = dev.observable_covariances(circuits, params, ops)
    for k, op in enumerate(ops):
        dev.set_operator(op)
        alone_values, alone = dev.variances(circuits, params)
        s = max(1.0, cr.spread(op))
        assert np.abs(cov[:, k, k] - alone).max() <= 1e-11 * s * s
        assert np.abs(values[:, k] - alone_values).max() <= cr.TOL_VALUES
    rng = np.random.default_rng(n)
    for _ in range(3):
        w = rng.uniform(-1.0, 1.0, size=m)
        total = cr.combined(ops, w)
        dev.set_operator(total)
        _, whole = dev.variances(circuits, params)
        s = max(1.0, cr.spread(total))
        assert np.abs(np.einsum("a,nab,b->n", w, cov, w) - whole).max() <= 1e-11 * s * s
    dev.close()


# ---- 4. fp32 handles ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", (8, 13))
def test_fp32_handles(n):
    circuits, params, states = cr.population(n, 3, 3, 0)
    ops = observable_set(n, 33)
    ref_values, _ = cr.reference(ops, states)
    dev = StatevectorDevice(n, dtype="fp32")
    e1 = 0.0
    for k, op in enumerate(ops):
        single = OperatorCircuitEvaluator(op, statevector_device=dev)
        e1 = max(e1, float(np.abs(np.asarray(single.evaluate_circuits(circuits, params)) - ref_values[:, k]).max()) / cr.spread(op))
    print(f"n={n}: e1 = {e1:.3e}")
    values, cov = dev.observable_covariances(circuits, params, ops)
    s = cr.spreads(ops)
    _, ref_cov = cr.reference(ops, states)
    rel = float((np.abs(cov - ref_cov) / np.outer(s, s)).max())
    print(f"n={n}: |dC| / (S_a S_b) = {rel:.3e}")
    assert np.all(np.abs(cov - ref_cov) <= np.outer(s, s) * TOL_FP32_REL)
    assert np.all(np.abs(values - ref_values) <= s * TOL_FP32_REL)
    _assert_symmetric(cov)
    dev.close()


# ---- 5. bits ---------------------------------------------------------------------------------------------------------------------------


def test_an_evaluations_numbers_are_the_same_bits_wherever_it_stands():
    n = 6
    ops = observable_set(n, 17)
    dev = StatevectorDevice(n)
    count = int(dev._lib.qsv_group_size(dev._handle)) + 3  # (two launch groups)
    base_circuits, base_params, _ = cr.population(n, 3, 4, 0)
    rng = np.random.default_rng(8)
    circuits = [base_circuits[i % 4] for i in range(count)]
    params = [[float(v + rng.normal(0.0, 0.4)) for v in base_params[i % 4]] for i in range(count)]

    def run(order):
        values, cov = dev.observable_covariances([circuits[i] for i in order], [params[i] for i in order], ops)
        return {i: (values[k].tobytes(), cov[k].tobytes()) for k, i in enumerate(order)}

    whole = run(list(range(count)))
    probe = 5
    alone = run([probe])
    first = run([probe] + [i for i in range(count) if i != probe])
    last = run([i for i in range(count) if i != probe] + [probe])
    again = run(list(range(count)))
    assert alone[probe] == first[probe] == last[probe] == whole[probe]
    assert again == whole
    assert len(set(whole.values())) > count // 2  # (the evaluations do differ)
    dev.close()


@pytest.mark.parametrize("kind", ["ising", "general"])
def test_a_covariance_call_leaves_the_operator_and_a_replayed_batch_their_bits(kind):
    n = 10
    circuits, params, _ = cr.population(n, 3, 5, 10)
    op = helpers.random_ising_operator(n, seed=2020) if kind == "ising" else helpers.random_pauli_operator(n, 20, seed=1234)
    ops = observable_set(n, 17)
    evaluator = OperatorCircuitEvaluator(op, gradient_method="adjoint")
    dev = evaluator.statevector_device
    before = evaluator.evaluate_circuits(circuits, params)
    replays = dev.replayed_pushes()
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert dev.replayed_pushes() == replays + 1  # (the second call did replay)
    observables = evaluator.evaluate_observables(circuits, params, ops)
    variances = evaluator.evaluate_variances(circuits, params)
    gradients = evaluator.evaluate_gradients(circuits, params)
    values, cov = evaluator.evaluate_covariances(circuits, params, ops, with_values=True)
    assert dev._operator is op  # (the handle's operator is still the installed one)
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert evaluator.evaluate_covariances(circuits, params, ops).tobytes() == cov.tobytes()
    assert evaluator.evaluate_observables(circuits, params, ops) == observables
    assert evaluator.evaluate_variances(circuits, params) == variances
    again = evaluator.evaluate_gradients(circuits, params)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gradients, again))
    assert evaluator.evaluate_circuits(circuits, params) == before


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------


def _raw(dev, set_id, circuits, params, m, n_evals=None, with_cov=True, with_values=True):
    """qsv_observables_covariance as the C ABI returns it: (return code, values, covariances)."""
    n = len(circuits)
    ids, offsets, flat = dev._batch_arguments(circuits, params) if n else (np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1))
    values, cov = np.full((max(1, n), m), np.nan), np.full((max(1, n), m, m), np.nan)
    rc = dev._lib.qsv_observables_covariance(dev._handle, set_id, n if n_evals is None else n_evals, _lib.as_ptr(ids), _lib.as_ptr(offsets),
                                             _lib.as_ptr(flat), _lib.as_ptr(values) if with_values else None, _lib.as_ptr(cov) if with_cov else None)
    return rc, values, cov


def test_refusals_leave_the_handle_working():
    n = 8
    circuits, params, states = cr.population(n, 3, 3, 0)
    ops = observable_set(n, 15)
    dev = StatevectorDevice(n)
    set_id = dev._observable_set(list(ops))

    def works():
        rc, values, cov = _raw(dev, set_id, circuits, params, 15)
        assert rc == _lib.QSV_OK
        _compare(ops, values, cov, states)
        rc, _, only = _raw(dev, set_id, circuits, params, 15, with_values=False)  # (out_values may be NULL)
        assert rc == _lib.QSV_OK and only.tobytes() == cov.tobytes()

    works()  # (no operator is set on the handle)
    assert _raw(dev, 987654, circuits, params, 15)[0] == _lib.QSV_E_ARG
    assert _raw(dev, set_id, circuits, params, 15, with_cov=False)[0] == _lib.QSV_E_ARG
    assert _raw(dev, set_id, circuits, params, 15, n_evals=-1)[0] == _lib.QSV_E_ARG
    assert _raw(dev, set_id, [], [], 15, n_evals=0)[0] == _lib.QSV_OK
    assert _raw(dev, set_id, [], [], 15, n_evals=0, with_cov=False)[0] == _lib.QSV_OK
    works()
    # 65 observables: the set exists, its covariances are refused
    many = [ops[k % 15] for k in range(65)]
    big_id = dev._observable_set(many)
    assert dev.observable_values(circuits, params, many).shape == (3, 65)
    assert _raw(dev, big_id, circuits, params, 65)[0] == _lib.QSV_E_UNSUPPORTED
    with pytest.raises(ValueError, match="64"):
        dev.observable_covariances(circuits, params, many)
    works()
    front = CircuitIR(n).u(0.3, 0.2, 0.1, 0).cu3(0.5, 0.1, 0.2, 0, 1)
    state = dev.keep_states([front], [[]])[0]
    kept = CircuitIR(n).u(0.4, 0.0, 0.0, 2).continue_from(state)
    assert _raw(dev, set_id, [kept], [[]], 15)[0] == _lib.QSV_E_UNSUPPORTED
    with pytest.raises(ValueError, match="kept state"):
        dev.observable_covariances([kept], [[]], ops)
    works()
    # a batch left open on this thread
    dev.set_operator(ops[0])
    ids, offsets, flat = dev._batch_arguments(circuits, params)
    counts = np.ascontiguousarray(np.diff(offsets), dtype=np.int64)
    plain = np.zeros(len(circuits))
    assert dev._lib.qsv_eval_begin(dev._handle, len(circuits), _lib.as_ptr(ids), _lib.as_ptr(counts)) == _lib.QSV_OK
    values, cov = np.zeros((3, 15)), np.zeros((3, 15, 15))  # (the handle is locked: nothing but the library is called in between)
    assert dev._lib.qsv_observables_covariance(dev._handle, set_id, 3, _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(flat),
                                               _lib.as_ptr(values), _lib.as_ptr(cov)) == _lib.QSV_E_STATE
    assert dev._lib.qsv_eval_push(dev._handle, 0, len(circuits), _lib.as_ptr(flat)) == _lib.QSV_OK
    assert dev._lib.qsv_eval_end(dev._handle, _lib.as_ptr(plain)) == _lib.QSV_OK
    assert np.abs(plain - dev.observable_values(circuits, params, [ops[0]])[:, 0]).max() <= cr.TOL_VALUES
    works()
    with pytest.raises(ValueError):
        dev.observable_covariances(circuits, params[:-1], ops)
    with pytest.raises(ValueError):
        dev.observable_covariances(circuits, params, [])
    values, cov = dev.observable_covariances([], [], ops)
    assert values.shape == (0, 15) and cov.shape == (0, 15, 15) and values.dtype == cov.dtype == np.float64
    dev.close()


# ---- 7. the solver -------------------------------------------------------------------------------------------------------------------


def test_the_solver_reports_the_aux_operators_covariance_at_its_best_individual():
    from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    def config():
        return EVQEMinimumEigensolverConfiguration(
            optimizer=SPSA(maxiter=10, learning_rate=0.4, perturbation=0.3), population_size=6, max_generations=2, random_seed=5,
            n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
            use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
            parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
        )

    n = 6
    op = helpers.random_ising_operator(n, seed=6)
    aux = {"field": fam.from_masks(n, [(1 << q, 0, 1.0) for q in range(n)]), "cost": op, "pauli": helpers.random_pauli_operator(n, 9, seed=2)}
    plain = EVQEMinimumEigensolver(config()).compute_minimum_eigenvalue(OperatorCircuitEvaluator(op), aux_operators=aux)
    evaluator = OperatorCircuitEvaluator(op)
    asked = EVQEMinimumEigensolver(config()).compute_minimum_eigenvalue(evaluator, aux_operators=aux, aux_operators_covariance=True)
    assert plain.aux_operators_covariance is None and plain.aux_operators_variance is None
    for name in ("eigenvalue", "best_individual", "generations", "circuit_evaluations", "best_expectation_values",
                 "median_expectation_values", "mean_expectation_values", "aux_operators_evaluated"):
        assert getattr(plain, name) == getattr(asked, name), name
    best = asked.best_individual
    circuit, values = best.get_parameterized_quantum_circuit(), list(best.parameter_values)
    matrix = asked.aux_operators_covariance
    assert matrix.shape == (3, 3) and matrix.tobytes() == matrix.T.copy().tobytes()
    assert list(asked.aux_operators_variance) == ["field", "cost", "pauli"]
    assert list(asked.aux_operators_variance.values()) == [float(v) for v in np.diagonal(matrix)]
    ops = list(aux.values())
    assert np.all(np.abs(matrix - cr.dense_moments(ops, helpers.oracle_state(circuit, values))[1]) <= cr.tol_fp64(ops))
    assert abs(asked.aux_operators_variance["cost"] - evaluator.evaluate_variances([circuit], [values])[0]) <= cr.tol_fp64(ops)[1, 1]


# ---- 8. the estimator -----------------------------------------------------------------------------------------------------------------


def test_the_estimators_joint_moments_on_the_device():
    n, shots = 6, 1000
    circuits, params, _ = cr.population(n, 3, 4, 0)
    circuit = circuits[0]
    op_a, op_b = helpers.random_pauli_operator(n, 33, seed=1234), helpers.random_ising_operator(n, seed=2020)
    bindings = np.asarray([params[0], [v + 0.25 for v in params[0]], [v - 0.5 for v in params[0]]])
    pubs = [(circuit, [[op_a], [op_b]], bindings)]
    joint = GpuEstimator(shots=shots, seed=7, joint_moments=True).run(pubs).result()[0]
    default = GpuEstimator(shots=shots, seed=7).run(pubs).result()[0]
    assert joint.data.evs.shape == joint.data.stds.shape == default.data.stds.shape == (2, 3)
    assert joint.metadata == default.metadata == {"target_precision": 0.0, "shots": shots}
    # d sigma = d Var / (2 sigma shots), both routes within the fp64 bound of the reference
    tol = 2.0 * np.asarray([[1e-11 * max(1.0, cr.spread(op)) ** 2] * 3 for op in (op_a, op_b)])
    assert (default.data.stds > 1e-3).all()
    assert np.all(np.abs(joint.data.stds - default.data.stds) <= tol / (2.0 * default.data.stds * shots))
    # the same draws: the generator's standard normals entry by entry
    assert np.abs((joint.data.evs - default.data.evs)).max() <= 1e-9
