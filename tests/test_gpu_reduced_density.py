"""Reduced density matrices of qubit subsets on the device (``qsv_reduced_density_circuits``) against
tests/rdm_reference.py: reshape, transpose and einsum on the NumPy oracle's states -- registers below, at and above one block of a
subset's qubits and the six lowest others, subsets on the lowest and the highest qubits, across the boundary between qubit 5 and
qubit 6 and in non-ascending order, the Hermitian, determinism and no-disturbance contracts to the bit, the refusals, fp32
handles, ``queasars_amd.entanglement`` and the solver's option.

Workgroups per (evaluation, subset) are min(64, 2^(n - 10)) (csrc/reduced_density.hpp rdm_blocks): one up to n = 10, where a
four-qubit subset has one block; from n = 8 on a single-qubit subset's workgroup walks more than one block (2^(n - 7) blocks), and
n = 17 is the smallest register at which the cap of 64 binds, so that a four-qubit subset's workgroup walks two.

Seen on an MI355X: fp64, the largest |rho - reference| per component is 7.6e-15 (n = 17; 6.9e-15 at n = 20, allowed 1e-11); fp32
handles, e_s = 1.7e-7 (n = 6) and 2.5e-7 (n = 11), so the floor of 2e-6 decides, and the largest error is 1.9e-7."""

from __future__ import annotations

import numpy as np
import pytest

import helpers
import rdm_reference as rr
from queasars_amd import _lib, entanglement as ent
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.ir import CircuitIR

pytestmark = pytest.mark.gpu

# (n, evaluations): batches of 1, 2 and 17 (group + 3 is test_more_evaluations_and_subsets_than_one_launch_takes); from n = 11 on
# the second half of a batch is the first half's circuits at perturbed parameters (rdm_reference.case)
PARITY_CASES = [(1, 1), (2, 2), (3, 17), (5, 2), (9, 17), (10, 1), (11, 17), (13, 4), (17, 4)]


def check(name, got, want, tol):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == np.complex128, (name, g.shape, w.shape)
    err = rr.largest_error(got, want)
    print(f"{name}: largest component error {err:.3e} (allowed {tol:.3e})")
    assert err <= tol, (name, err, tol)
    return err


def assert_hermitian_to_the_bit(matrices):
    for m in matrices:
        assert np.array_equal(m, m.conj().transpose(0, 2, 1))
        diagonal = np.diagonal(m, axis1=1, axis2=2)
        assert not diagonal.imag.any() and not np.signbit(diagonal.imag).any()  # (0.0, not -0.0)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,count", PARITY_CASES)
def test_parity_with_the_reference(n, count):
    circuits, params, states = rr.case(n, count)
    subsets = rr.subsets_for(n)
    dev = StatevectorDevice(n)
    got = dev.reduced_density_matrices(circuits, params, subsets)
    check(f"rho n={n}, {count} evaluations, {len(subsets)} subsets", got, rr.reduced_density_matrices(states, subsets), rr.TOL)
    assert_hermitian_to_the_bit(got)
    for m in got:
        assert np.abs(np.trace(m, axis1=1, axis2=2) - 1.0).max() <= rr.TOL * m.shape[1]
    if n <= 4:  # k = n: rho = |psi><psi| of the handle's own statevector()
        whole = got[subsets.index(tuple(range(n)))]
        for e, (c, p) in enumerate(zip(circuits, params)):
            psi = dev.statevector(c, p)
            assert rr.max_component_error(whole[e], np.outer(psi, psi.conj())) <= 1e-14


def test_all_pairs_of_eleven_qubits():
    n = 11
    circuits, params, states = rr.case(n, 4)
    pairs = rr.all_pairs(n)
    assert len(pairs) == 55
    dev = StatevectorDevice(n)
    got = dev.reduced_density_matrices(circuits, params, pairs)
    check("all pairs, n=11", got, rr.reduced_density_matrices(states, pairs), rr.TOL)
    assert_hermitian_to_the_bit(got)


def test_twenty_qubits_against_the_c_oracle(c_oracle):
    n = 20
    _, circuits, params = helpers.population_circuits(n, 4, 1, seed=20)
    state = c_oracle.simulate(circuits[0], list(params[0]))
    subsets = [(0,), (19,), (5, 6), (0, 5, 6, 19), (16, 17, 18, 19), (19, 7, 12, 0), (3, 2, 1, 0), (13, 9, 2)]
    dev = StatevectorDevice(n)
    got = dev.reduced_density_matrices(circuits, [list(params[0])], subsets)
    check("rho n=20", got, rr.reduced_density_matrices([state], subsets), rr.TOL)
    assert_hermitian_to_the_bit(got)


# ---- 2. the same bits ------------------------------------------------------------------------------------------------------


def test_a_matrix_is_the_same_bits_wherever_it_stands():
    n, count = 11, 17
    circuits, params, _ = rr.case(n, count)
    subsets = rr.subsets_for(n)
    dev = StatevectorDevice(n)

    def run(order, chosen):
        got = dev.reduced_density_matrices([circuits[i] for i in order], [params[i] for i in order], chosen)
        return {(i, s): got[j][k].tobytes() for j, s in enumerate(chosen) for k, i in enumerate(order)}

    whole = run(list(range(count)), subsets)
    probe, others = 5, [i for i in range(count) if i != 5]
    alone = run([probe], subsets)
    assert all(whole[key] == value for key, value in alone.items())
    for order in ([probe] + others, others + [probe], [int(i) for i in np.random.default_rng(3).permutation(count)]):
        assert run(order, subsets) == whole
    assert run(list(range(count)), list(reversed(subsets))) == whole
    few = [subsets[7], subsets[2]]
    assert all(whole[key] == value for key, value in run([probe, 0], few).items())
    assert len(set(whole.values())) > len(whole) // 2  # (the matrices do differ)
    # a repeated subset: two identical blocks
    twice = dev.reduced_density_matrices(circuits[:3], params[:3], [subsets[4], subsets[9], subsets[4]])
    assert twice[0].tobytes() == twice[2].tobytes() and twice[0].tobytes() != twice[1].tobytes()


def test_more_evaluations_and_subsets_than_one_launch_takes():
    """group + 3 evaluations and 70 subsets at n = 6: a launch's partial tiles stay inside 64 MiB, 16384 (evaluation, subset)
    pairs of 4 KiB at one workgroup each, so the first launch group of 256 takes 64 subsets at a time -- a second launch group
    and a second run of subsets, every matrix at its place with the bits it has alone."""
    n = 6
    dev = StatevectorDevice(n)
    group = int(dev._lib.qsv_group_size(dev._handle))
    count = group + 3
    subsets = (rr.singles_and_pairs(n) + rr.subsets_for(n) + [(a, b, c) for a in range(4) for b in range(4, 6) for c in (3, 5) if len({a, b, c}) == 3]
               + [(5, 4, 3, 2), (1, 3, 5, 0), (2, 4), (4, 2), (0, 1, 2, 3), (1, 0, 3, 2)] * 5)[:70]
    assert len(subsets) == 70 and group * 64 <= 16384 < group * len(subsets)
    base_circuits, base_params, _ = rr.population(n, 3, 4, 0)
    rng = np.random.default_rng(9)
    circuits = [base_circuits[i % 4] for i in range(count)]
    params = [[float(v + rng.normal(0.0, 0.4)) for v in base_params[i % 4]] for i in range(count)]
    probes = [0, group - 1, group, count - 1]
    got = dev.reduced_density_matrices(circuits, params, subsets)
    states = {i: helpers.oracle_state(circuits[i], params[i]) for i in probes + [7, group + 1]}
    for i, state in states.items():
        check(f"evaluation {i} of {count}", [g[i:i + 1] for g in got], rr.reduced_density_matrices([state], subsets), rr.TOL)
    assert_hermitian_to_the_bit(got)
    for i in probes:
        alone = dev.reduced_density_matrices([circuits[i]], [params[i]], subsets[60:] + subsets[:3])
        for j, s in enumerate(list(range(60, 70)) + [0, 1, 2]):
            assert alone[j][0].tobytes() == got[s][i].tobytes()


def test_the_call_leaves_the_other_calls_their_bits():
    n = 10
    circuits, params, _ = rr.population(n, 3, 5, 10)
    op = helpers.random_pauli_operator(n, 20, seed=1234)
    evaluator = OperatorCircuitEvaluator(op)
    dev = evaluator.statevector_device
    subsets = rr.subsets_for(n)
    before = evaluator.evaluate_circuits(circuits, params)
    replays = dev.replayed_pushes()
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert dev.replayed_pushes() == replays + 1  # (the second call did replay)
    variances = evaluator.evaluate_variances(circuits, params)
    states_before = [dev.statevector(c, p).tobytes() for c, p in zip(circuits[:3], params[:3])]
    rho = evaluator.reduced_density_matrices(circuits, params, subsets)
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert evaluator.evaluate_variances(circuits, params) == variances
    again = evaluator.reduced_density_matrices(circuits, params, subsets)
    assert [a.tobytes() for a in again] == [r.tobytes() for r in rho]
    assert [dev.statevector(c, p).tobytes() for c, p in zip(circuits[:3], params[:3])] == states_before
    assert dev._operator is op  # (no operator was installed or removed)


def test_a_handle_without_an_operator_and_an_initial_state():
    n = 7
    circuits, params, _ = rr.population(n, 3, 3, 7)
    dev = StatevectorDevice(n)  # (no operator was ever set)
    subsets = rr.subsets_for(n)
    plain = dev.reduced_density_matrices(circuits, params, subsets)
    initial = CircuitIR(n).u(0.7, 0.2, 0.3, 0).cu3(1.1, 0.3, 0.2, 0, 6).u(0.4, 0.1, 0.9, 3)
    evaluator = OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=1), initial_state_circuit=initial)
    got = evaluator.reduced_density_matrices(circuits, params, subsets)
    states = [helpers.oracle_state(initial.compose(c), p) for c, p in zip(circuits, params)]
    check("behind an initial state", got, rr.reduced_density_matrices(states, subsets), rr.TOL)
    assert rr.largest_error(got, plain) > 1e-3  # (the initial state is seen)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------


def _raw(dev, circuits, params, subsets, n_evals=None, n_subsets=None, out_given=True, offsets_given=True, qubits_given=True):
    """qsv_reduced_density_circuits as the C ABI returns it: (return code, message, out)."""
    n = len(circuits)
    ids, offsets, flat = dev._batch_arguments(circuits, params) if n else (np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1))
    starts = np.zeros(len(subsets) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in subsets], out=starts[1:])
    qubits = np.asarray([q for s in subsets for q in s] + [0], dtype=np.int32)
    out = np.full((max(1, n), max(1, sum(4 ** len(s) for s in subsets))), np.nan, dtype=np.complex128)
    rc = dev._lib.qsv_reduced_density_circuits(
        dev._handle, len(subsets) if n_subsets is None else n_subsets, _lib.as_ptr(starts) if offsets_given else None,
        _lib.as_ptr(qubits) if qubits_given else None, n if n_evals is None else n_evals, _lib.as_ptr(ids), _lib.as_ptr(offsets),
        _lib.as_ptr(flat), _lib.as_ptr(out) if out_given else None)
    return rc, _lib.last_error(dev._lib, dev._handle), out


def test_refusals_leave_the_handle_working():
    n = 6
    circuits, params, states = rr.population(n, 3, 3, 6)
    dev = StatevectorDevice(n)
    subsets = [(0,), (5, 2), (1, 3, 4, 0)]
    want = np.concatenate([m.reshape(3, -1) for m in rr.reduced_density_matrices(states, subsets)], axis=1)
    first = []

    def works():
        rc, _, out = _raw(dev, circuits, params, subsets)
        assert rc == _lib.QSV_OK and rr.max_component_error(out, want) <= rr.TOL
        first.append(out.tobytes())
        assert first[0] == first[-1]

    def refused(code, word, chosen=subsets, **kwargs):
        rc, message, out = _raw(dev, kwargs.pop("circuits", circuits), kwargs.pop("params", params), chosen, **kwargs)
        assert rc == code and word in message, (rc, message)
        assert np.isnan(out).all()  # (nothing was written)

    works()
    refused(_lib.QSV_E_ARG, "out", out_given=False)
    refused(_lib.QSV_E_ARG, "subset_offsets", offsets_given=False)
    refused(_lib.QSV_E_ARG, "subset_qubits", qubits_given=False)
    refused(_lib.QSV_E_ARG, "n_subsets", n_subsets=0)
    refused(_lib.QSV_E_ARG, "n_subsets", n_subsets=-2)
    refused(_lib.QSV_E_ARG, "empty", chosen=[(0,), (), (1,)])
    refused(_lib.QSV_E_ARG, "out of range", chosen=[(0,), (1, 6)])
    refused(_lib.QSV_E_ARG, "out of range", chosen=[(-1,)])
    refused(_lib.QSV_E_ARG, "twice", chosen=[(0,), (2, 4, 2)])
    refused(_lib.QSV_E_ARG, "n_evals", n_evals=-1)
    refused(_lib.QSV_E_UNSUPPORTED, "up to 4", chosen=[(0,), (0, 1, 2, 3, 4)])
    refused(_lib.QSV_E_UNSUPPORTED, "1024 subsets", chosen=[(q % n,) for q in range(1025)])
    works()
    kept = dev.keep_states(circuits[:1], params[:1])
    continued = CircuitIR(n).u(0.4, 0.0, 0.0, 2).continue_from(kept[0])
    refused(_lib.QSV_E_UNSUPPORTED, "kept state", circuits=[continued], params=[[]])
    with pytest.raises(ValueError, match="kept state"):
        dev.reduced_density_matrices([continued], [[]], subsets)
    # nothing to evaluate: fine once the subsets were checked, also without an output
    assert _raw(dev, [], [], subsets, n_evals=0)[0] == _lib.QSV_OK
    assert _raw(dev, [], [], subsets, n_evals=0, out_given=False)[0] == _lib.QSV_OK
    refused(_lib.QSV_E_ARG, "twice", chosen=[(3, 3)], circuits=[], params=[], n_evals=0)
    # 1024 subsets are taken
    many = [(q % n, (q + 1 + q // n % (n - 1)) % n) for q in range(1024)]
    rc, _, out = _raw(dev, circuits[:1], params[:1], many)
    assert rc == _lib.QSV_OK
    assert rr.max_component_error(out[0].reshape(1024, 4, 4), np.stack([rr.reduced_density_matrix(states[0], s) for s in many])) <= rr.TOL
    # inside an open batch, from the thread that holds it
    dev.set_operator(helpers.random_ising_operator(n, seed=2))
    batch_ids, offsets, flat = dev._batch_arguments(circuits, params)
    counts = np.diff(offsets).astype(np.int64)
    values = np.zeros(len(circuits))
    assert dev._lib.qsv_eval_begin(dev._handle, len(circuits), _lib.as_ptr(batch_ids), _lib.as_ptr(counts)) == _lib.QSV_OK
    refused(_lib.QSV_E_STATE, "(qsv_reduced_density_circuits goes between batches)")
    assert dev._lib.qsv_eval_push(dev._handle, 0, len(circuits), _lib.as_ptr(flat)) == _lib.QSV_OK
    assert dev._lib.qsv_eval_end(dev._handle, _lib.as_ptr(values)) == _lib.QSV_OK
    assert np.abs(values - dev.expectation_values(circuits, params)).max() <= 1e-12
    works()


def test_a_register_above_28_qubits_is_refused():
    """More than 28 qubits -> QSV_E_UNSUPPORTED, with a sentence that names the limit: a 29-qubit fp32 handle (one state slot of
    4 GiB), asked before anything is uploaded."""
    n = 29
    dev = StatevectorDevice(n, dtype="fp32")
    circuit = CircuitIR(n).u(0.3, 0.2, 0.1, 0)
    rc, message, _ = _raw(dev, [circuit], [[]], [(0,), (28, 3)])
    assert rc == _lib.QSV_E_UNSUPPORTED and "28 qubits" in message and "29" in message, (rc, message)
    with pytest.raises(ValueError, match="28 qubits"):
        dev.reduced_density_matrices([circuit], [[]], [(0,)])


# ---- 4. fp32 handles ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,count", [(6, 17), (11, 6)])
def test_fp32_handles(n, count):
    """|d rho| <= max(2e-6, 4 e_s), e_s the largest |psi_32 - psi_ref|_2 of the fp32 handle's own statevector() over this test's
    circuits -- the existing route, not the new one."""
    circuits, params, states = rr.case(n, count)
    dev = StatevectorDevice(n, dtype="fp32")
    e_s = max(float(np.linalg.norm(dev.statevector(c, p) - s)) for c, p, s in zip(circuits, params, states))
    tol = rr.tol_fp32(e_s)
    print(f"n={n} fp32: e_s = {e_s:.3e}, allowed |d rho| = {tol:.3e}")
    subsets = rr.subsets_for(n)
    got = dev.reduced_density_matrices(circuits, params, subsets)
    check(f"fp32 rho n={n}", got, rr.reduced_density_matrices(states, subsets), tol)
    assert_hermitian_to_the_bit(got)


# ---- 5. entanglement.py and the solver ------------------------------------------------------------------------------------------


def test_mutual_information_finds_the_one_entangler():
    """u on every qubit and one cu3 between qubits 2 and 7 of 10: a product state but for that pair."""
    n = 10
    rng = np.random.default_rng(12)
    circuit = CircuitIR(n)
    for q in range(n):
        circuit.u(*rng.uniform(0.4, 2.6, size=3), q)
    circuit.cu3(1.3, 0.4, 0.7, 2, 7)
    evaluator = OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=3))
    entropies, information = ent.mutual_information(evaluator, [circuit], [[]], with_entropies=True)
    assert information.shape == (1, n, n) and entropies.shape == (1, n)
    print(f"I(2, 7) = {information[0, 2, 7]:.6f} bits, S_2 = {entropies[0, 2]:.6f}")
    assert information[0, 2, 7] > 1e-2 and information[0, 2, 7] == information[0, 7, 2]
    assert abs(information[0, 2, 7] - 2 * entropies[0, 2]) <= 1e-9  # (a pure pair: S_27 = 0, S_2 = S_7)
    rest = information[0].copy()
    rest[2, 7] = rest[7, 2] = 0.0
    assert np.abs(rest).max() <= 1e-9
    others = np.delete(entropies[0], [2, 7])
    assert np.abs(others).max() <= 1e-9
    assert np.array_equal(ent.qubit_entropies(evaluator, [circuit], [[]]), entropies)
    marginal = ent.marginal_distributions(evaluator, [circuit], [[]], [(7, 2)])[0][0]
    state = helpers.oracle_state(circuit, [])
    want = ent.marginal_distribution(rr.reduced_density_matrix(state, (7, 2)))
    assert [marginal[format(a, "02b")] for a in range(4)] == pytest.approx(want.tolist(), abs=1e-12)


def test_the_solver_reports_the_best_individuals_correlations():
    from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    def config():
        return EVQEMinimumEigensolverConfiguration(
            optimizer=SPSA(maxiter=10, learning_rate=0.4, perturbation=0.3), population_size=6, max_generations=2, random_seed=5,
            n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
            use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
            parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
        )

    n = 6
    op = helpers.random_pauli_operator(n, 33, seed=1234)
    solvers = [EVQEMinimumEigensolver(config()), EVQEMinimumEigensolver(config())]
    plain = solvers[0].compute_minimum_eigenvalue(OperatorCircuitEvaluator(op))
    asked = solvers[1].compute_minimum_eigenvalue(OperatorCircuitEvaluator(op), qubit_correlations=True)
    assert plain.qubit_entropies is None and plain.mutual_information is None
    for name in ("eigenvalue", "best_individual", "generations", "circuit_evaluations", "best_expectation_values",
                 "median_expectation_values", "mean_expectation_values"):
        assert getattr(plain, name) == getattr(asked, name), name
    for stream in ("_rng_last_layer", "_rng_speciation", "_rng_selection", "_rng_parameter_search", "_rng_topological", "_rng_layer_removal"):
        assert getattr(solvers[0], stream).getstate() == getattr(solvers[1], stream).getstate(), stream
    assert asked.qubit_entropies.shape == (n,) and asked.mutual_information.shape == (n, n)
    best = asked.best_individual
    state = helpers.oracle_state(best.get_parameterized_quantum_circuit(), list(best.parameter_values))
    want = np.asarray([ent.von_neumann_entropy(rr.reduced_density_matrix(state, (q,))) for q in range(n)])
    assert np.abs(asked.qubit_entropies - want).max() <= 1e-9
    i, j = 1, 4
    want_ij = want[i] + want[j] - ent.von_neumann_entropy(rr.reduced_density_matrix(state, (i, j)))
    assert abs(asked.mutual_information[i, j] - want_ij) <= 1e-9
    assert np.array_equal(asked.mutual_information, asked.mutual_information.T) and not np.diagonal(asked.mutual_information).any()
