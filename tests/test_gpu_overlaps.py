"""Overlaps and operator matrix elements against kept states on the device (``qsv_overlap_circuits``) against
tests/overlap_reference.py: vdot on the NumPy oracle's states, the operator dense up to eight qubits and matrix-free above --
every block edge of the 16 x 16 tiles on both sides, registers below, at and above one chunk of 64 amplitudes, the lane map on
basis states, the identities, the determinism and no-disturbance contracts, the refusals, fp32 handles, the EVQE result and
GpuStateFidelity."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import helpers
import operator_families as fam
import overlap_reference as ovr
from dense_gradient import dense_operator
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.ir import CircuitIR
from queasars_amd.primitives import GpuStateFidelity

pytestmark = pytest.mark.gpu

X = (np.pi, 0.0, np.pi)

# (n, evaluations, kept states): every block edge -- 1, 15, 16, 17, 33 evaluations; 1, 2, 15, 16, 17, 33, 64 kept states -- on each
# side at least once; n = 3 is less than one chunk of 64 amplitudes, 6 exactly one, 17 more chunks than workgroups (2048 on 512).
# From n = 11 on each circuit comes a second time at slightly perturbed parameters, so overlaps of order 1 occur.
PARITY_CASES = [(3, 1, 1), (3, 17, 2), (6, 15, 16), (6, 33, 15), (8, 16, 17), (8, 2, 64), (11, 17, 33), (13, 33, 16), (13, 4, 64), (17, 2, 3)]

# fp32 handles (test_fp32_handles): e_s, the largest |psi_32 - psi_ref|_2 of the fp32 handle's statevector() over the test's own
# circuits, seen on an MI355X: 1.4e-7 (n = 6), 1.6e-7 (n = 11), so the floor of 2e-6 decides; the largest |dS| seen is 1.9e-7, the
# largest |dT| 8.4e-7 under sum|c_k| = 17.7 (allowed 3.5e-5).


@functools.lru_cache(maxsize=None)
def operators(n: int) -> dict:
    ops = {
        "ising": helpers.random_ising_operator(n, seed=2020),
        "pauli": helpers.random_pauli_operator(n, min(33, 4 ** n // 2), seed=1234),
        "one group": fam.one_group(n, min(24, 1 << n)),
    }
    assert ops["ising"].is_diagonal() and (ops["pauli"].x_mask & ops["pauli"].z_mask).any() and len(set(ops["one group"].x_mask.tolist())) == 1
    return ops


def case_states(n: int, n_evals: int, n_kept: int):
    """(circuits, params, states) of the kept states and of the evaluations: the head and the tail of one population."""
    count = max(n_evals, n_kept) + (1 if n < 11 else 0)
    if n >= 11:
        count = max(count, 2 * min(n_evals, n_kept))  # (the perturbed copies of the head are in the tail)
    circuits, params, states = ovr.population(n, 3, count, n, n >= 11)
    head = (circuits[:n_kept], params[:n_kept], states[:n_kept])
    tail = (circuits[count - n_evals:], params[count - n_evals:], states[count - n_evals:])
    return head, tail


def check(name, got, want, tol):
    err = ovr.max_component_error(got, want)
    print(f"{name}: largest component error {err:.3e} (allowed {tol:.3e}), largest |reference| {np.abs(want).max():.3f}")
    assert got.shape == want.shape and got.dtype == np.complex128
    assert err <= tol, (name, err, tol)
    return err


# ---- 1. parity -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,n_evals,n_kept", PARITY_CASES)
def test_parity_with_the_reference(n, n_evals, n_kept):
    (kc, kp, kstates), (ec, ep, estates) = case_states(n, n_evals, n_kept)
    dev = StatevectorDevice(n)
    kept = dev.keep_states(kc, kp)
    want_s = ovr.overlaps(kstates, estates)
    if n >= 11:
        assert np.abs(want_s).max() > 0.5  # (overlaps of order 1 do occur)
    s = dev.overlaps(ec, ep, kept)
    check(f"S n={n} {n_evals}x{n_kept}", s, want_s, ovr.TOL_S)
    ops = operators(n)
    for name, op in ops.items() if n < 17 else [("pauli", ops["pauli"])]:
        evaluator = OperatorCircuitEvaluator(op, statevector_device=dev)
        s_op, t = evaluator.evaluate_overlaps(ec, ep, kept, with_operator=True)
        assert s_op.tobytes() == s.tobytes()  # (S is the same sum with and without the operator)
        check(f"T n={n} {n_evals}x{n_kept} {name} (sum|c|={ovr.spread(op):.2f})", t, ovr.elements(op, kstates, estates), ovr.tol_t(op))


# ---- 2. the lane map -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_kept", [16, 17])
def test_basis_states_pick_amplitudes(n_kept):
    """Kept states prepared as distinct computational basis states: S[e][k] is amplitude b_k of psi_e, and every (row, column) of a
    tile carries a different number."""
    n, n_evals = 6, 17
    dev = StatevectorDevice(n)
    basis = [(7 * k + 3) % (1 << n) for k in range(n_kept)]
    assert len(set(basis)) == n_kept
    flips = []
    for b in basis:
        circuit = CircuitIR(n).u(0.0, 0.0, 0.0, 0)
        for q in range(n):
            if (b >> q) & 1:
                circuit.u(*X, q)
        flips.append(circuit)
    kept = dev.keep_states(flips, [[] for _ in flips])
    # (rotations on every qubit and a ring of controlled ones, all at random angles: no amplitude is zero and no two are equal)
    rng = np.random.default_rng(21)
    circuits, params = [], [[] for _ in range(n_evals)]
    for _ in range(n_evals):
        circuit = CircuitIR(n)
        for q in range(n):
            circuit.u(*rng.uniform(0.3, 2.8, size=3), q)
        for q in range(n):
            circuit.cu3(*rng.uniform(0.3, 2.8, size=3), q, (q + 1) % n)
        circuits.append(circuit)
    s = dev.overlaps(circuits, params, kept)
    amplitudes = np.asarray([dev.statevector(c, p) for c, p in zip(circuits, params)])
    want = amplitudes[:, basis]
    assert len({complex(v) for v in want.ravel()}) == want.size
    err = ovr.max_component_error(s, want)
    print(f"lane map, {n_kept} basis states: largest component error {err:.3e}")
    assert err <= 1e-12


# ---- 3. identities ---------------------------------------------------------------------------------------------------------


def test_identities_among_a_population():
    n = 8
    circuits, params, _ = ovr.population(n, 3, 5, 8)
    for name, op in operators(n).items():
        evaluator = OperatorCircuitEvaluator(op)
        s, h = evaluator.evaluate_subspace_matrices(circuits, params)
        assert np.abs(np.diagonal(s) - 1.0).max() <= 1e-12
        assert ovr.max_component_error(s, s.conj().T) <= ovr.TOL_S
        assert ovr.max_component_error(h, h.conj().T) <= ovr.tol_t(op)
        values = np.asarray(evaluator.evaluate_circuits(circuits, params))
        assert np.abs(np.real(np.diagonal(h)) - values).max() <= 1e-10, name
        assert evaluator.statevector_device.kept_state_count() == 0  # (the blocks were released)


def test_a_complete_basis_resolves_the_identity():
    n = 4
    dev = StatevectorDevice(n)
    flips = []
    for b in range(1 << n):
        circuit = CircuitIR(n).u(0.0, 0.0, 0.0, 0)
        for q in range(n):
            if (b >> q) & 1:
                circuit.u(*X, q)
        flips.append(circuit)
    kept = dev.keep_states(flips, [[] for _ in flips])
    circuits, params, _ = ovr.population(n, 3, 3, 4)
    s = dev.overlaps(circuits, params, kept)
    assert np.abs((np.abs(s) ** 2).sum(axis=1) - 1.0).max() <= 1e-12


# ---- 4. the same bits ------------------------------------------------------------------------------------------------------


def test_rows_and_columns_are_the_same_bits_wherever_they_stand():
    n, count = 6, 33
    op = helpers.random_pauli_operator(n, 33, seed=1234)
    evaluator = OperatorCircuitEvaluator(op)
    base_circuits, base_params, _ = ovr.population(n, 3, 4, 0)
    rng = np.random.default_rng(8)
    circuits = [base_circuits[i % 4] for i in range(count)]
    params = [[float(v + rng.normal(0.0, 0.4)) for v in base_params[i % 4]] for i in range(count)]
    kept = evaluator.keep_states(circuits[:20], params[:20])

    def run(order, states):
        s, t = evaluator.evaluate_overlaps([circuits[i] for i in order], [params[i] for i in order], states, with_operator=True)
        return s, t, {i: (s[k].tobytes(), t[k].tobytes()) for k, i in enumerate(order)}

    # an evaluation's row: alone, first and last of 33, in two different batches, again
    states = kept[:17]
    _, _, whole = run(list(range(count)), states)
    probe = 5
    others = [i for i in range(count) if i != probe]
    assert run([probe], states)[2][probe] == run([probe] + others, states)[2][probe] == run(others + [probe], states)[2][probe] == whole[probe]
    assert run([int(i) for i in rng.permutation(count)], states)[2] == whole
    assert run(list(range(count)), states)[2] == whole
    assert len(set(whole.values())) > count // 2  # (the rows do differ)
    # a kept state's column: listed first, seventeenth and twice, and in a shorter list
    long_list = [kept[0]] + kept[1:16] + [kept[0]] + kept[16:18]
    s, t, _ = run(list(range(count)), long_list)
    s2, t2, _ = run(list(range(count)), kept[1:5] + [kept[0]])
    for got in ((s, s2), (t, t2)):
        first, seventeenth, short = got[0][:, 0], got[0][:, 16], got[1][:, 4]
        assert first.tobytes() == seventeenth.tobytes() == short.tobytes()
        assert got[0][:, 1].tobytes() == got[1][:, 0].tobytes()


def test_more_evaluations_than_a_launch_group():
    """group + 3 evaluations: the second launch group's rows land at their positions, with the bits they have alone."""
    n = 6
    op = helpers.random_pauli_operator(n, 33, seed=1234)
    evaluator = OperatorCircuitEvaluator(op)
    dev = evaluator.statevector_device
    count = int(dev._lib.qsv_group_size(dev._handle)) + 3
    base_circuits, base_params, _ = ovr.population(n, 3, 4, 0)
    rng = np.random.default_rng(9)
    circuits = [base_circuits[i % 4] for i in range(count)]
    params = [[float(v + rng.normal(0.0, 0.4)) for v in base_params[i % 4]] for i in range(count)]
    states = [helpers.oracle_state(c, p) for c, p in zip(circuits, params)]
    kept = evaluator.keep_states(circuits[:3], params[:3])
    s, t = evaluator.evaluate_overlaps(circuits, params, kept, with_operator=True)
    check(f"S, {count} evaluations", s, ovr.overlaps(states[:3], states), ovr.TOL_S)
    check(f"T, {count} evaluations", t, ovr.elements(op, states[:3], states), ovr.tol_t(op))
    for probe in (0, count - 4, count - 1):
        s1, t1 = evaluator.evaluate_overlaps([circuits[probe]], [params[probe]], kept, with_operator=True)
        assert s1[0].tobytes() == s[probe].tobytes() and t1[0].tobytes() == t[probe].tobytes()


def test_an_overlap_call_leaves_the_other_calls_their_bits():
    n = 10
    circuits, params, _ = ovr.population(n, 3, 5, 10)
    op = helpers.random_pauli_operator(n, 20, seed=1234)
    evaluator = OperatorCircuitEvaluator(op)
    dev = evaluator.statevector_device
    kept = evaluator.keep_states(circuits[:3], params[:3])
    continued = [CircuitIR(n).u(0.4, 0.1, 0.2, 2).cu3(0.3, 0.2, 0.1, 2, 5).continue_from(kept[1])]
    before = evaluator.evaluate_circuits(circuits, params)
    replays = dev.replayed_pushes()
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert dev.replayed_pushes() == replays + 1  # (the second call did replay)
    variances = evaluator.evaluate_variances(circuits, params)
    on_kept = evaluator.evaluate_circuits(continued, [[]])
    states_before = [dev.statevector(c, p).tobytes() for c, p in zip(circuits[:3], params[:3])]
    s, t = evaluator.evaluate_overlaps(circuits, params, kept, with_operator=True)
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert evaluator.evaluate_variances(circuits, params) == variances
    assert evaluator.evaluate_circuits(continued, [[]]) == on_kept
    again = evaluator.evaluate_overlaps(circuits, params, kept, with_operator=True)
    assert again[0].tobytes() == s.tobytes() and again[1].tobytes() == t.tobytes()  # (the kept-state buffer was only read)
    assert evaluator.evaluate_overlaps(circuits, params, kept).tobytes() == s.tobytes()
    assert [dev.statevector(c, p).tobytes() for c, p in zip(circuits[:3], params[:3])] == states_before


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------


def _raw(dev, circuits, params, prefix_ids, with_operator=0, n_evals=None, n_states=None, s_out=True, t_out=True, ids_given=True):
    """qsv_overlap_circuits as the C ABI returns it: (return code, message, S, T)."""
    n = len(circuits)
    ids, offsets, flat = dev._batch_arguments(circuits, params) if n else (np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1))
    prefix = np.asarray(list(prefix_ids) + [0], dtype=np.int32)
    k = len(prefix_ids) if n_states is None else n_states
    s = np.full((max(1, n), max(1, k)), np.nan, dtype=np.complex128)
    t = np.full((max(1, n), max(1, k)), np.nan, dtype=np.complex128)
    rc = dev._lib.qsv_overlap_circuits(dev._handle, k, _lib.as_ptr(prefix) if ids_given else None, with_operator, n if n_evals is None else n_evals,
                                       _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(flat), _lib.as_ptr(s) if s_out else None,
                                       _lib.as_ptr(t) if t_out else None)
    return rc, _lib.last_error(dev._lib, dev._handle), s, t


def test_refusals_leave_the_handle_working():
    n = 10
    circuits, params, states = ovr.population(n, 3, 4, 0)
    op = helpers.random_pauli_operator(n, 20, seed=1234)
    dev = StatevectorDevice(n)
    kept = dev.keep_states(circuits[:2], params[:2])
    ids = [k._id for k in kept]
    want_s, want_t = ovr.overlaps(states[:2], states), ovr.elements(op, states[:2], states)

    def works(with_operator):
        rc, _, s, t = _raw(dev, circuits, params, ids, with_operator)
        assert rc == _lib.QSV_OK and ovr.max_component_error(s, want_s) <= ovr.TOL_S
        if with_operator:
            assert ovr.max_component_error(t, want_t) <= ovr.tol_t(op)
        else:
            assert np.isnan(t).all()  # (not looked at)
        rc, _, only, _ = _raw(dev, circuits, params, ids, 0, t_out=False)  # (out_elements may be NULL without the operator)
        assert rc == _lib.QSV_OK and only.tobytes() == s.tobytes()

    def refused(code, word, **kwargs):
        rc, message, _, _ = _raw(dev, kwargs.pop("circuits", circuits), kwargs.pop("params", params), kwargs.pop("prefix_ids", ids), **kwargs)
        assert rc == code and word in message, (rc, message)

    refused(_lib.QSV_E_STATE, "with_operator", with_operator=1)  # no operator set
    works(0)
    dev.set_operator(op)
    works(1)
    refused(_lib.QSV_E_ARG, "out_overlaps", s_out=False)
    refused(_lib.QSV_E_ARG, "out_elements", with_operator=1, t_out=False)
    refused(_lib.QSV_E_ARG, "n_states", n_states=0)
    refused(_lib.QSV_E_ARG, "n_states", n_states=-3)
    refused(_lib.QSV_E_ARG, "prefix_ids", ids_given=False)
    refused(_lib.QSV_E_ARG, "unknown kept state 9999", prefix_ids=[ids[0], 9999])
    refused(_lib.QSV_E_UNSUPPORTED, "n_states", prefix_ids=[ids[0]] * 65)
    works(1)
    gone = dev.keep_states(circuits[2:3], params[2:3])[0]
    gone_id = gone._id
    gone.release()
    assert dev.kept_state_count() == 2  # (the release has reached the library)
    refused(_lib.QSV_E_ARG, f"unknown kept state {gone_id}", prefix_ids=[ids[0], gone_id])
    continued = CircuitIR(n).u(0.4, 0.0, 0.0, 2).continue_from(kept[0])
    refused(_lib.QSV_E_UNSUPPORTED, "circuit_ids", circuits=[continued], params=[[]])
    with pytest.raises(ValueError, match="kept state"):
        dev.overlaps([continued], [[]], kept)
    assert _raw(dev, [], [], ids, n_evals=0)[0] == _lib.QSV_OK
    assert _raw(dev, [], [], ids, n_evals=0, s_out=False, t_out=False)[0] == _lib.QSV_OK
    refused(_lib.QSV_E_ARG, "n_evals", n_evals=-1)
    # inside an open batch, from the thread that holds it
    batch_ids, offsets, flat = dev._batch_arguments(circuits, params)
    counts = np.diff(offsets).astype(np.int64)
    out = np.zeros(len(circuits))
    assert dev._lib.qsv_eval_begin(dev._handle, len(circuits), _lib.as_ptr(batch_ids), _lib.as_ptr(counts)) == _lib.QSV_OK
    refused(_lib.QSV_E_STATE, "(qsv_overlap_circuits goes between batches)")
    assert dev._lib.qsv_eval_push(dev._handle, 0, len(circuits), _lib.as_ptr(flat)) == _lib.QSV_OK
    assert dev._lib.qsv_eval_end(dev._handle, _lib.as_ptr(out)) == _lib.QSV_OK
    assert np.abs(out - dev.expectation_values(circuits, params)).max() <= 1e-12
    works(1)
    works(0)


def test_a_register_above_28_qubits_is_refused():
    """More than 28 qubits -> QSV_E_UNSUPPORTED, with a sentence that names the limit: a 29-qubit fp32 handle (one state slot of
    4 GiB), asked before the kept states are looked up, so the handle needs to hold none."""
    n = 29
    dev = StatevectorDevice(n, dtype="fp32")
    circuit = CircuitIR(n).u(0.3, 0.2, 0.1, 0)
    for with_operator in (0, 1):
        rc, message, _, _ = _raw(dev, [circuit], [[]], [12345], with_operator)
        assert rc == _lib.QSV_E_UNSUPPORTED and "28 qubits" in message and "29" in message, (rc, message)
    assert _raw(dev, [], [], [12345], n_evals=0)[0] == _lib.QSV_E_ARG  # (nothing to evaluate: the ids are still looked up)


def test_more_kept_states_than_one_call_takes_are_served_in_blocks():
    n = 5
    circuits, params, states = ovr.population(n, 2, 70, 5)
    dev = StatevectorDevice(n)
    kept = dev.keep_states(circuits, params)
    s = dev.overlaps(circuits[:3], params[:3], kept)
    check("S against 70 kept states", s, ovr.overlaps(states, states[:3]), ovr.TOL_S)
    assert s[:, 64:].tobytes() == dev.overlaps(circuits[:3], params[:3], kept[64:]).tobytes()


# ---- 6. fp32 handles ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,n_evals,n_kept", [(6, 17, 16), (11, 17, 33)])
def test_fp32_handles(n, n_evals, n_kept):
    """|dS| <= max(2e-6, 4 e_s) and |dT| <= that times max(1, sum|c_k|), e_s the largest |psi_32 - psi_ref|_2 of the fp32 handle's
    own statevector() over this test's circuits -- the existing route, not the new one."""
    (kc, kp, kstates), (ec, ep, estates) = case_states(n, n_evals, n_kept)
    dev = StatevectorDevice(n, dtype="fp32")
    e_s = max(float(np.linalg.norm(dev.statevector(c, p) - s)) for c, p, s in zip(list(kc) + list(ec), list(kp) + list(ep), list(kstates) + list(estates)))
    tol = ovr.tol_fp32(e_s)
    print(f"n={n} fp32: e_s = {e_s:.3e}, allowed |dS| = {tol:.3e}")
    kept = dev.keep_states(kc, kp)
    check(f"fp32 S n={n}", dev.overlaps(ec, ep, kept), ovr.overlaps(kstates, estates), tol)
    for name, op in operators(n).items():
        evaluator = OperatorCircuitEvaluator(op, statevector_device=dev)
        _, t = evaluator.evaluate_overlaps(ec, ep, kept, with_operator=True)
        check(f"fp32 T n={n} {name}", t, ovr.elements(op, kstates, estates), tol * max(1.0, ovr.spread(op)))


# ---- 7. the solver and the fidelity ----------------------------------------------------------------------------------------


def test_the_solver_refines_its_result_in_the_span_of_its_population():
    from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    def config():
        return EVQEMinimumEigensolverConfiguration(
            optimizer=SPSA(maxiter=10, learning_rate=0.4, perturbation=0.3), population_size=6, max_generations=1, random_seed=5,
            n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
            use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
            parameter_search_probability=0.3, topological_search_probability=0.4, layer_removal_probability=0.05,
        )

    # One scored generation: its individuals are still distinct species (the NumPy oracle's states of this run give 0.79 for the
    # smallest eigenvalue of S; after three generations selection has filled the population with near copies, and 2e-3).
    n = 6
    op = helpers.random_pauli_operator(n, 33, seed=1234)
    plain = EVQEMinimumEigensolver(config()).compute_minimum_eigenvalue(OperatorCircuitEvaluator(op))
    asked = EVQEMinimumEigensolver(config()).compute_minimum_eigenvalue(OperatorCircuitEvaluator(op), subspace_states=4)
    assert plain.subspace_eigenvalue is None and plain.subspace_overlaps is None
    for name in ("eigenvalue", "best_individual", "generations", "circuit_evaluations", "best_expectation_values",
                 "median_expectation_values", "mean_expectation_values"):
        assert getattr(plain, name) == getattr(asked, name), name
    assert asked.subspace_overlaps.shape == (4, 4) and asked.subspace_coefficients.shape == (4,)
    s = (asked.subspace_overlaps + asked.subspace_overlaps.conj().T) / 2
    s_min = float(np.linalg.eigvalsh(s)[0])
    print(f"subspace: eigenvalue {asked.subspace_eigenvalue:.12f}, best individual {asked.eigenvalue:.12f}, smallest eigenvalue of S {s_min:.3e}")
    assert asked.subspace_rank == 4 and s_min >= 1e-2
    exact_ground = float(np.linalg.eigvalsh(dense_operator(op))[0])
    tol = 1e-9 * max(1.0, ovr.spread(op))
    assert exact_ground - tol <= asked.subspace_eigenvalue <= asked.eigenvalue + tol


def test_state_fidelities_of_pairs():
    n = 6
    circuits, params, states = ovr.population(n, 3, 4, 6)
    first = [circuits[0], circuits[1], circuits[0]]
    second = [circuits[2], circuits[2], circuits[0]]
    values_1 = [params[0], params[1], params[0]]
    values_2 = [params[2], params[2], [v + 0.1 for v in params[0]]]
    result = GpuStateFidelity().run(first, second, values_1, values_2).result()
    shifted = helpers.oracle_state(circuits[0], values_2[2])
    want = [abs(np.vdot(states[2], states[0])) ** 2, abs(np.vdot(states[2], states[1])) ** 2, abs(np.vdot(shifted, states[0])) ** 2]
    assert len(result.fidelities) == 3 and want[2] > 0.5
    assert np.abs(np.asarray(result.fidelities) - np.asarray(want)).max() <= 1e-11
