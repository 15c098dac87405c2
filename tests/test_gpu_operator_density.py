"""Operator-weighted reduced density matrices on the device (``qsv_operator_density_circuits``) against
tests/operator_density_reference.py: W_A = Tr_rest(H_h |psi><psi|) from the NumPy oracle's states and lambda = H_h psi -- the
shapes of tests/test_gpu_reduced_density.py (registers below, at and above one block of a subset's qubits and the six lowest
others, the first register with two workgroups, workgroups that walk several blocks), operators of every kind, the same-bits and
no-disturbance contracts, the refusals, fp32 handles, ``queasars_amd.evqe.growth`` against the adjoint sweep, and the solver's
option.

Tolerance per component: overlap_reference.tol_t(op), the project's bound for <phi|H|psi>, the same kind of sum.

Seen on an MI355X: fp64, the largest |W - reference| per component is 1.2e-14 (n = 11 under the Heisenberg operator, allowed
3.2e-10; 7.4e-15 at n = 20); <H> against the variance call's 6.9e-17; fp32 handles, e_s = 2.5e-7 (n = 9) and 2.8e-7 (n = 13), the
largest error 2.0e-7; layer_gradient against the adjoint sweep 7.8e-16 (n = 10) and 5.3e-16 (n = 14); pool gradients 1.2e-15."""

from __future__ import annotations

import copy

import numpy as np
import pytest

import helpers
import operator_density_reference as odr
import operator_walk as ow
import overlap_reference as ovr
import rdm_reference as rr
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.circuit_evaluation.circuit_evaluation import CircuitEvaluatorException
from queasars_amd.evqe import growth
from queasars_amd.evqe.genome import EVQECircuitLayer, parameter_names, sorted_parameter_rank
from queasars_amd.ir import CircuitIR, ParamRef

pytestmark = pytest.mark.gpu

PARITY_CASES = [(1, 1), (2, 2), (3, 17), (5, 2), (9, 17), (10, 1), (11, 17), (13, 4), (17, 4)]
ADJOINT_TOL = 1e-10  # the adjoint sweep's own bound against its reference (tests/test_gpu_adjoint.py EXP_TOL)


def check(name, got, want, tol):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == np.complex128, (name, g.shape, w.shape)
    err = odr.largest_error(got, want)
    print(f"{name}: largest component error {err:.3e} (allowed {tol:.3e})")
    assert err <= tol, (name, err, tol)
    return err


def parity(n, count, op, name):
    circuits, params, states = rr.case(n, count)
    subsets = rr.subsets_for(n)
    evaluator = OperatorCircuitEvaluator(op)
    got, values = evaluator.operator_density_matrices(circuits, params, subsets, with_values=True)
    tol = ovr.tol_t(op)
    check(f"W n={n} {name}, {count} evaluations, {len(subsets)} subsets", got, odr.operator_density_matrices(op, states, subsets), tol)
    want_values = odr.values(op, states)
    assert np.abs(values - want_values).max() <= tol
    for m in got:  # Tr W_A = <H> on every subset
        assert np.abs(np.trace(m, axis1=1, axis2=2) - want_values).max() <= tol
    return evaluator, got


# ---- 1. parity -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,count", PARITY_CASES)
def test_parity_under_a_general_operator(n, count):
    op = odr.general_operator(n)
    assert n == 1 or np.abs(op.coeffs.imag).max() > 0.1  # (H_h != H)
    evaluator, got = parity(n, count, op, "general")
    if n <= 4:  # k = n: W = (H_h psi) psi^H of the handle's own statevector()
        circuits, params, _ = rr.case(n, count)
        whole = got[rr.subsets_for(n).index(tuple(range(n)))]
        for e, (c, p) in enumerate(zip(circuits, params)):
            psi = evaluator.statevector_device.statevector(c, p)
            assert odr.largest_error([whole[e]], [np.outer(ovr.apply_operator(op, psi), psi.conj())]) <= 1e-13 * max(1.0, ovr.spread(op))


@pytest.mark.parametrize("kind", ow.KINDS)
@pytest.mark.parametrize("n,count", [(9, 17), (11, 17)])
def test_parity_under_operators_of_every_kind(n, count, kind):
    parity(n, count, ow.kinds(n)[kind], kind)


# ---- 2. values, traces ----------------------------------------------------------------------------------------------------


def test_values_are_the_variance_calls_values():
    n = 10
    circuits, params, _ = rr.population(n, 3, 5, 10)
    op = odr.general_operator(n, seed=1)
    evaluator = OperatorCircuitEvaluator(op)
    want, _ = evaluator.evaluate_variances(circuits, params, with_values=True)
    subsets = rr.singles_and_pairs(n)
    got, values = evaluator.operator_density_matrices(circuits, params, subsets, with_values=True)
    scale = max(1.0, ovr.spread(op))
    print(f"largest |value - variance call's value| {np.abs(values - np.asarray(want)).max():.3e} (allowed {1e-12 * scale:.3e})")
    assert np.abs(values - np.asarray(want)).max() <= 1e-12 * scale
    for m in got:
        assert np.abs(np.trace(m, axis1=1, axis2=2) - np.asarray(want)).max() <= ovr.tol_t(op)
    assert [g.tobytes() for g in evaluator.operator_density_matrices(circuits, params, subsets)] == [g.tobytes() for g in got]


# ---- 3. the same bits ------------------------------------------------------------------------------------------------------


def test_a_matrix_is_the_same_bits_wherever_it_stands():
    n, count = 11, 17
    circuits, params, _ = rr.case(n, count)
    subsets = rr.subsets_for(n)
    evaluator = OperatorCircuitEvaluator(odr.general_operator(n))

    def run(order, chosen):
        got, values = evaluator.operator_density_matrices([circuits[i] for i in order], [params[i] for i in order], chosen, with_values=True)
        out = {(i, s): got[j][k].tobytes() for j, s in enumerate(chosen) for k, i in enumerate(order)}
        out.update({(i, "value"): values[k].tobytes() for k, i in enumerate(order)})
        return out

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
    twice = evaluator.operator_density_matrices(circuits[:3], params[:3], [subsets[4], subsets[9], subsets[4]])
    assert twice[0].tobytes() == twice[2].tobytes() and twice[0].tobytes() != twice[1].tobytes()


def test_more_evaluations_and_subsets_than_one_launch_takes():
    """group + 3 evaluations and 1024 subsets at n = 11: two workgroups per pair, so a launch's partial tiles (64 MiB) take 8192
    (evaluation, subset) pairs -- a second launch group and, behind the first, 32 subsets per launch; every probed matrix at its
    place with the bits it has in a call of one subset."""
    n = 11
    op = ow.kinds(n)["mixed"]
    evaluator = OperatorCircuitEvaluator(op)
    dev = evaluator.statevector_device
    group = int(dev._lib.qsv_group_size(dev._handle))
    count = group + 3
    pool = rr.singles_and_pairs(n) + [(b, a) for a, b in rr.all_pairs(n)]
    subsets = (pool * 9)[:1024]
    assert len(subsets) == 1024 and group * len(subsets) > 8192
    base_circuits, base_params, _ = rr.population(n, 3, 4, 0)
    rng = np.random.default_rng(9)
    circuits = [base_circuits[i % 4] for i in range(count)]
    params = [[float(v + rng.normal(0.0, 0.4)) for v in base_params[i % 4]] for i in range(count)]
    got, values = evaluator.operator_density_matrices(circuits, params, subsets, with_values=True)
    probes = [0, group - 1, group, count - 1]
    picks = [0, 31, 32, 500, 1023]
    for i in probes:
        state = helpers.oracle_state(circuits[i], params[i])
        check(f"evaluation {i} of {count}", [got[s][i:i + 1] for s in picks], odr.operator_density_matrices(op, [state], [subsets[s] for s in picks]),
              ovr.tol_t(op))
        for s in picks:
            alone, value = evaluator.operator_density_matrices([circuits[i]], [params[i]], [subsets[s]], with_values=True)
            assert alone[0][0].tobytes() == got[s][i].tobytes() and value[0].tobytes() == values[i].tobytes()


def test_the_call_leaves_the_other_calls_their_bits():
    n = 10
    circuits, params, _ = rr.population(n, 3, 5, 10)
    op = helpers.random_pauli_operator(n, 20, seed=1234)
    evaluator = OperatorCircuitEvaluator(op, gradient_method="adjoint")
    dev = evaluator.statevector_device
    subsets = rr.subsets_for(n)
    before = evaluator.evaluate_circuits(circuits, params)
    replays = dev.replayed_pushes()
    assert evaluator.evaluate_circuits(circuits, params) == before
    assert dev.replayed_pushes() == replays + 1  # (the second call did replay)
    variances = evaluator.evaluate_variances(circuits, params)
    rho = [m.tobytes() for m in evaluator.reduced_density_matrices(circuits, params, subsets)]
    gradients = [g.tobytes() for g in evaluator.evaluate_gradients(circuits, params)]
    states_before = [dev.statevector(c, p).tobytes() for c, p in zip(circuits[:3], params[:3])]
    w = evaluator.operator_density_matrices(circuits, params, subsets)
    assert evaluator.evaluate_circuits(circuits, params) == before  # (the recorded batch was dropped: laid out again ...)
    replays = dev.replayed_pushes()
    assert evaluator.evaluate_circuits(circuits, params) == before  # (... and replayed)
    assert dev.replayed_pushes() == replays + 1
    assert evaluator.evaluate_variances(circuits, params) == variances
    assert [m.tobytes() for m in evaluator.reduced_density_matrices(circuits, params, subsets)] == rho
    assert [g.tobytes() for g in evaluator.evaluate_gradients(circuits, params)] == gradients
    again = evaluator.operator_density_matrices(circuits, params, subsets)
    assert [a.tobytes() for a in again] == [m.tobytes() for m in w]
    assert [dev.statevector(c, p).tobytes() for c, p in zip(circuits[:3], params[:3])] == states_before
    assert dev._operator is op


def test_two_evaluators_on_one_device_each_get_their_own():
    n = 9
    circuits, params, states = rr.population(n, 3, 3, 9)
    kinds = ow.kinds(n)
    first = OperatorCircuitEvaluator(kinds["mixed"])
    second = OperatorCircuitEvaluator(kinds["offdiag"], statevector_device=first.statevector_device)
    initial = CircuitIR(n).u(0.7, 0.2, 0.3, 0).cu3(1.1, 0.3, 0.2, 0, 8).u(0.4, 0.1, 0.9, 3)
    third = OperatorCircuitEvaluator(kinds["cubic"], initial_state_circuit=initial, statevector_device=first.statevector_device)
    subsets = rr.subsets_for(n)
    behind = [helpers.oracle_state(initial.compose(c), p) for c, p in zip(circuits, params)]
    for evaluator, these in [(first, states), (second, states), (third, behind), (first, states)]:
        op = evaluator._operator
        got = evaluator.operator_density_matrices(circuits, params, subsets)
        check(f"shared device, {len(op)} terms", got, odr.operator_density_matrices(op, these, subsets), ovr.tol_t(op))
        assert first.statevector_device._operator is op


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------


def _raw(dev, circuits, params, subsets, n_evals=None, n_subsets=None, out_given=True, offsets_given=True, qubits_given=True, values_given=True):
    """qsv_operator_density_circuits as the C ABI returns it: (return code, message, out, values)."""
    n = len(circuits)
    ids, offsets, flat = dev._batch_arguments(circuits, params) if n else (np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1))
    starts = np.zeros(len(subsets) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in subsets], out=starts[1:])
    qubits = np.asarray([q for s in subsets for q in s] + [0], dtype=np.int32)
    out = np.full((max(1, n), max(1, sum(4 ** len(s) for s in subsets))), np.nan, dtype=np.complex128)
    values = np.full(max(1, n), np.nan)
    rc = dev._lib.qsv_operator_density_circuits(
        dev._handle, len(subsets) if n_subsets is None else n_subsets, _lib.as_ptr(starts) if offsets_given else None,
        _lib.as_ptr(qubits) if qubits_given else None, n if n_evals is None else n_evals, _lib.as_ptr(ids), _lib.as_ptr(offsets),
        _lib.as_ptr(flat), _lib.as_ptr(out) if out_given else None, _lib.as_ptr(values) if values_given else None)
    return rc, _lib.last_error(dev._lib, dev._handle), out, values


def test_refusals_leave_the_handle_working():
    n = 6
    circuits, params, states = rr.population(n, 3, 3, 6)
    op = odr.general_operator(n)
    dev = StatevectorDevice(n)
    subsets = [(0,), (5, 2), (1, 3, 4, 0)]
    want = np.concatenate([m.reshape(3, -1) for m in odr.operator_density_matrices(op, states, subsets)], axis=1)
    first = []

    def works(**kwargs):
        rc, _, out, values = _raw(dev, circuits, params, subsets, **kwargs)
        assert rc == _lib.QSV_OK and odr.largest_error([out], [want]) <= ovr.tol_t(op)
        first.append(out.tobytes())
        assert first[0] == first[-1]
        return values

    def refused(code, word, chosen=subsets, **kwargs):
        rc, message, out, values = _raw(dev, kwargs.pop("circuits", circuits), kwargs.pop("params", params), chosen, **kwargs)
        assert rc == code and word in message, (rc, message)
        assert np.isnan(out).all() and np.isnan(values).all()  # (nothing was written)

    # no operator was ever set
    refused(_lib.QSV_E_STATE, "no operator set")
    with pytest.raises(CircuitEvaluatorException, match="no operator set"):
        dev.operator_density_matrices(circuits, params, subsets)
    refused(_lib.QSV_E_ARG, "twice", chosen=[(2, 2)])  # (the subsets are checked first, as the reduced density call checks them)
    assert _raw(dev, [], [], subsets, n_evals=0)[0] == _lib.QSV_OK
    dev.set_operator(op)
    assert np.abs(works() - odr.values(op, states)).max() <= ovr.tol_t(op)
    assert np.isnan(works(values_given=False)).all()  # (out_values may be NULL)
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
        dev.operator_density_matrices([continued], [[]], subsets)
    assert _raw(dev, [], [], subsets, n_evals=0, out_given=False)[0] == _lib.QSV_OK
    refused(_lib.QSV_E_ARG, "twice", chosen=[(3, 3)], circuits=[], params=[], n_evals=0)
    # inside an open batch, from the thread that holds it
    batch_ids, offsets, flat = dev._batch_arguments(circuits, params)
    counts = np.diff(offsets).astype(np.int64)
    values = np.zeros(len(circuits))
    assert dev._lib.qsv_eval_begin(dev._handle, len(circuits), _lib.as_ptr(batch_ids), _lib.as_ptr(counts)) == _lib.QSV_OK
    refused(_lib.QSV_E_STATE, "(qsv_operator_density_circuits goes between batches)")
    assert dev._lib.qsv_eval_push(dev._handle, 0, len(circuits), _lib.as_ptr(flat)) == _lib.QSV_OK
    assert dev._lib.qsv_eval_end(dev._handle, _lib.as_ptr(values)) == _lib.QSV_OK
    assert np.abs(values - dev.expectation_values(circuits, params)).max() <= 1e-12
    works()


def test_a_register_above_28_qubits_is_refused():
    """More than 28 qubits -> QSV_E_UNSUPPORTED, with a sentence that names the limit: a 29-qubit fp32 handle, asked before
    anything is uploaded (and before the operator is looked for)."""
    n = 29
    dev = StatevectorDevice(n, dtype="fp32")
    circuit = CircuitIR(n).u(0.3, 0.2, 0.1, 0)
    rc, message, _, _ = _raw(dev, [circuit], [[]], [(0,), (28, 3)])
    assert rc == _lib.QSV_E_UNSUPPORTED and "28 qubits" in message and "29" in message, (rc, message)
    with pytest.raises(ValueError, match="28 qubits"):
        dev.operator_density_matrices([circuit], [[]], [(0,)])


# ---- 5. fp32 handles ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,count", [(9, 6), (13, 4)])
def test_fp32_handles(n, count):
    """|dW| <= tol_fp32(e_s) max(1, spread), e_s the largest |psi_32 - psi_ref|_2 of the fp32 handle's own statevector() over this
    test's circuits -- the existing route, not the new one; lambda is fp32 there too, one more rounding of the same size."""
    circuits, params, states = rr.case(n, count)
    op = odr.general_operator(n)
    evaluator = OperatorCircuitEvaluator(op, dtype="fp32")
    dev = evaluator.statevector_device
    e_s = max(float(np.linalg.norm(dev.statevector(c, p) - s)) for c, p, s in zip(circuits, params, states))
    tol = ovr.tol_fp32(e_s) * max(1.0, ovr.spread(op))
    print(f"n={n} fp32: e_s = {e_s:.3e}, allowed |dW| = {tol:.3e}")
    subsets = rr.subsets_for(n)
    got, values = evaluator.operator_density_matrices(circuits, params, subsets, with_values=True)
    check(f"fp32 W n={n}", got, odr.operator_density_matrices(op, states, subsets), tol)
    assert np.abs(values - odr.values(op, states)).max() <= tol


# ---- 6. growth.py: two independent device paths ---------------------------------------------------------------------------------


def _grown(circuit, layer):
    """`circuit` with `layer` appended on new parameters behind its own, in the layer's parameter order."""
    rank = sorted_parameter_rank(parameter_names(0, layer.gates))
    base = circuit.num_parameters
    out = copy.copy(circuit)
    layer.lower(out, 0, {name: ParamRef(base + r) for name, r in rank.items()})
    return out.declare_parameters(base + layer.n_parameters)


@pytest.mark.parametrize("n", [10, 14])
def test_layer_gradients_are_the_adjoint_gradients_of_the_grown_circuits(n):
    """Four parents of operator_walk.population(n), a random layer appended at zeros: layer_gradient from ONE operator density
    call against the new parameters' entries of the adjoint sweep over the grown circuit.  Bound: a gradient entry is 2 Re sum D
    conj W over at most two entries of D with |D| <= 1, each W component within tol_t(op), plus the adjoint sweep's own bound."""
    op = ow.kinds(n)["mixed"]
    individuals, made = ow.population(n)
    parents = made[:4]
    assert len(parents) == 4
    evaluator = OperatorCircuitEvaluator(op, gradient_method="adjoint")
    circuits, params = [c for _, c, _ in parents], [list(p) for _, _, p in parents]
    u, cu3 = growth.appended_gate_gradients(evaluator, circuits, params)
    bound = ovr.tol_t(op) * 2 * 2 + ADJOINT_TOL
    layers, grown, points = [], [], []
    for e, (circuit, values) in enumerate(zip(circuits, params)):
        previous = individuals[e].layers[-1] if e < len(individuals) else None
        layer = EVQECircuitLayer.random_layer(n, previous_layer=previous, random_seed=50 + e)
        layers.append(layer)
        grown.append(_grown(circuit, layer))
        points.append(list(values)[: circuit.num_parameters] + [0.0] * layer.n_parameters)
    full = evaluator.evaluate_gradients(grown, points)
    worst, largest = 0.0, 0.0
    for e, (layer, circuit) in enumerate(zip(layers, circuits)):
        want = np.asarray(full[e])[circuit.num_parameters:]
        got = growth.layer_gradient(layer, u[e], cu3[e])
        assert got.shape == want.shape == (layer.n_parameters,)
        worst, largest = max(worst, float(np.abs(got - want).max())), max(largest, float(np.abs(want).max()))
    print(f"n={n}: largest |layer_gradient - adjoint| {worst:.3e} (allowed {bound:.3e}), largest entry {largest:.3e}")
    assert worst <= bound and largest > 1e-3


def test_pool_gradients_of_twenty_random_generators():
    n = 10
    op = odr.general_operator(n, seed=2)
    circuits, params, states = rr.population(n, 3, 3, 10)
    generators = odr.random_generators(n, 20, seed=5)
    assert {len(q) for _, q in generators} == {1, 2, 3, 4}
    got = growth.pool_gradients(OperatorCircuitEvaluator(op), circuits, params, generators)
    lams = [ovr.apply_operator(op, s) for s in states]
    want = np.asarray([[odr.pool_gradient(op, s, label, qubits, lam) for label, qubits in generators] for s, lam in zip(states, lams)])
    bound = ovr.tol_t(op) * 2 * 16  # (2 Re sum over the at most 16 nonzero entries of -i P / 2, each of size 1/2 ... 1)
    err = float(np.abs(got - want).max())
    print(f"pool gradients: largest error {err:.3e} (allowed {bound:.3e})")
    assert err <= bound and np.abs(want).max() > 1e-2


def test_a_solver_run_with_four_growth_candidates():
    from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    n = 6
    config = EVQEMinimumEigensolverConfiguration(
        optimizer=SPSA(maxiter=10, learning_rate=0.4, perturbation=0.3), population_size=6, max_generations=3, random_seed=5,
        n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
        use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
        parameter_search_probability=0.3, topological_search_probability=0.6, layer_removal_probability=0.05, growth_candidates=4,
    )
    seen, scores = [], []
    solver = EVQEMinimumEigensolver(config, on_generation=lambda g: (seen.append(g["population"].individuals), scores.append(list(solver.last_growth_scores))))
    result = solver.compute_minimum_eigenvalue(OperatorCircuitEvaluator(helpers.random_pauli_operator(n, 33, seed=1234)))
    assert result.generations == 3 and len(seen) == 3
    for individuals in seen:
        assert all(i.is_valid() and all(layer.is_valid() for layer in i.layers) for i in individuals)
    assert any(scores) and all(norms[best] == max(norms) for generation in scores for best, norms in generation)
    assert max(len(i.layers) for i in seen[-1]) > 2  # (layers were grown)
