"""Exact readout on the device (``qsv_top_states``): the k most probable basis states of a circuit under the order
probability descending, basis-state index ascending, against the NumPy oracle's probabilities
(``so.probabilities(helpers.oracle_state(c, p))``) through tests/top_states_reference.py's checks -- both routes (split
circuits read from their side tables, the others from the probabilities of their last gate pass) in one batch, both dtypes,
several launch groups, exact ties, the values of a diagonal operator, the refusals, and the solver's ``eigenstate``."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import helpers
from oracle import statevector_oracle as so
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice, most_probable_states
from queasars_amd.ir import CircuitIR
from top_states_reference import FP32_REL, TOL_FP64, check_top, expected_top

pytestmark = pytest.mark.gpu

X = (np.pi, 0.0, np.pi)
MIXED_SEED = {12: 0, 14: 0}  # (population seeds at which the batch below holds both routes: asserted through qsv_circuit_form)
# A circuit splits only when the register is wider than a tile, and the default tile holds twelve qubits: the 12-qubit handle
# gets ten-qubit tiles (a geometry tests/test_gpu_parity.py runs too), so that both routes meet at both sizes.
GEOMETRY = {12: dict(tile_bits=10, reg_bits=3, low_bits=3), 14: {}}


def _oracle_probs(circuit, params):
    return so.probabilities(helpers.oracle_state(circuit, params))


def _raw(dev, circuits, params, k, with_values=False):
    """qsv_top_states as the C ABI returns it: (return code, states, probabilities, values)."""
    n = len(circuits)
    ids, offsets, flat = dev._batch_arguments(circuits, params)
    room = max(1, min(k, 2048))
    states = np.zeros((n, room), dtype=np.uint64)
    probs = np.zeros((n, room))
    values = np.zeros((n, room)) if with_values else None
    rc = dev._lib.qsv_top_states(dev._handle, n, _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(flat), k, _lib.as_ptr(states),
                                 _lib.as_ptr(probs), _lib.as_ptr(values) if with_values else None)
    return rc, states, probs, values


@functools.lru_cache(maxsize=None)
def _mixed_batch(n):
    """Populations of two, three and four layers: shallow circuits that the sampler branch reads from their side tables and
    deeper ones that run their gate passes; with the oracle's probabilities, computed once."""
    circuits, params = [], []
    for layers in (2, 3, 4):
        _, c, p = helpers.population_circuits(n, layers, 6, seed=MIXED_SEED[n] + layers)
        circuits += c
        params += p
    return circuits, params, [_oracle_probs(c, p) for c, p in zip(circuits, params)]


# ---- tiny, ties, extremes -------------------------------------------------------------------------------------------


def test_the_whole_distribution_in_order_and_k_out_of_range():
    n = 3
    _, circuits, params = helpers.population_circuits(n, 2, 2, seed=1)
    dev = StatevectorDevice(n)
    states, probs, values = dev.top_states(circuits, params, 8)
    assert values is None and states.dtype == np.uint64 and states.shape == probs.shape == (2, 8)
    for i, (c, p) in enumerate(zip(circuits, params)):
        oracle = _oracle_probs(c, p)
        check_top(states[i], probs[i], oracle, 8, TOL_FP64)
        assert sorted(states[i].tolist()) == list(range(8))
        assert abs(probs[i].sum() - 1.0) < 1e-13
        assert most_probable_states(dev, [c], [p], 1)[0] == {format(int(states[i, 0]), "03b"): float(probs[i, 0])}
    for k in (9, 0, -1):
        assert _raw(dev, circuits, params, k)[0] == _lib.QSV_E_ARG, k
        with pytest.raises(ValueError):
            dev.top_states(circuits, params, k)
    wide = StatevectorDevice(12)
    _, circuits, params = helpers.population_circuits(12, 2, 1, seed=1)
    assert _raw(wide, circuits, params, 1025)[0] == _lib.QSV_E_ARG
    assert _raw(wide, circuits, params, 1024)[0] == _lib.QSV_OK
    assert wide.top_states([], [], 4)[0].shape == (0, 4)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_exact_ties_at_zero_come_in_index_order(dtype):
    """An id-only circuit: probability one at state 0 and exact zeros everywhere else -- the tie rule alone decides."""
    n = 10
    idle = CircuitIR(n)
    for q in range(n):
        idle.id(q)
    for split in (1, 0):
        dev = StatevectorDevice(n, dtype=dtype)
        dev.set_option("split", split)
        states, probs, _ = dev.top_states([idle], [[]], 8)
        assert states[0].tolist() == list(range(8))
        assert probs[0].tolist() == [1.0] + [0.0] * 7


@pytest.mark.parametrize("split", [1, 0])
def test_the_top_state_in_the_last_block_and_the_last_tile(split):
    """X-like gates on every qubit: the top state is 2^n - 1, the very last one a workgroup reads."""
    n = 14
    flip = CircuitIR(n)
    for q in range(n):
        flip.u(*X, q)
    dev = StatevectorDevice(n)
    dev.set_option("split", split)
    states, probs, _ = dev.top_states([flip], [[]], 4)
    assert int(states[0, 0]) == (1 << n) - 1 and abs(probs[0, 0] - 1.0) < TOL_FP64
    check_top(states[0], probs[0], _oracle_probs(flip, []), 4, TOL_FP64)


# ---- both routes in one batch -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [12, 14])
def test_both_routes_in_one_batch(n, dtype):
    circuits, params, oracle = _mixed_batch(n)
    tol = TOL_FP64 if dtype == "fp64" else FP32_REL
    for split in (1, 0):
        dev = StatevectorDevice(n, dtype=dtype, **GEOMETRY[n])
        dev.set_option("split", split)
        sampled = [dev.circuit_form(c)["split_sampled"] for c in circuits]
        if split:
            assert any(sampled) and not all(sampled), sampled
        else:
            assert not any(sampled), sampled
        for k in (1, 16, 1024):
            states, probs, _ = dev.top_states(circuits, params, k)
            for i in range(len(circuits)):
                check_top(states[i], probs[i], oracle[i], k, tol)
        dev.close()


# ---- groups, determinism ----------------------------------------------------------------------------------------------


def test_rows_of_several_launch_groups_land_at_the_callers_index():
    n, k = 10, 16
    dev = StatevectorDevice(n)
    count = int(dev._lib.qsv_group_size(dev._handle)) + 3
    _, circuits, params = helpers.population_circuits(n, 2, 12, seed=4)
    rng = np.random.default_rng(7)
    picks = rng.integers(0, len(circuits), size=count)
    batch_c = [circuits[j] for j in picks]
    batch_p = [list(rng.uniform(0, 2 * np.pi, len(params[j]))) for j in picks]
    states, probs, _ = dev.top_states(batch_c, batch_p, k)
    again = dev.top_states(batch_c, batch_p, k)
    assert states.tobytes() == again[0].tobytes() and probs.tobytes() == again[1].tobytes()
    for i in range(count):
        alone = dev.top_states([batch_c[i]], [batch_p[i]], k)
        assert alone[0].tobytes() == states[i].tobytes() and alone[1].tobytes() == probs[i].tobytes(), i
    for i in (0, count // 2, count - 1):
        check_top(states[i], probs[i], _oracle_probs(batch_c[i], batch_p[i]), k, TOL_FP64)


def test_the_same_call_twice_gives_the_same_bytes():
    n = 14
    circuits, params, _ = _mixed_batch(n)
    op = helpers.random_ising_operator(n, seed=14)
    dev = StatevectorDevice(n)
    dev.set_operator(op)
    first = dev.top_states(circuits, params, 1024, with_values=True)
    second = dev.top_states(circuits, params, 1024, with_values=True)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


# ---- values -----------------------------------------------------------------------------------------------------------


def _diag_table(op):
    """D[i] = sum_k c_k (-1)^popcount(i & z_k) of a diagonal operator."""
    index = np.arange(1 << op.num_qubits, dtype=np.uint64)
    table = np.zeros(index.size)
    for z, c in zip(op.z_mask, op.coeffs):
        parity = index & np.uint64(z)
        for shift in (32, 16, 8, 4, 2, 1):
            parity ^= parity >> np.uint64(shift)
        table += np.where(parity & np.uint64(1), -c.real, c.real)
    return table


def test_values_are_the_diagonal_operators_at_the_states():
    n = 12
    circuits, params, oracle = _mixed_batch(n)
    op = helpers.random_ising_operator(n, seed=12)
    table, spread = _diag_table(op), float(np.abs(op.coeffs).sum())
    dev = StatevectorDevice(n)
    rc = _raw(dev, circuits, params, 16, with_values=True)[0]
    assert rc == _lib.QSV_E_STATE  # no operator set
    dev.set_operator(helpers.random_pauli_operator(n, 12, seed=4))
    assert _raw(dev, circuits, params, 16, with_values=True)[0] == _lib.QSV_E_STATE  # not diagonal
    assert _raw(dev, circuits, params, 16)[0] == _lib.QSV_OK  # (without values no operator is looked at)
    dev.set_operator(op)
    states, probs, values = dev.top_states(circuits, params, 16, with_values=True)
    assert values.shape == (len(circuits), 16)
    assert np.abs(values - table[states.astype(np.int64)]).max() <= 1e-12 * spread
    for i in range(len(circuits)):
        check_top(states[i], probs[i], oracle[i], 16, TOL_FP64)
    # the evaluator's own call: behind its operator, values included
    got = OperatorCircuitEvaluator(op, statevector_device=dev).top_states(circuits[:2], params[:2], 16)
    assert got[0].tobytes() == states[:2].tobytes() and got[2].tobytes() == values[:2].tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------------


def test_circuits_on_kept_states_are_refused():
    n = 10
    dev = StatevectorDevice(n)
    front = CircuitIR(n).u(0.3, 0.2, 0.1, 0).cu3(0.5, 0.1, 0.2, 0, 1)
    rest = CircuitIR(n).u(0.4, 0.0, 0.0, 2)
    state = dev.keep_states([front], [[]])[0]
    kept = rest.continue_from(state)
    assert _raw(dev, [kept], [[]], 4)[0] == _lib.QSV_E_UNSUPPORTED
    whole = CircuitIR(n).u(0.3, 0.2, 0.1, 0).cu3(0.5, 0.1, 0.2, 0, 1).u(0.4, 0.0, 0.0, 2)
    assert _raw(dev, [whole], [[]], 4)[0] == _lib.QSV_OK


# ---- end to end -------------------------------------------------------------------------------------------------------


def test_the_solvers_eigenstate_decodes_to_the_schedule():
    """BASELINE config 4 (tests/test_gpu_parity.py test_config4_jssp_end_to_end_evqe: the notebook's 12-qubit JSSP instance,
    sampler + CVaR 0.5) with eigenstate_states=8: the first key decodes to the valid makespan-5 schedule, its value is the
    operator's at that bitstring, the probabilities are probabilities()'s at those states."""
    import jssp_instances as inst
    from queasars_amd.circuit_evaluation import OperatorSamplerCircuitEvaluator
    from queasars_amd.evqe.solver import (
        SPSA, BestIndividualRelativeChangeTolerance, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration, SPSATerminationChecker,
    )
    from queasars_amd.job_shop_scheduling import JSSPDomainWallHamiltonianEncoder

    enc = JSSPDomainWallHamiltonianEncoder(inst.notebook_2x3(), makespan_limit=6, **inst.NOTEBOOK_PENALTIES)
    op = enc.get_problem_hamiltonian()
    evaluator = OperatorSamplerCircuitEvaluator(512, op, alpha=0.5, seed=0)
    cfg = EVQEMinimumEigensolverConfiguration(
        optimizer=SPSA(maxiter=33, perturbation=0.35, learning_rate=0.43, trust_region=True,
                       termination_checker=SPSATerminationChecker(0.01, 2)),
        population_size=10, max_generations=8, termination_criterion=BestIndividualRelativeChangeTolerance(0.01, 1),
        random_seed=0, n_initial_layers=2, randomize_initial_population_parameters=True,
        speciation_genetic_distance_threshold=1, use_tournament_selection=True, tournament_size=2,
        selection_alpha_penalty=0.15, selection_beta_penalty=0.02, parameter_search_probability=0.39,
        topological_search_probability=0.79, layer_removal_probability=0.02,
    )
    result = EVQEMinimumEigensolver(cfg).compute_minimum_eigenvalue(evaluator, eigenstate_states=8)
    assert abs(result.eigenvalue - 22.75) < 1e-6
    assert len(result.eigenstate) == 8 and list(result.eigenstate_values) == list(result.eigenstate)
    top = next(iter(result.eigenstate))
    schedule = enc.translate_result_bitstring(top)
    assert schedule.is_valid and schedule.makespan == 5
    table, spread = _diag_table(op), float(np.abs(op.coeffs).sum())
    for name, value in result.eigenstate_values.items():
        assert abs(value - table[int(name, 2)]) <= 1e-12 * spread
    best = result.best_individual
    probs = evaluator.statevector_device.probabilities(best.get_parameterized_quantum_circuit(), list(best.parameter_values))
    got = np.asarray(list(result.eigenstate.values()))
    states = np.asarray([int(name, 2) for name in result.eigenstate], dtype=np.uint64)
    assert np.abs(got - probs[states.astype(np.int64)]).max() <= TOL_FP64
    check_top(states, got, probs, 8, TOL_FP64)
    assert int(states[0]) == int(expected_top(probs, 1)[0][0])
