"""Operator-weighted reduced density matrices without a device: tests/operator_density_reference.py held to
facts, queasars_amd/evqe/growth.py held to the reference, the Python layer on recording stand-ins
(tests/test_evaluator_layer_host.py's device), the prototype in header, binding and docstring, and the solver's
``growth_candidates`` on an evaluator that answers from NumPy oracle states."""

from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import dense_gradient
import factorised_reference as fr
import helpers
import operator_density_reference as odr
import overlap_reference as ovr
import rdm_reference as rr
import test_evaluator_layer_host as layer
from oracle import statevector_oracle as so
from queasars_amd import _build, _lib
from queasars_amd.circuit_evaluation.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe import growth
from queasars_amd.evqe.genome import EVQECircuitLayer, EVQEIndividual
from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration
from queasars_amd.ir import OP_CU3, OP_U, CircuitIR, PauliOperator


def _states(n, count=3, seed=5):
    return rr.population(n, 3, count, seed)[2]


# ---- the reference against facts ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 2, 5, 7, 9])
def test_the_trace_is_the_expectation_value_on_every_subset(n):
    op = odr.general_operator(n)
    assert np.abs(op.coeffs.imag).max() > 0.1  # (H_h != H)
    for state in _states(n):
        want = float(np.real(np.vdot(state, ovr.apply_operator(op, state))))
        for subset in rr.subsets_for(n):
            w = odr.operator_density_matrix(op, state, subset)
            assert w.shape == (1 << len(subset),) * 2
            assert abs(np.trace(w) - want) <= 1e-13 * max(1.0, ovr.spread(op))
    assert abs(odr.values(op, _states(n))[0] - float(np.real(np.vdot(_states(n)[0], ovr.apply_operator(op, _states(n)[0]))))) <= 1e-15


def test_the_whole_register_gives_h_psi_psi_dagger():
    for n in (1, 3, 4):
        op, state = odr.general_operator(n), _states(n)[0]
        h = dense_gradient.dense_operator(op)
        want = np.outer(h @ state, state.conj())
        assert np.abs(odr.operator_density_matrix(op, state, tuple(range(n))) - want).max() <= 1e-14
        # W is not Hermitian; under the identity it is the reduced density matrix
        assert np.abs(want - want.conj().T).max() > 1e-3
        one = PauliOperator(["I" * n], [1.0])
        for subset in rr.subsets_for(n):
            assert np.abs(odr.operator_density_matrix(one, state, subset) - rr.reduced_density_matrix(state, subset)).max() <= 1e-15


def _energy_behind(state, h, kind, target, control, angles):
    n = int(state.size).bit_length() - 1
    psi = so.simulate(n, [(kind, target, control, *angles)], initial_state=state.copy())
    return float(np.real(np.vdot(psi, h @ psi)))


def test_gate_gradients_are_central_differences_of_the_dense_energy():
    """u on every qubit and cu3 on every ordered pair of five qubits, all three angles, a step of 1e-6: the difference
    quotient's own error is O(step^2) times third derivatives (|H| <= spread) plus rounding / step, a few 1e-10 spread."""
    n, step = 5, 1e-6
    op = odr.general_operator(n, seed=3)
    h = dense_gradient.dense_operator(op)
    state = _states(n, seed=9)[1]
    bound = 1e-8 * max(1.0, ovr.spread(op))
    u, cu3 = odr.u_gradients(op, state), odr.cu3_gradients(op, state)
    worst = 0.0
    for angle in range(3):
        plus, minus = [0.0] * 3, [0.0] * 3
        plus[angle], minus[angle] = step, -step
        for q in range(n):
            want = (_energy_behind(state, h, OP_U, q, -1, plus) - _energy_behind(state, h, OP_U, q, -1, minus)) / (2 * step)
            worst = max(worst, abs(u[q, angle] - want))
        for c in range(n):
            for t in range(n):
                if c != t:
                    want = (_energy_behind(state, h, OP_CU3, t, c, plus) - _energy_behind(state, h, OP_CU3, t, c, minus)) / (2 * step)
                    worst = max(worst, abs(cu3[c, t, angle] - want))
    print(f"largest |formula - central difference| {worst:.2e} (allowed {bound:.2e})")
    assert worst <= bound
    assert np.abs(u).max() > 1e-2 and np.abs(cu3).max() > 1e-2 and not cu3[np.arange(n), np.arange(n)].any()


def test_pool_gradients_are_central_differences_of_the_dense_energy():
    n, step = 5, 1e-6
    op = odr.general_operator(n, seed=4)
    h = dense_gradient.dense_operator(op)
    state = _states(n, seed=8)[0]
    for label, qubits in odr.random_generators(n, 12, seed=2):
        letters = ["I"] * n
        for letter, q in zip(label, qubits):
            letters[n - 1 - q] = letter  # (Qiskit's order: the rightmost letter is qubit 0)
        p = so.dense_pauli("".join(letters))

        def energy(theta):
            psi = np.cos(theta / 2) * state - 1j * np.sin(theta / 2) * (p @ state)  # exp(-i theta P / 2) psi
            return float(np.real(np.vdot(psi, h @ psi)))

        want = (energy(step) - energy(-step)) / (2 * step)
        assert abs(odr.pool_gradient(op, state, label, qubits) - want) <= 1e-8 * max(1.0, ovr.spread(op)), (label, qubits)


def test_x_fields_on_the_zero_state():
    """psi = |0..0> and H = sum_q c_q X_q: E(theta on q) = c_q sin(theta), so the u theta-gradient on q is c_q; the control of
    every cu3 is |0>, so it does nothing."""
    n = 4
    c = [0.7, -1.3, 0.25, 2.0]
    op = PauliOperator.from_sparse_list([("X", [q], c[q]) for q in range(n)], n)
    state = np.eye(1, 1 << n).ravel().astype(complex)
    u, cu3 = odr.u_gradients(op, state), odr.cu3_gradients(op, state)
    assert np.abs(u[:, 0] - np.asarray(c)).max() <= 1e-15 and not u[:, 1:].any()
    assert not cu3.any()


@pytest.mark.parametrize("n,sizes", [(9, (5, 4)), (12, (4, 4, 4))])
def test_the_factorised_form_against_the_full_state(n, sizes):
    blocks = fr.interleaved_blocks(n, sizes, seed=n)
    pc = fr.product_circuit(n, blocks, "generic", seed=n)
    f = fr.Factorised(blocks, pc.states())
    state = fr.full_state(f)
    op = fr.general_operator(n, blocks, seed=1)
    owner = {q: b for b, qubits in enumerate(blocks) for q in qubits}
    subsets = [(blocks[0][0],), (blocks[0][2], blocks[0][0]), (blocks[1][1], blocks[0][0], blocks[1][0]),
               (blocks[-1][3], blocks[0][1], blocks[-1][2], blocks[1][0]), (n - 1, 0)]
    assert all(len(set(s)) == len(s) for s in subsets)
    assert {len({owner[q] for q in s}) for s in subsets} >= {1, 2}
    lam = ovr.apply_operator(op, state)
    for subset in subsets:
        want = odr.cross_matrix(lam, state, subset)
        assert np.abs(odr.factorised_matrix(op, f, subset) - want).max() <= 1e-13 * max(1.0, fr.spread(op)), subset


# ---- growth.py against the reference ------------------------------------------------------------------------------------------------


class NumpyEvaluator:
    """``evaluate_circuits`` and ``operator_density_matrices`` from the NumPy oracle; counts its calls."""

    def __init__(self, operator):
        self.operator, self.density_calls, self.evaluations = operator, [], 0

    @property
    def n_qubits(self):
        return self.operator.num_qubits

    def evaluate_circuits(self, circuits, parameter_values):
        self.evaluations += len(circuits)
        return [helpers.oracle_expectation(c, p, self.operator) for c, p in zip(circuits, parameter_values)]

    def operator_density_matrices(self, circuits, parameter_values, subsets, with_values=False):
        self.density_calls.append((len(circuits), list(subsets)))
        states = [helpers.oracle_state(c, p) for c, p in zip(circuits, parameter_values)]
        matrices = odr.operator_density_matrices(self.operator, states, subsets)
        return (matrices, odr.values(self.operator, states)) if with_values else matrices


def test_the_derivative_matrices_are_the_references():
    assert np.array_equal(growth.D_THETA, odr.D_THETA) and np.array_equal(growth.D_PHI, odr.D_PHI) and np.array_equal(growth.D_LAMBDA, odr.D_LAMBDA)
    for bit in (0, 1):
        for d in odr.DERIVATIVES:
            assert np.array_equal(growth.controlled_derivative(d, bit), odr.controlled(d, bit))
    assert np.array_equal(growth.pauli_matrix("XZY"), odr.pauli_on("XZY"))
    # the Qiskit matrix of u, differentiated numerically at identity
    for slot, d in enumerate(odr.DERIVATIVES):
        plus, minus = [0.0] * 3, [0.0] * 3
        plus[slot], minus[slot] = 1e-6, -1e-6
        assert np.abs((so.u_matrix(*plus) - so.u_matrix(*minus)) / 2e-6 - d).max() <= 1e-9
        assert np.abs(dense_gradient.du_matrix(0.0, 0.0, 0.0, slot) - d).max() == 0.0


def test_appended_gate_gradients_make_one_call_over_singles_and_pairs():
    n = 5
    op = odr.general_operator(n, seed=6)
    circuits, params, states = rr.population(n, 3, 3, 4)
    ev = NumpyEvaluator(op)
    u, cu3 = growth.appended_gate_gradients(ev, circuits, params)
    assert ev.density_calls == [(3, rr.singles_and_pairs(n))] and growth.growth_subsets(n) == rr.singles_and_pairs(n)
    assert u.shape == (3, n, 3) and cu3.shape == (3, n, n, 3)
    for e, state in enumerate(states):
        assert np.abs(u[e] - odr.u_gradients(op, state)).max() <= 1e-14
        assert np.abs(cu3[e] - odr.cu3_gradients(op, state)).max() <= 1e-14
    assert not cu3[:, np.arange(n), np.arange(n)].any()


def test_pool_gradients_make_one_call_over_the_distinct_subsets():
    n = 6
    op = odr.general_operator(n, seed=7)
    circuits, params, states = rr.population(n, 3, 2, 6)
    generators = odr.random_generators(n, 20, seed=1) + [("XY", (3, 1)), ("ZZ", (3, 1))]
    ev = NumpyEvaluator(op)
    got = growth.pool_gradients(ev, circuits, params, generators)
    (call,) = ev.density_calls
    assert call[1] == list(dict.fromkeys(q for _, q in generators)) and got.shape == (2, 22)
    for e, state in enumerate(states):
        want = [odr.pool_gradient(op, state, label, qubits) for label, qubits in generators]
        assert np.abs(got[e] - want).max() <= 1e-14
    with pytest.raises(ValueError):
        growth.pool_gradients(ev, circuits, params, [("XX", (1,))])
    with pytest.raises(ValueError):
        growth.pool_gradients(ev, circuits, params, [("XXXXX", (0, 1, 2, 3, 4))])
    assert growth.pool_gradients(ev, circuits, params, []).shape == (2, 0)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_layer_gradient_is_the_dense_gradient_of_the_grown_circuit(seed):
    """A random layer appended at zeros: layer_gradient against tests/dense_gradient.py's derivative of the grown circuit by the
    new layer's parameters, in the grown circuit's parameter order."""
    n = 6
    op = odr.general_operator(n, seed=seed)
    h = dense_gradient.dense_operator(op)
    parent = EVQEIndividual.random_individual(n, 2, True, random_seed=seed)
    layer_ = EVQECircuitLayer.random_layer(n, previous_layer=parent.layers[-1], random_seed=100 + seed)
    grown = EVQEIndividual(n, (*parent.layers, layer_), (*parent.parameter_values, *((0.0,) * layer_.n_parameters)))
    ev = NumpyEvaluator(op)
    u, cu3 = growth.appended_gate_gradients(ev, [parent.get_parameterized_quantum_circuit()], [list(parent.parameter_values)])
    got = growth.layer_gradient(layer_, u[0], cu3[0])
    full = dense_gradient.gradient(grown.get_parameterized_quantum_circuit(), list(grown.parameter_values), h)
    want = full[len(parent.parameter_values):]
    assert got.shape == want.shape == (layer_.n_parameters,) and layer_.n_parameters > 0
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, ovr.spread(op))
    assert np.abs(want).max() > 1e-3


# ---- the Python layer on recording stand-ins ------------------------------------------------------------------------------------

SUBSETS = [(0,), (2, 0)]


class RecordingDevice(layer.RecordingDevice):
    def operator_density_matrices(self, circuits, parameter_values, subsets, with_values=False):
        n = self._note("operator_density_matrices", circuits)
        self.calls[-1].parameter_values = list(parameter_values)
        matrices = [np.zeros((n, 1 << len(s), 1 << len(s)), dtype=complex) for s in subsets]
        return (matrices, np.zeros(n)) if with_values else matrices


def test_the_method_is_no_evaluate_method():
    """tests/test_evaluator_layer_host.py lists every ``evaluate_*`` method: this one is held to its rules here instead."""
    assert callable(getattr(OperatorCircuitEvaluator, "operator_density_matrices"))
    assert not hasattr(OperatorCircuitEvaluator, "evaluate_operator_density_matrices")


def test_the_evaluator_method_runs_inside_the_operator_guard():
    device = RecordingDevice()
    ev = layer.operator_evaluator(device)
    layer.leave_another_operator(device)
    got, values = ev.operator_density_matrices(layer.make_circuits(), layer.VALUES, SUBSETS, with_values=True)
    assert [g.shape for g in got] == [(3, 2, 2), (3, 4, 4)] and values.shape == (3,)
    assert [c.name for c in device.calls] == ["operator_density_matrices"]
    layer.assert_guarded(device, layer.NON_DIAGONAL)


def test_the_evaluator_method_composes_behind_the_initial_state_per_call():
    device = RecordingDevice()
    ev = layer.operator_evaluator(device, initial=layer.INITIAL)
    circuits = layer.make_circuits()
    device.calls.clear()
    ev.operator_density_matrices(circuits, layer.VALUES, SUBSETS)
    (call,) = device.calls
    assert all(layer.same_circuit(got, layer.INITIAL.compose(c)) for got, c in zip(call.circuits, circuits))
    assert all(seen is not given for seen, given in zip(call.circuits, circuits))
    circuits[0].u(0.3, 0.2, 0.1, 2)  # the same object, one gate longer
    device.calls.clear()
    ev.operator_density_matrices(circuits, layer.VALUES, SUBSETS)
    assert all(layer.same_circuit(got, layer.INITIAL.compose(c)) for got, c in zip(device.calls[0].circuits, circuits))


def test_the_evaluator_method_drops_none_pairs():
    device = RecordingDevice()
    ev = layer.operator_evaluator(device)
    device.calls.clear()
    circuits = layer.make_circuits()
    got = ev.operator_density_matrices([circuits[0], None, circuits[2], circuits[1]], [layer.VALUES[0], [], None, layer.VALUES[1]], SUBSETS)
    (call,) = device.calls
    assert call.circuits == [circuits[0], circuits[1]] and call.parameter_values == [layer.VALUES[0], layer.VALUES[1]]
    assert got[0].shape == (2, 2, 2)
    with pytest.raises(ValueError):
        ev.operator_density_matrices(circuits, layer.VALUES[:2], SUBSETS)


class RecordingLibrary:
    """``qsv_operator_density_circuits`` that notes its subsets and fills the outputs with the call's number."""

    def __init__(self):
        self.calls = []

    def qsv_operator_density_circuits(self, handle, n_subsets, offsets, qubits, n_evals, ids, param_offsets, params, out, out_values):
        offsets = np.ctypeslib.as_array(C.cast(offsets, C.POINTER(C.c_int32)), shape=(n_subsets + 1,)).copy()
        qubits = np.ctypeslib.as_array(C.cast(qubits, C.POINTER(C.c_int32)), shape=(int(offsets[-1]),)).copy()
        subsets = [tuple(int(q) for q in qubits[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
        self.calls.append((n_evals, subsets, out_values is not None))
        count = n_evals * sum(2 * 4 ** len(s) for s in subsets)
        np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_double)), shape=(count,))[:] = float(len(self.calls))
        if out_values is not None:
            np.ctypeslib.as_array(C.cast(out_values, C.POINTER(C.c_double)), shape=(n_evals,))[:] = -float(len(self.calls))
        return _lib.QSV_OK


def _bare_device(n_qubits):
    dev = object.__new__(StatevectorDevice)  # no GPU here: the method's own work around the library call
    dev._lib, dev._handle, dev._n_qubits = RecordingLibrary(), 1, n_qubits
    dev._batch_arguments = lambda circuits, values: (np.zeros(len(circuits), np.int32), np.zeros(len(circuits) + 1, np.int64), np.zeros(1))
    return dev


def test_the_device_method_splits_1025_subsets_and_asks_for_values_once():
    dev = _bare_device(12)
    try:
        subsets = [((s * 5) % 12, (s * 5 + 1 + s % 7) % 12) if s % 3 else (s % 12,) for s in range(1025)]
        circuits = [CircuitIR(12).u(0.1, 0.2, 0.3, 0)] * 2
        got, values = dev.operator_density_matrices(circuits, [[], []], subsets, with_values=True)
        assert [(n, len(s), v) for n, s, v in dev._lib.calls] == [(2, 1024, True), (2, 1, False)]
        assert [g.shape for g in got] == [(2, 1 << len(s), 1 << len(s)) for s in subsets]
        assert all((g == 1.0 + 1.0j).all() for g in got[:1024]) and (got[1024] == 2.0 + 2.0j).all()
        assert values.tolist() == [-1.0, -1.0]
        plain = dev.operator_density_matrices(circuits, [[], []], subsets[:2])
        assert isinstance(plain, list) and dev._lib.calls[-1] == (2, subsets[:2], False)
    finally:
        dev._handle = None  # keep __del__ from calling qsv_destroy on the stand-in


def test_the_device_method_checks_before_it_calls():
    dev = _bare_device(3)
    try:
        circuit = CircuitIR(3).u(0.1, 0.2, 0.3, 0)
        for bad, word in [([], "at least one"), ([()], "1 to 4"), ([(0, 1, 2, 0, 1)], "1 to 4"), ([(0, 0)], "distinct"), ([(3,)], "distinct"),
                          ([(-1,)], "distinct")]:
            with pytest.raises(ValueError, match=word):
                dev.operator_density_matrices([circuit], [[]], bad)
        with pytest.raises(ValueError):
            dev.operator_density_matrices([circuit], [[], []], [(0,)])
        empty, values = dev.operator_density_matrices([], [], [(0,), (1, 2)], with_values=True)
        assert [e.shape for e in empty] == [(0, 2, 2), (0, 4, 4)] and values.shape == (0,) and dev._lib.calls == []
    finally:
        dev._handle = None


# ---- header, binding, docstring, build list ------------------------------------------------------------------------------------------


def test_header_binding_and_docstring_agree_on_the_prototype():
    text = re.sub(r"/\*.*?\*/", "", (helpers.ROOT / "include" / "qsv.h").read_text(), flags=re.S)
    match = re.search(r"int\s+qsv_operator_density_circuits\s*\((.*?)\)\s*;", text, flags=re.S)
    assert match, "include/qsv.h does not declare qsv_operator_density_circuits"
    arguments = [" ".join(a.split()) for a in match.group(1).split(",")]
    assert arguments == ["qsv_t* h", "int n_subsets", "const int32_t* subset_offsets", "const int32_t* subset_qubits", "int n_evals",
                         "const int* circuit_ids", "const int64_t* param_offsets", "const double* params", "double* out", "double* out_values"]
    restype, argtypes = _lib.SIGNATURES["qsv_operator_density_circuits"]
    assert restype is C.c_int and len(argtypes) == len(arguments)
    for kind, argument in zip(argtypes, arguments):
        assert (kind is C.c_int) == (argument.startswith("int ")), argument
    # the reduced density call's prototype and one more pointer
    rdm = re.search(r"int\s+qsv_reduced_density_circuits\s*\((.*?)\)\s*;", text, flags=re.S)
    assert [" ".join(a.split()) for a in rdm.group(1).split(",")] == arguments[:-1]
    assert "qsv_operator_density_circuits" in StatevectorDevice.operator_density_matrices.__doc__
    assert "operator_density.hip" in _build.SOURCES and "operator_density.hpp" in _build.HEADERS


# ---- the solver's option --------------------------------------------------------------------------------------------------------------


def _config(**overrides):
    args = dict(
        optimizer=SPSA(maxiter=8, learning_rate=0.4, perturbation=0.3), population_size=6, max_generations=4, random_seed=11,
        n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
        use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
        parameter_search_probability=0.3, topological_search_probability=0.6, layer_removal_probability=0.05,
    )
    args.update(overrides)
    return EVQEMinimumEigensolverConfiguration(**args)


STREAMS = ("_rng_last_layer", "_rng_speciation", "_rng_selection", "_rng_parameter_search", "_rng_topological", "_rng_layer_removal")


def _run(op, **overrides):
    generations = []
    solver = EVQEMinimumEigensolver(_config(**overrides), on_generation=lambda g: generations.append((g["population"].individuals, g["values"])))
    ev = NumpyEvaluator(op)
    return solver, ev, solver.compute_minimum_eigenvalue(ev), generations


def test_one_growth_candidate_is_the_solver_as_it_was():
    assert EVQEMinimumEigensolverConfiguration.__dataclass_fields__["growth_candidates"].default == 1
    op = odr.general_operator(4, seed=2)
    unset_solver, unset_ev, unset, unset_generations = _run(op)
    one_solver, one_ev, one, one_generations = _run(op, growth_candidates=1)
    assert one_generations == unset_generations and len(one_generations) == 4
    for name in ("eigenvalue", "best_individual", "generations", "circuit_evaluations", "best_expectation_values",
                 "median_expectation_values", "mean_expectation_values"):
        assert getattr(one, name) == getattr(unset, name), name
    for stream in STREAMS:
        assert getattr(one_solver, stream).getstate() == getattr(unset_solver, stream).getstate(), stream
    assert one_ev.density_calls == [] and unset_ev.density_calls == [] and one_ev.evaluations == unset_ev.evaluations
    with pytest.raises(ValueError):
        _config(growth_candidates=0)


def test_four_growth_candidates_keep_a_layer_no_worse_than_the_first():
    n = 4
    op = odr.general_operator(n, seed=2)
    solver = EVQEMinimumEigensolver(_config(growth_candidates=4, topological_search_probability=1.0))
    plain = EVQEMinimumEigensolver(_config(topological_search_probability=1.0))
    from queasars_amd.evqe.genome import EVQEPopulation

    population = EVQEPopulation.random_population(n, 2, 6, True, 3)
    ev = NumpyEvaluator(op)
    grown = solver._topological_search(population, ev)
    first = plain._topological_search(population)
    assert solver._rng_topological.getstate() == plain._rng_topological.getstate()  # (consumed exactly as before)
    assert ev.density_calls == [(6, rr.singles_and_pairs(n))] and ev.evaluations == 0  # one call for all chosen parents
    assert len(solver.last_growth_scores) == 6
    kept_another = 0
    for before, after, zero, (best, norms) in zip(population.individuals, grown.individuals, first.individuals, solver.last_growth_scores):
        assert len(after.layers) == len(before.layers) + 1 and after.layers[:-1] == before.layers and after.is_valid()
        assert after.parameter_values[: len(before.parameter_values)] == before.parameter_values
        assert not any(after.parameter_values[len(before.parameter_values):])
        assert len(norms) == 4 and norms[best] == max(norms) and best == norms.index(max(norms))  # (the lowest index wins a tie)
        assert norms[best] >= norms[0]
        # candidate 0 is the layer that is drawn without the option
        state = helpers.oracle_state(before.get_parameterized_quantum_circuit(), list(before.parameter_values))
        u, cu3 = odr.u_gradients(op, state), odr.cu3_gradients(op, state)
        assert abs(float(np.linalg.norm(growth.layer_gradient(zero.layers[-1], u, cu3))) - norms[0]) <= 1e-13
        assert abs(float(np.linalg.norm(growth.layer_gradient(after.layers[-1], u, cu3))) - norms[best]) <= 1e-13
        kept_another += best != 0
        if best == 0:
            assert after == zero
    assert kept_another > 0  # (the option changes something here)


def test_all_norms_zero_keep_candidate_zero_and_a_full_run_completes():
    n = 4
    # H = Z on every qubit and parents in |0..0>: every first-order gradient at identity vanishes
    op = PauliOperator.from_sparse_list([("Z", [q], 1.0) for q in range(n)], n)
    from queasars_amd.evqe.genome import EVQEPopulation

    population = EVQEPopulation.random_population(n, 1, 4, False, 5)
    solver = EVQEMinimumEigensolver(_config(growth_candidates=3, topological_search_probability=1.0))
    plain = EVQEMinimumEigensolver(_config(topological_search_probability=1.0))
    grown = solver._topological_search(population, NumpyEvaluator(op))
    assert all(best == 0 and not any(norms) for best, norms in solver.last_growth_scores)
    assert grown.individuals == plain._topological_search(population).individuals
    solver, ev, result, generations = _run(odr.general_operator(n, seed=2), growth_candidates=4)
    assert result.generations == 4 and len(ev.density_calls) >= 1 and all(i.is_valid() for g, _ in generations for i in g)
    assert sum(result.circuit_evaluations) == ev.evaluations  # (screening counts no circuit evaluation)


def test_the_solver_refuses_an_evaluator_without_the_method():
    class Bare:
        n_qubits = 3

        def evaluate_circuits(self, circuits, parameter_values):
            raise AssertionError("not reached")

    with pytest.raises(ValueError, match="operator_density_matrices"):
        EVQEMinimumEigensolver(_config(growth_candidates=2)).compute_minimum_eigenvalue(Bare())
    # the search itself says the same where it is called without an evaluator
    from queasars_amd.evqe.genome import EVQEPopulation

    solver = EVQEMinimumEigensolver(_config(growth_candidates=2))
    assert solver.last_growth_scores == [] and "last_growth_scores" not in vars(EVQEMinimumEigensolver)
    with pytest.raises(ValueError, match="operator_density_matrices"):
        solver._topological_search(EVQEPopulation.random_population(3, 1, 2, False, 1))
