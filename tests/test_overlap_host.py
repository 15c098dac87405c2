"""Overlaps and operator matrix elements between states, the parts that need no GPU: the two reference forms
against each other, the host's subspace diagonalisation, the Python layer's argument checks, the solver's option on an oracle
evaluator, and csrc/overlap.hpp's sizing as a stand-alone program under the address and undefined-behaviour sanitizers."""

import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import helpers
import overlap_reference as ovr
from dense_gradient import dense_operator
from queasars_amd import _build, _lib
from queasars_amd.circuit_evaluation import KeptState, OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe.solver import EVQEMinimumEigensolver, EVQEResult
from queasars_amd.evqe.subspace import lowest_subspace_eigenvalue
from queasars_amd.ir import CircuitIR
from queasars_amd.primitives import GpuStateFidelity
from test_observables_host import OracleEvaluator, _same_run, make_config


# ---- the references ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [3, 6, 8])
def test_dense_and_matrix_free_references_agree(n):
    _, _, states = ovr.population(n, 3, 5, 2)
    kept, evaluated = states[:3], states[1:]
    for op in (helpers.random_ising_operator(n, seed=2020), helpers.random_pauli_operator(n, 20, seed=1234)):
        dense = ovr.elements(op, kept, evaluated, dense=True)
        free = ovr.elements(op, kept, evaluated, dense=False)
        assert dense.shape == free.shape == (4, 3)
        assert ovr.max_component_error(dense, free) <= 1e-13 * max(1.0, ovr.spread(op))
    s = ovr.overlaps(kept, evaluated)
    assert abs(s[0, 1] - 1.0) <= 1e-13 and abs(s[1, 2] - 1.0) <= 1e-13  # (a state against itself)
    assert abs(s[1, 1] - np.conj(ovr.overlaps(states[2:3], states[1:2])[0, 0])) <= 1e-15  # S_ij = conj(S_ji)


def test_the_perturbed_population_has_overlaps_of_order_one():
    circuits, params, states = ovr.population(11, 3, 6, 4, True)
    assert len(circuits) == len(params) == len(states) == 6 and circuits[3] is circuits[0]
    s = ovr.overlaps(states[:3], states[3:])
    assert np.abs(np.diagonal(s)).min() > 0.5 and np.abs(np.diagonal(s)).max() < 1.0 - 1e-6


# ---- the subspace diagonalisation --------------------------------------------------------------------------------------


def _pencil(n_dim=32, k=5, seed=0, with_ground=True):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n_dim, n_dim)) + 1j * rng.normal(size=(n_dim, n_dim))
    h = (a + a.conj().T) / 2
    w, v = np.linalg.eigh(h)
    vectors = rng.normal(size=(n_dim, k)) + 1j * rng.normal(size=(n_dim, k))
    vectors /= np.linalg.norm(vectors, axis=0)
    if with_ground:
        vectors[:, 2] = v[:, 0] * np.exp(0.7j)
    return h, w, vectors


def _matrices(h, vectors):
    return vectors.conj().T @ vectors, vectors.conj().T @ h @ vectors


def test_the_exact_ground_energy_when_the_span_holds_the_ground_vector():
    h, w, vectors = _pencil()
    e, c, rank, s_min = lowest_subspace_eigenvalue(*_matrices(h, vectors), 1e-8)
    assert abs(e - w[0]) <= 1e-12 and rank == 5 and s_min > 1e-2
    s, _ = _matrices(h, vectors)
    assert abs(np.vdot(c, s @ c) - 1.0) <= 1e-12
    combined = vectors @ c
    assert abs(abs(np.vdot(combined, np.linalg.eigh(h)[1][:, 0])) - 1.0) <= 1e-10


def test_the_bound_is_between_the_ground_energy_and_the_best_state():
    h, w, vectors = _pencil(with_ground=False)
    s, hm = _matrices(h, vectors)
    e, _, rank, _ = lowest_subspace_eigenvalue(s, hm, 1e-8)
    assert rank == 5 and w[0] - 1e-12 <= e <= float(np.min(np.real(np.diagonal(hm)))) + 1e-12


def test_a_duplicated_state_is_dropped():
    h, w, vectors = _pencil(with_ground=False)
    e, _, rank, _ = lowest_subspace_eigenvalue(*_matrices(h, vectors), 1e-8)
    doubled = np.concatenate([vectors, vectors[:, 1:2]], axis=1)
    e2, c2, rank2, s_min2 = lowest_subspace_eigenvalue(*_matrices(h, doubled), 1e-8)
    assert rank == 5 and rank2 == 5 and c2.shape == (6,) and abs(e2 - e) <= 1e-12 and s_min2 > 1e-2


def test_the_eigenvalue_does_not_depend_on_the_order_of_the_states():
    h, _, vectors = _pencil(k=7, seed=3, with_ground=False)
    e, c, rank, s_min = lowest_subspace_eigenvalue(*_matrices(h, vectors), 1e-8)
    order = np.random.default_rng(1).permutation(7)
    e2, c2, rank2, s_min2 = lowest_subspace_eigenvalue(*_matrices(h, vectors[:, order]), 1e-8)
    assert abs(e2 - e) <= 1e-12 and rank2 == rank and abs(s_min2 - s_min) <= 1e-12
    assert abs(abs(np.vdot(vectors @ c, vectors[:, order] @ c2)) - 1.0) <= 1e-10


def test_raw_matrices_are_hermitised_and_bad_ones_refused():
    h, _, vectors = _pencil()
    s, hm = _matrices(h, vectors)
    noise = 1e-13 * np.random.default_rng(5).normal(size=s.shape)
    assert abs(lowest_subspace_eigenvalue(s + noise, hm - noise, 1e-8)[0] - lowest_subspace_eigenvalue(s, hm, 1e-8)[0]) <= 1e-10
    with pytest.raises(ValueError, match="square"):
        lowest_subspace_eigenvalue(s[:, :3], hm[:, :3], 1e-8)
    with pytest.raises(ValueError, match="rcond"):
        lowest_subspace_eigenvalue(s, hm, 0.0)
    with pytest.raises(ValueError, match="positive eigenvalue"):
        lowest_subspace_eigenvalue(np.zeros((2, 2)), np.zeros((2, 2)), 1e-8)


# ---- the entry point and the Python layer ------------------------------------------------------------------------------------


def test_the_entry_point_is_declared_and_bound():
    header = (helpers.ROOT / "include" / "qsv.h").read_text()
    assert re.search(r"\bint qsv_overlap_circuits\(", header)
    assert re.search(r"#define QSV_OVERLAP_MAX_STATES 64\b", header)
    assert "qsv_overlap_circuits" in _lib.SIGNATURES and len(_lib.SIGNATURES["qsv_overlap_circuits"][1]) == 10
    assert StatevectorDevice.MAX_OVERLAP_STATES == 64
    assert "overlap.hip" in _build.SOURCES and "overlap.hpp" in _build.HEADERS


def _fake_device(serial=1):
    dev = object.__new__(StatevectorDevice)  # (no handle: every check below comes before the library is called)
    dev._n_qubits = 3
    dev._serial = serial
    dev._dead_states = []
    return dev


def test_the_device_checks_its_arguments_before_it_calls_the_library():
    dev, other = _fake_device(1), _fake_device(2)
    circuit = CircuitIR(3).u(0.1, 0.2, 0.3, 0)
    mine, foreign, released = KeptState(dev, 4), KeptState(other, 4), KeptState(dev, 5)
    released.release()
    with pytest.raises(ValueError, match="same length"):
        dev.overlaps([circuit], [], [mine])
    with pytest.raises(ValueError, match="at least one kept state"):
        dev.overlaps([circuit], [[]], [])
    with pytest.raises(ValueError, match="KeptState"):
        dev.overlaps([circuit], [[]], [7])
    with pytest.raises(ValueError, match="not kept on this device"):
        dev.overlaps([circuit], [[]], [mine, foreign])
    with pytest.raises(ValueError, match="released"):
        dev.overlaps([circuit], [[]], [released])
    with pytest.raises(ValueError, match="continues a kept state"):
        dev.overlaps([CircuitIR(3).u(0.1, 0.0, 0.0, 1).continue_from(mine)], [[]], [mine])
    s, t = dev.overlaps([], [], [mine, mine], with_operator=True)  # (nothing to evaluate: no call)
    assert s.shape == t.shape == (0, 2) and s.dtype == t.dtype == np.complex128
    assert dev.overlaps([], [], [mine]).shape == (0, 1)


def test_the_evaluator_and_the_fidelity_check_their_arguments_before_a_device():
    evaluator = object.__new__(OperatorCircuitEvaluator)
    circuit = CircuitIR(3).u(0.1, 0.2, 0.3, 0)
    with pytest.raises(ValueError, match="same length"):
        evaluator.evaluate_overlaps([circuit], [], [])
    with pytest.raises(ValueError, match="same length"):
        evaluator.evaluate_subspace_matrices([circuit], [])
    fidelity = GpuStateFidelity()
    with pytest.raises(ValueError, match="second circuits"):
        fidelity.run([circuit, circuit], [circuit], [[], []], [[]])
    with pytest.raises(ValueError, match="parameter vectors"):
        fidelity.run([circuit, circuit], [circuit, circuit], [[]], [[], []])
    with pytest.raises(ValueError, match="parameters"):
        fidelity.run([circuit], [circuit], [[0.5]], [[]])
    with pytest.raises(ValueError, match="different sizes"):
        fidelity.run([circuit], [CircuitIR(4).u(0.1, 0.2, 0.3, 0)], [[]], [[]])
    assert fidelity.run([], [], [], []).result().fidelities == []


# ---- the solver -------------------------------------------------------------------------------------------------------------


class OracleSubspaceEvaluator(OracleEvaluator):
    def __init__(self, operator):
        super().__init__(operator)
        self.subspace_calls = []

    def evaluate_subspace_matrices(self, circuits, parameter_values):
        self.subspace_calls.append((list(circuits), [list(p) for p in parameter_values]))
        states = [helpers.oracle_state(c, p) for c, p in zip(circuits, parameter_values)]
        return ovr.overlaps(states, states).T.copy(), ovr.elements(self.operator, states, states).T.copy()


def _ising(n=4):
    return helpers.random_pauli_operator(n, 12, seed=77)


def test_the_result_has_no_subspace_fields_unless_asked_for():
    result = EVQEResult(eigenvalue=0.0, best_individual=object(), generations=0, circuit_evaluations=[])
    assert result.subspace_eigenvalue is None and result.subspace_coefficients is None
    assert result.subspace_rank is None and result.subspace_overlaps is None


def test_subspace_states_needs_an_evaluator_that_has_it_and_a_sane_count():
    solver = EVQEMinimumEigensolver(make_config())
    with pytest.raises(ValueError, match="evaluate_subspace_matrices"):
        solver.compute_minimum_eigenvalue(OracleEvaluator(_ising()), subspace_states=4)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="between 1 and 64"):
            solver.compute_minimum_eigenvalue(OracleSubspaceEvaluator(_ising()), subspace_states=bad)
    with pytest.raises(ValueError, match="subspace_rcond"):
        solver.compute_minimum_eigenvalue(OracleSubspaceEvaluator(_ising()), subspace_rcond=1e-6)
    with pytest.raises(ValueError, match="subspace_rcond"):
        solver.compute_minimum_eigenvalue(OracleSubspaceEvaluator(_ising()), subspace_states=4, subspace_rcond=-1.0)


def test_the_subspace_refinement_is_one_call_after_the_run_and_leaves_the_run_unchanged():
    op = _ising()
    plain = EVQEMinimumEigensolver(make_config()).compute_minimum_eigenvalue(OracleSubspaceEvaluator(op))
    evaluator = OracleSubspaceEvaluator(op)
    seen = []
    solver = EVQEMinimumEigensolver(make_config(), on_generation=lambda info: seen.append((info["population"], info["values"])))
    asked = solver.compute_minimum_eigenvalue(evaluator, subspace_states=4)
    _same_run(plain, asked)
    assert plain.subspace_eigenvalue is None and len(evaluator.subspace_calls) == 1
    circuits, values = evaluator.subspace_calls[0]
    # the picks: the best individual, then the last scored generation in ascending value, repeats skipped
    population, scores = seen[-1]
    best = asked.best_individual
    wanted, keys = [], set()
    for ind in [best] + [population.individuals[i] for i in sorted(range(len(scores)), key=lambda i: (scores[i], i))]:
        key = (ind.layers, tuple(ind.parameter_values))
        if key not in keys:
            keys.add(key)
            wanted.append(ind)
    wanted = wanted[:4]
    assert values == [list(ind.parameter_values) for ind in wanted] and len(circuits) == len(wanted)
    assert values[0] == list(best.parameter_values)
    k = len(wanted)
    assert asked.subspace_overlaps.shape == (k, k) and asked.subspace_coefficients.shape == (k,)
    assert 1 <= asked.subspace_rank <= k
    exact_ground = float(np.linalg.eigvalsh(dense_operator(op))[0])
    assert exact_ground - 1e-9 <= asked.subspace_eigenvalue <= asked.eigenvalue + 1e-9
    states = [helpers.oracle_state(c, p) for c, p in zip(circuits, values)]
    combined = sum(c * s for c, s in zip(asked.subspace_coefficients, states))
    assert abs(np.vdot(combined, combined) - 1.0) <= 1e-9
    assert abs(np.vdot(combined, dense_operator(op) @ combined).real - asked.subspace_eigenvalue) <= 1e-9


# ---- the sizes, under the sanitizers ---------------------------------------------------------------------------------------


def test_the_sizing_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/overlap.hpp's overlap_blocks, launch group and scratch sizes as host code in a program of its own
    (tests/native/overlap_sizes_main.cpp): n = 1 .. 28, K = 1 .. 64, group limits 1 .. 256, with and without the operator."""
    # (g++ or clang++ where there is one, else the clang the project is built with: never skipped for want of a compiler)
    compiler = shutil.which("g++") or shutil.which("clang++") or _build._hipcc()
    hip_include = Path(_build._hipcc()).resolve().parent.parent / "include"
    program = tmp_path / "overlap_sizes"
    build = subprocess.run(
        [compiler, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
         f"-I{hip_include}", f"-I{_build.CSRC}", str(helpers.ROOT / "tests" / "native" / "overlap_sizes_main.cpp"), "-o", str(program)],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([str(program)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert re.search(r"^917504 cases, 0 failures$", run.stdout, flags=re.M), run.stdout
