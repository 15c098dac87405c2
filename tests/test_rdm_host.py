"""Reduced density matrices without a device: tests/rdm_reference.py and queasars_amd/entanglement.py held to
facts, csrc/reduced_density.hpp's subset table held to the reference's index convention, and the Python layer on recording
stand-ins (tests/test_evaluator_layer_host.py's device, a library that writes nothing)."""

from __future__ import annotations

import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import helpers
import rdm_reference as rr
import test_evaluator_layer_host as layer
from queasars_amd import _build, _lib, entanglement as ent
from queasars_amd.circuit_evaluation.circuit_evaluation import StatevectorDevice
from queasars_amd.ir import CircuitIR

PI = np.pi
H = (PI / 2, 0.0, PI)
X = (PI, 0.0, PI)
Z2 = np.diag([1.0, -1.0])


def _states(n, count=3, seed=5):
    return rr.population(n, 3, count, seed)[2]


def _bell(n):
    """(|0..0> + |1 0..0 1>) / sqrt 2: a Bell pair between qubit 0 and qubit n - 1, the rest in |0>."""
    return helpers.oracle_state(CircuitIR(n).u(*H, 0).cu3(*X, 0, n - 1), [])


def _product(n, seed=3):
    rng = np.random.default_rng(seed)
    circuit = CircuitIR(n)
    for q in range(n):
        circuit.u(*rng.uniform(0.2, 2.8, size=3), q)
    return helpers.oracle_state(circuit, [])


# ---- the reference and entanglement.py --------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 2, 5, 7])
def test_reference_matrices_are_density_matrices(n):
    for state in _states(n):
        for subset in rr.subsets_for(n):
            rho = rr.reduced_density_matrix(state, subset)
            assert rho.shape == (1 << len(subset),) * 2
            assert abs(np.trace(rho) - 1.0) <= 1e-13
            assert np.abs(rho - rho.conj().T).max() <= 1e-15
            assert np.linalg.eigvalsh(rho).min() >= -1e-14


def test_the_whole_register_gives_the_projector():
    for n in (1, 3, 4):
        state = _states(n)[0]
        assert np.abs(rr.reduced_density_matrix(state, tuple(range(n))) - np.outer(state, state.conj())).max() <= 1e-15


def test_a_pair_traced_over_one_qubit_is_the_other_qubits_matrix():
    n = 6
    for state in _states(n):
        for i, j in [(0, 5), (3, 1), (4, 5)]:
            pair = rr.reduced_density_matrix(state, (i, j)).reshape(2, 2, 2, 2)  # [j, i, j', i']
            assert np.abs(np.einsum("jajb->ab", pair) - rr.reduced_density_matrix(state, (i,))).max() <= 1e-14
            assert np.abs(np.einsum("ajbj->ab", pair) - rr.reduced_density_matrix(state, (j,))).max() <= 1e-14


def test_product_states_are_pure_on_every_subset():
    n = 6
    for state in (np.eye(1, 1 << n).ravel().astype(complex), _product(n)):
        for subset in rr.subsets_for(n):
            rho = rr.reduced_density_matrix(state, subset)
            assert abs(np.trace(rho @ rho).real - 1.0) <= 1e-13
            assert abs(ent.von_neumann_entropy(rho)) <= 1e-12


@pytest.mark.parametrize("n", [2, 5, 8])
def test_a_bell_pair_between_the_first_and_the_last_qubit(n):
    state = _bell(n)
    for q in (0, n - 1):
        assert abs(ent.von_neumann_entropy(rr.reduced_density_matrix(state, (q,))) - 1.0) <= 1e-12
    pair = rr.reduced_density_matrix(state, (0, n - 1))
    information = 2.0 - ent.von_neumann_entropy(pair)
    assert abs(information - 2.0) <= 1e-12
    assert ent.marginal_distribution(pair) == pytest.approx([0.5, 0.0, 0.0, 0.5], abs=1e-14)
    assert abs(ent.von_neumann_entropy(rr.reduced_density_matrix(state, (0,)), base=np.e) - np.log(2)) <= 1e-12


def test_permuting_a_subset_permutes_rows_and_columns():
    n = 6
    state = _states(n)[1]
    subset, order = (1, 4, 5), (2, 0, 1)  # the permuted subset's j-th qubit is subset[order[j]]
    base = rr.reduced_density_matrix(state, subset)
    permuted = rr.reduced_density_matrix(state, tuple(subset[o] for o in order))
    index = np.arange(8)
    source = np.zeros_like(index)
    for j, o in enumerate(order):
        source |= ((index >> j) & 1) << o
    assert np.abs(permuted - base[np.ix_(source, source)]).max() <= 1e-15
    assert np.abs(permuted - base).max() > 1e-3  # (the permutation is seen)


def test_local_expectation_of_zz_is_the_oracles():
    from oracle import statevector_oracle as so

    n = 6
    for state in _states(n):
        for i, j in [(0, 5), (4, 2)]:
            want = so.pauli_expectation(state, [0], [(1 << i) | (1 << j)], [1.0]).real
            got = ent.local_expectation(rr.reduced_density_matrix(state, (i, j)), np.kron(Z2, Z2))
            assert abs(got - want) <= 1e-13
            # Z on the subset's first qubit alone: kron(identity on the second, Z on the first)
            want = so.pauli_expectation(state, [0], [1 << i], [1.0]).real
            assert abs(ent.local_expectation(rr.reduced_density_matrix(state, (i, j)), np.kron(np.eye(2), Z2)) - want) <= 1e-13


def test_entropy_takes_a_raw_matrix_and_refuses_what_is_none():
    rho = rr.reduced_density_matrix(_states(5)[0], (0, 3))
    assert abs(ent.von_neumann_entropy(3.0 * rho) - ent.von_neumann_entropy(rho)) <= 1e-12
    assert ent.von_neumann_entropy(np.diag([1.0, 0.0])) == 0.0  # (0 log 0 = 0)
    assert abs(ent.von_neumann_entropy(np.eye(4) / 4) - 2.0) <= 1e-14
    with pytest.raises(ValueError):
        ent.von_neumann_entropy(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        ent.von_neumann_entropy(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        ent.local_expectation(np.eye(2), np.eye(4))


def test_kron_reordered_is_the_matrix_of_a_product_state():
    n = 6
    a, b = _states(3, seed=1)[0], _states(3, seed=2)[1]  # blocks on qubits (0, 2, 4) and (1, 3, 5)
    state = np.zeros(1 << n, dtype=complex)
    for i in range(1 << n):
        ia = (i & 1) | ((i >> 2) & 1) << 1 | ((i >> 4) & 1) << 2
        ib = ((i >> 1) & 1) | ((i >> 3) & 1) << 1 | ((i >> 5) & 1) << 2
        state[i] = a[ia] * b[ib]
    subset = (3, 0, 4, 1)
    factors = [(rr.reduced_density_matrix(a, (0, 2)), [0, 4]), (rr.reduced_density_matrix(b, (0, 1)), [1, 3])]
    assert np.abs(rr.kron_reordered(factors, subset) - rr.reduced_density_matrix(state, subset)).max() <= 1e-15


# ---- entanglement.py's batch functions on an evaluator that answers from oracle states ---------------------------------------


class OracleEvaluator:
    """``reduced_density_matrices`` from the NumPy oracle; counts its calls."""

    def __init__(self, n):
        self.n_qubits, self.calls = n, []

    def reduced_density_matrices(self, circuits, parameter_values, subsets):
        self.calls.append(list(subsets))
        return rr.reduced_density_matrices([helpers.oracle_state(c, p) for c, p in zip(circuits, parameter_values)], subsets)


def test_mutual_information_comes_from_one_call_over_singles_and_pairs():
    n = 5
    circuits, params, states = rr.population(n, 3, 2, 4)
    circuits, params = list(circuits) + [CircuitIR(n).u(*H, 0).cu3(*X, 0, n - 1)], [list(p) for p in params] + [[]]
    ev = OracleEvaluator(n)
    information = ent.mutual_information(ev, circuits, params)
    assert len(ev.calls) == 1 and ev.calls[0] == rr.singles_and_pairs(n)
    assert information.shape == (3, n, n)
    assert np.array_equal(information, information.transpose(0, 2, 1)) and not information[:, np.arange(n), np.arange(n)].any()
    bell = np.zeros((n, n))
    bell[0, n - 1] = bell[n - 1, 0] = 2.0
    assert np.abs(information[2] - bell).max() <= 1e-12
    entropies = ent.qubit_entropies(ev, circuits, params)
    assert entropies.shape == (3, n) and entropies[2] == pytest.approx([1.0, 0, 0, 0, 1.0], abs=1e-12)
    for e, state in enumerate(states):
        s_01 = ent.von_neumann_entropy(rr.reduced_density_matrix(state, (0, 1)))
        assert abs(information[e, 0, 1] - (entropies[e, 0] + entropies[e, 1] - s_01)) <= 1e-13
        assert information[e].min() >= -1e-12  # (subadditivity)
    both = ent.mutual_information(ev, circuits, params, with_entropies=True)
    assert np.array_equal(both[0], entropies) and np.array_equal(both[1], information)


def test_marginal_distributions_spell_the_first_qubit_last():
    n = 4
    circuit = CircuitIR(n).u(*X, 1).u(*H, 3)  # qubit 1 is |1>, qubit 3 is |+>
    got = ent.marginal_distributions(OracleEvaluator(n), [circuit], [[]], [(1, 0), (3, 1, 2)])
    assert len(got) == 1 and len(got[0]) == 2
    assert got[0][0] == pytest.approx({"00": 0.0, "01": 1.0, "10": 0.0, "11": 0.0}, abs=1e-14)  # (qubit 1, the first, last)
    want = {format(a, "03b"): 0.0 for a in range(8)}
    want["010"] = want["011"] = 0.5  # bits (qubit 2, qubit 1, qubit 3): qubit 1 set, qubit 3 either
    assert got[0][1] == pytest.approx(want, abs=1e-14)


# ---- the subset table the kernels read (csrc/reduced_density.hpp), as a host program ------------------------------------------


def test_the_subset_table_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/reduced_density.hpp's subset table, workgroup count and scratch sizes as host code in a program of its own
    (tests/native/rdm_table_main.cpp): the kernel's walk with the table's numbers reads inside the state, reads every amplitude
    once and puts it at the row of the subset's bits, n = 1 .. 28."""
    compiler = shutil.which("g++") or shutil.which("clang++") or _build._hipcc()
    hip_include = Path(_build._hipcc()).resolve().parent.parent / "include"
    program = tmp_path / "rdm_table"
    build = subprocess.run(
        [compiler, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
         f"-I{hip_include}", f"-I{_build.CSRC}", str(helpers.ROOT / "tests" / "native" / "rdm_table_main.cpp"), "-o", str(program)],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([str(program)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert re.search(r"^\d+ cases, 0 failures$", run.stdout, flags=re.M), run.stdout


def test_the_sources_are_in_the_build():
    assert "reduced_density.hip" in _build.SOURCES and "reduced_density.hpp" in _build.HEADERS


def test_the_c_abi_declares_the_call():
    restype, argtypes = _lib.SIGNATURES["qsv_reduced_density_circuits"]
    assert restype is C.c_int and len(argtypes) == 9


# ---- the Python layer on recording stand-ins ------------------------------------------------------------------------------------


class RecordingDevice(layer.RecordingDevice):
    def reduced_density_matrices(self, circuits, parameter_values, subsets):
        n = self._note("reduced_density_matrices", circuits)
        self.calls[-1].parameter_values = list(parameter_values)
        return [np.zeros((n, 1 << len(s), 1 << len(s)), dtype=complex) for s in subsets]


SUBSETS = [(0,), (2, 0)]


def test_the_evaluator_method_composes_behind_the_initial_state():
    device = RecordingDevice()
    ev = layer.operator_evaluator(device, initial=layer.INITIAL)
    device.calls.clear()
    circuits = layer.make_circuits()
    got = ev.reduced_density_matrices(circuits, layer.VALUES, SUBSETS)
    assert [g.shape for g in got] == [(3, 2, 2), (3, 4, 4)]
    (call,) = device.calls
    assert call.name == "reduced_density_matrices"
    assert [len(c) for c in call.circuits] == [len(layer.INITIAL) + len(c) for c in circuits]
    assert all(seen is not given for seen, given in zip(call.circuits, circuits))


def test_the_evaluator_method_leaves_another_evaluators_operator_installed():
    device = RecordingDevice()
    ev = layer.operator_evaluator(device)
    layer.leave_another_operator(device)
    ev.reduced_density_matrices(layer.make_circuits(), layer.VALUES, SUBSETS)
    assert device.installed == [] and device._operator is layer.OTHER
    assert [c.name for c in device.calls] == ["reduced_density_matrices"] and not device.operator_lock.held()


def test_the_evaluator_method_drops_none_pairs():
    device = RecordingDevice()
    ev = layer.operator_evaluator(device)
    device.calls.clear()
    circuits = layer.make_circuits()
    got = ev.reduced_density_matrices([circuits[0], None, circuits[2], circuits[1]], [layer.VALUES[0], [], None, layer.VALUES[1]], SUBSETS)
    (call,) = device.calls
    assert call.circuits == [circuits[0], circuits[1]] and call.parameter_values == [layer.VALUES[0], layer.VALUES[1]]
    assert got[0].shape == (2, 2, 2)
    with pytest.raises(ValueError):
        ev.reduced_density_matrices(circuits, layer.VALUES[:2], SUBSETS)


class RecordingLibrary:
    """``qsv_reduced_density_circuits`` that notes its subsets and fills the output with the call's number."""

    def __init__(self):
        self.calls = []

    def qsv_reduced_density_circuits(self, handle, n_subsets, offsets, qubits, n_evals, ids, param_offsets, params, out):
        offsets = np.ctypeslib.as_array(C.cast(offsets, C.POINTER(C.c_int32)), shape=(n_subsets + 1,)).copy()
        qubits = np.ctypeslib.as_array(C.cast(qubits, C.POINTER(C.c_int32)), shape=(int(offsets[-1]),)).copy()
        subsets = [tuple(int(q) for q in qubits[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
        self.calls.append((n_evals, subsets))
        count = n_evals * sum(2 * 4 ** len(s) for s in subsets)
        np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_double)), shape=(count,))[:] = float(len(self.calls))
        return _lib.QSV_OK


def _bare_device(n_qubits):
    dev = object.__new__(StatevectorDevice)  # no GPU here: the method's own work around the library call
    dev._lib, dev._handle, dev._n_qubits = RecordingLibrary(), 1, n_qubits
    dev._batch_arguments = lambda circuits, values: (np.zeros(len(circuits), np.int32), np.zeros(len(circuits) + 1, np.int64), np.zeros(1))
    return dev


def test_the_device_method_splits_1025_subsets_into_two_calls():
    dev = _bare_device(12)
    try:
        subsets = [((s * 5) % 12, (s * 5 + 1 + s % 7) % 12) if s % 3 else (s % 12,) for s in range(1025)]
        assert all(len(set(s)) == len(s) for s in subsets)
        circuits = [CircuitIR(12).u(0.1, 0.2, 0.3, 0)] * 2
        got = dev.reduced_density_matrices(circuits, [[], []], subsets)
        assert [(n, len(s)) for n, s in dev._lib.calls] == [(2, 1024), (2, 1)]
        assert dev._lib.calls[0][1] == subsets[:1024] and dev._lib.calls[1][1] == subsets[1024:]
        assert [g.shape for g in got] == [(2, 1 << len(s), 1 << len(s)) for s in subsets]
        assert all((g == 1.0 + 1.0j).all() for g in got[:1024]) and (got[1024] == 2.0 + 2.0j).all()
    finally:
        dev._handle = None  # keep __del__ from calling qsv_destroy on the stand-in


def test_the_device_method_checks_before_it_calls():
    dev = _bare_device(3)
    try:
        circuit = CircuitIR(3).u(0.1, 0.2, 0.3, 0)
        for bad, word in [([], "at least one"), ([()], "1 to 4"), ([(0, 1, 2, 0, 1)], "1 to 4"), ([(0, 0)], "distinct"), ([(3,)], "distinct"),
                          ([(-1,)], "distinct")]:
            with pytest.raises(ValueError, match=word):
                dev.reduced_density_matrices([circuit], [[]], bad)
        with pytest.raises(ValueError):
            dev.reduced_density_matrices([circuit], [[], []], [(0,)])
        empty = dev.reduced_density_matrices([], [], [(0,), (1, 2)])
        assert [e.shape for e in empty] == [(0, 2, 2), (0, 4, 4)] and dev._lib.calls == []
    finally:
        dev._handle = None


# ---- the solver's option ------------------------------------------------------------------------------------------------------


def test_the_solver_refuses_an_evaluator_without_the_method():
    from queasars_amd.evqe.solver import EVQEMinimumEigensolver, EVQEResult

    assert EVQEResult.__dataclass_fields__["qubit_entropies"].default is None
    assert EVQEResult.__dataclass_fields__["mutual_information"].default is None

    class Bare:
        n_qubits = 3

    solver = EVQEMinimumEigensolver.__new__(EVQEMinimumEigensolver)
    solver.configuration = None
    with pytest.raises(ValueError, match="reduced_density_matrices"):
        solver.compute_minimum_eigenvalue(Bare(), qubit_correlations=True)
