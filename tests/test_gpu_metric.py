"""The Fubini-Study metric on the device (``qsv_metric_circuits``) against tests/metric_reference.py.

Registers: below the tile's low bits (n = 1, 3), inside one tile (6), one exact tile (11), two tiles (12), several (13) and, at
n = 17, 64 tiles per state with ``wrt`` = the last layer.  Circuits: EVQE populations of two and three layers, ``generic`` with
shared and literal angles and ``id``, ``ladder``, ``star`` (whose controls leave the tile from n = 12 on) and ``two_blocks``.
Column counts 1, 15, 16, 17, 33 and more than 64 through ``wrt``: one block of the Gram matrix exactly full with i psi (15),
psi alone in a second block (16), two and three blocks, five and more.

Tolerances (the issue's): fp64 |G - ref| <= 1e-10 max(1, s_i s_j), s the number of slots that read a parameter; fp32
max(2e-6, 8 e_s) s_i s_j against the fp64 reference, e_s the fp32 handle's own largest |psi_32 - psi_ref|_2 over the test's
circuits.  What an MI355X gave is in DESIGN.md 4.17."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import circuit_families as cf
import helpers
import metric_reference as mr
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.ir import CircuitIR, ParamRef

pytestmark = pytest.mark.gpu

TOL64 = 1e-10


@functools.lru_cache(maxsize=None)
def family_circuits(n: int):
    """(name, circuit, values) of every family the register takes; built once."""
    out = []
    if n >= 2:
        for layers in (2, 3):
            _, circuits, params = helpers.population_circuits(n, layers, 2, seed=10 * n + layers)
            out += [(f"evqe {layers} layers #{i}", c, list(p)) for i, (c, p) in enumerate(zip(circuits, params))]
        out.append(("generic", *cf.generic(n, 4 * n + 12, share=0.3, literal=0.2, seed=n)))
        out.append(("star", *cf.star(n, seed=n)))
    out.append(("ladder", *cf.ladder(n, seed=n)))
    if n >= 4:
        out.append(("two_blocks", *cf.two_blocks(n, 2, seed=n)))
    return tuple((name, c, list(v[:c.num_parameters])) for name, c, v in out)


@functools.lru_cache(maxsize=None)
def reference(n: int):
    """The full metric of every circuit of ``family_circuits(n)``, computed once and never written to."""
    out = tuple(mr.backward(c, v) for _, c, v in family_circuits(n))
    for m in out:
        m.setflags(write=False)
    return out


def allowed(circuit, wrt=None, unit=TOL64):
    s = mr.slot_counts(circuit).astype(np.float64)
    s = s if wrt is None else s[np.asarray(wrt, dtype=np.int64)]
    return unit * np.maximum(1.0, np.outer(s, s))


def check(name, got, want, tol):
    assert got.shape == want.shape and got.dtype == np.float64, (name, got.shape, want.shape)
    err = np.abs(got - want)
    worst = float((err / tol).max()) if err.size else 0.0
    print(f"{name}: largest |G - ref| {float(err.max()) if err.size else 0.0:.3e}, {worst:.3f} of what is allowed")
    assert worst <= 1.0, (name, float(err.max()), worst)
    return float(err.max()) if err.size else 0.0


def assert_symmetric_to_the_bit(matrices):
    for m in matrices:
        assert np.array_equal(m, m.T)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 3, 6, 11, 12, 13])
def test_fp64_metrics_are_the_reference(n):
    cases = family_circuits(n)
    dev = StatevectorDevice(n)
    got = dev.metric_tensors([c for _, c, _ in cases], [v for _, _, v in cases])
    assert_symmetric_to_the_bit(got)
    for (name, circuit, _), g, want in zip(cases, got, reference(n)):
        check(f"n={n} {name} ({circuit.num_parameters} parameters)", g, want, allowed(circuit))
        assert np.linalg.eigvalsh(g).min() >= -TOL64 * max(1, circuit.num_parameters) * float(mr.slot_counts(circuit).max(initial=1)) ** 2
    stats = dev.metric_stats()
    assert stats["n_columns"] == sum(int(mr.slot_counts(c).sum()) for _, c, _ in cases)
    assert stats["n_run_launches"] >= 1 and stats["n_gram_launches"] >= 1 and stats["scratch_bytes"] > 0


@pytest.mark.parametrize("n", [6, 11])
def test_fp32_handles(n):
    cases = family_circuits(n)
    circuits, values = [c for _, c, _ in cases], [v for _, _, v in cases]
    dev = StatevectorDevice(n, dtype="fp32")
    e_s = max(float(np.linalg.norm(dev.statevector(c, v) - helpers.oracle_state(c, v))) for c, v in zip(circuits, values))
    unit = max(2e-6, 8.0 * e_s)
    print(f"n={n} fp32: e_s = {e_s:.3e}, allowed per slot pair {unit:.3e}")
    got = dev.metric_tensors(circuits, values)
    assert_symmetric_to_the_bit(got)
    for (name, circuit, _), g, want in zip(cases, got, reference(n)):
        check(f"fp32 n={n} {name}", g, want, allowed(circuit, unit=unit))


def test_seventeen_qubits_by_the_last_layer():
    n = 17
    pop, circuits, params = helpers.population_circuits(n, 3, 2, seed=173)
    wrt = [list(range(c.num_parameters - ind.layers[-1].n_parameters, c.num_parameters)) for c, ind in zip(circuits, pop.individuals)]
    ladder, ladder_values = cf.ladder(n, seed=17)
    circuits, params = list(circuits) + [ladder], [list(p) for p in params] + [ladder_values]
    wrt.append(list(range(ladder.num_parameters - 9, ladder.num_parameters)))  # (the last three u gates)
    assert all(len(w) > 0 for w in wrt)
    dev = StatevectorDevice(n)
    got = dev.metric_tensors(circuits, params, wrt)
    assert_symmetric_to_the_bit(got)
    for e, (c, p, w, g) in enumerate(zip(circuits, params, wrt, got)):
        check(f"n=17 circuit {e}, {len(w)} parameters", g, mr.backward(c, p, w), allowed(c, w))


# ---- 2. column counts -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [6, 12])
def test_column_counts_through_wrt(n):
    """ladder: every parameter is read by one slot, so a wrt of k parameters carries k columns."""
    index = [name for name, _, _ in family_circuits(n)].index("ladder")
    _, circuit, values = family_circuits(n)[index]
    full = reference(n)[index]
    assert circuit.num_parameters > 64 and mr.slot_counts(circuit).max() == 1
    dev = StatevectorDevice(n)
    whole = dev.metric_tensors([circuit], [values])[0]
    rng = np.random.default_rng(n)
    for count in (1, 15, 16, 17, 33, 70):
        wrt = [int(p) for p in rng.choice(circuit.num_parameters, size=count, replace=False)]
        got = dev.metric_tensors([circuit], [values], wrt)[0]
        assert dev.metric_stats()["n_columns"] == count
        check(f"n={n}, {count} columns", got, full[np.ix_(wrt, wrt)], allowed(circuit, wrt))
        assert np.array_equal(got, whole[np.ix_(wrt, wrt)])  # (bit for bit the submatrix)
    # all of them in one batch, a wrt per circuit
    lists = [[int(p) for p in rng.choice(circuit.num_parameters, size=count, replace=False)] for count in (17, 1, 70, 16, 0)]
    got = dev.metric_tensors([circuit] * 5, [values] * 5, lists)
    assert got[4].shape == (0, 0)
    for wrt, g in zip(lists, got):
        assert np.array_equal(g, whole[np.ix_(wrt, wrt)])


# ---- 3. launch groups and the scratch bound ---------------------------------------------------------------------------------------


def test_a_second_launch_group_and_the_refusal_when_one_evaluation_does_not_fit():
    n = 12  # a state is 64 KiB in fp64: 1 MiB holds sixteen
    cases = family_circuits(n)[:5]
    circuits, values = [c for _, c, _ in cases], [v for _, _, v in cases]
    wrt = [[0, 3, 4, 7, 9]] * 5
    dev = StatevectorDevice(n)
    want = dev.metric_tensors(circuits, values, wrt)
    launches = dev.metric_stats()["n_gram_launches"]
    dev.set_option("metric_scratch_mib", 1)
    columns = [int(mr.slot_counts(c)[wrt[0]].sum()) for c in circuits]
    group = 16 // (max(columns) + 2)
    assert 1 <= group < 5, columns
    got = dev.metric_tensors(circuits, values, wrt)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert dev.metric_stats()["n_gram_launches"] == -(-5 // group) > launches
    # fifteen columns of the ladder: seventeen states
    index = [name for name, _, _ in family_circuits(n)].index("ladder")
    _, ladder, ladder_values = family_circuits(n)[index]
    with pytest.raises(ValueError, match=r"15 columns.*room for 14 at 12 qubits"):
        dev.metric_tensors([ladder], [ladder_values], list(range(15)))
    fits = dev.metric_tensors([ladder], [ladder_values], list(range(14)))[0]
    dev.set_option("metric_scratch_mib", 8192)
    assert np.array_equal(fits, dev.metric_tensors([ladder], [ladder_values], list(range(14)))[0])
    with pytest.raises(ValueError, match="metric_scratch_mib"):
        dev.set_option("metric_scratch_mib", 0)


# ---- 4. the same bits -----------------------------------------------------------------------------------------------------------


def bits_of(matrices):
    return [m.tobytes() for m in matrices]


def test_a_matrix_is_the_same_bits_in_any_batch_and_at_any_position():
    n = 11
    cases = family_circuits(n)
    circuits, values = [c for _, c, _ in cases], [v for _, _, v in cases]
    count = len(circuits)
    dev = StatevectorDevice(n)
    whole = bits_of(dev.metric_tensors(circuits, values))
    assert len(set(whole)) == count
    for order in ([3] + [i for i in range(count) if i != 3], list(reversed(range(count))), [int(i) for i in np.random.default_rng(4).permutation(count)]):
        got = bits_of(dev.metric_tensors([circuits[i] for i in order], [values[i] for i in order]))
        assert got == [whole[i] for i in order]
    for i in (0, 3, count - 1):
        assert bits_of(dev.metric_tensors([circuits[i]], [values[i]])) == [whole[i]]
    assert bits_of(dev.metric_tensors([circuits[2]] * 3, [values[2]] * 3)) == [whole[2]] * 3
    assert bits_of(dev.metric_tensors(circuits, values)) == whole  # (and on every call)


@pytest.mark.parametrize("n", [6, 12])
def test_a_wrt_subset_is_that_submatrix_bit_for_bit(n):
    dev = StatevectorDevice(n)
    rng = np.random.default_rng(100 + n)
    for name, circuit, values in family_circuits(n):
        if name.startswith("evqe") and not name.endswith("#0"):
            continue
        whole = dev.metric_tensors([circuit], [values])[0]
        p = circuit.num_parameters
        subsets = [[p - 1], [0], list(range(p - 1, -1, -2)), [int(i) for i in rng.choice(p, size=min(p, 7), replace=False)],
                   list(range(max(0, p - 6), p)), [1, 1, 0]]
        shared = np.flatnonzero(mr.slot_counts(circuit) > 1)
        if shared.size:  # (parameters several slots read, in both orders)
            subsets += [[int(shared[0]), p - 1, int(shared[-1])], [int(shared[-1]), int(shared[0])]]
        got = dev.metric_tensors([circuit] * len(subsets), [values] * len(subsets), subsets)
        for wrt, g in zip(subsets, got):
            assert np.array_equal(g, whole[np.ix_(wrt, wrt)]), (name, wrt)


def test_other_calls_return_the_same_bytes_before_and_after():
    n = 11
    cases = family_circuits(n)
    circuits, values = [c for _, c, _ in cases], [v for _, _, v in cases]
    ev = OperatorCircuitEvaluator(helpers.random_pauli_operator(n, 12, seed=3), gradient_method="adjoint")
    dev = ev.statevector_device

    def everything():
        return (np.asarray(ev.evaluate_circuits(circuits, values)).tobytes(), bits_of(ev.evaluate_gradients(circuits, values)),
                [dev.statevector(c, v).tobytes() for c, v in zip(circuits[:3], values[:3])])

    before = everything()
    metrics = ev.metric_tensors(circuits, values)
    assert everything() == before
    assert bits_of(ev.metric_tensors(circuits, values)) == bits_of(metrics)
    assert bits_of(StatevectorDevice(n).metric_tensors(circuits, values)) == bits_of(metrics)  # (a handle without an operator)
    for g, want, (name, circuit, _) in zip(metrics, reference(n), cases):
        check(f"through the evaluator, {name}", g, want, allowed(circuit))


def test_behind_an_initial_state_and_unread_parameters():
    n = 6
    initial = CircuitIR(n)
    for q in range(n):
        initial.u(0.3 + 0.2 * q, 0.1 * q, -0.4, q)
    circuit = CircuitIR(n).u(ParamRef(0), ParamRef(1), ParamRef(3), 2).cu3(ParamRef(0), 0.2, ParamRef(3), 2, 4).id(1)
    circuit.declare_parameters(6)  # (2, 4 and 5 are read by nothing; 0 and 3 by two slots each)
    values = [0.7, -0.2, 9.0, 1.3, 9.0, 9.0]
    ev = OperatorCircuitEvaluator(helpers.random_ising_operator(n, seed=1), initial_state_circuit=initial)
    got = ev.metric_tensors([circuit], [values])[0]
    composed = initial.compose(circuit)
    check("behind an initial state", got, mr.backward(composed, values), allowed(composed))
    assert got.shape == (6, 6) and not got[[2, 4, 5]].any() and not got[:, [2, 4, 5]].any()
    assert not np.signbit(got[[2, 4, 5]]).any()
    assert np.abs(got - mr.backward(circuit, values)).max() > 1e-3  # (the initial state is seen)
    # the closed form: one u on |0>
    one = CircuitIR(n).u(ParamRef(0), ParamRef(1), ParamRef(2), 3)
    g = ev.statevector_device.metric_tensors([one], [[0.7, -1.1, 2.3]])[0]
    assert np.abs(g - np.diag([0.25, np.sin(0.7) ** 2 / 4.0, 0.0])).max() <= TOL64
    # no parameters at all, and an empty batch
    assert ev.metric_tensors([initial], [[]])[0].shape == (0, 0)
    assert ev.metric_tensors([], []) == []


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------


def _raw(dev, circuits, params, wrt=None, out_width=None, out_given=True, n_evals=None):
    """qsv_metric_circuits as the C ABI returns it: (return code, message, out)."""
    n = len(circuits)
    ids, offsets, flat = dev._batch_arguments(circuits, params) if n else (np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1))
    wrt_offsets, wrt_flat, counts = StatevectorDevice._wrt_arguments(circuits, wrt)
    width = max(1, int(counts.max()) if n else 1) if out_width is None else out_width
    out = np.full((max(1, n), max(1, width), max(1, width)), np.nan, dtype=np.float64)
    rc = dev._lib.qsv_metric_circuits(
        dev._handle, n if n_evals is None else n_evals, _lib.as_ptr(ids), _lib.as_ptr(offsets), _lib.as_ptr(flat),
        None if wrt_offsets is None else _lib.as_ptr(wrt_offsets), None if wrt_flat is None else _lib.as_ptr(wrt_flat), width,
        _lib.as_ptr(out) if out_given else None)
    return rc, _lib.last_error(dev._lib, dev._handle), out


def test_refusals_leave_the_handle_working():
    n = 6
    cases = family_circuits(n)[:3]
    circuits, values = [c for _, c, _ in cases], [v for _, _, v in cases]
    dev = StatevectorDevice(n)
    first = []

    def works():
        rc, _, out = _raw(dev, circuits, values, [0, 2, 1])
        assert rc == _lib.QSV_OK and not np.isnan(out).any()
        first.append(out.tobytes())
        assert first[0] == first[-1]

    def refused(code, word, **kwargs):
        rc, message, out = _raw(dev, kwargs.pop("circuits", circuits), kwargs.pop("params", values), **kwargs)
        assert rc == code and word in message, (rc, message)
        assert np.isnan(out).all()  # (nothing was written)

    works()
    p = circuits[1].num_parameters
    refused(_lib.QSV_E_ARG, "out is null", out_given=False)
    refused(_lib.QSV_E_ARG, "wrt index", wrt=[[0], [p], [0]])
    refused(_lib.QSV_E_ARG, "wrt index", wrt=[[0], [-1], [0]])
    refused(_lib.QSV_E_ARG, "out_width 2 is too small for 3", wrt=[0, 1, 2], out_width=2)
    refused(_lib.QSV_E_ARG, "too small", out_width=p - 1)
    refused(_lib.QSV_E_ARG, "n_evals", n_evals=-1)
    with pytest.raises(ValueError, match="wrt index"):
        dev.metric_tensors(circuits, values, [[0], [p], [0]])
    works()
    # a wider output than needed: zeros behind an evaluation's entries
    rc, _, out = _raw(dev, circuits, values, [[0, 1], [2], []], out_width=4)
    assert rc == _lib.QSV_OK and not out[0, 2:].any() and not out[0, :, 2:].any() and not out[1, 1:].any() and not out[2].any()
    assert out[0, 0, 0] > 0 and out[1, 0, 0] > 0
    kept = dev.keep_states(circuits[:1], values[:1])
    continued = CircuitIR(n).u(ParamRef(0), 0.0, 0.0, 2).continue_from(kept[0])
    refused(_lib.QSV_E_UNSUPPORTED, "kept state", circuits=[continued], params=[[0.4]])
    with pytest.raises(ValueError, match="kept state"):
        dev.metric_tensors([continued], [[0.4]])
    assert _raw(dev, [], [], n_evals=0)[0] == _lib.QSV_OK
    assert _raw(dev, [], [], n_evals=0, out_given=False)[0] == _lib.QSV_OK
    # inside an open batch, from the thread that holds it
    dev.set_operator(helpers.random_ising_operator(n, seed=2))
    batch_ids, offsets, flat = dev._batch_arguments(circuits, values)
    counts = np.diff(offsets).astype(np.int64)
    results = np.zeros(len(circuits))
    assert dev._lib.qsv_eval_begin(dev._handle, len(circuits), _lib.as_ptr(batch_ids), _lib.as_ptr(counts)) == _lib.QSV_OK
    refused(_lib.QSV_E_STATE, "(qsv_metric_circuits goes between batches)")
    stats = _lib.QsvMetricStats()
    import ctypes as C

    assert dev._lib.qsv_metric_stats(dev._handle, C.byref(stats)) == _lib.QSV_E_STATE
    assert dev._lib.qsv_eval_push(dev._handle, 0, len(circuits), _lib.as_ptr(flat)) == _lib.QSV_OK
    assert dev._lib.qsv_eval_end(dev._handle, _lib.as_ptr(results)) == _lib.QSV_OK
    assert np.abs(results - dev.expectation_values(circuits, values)).max() <= 1e-12
    works()


def test_a_register_above_28_qubits_is_refused():
    """A 29-qubit fp32 handle (one state slot of 4 GiB), asked before anything is uploaded."""
    n = 29
    dev = StatevectorDevice(n, dtype="fp32")
    circuit = CircuitIR(n).u(ParamRef(0), 0.2, 0.1, 0)
    rc, message, _ = _raw(dev, [circuit], [[0.3]])
    assert rc == _lib.QSV_E_UNSUPPORTED and "28 qubits" in message and "29" in message, (rc, message)
    with pytest.raises(ValueError, match="28 qubits"):
        dev.metric_tensors([circuit], [[0.3]])


# ---- 6. the counters, the solver and the front end ---------------------------------------------------------------------------------


def test_metric_stats():
    n = 12
    index = [name for name, _, _ in family_circuits(n)].index("star")
    _, circuit, values = family_circuits(n)[index]
    runs = len(__import__("adjoint_reference").describe(circuit)["runs"])
    assert runs >= 2  # (controls outside the tile cut the sweep)
    dev = StatevectorDevice(n)
    zero = dev.metric_stats()
    assert zero["n_allocations"] == 0 and zero["n_columns"] == 0 and zero["scratch_bytes"] == 0
    dev.metric_tensors([circuit, circuit], [values, values], [[0, 1, 2], [5]])
    stats = dev.metric_stats()
    columns = int(mr.slot_counts(circuit)[[0, 1, 2]].sum() + mr.slot_counts(circuit)[5])
    assert stats["n_columns"] == columns and stats["n_run_launches"] == runs and stats["n_gram_launches"] == 1
    assert stats["run_ms"] == 0.0 and stats["gram_ms"] == 0.0
    assert stats["scratch_bytes"] >= 2 * (int(mr.slot_counts(circuit)[[0, 1, 2]].sum()) + 2) * (16 << n)
    allocations = stats["n_allocations"]
    dev.set_option("time_moments", 1)
    again = dev.metric_tensors([circuit], [values], [5])
    timed = dev.metric_stats()
    assert timed["n_allocations"] == allocations and timed["n_columns"] == int(mr.slot_counts(circuit)[5])  # (nothing grew)
    assert timed["run_ms"] > 0.0 and timed["gram_ms"] > 0.0
    dev.set_option("time_moments", 0)
    assert np.array_equal(again[0], dev.metric_tensors([circuit], [values], [5])[0])
    dev.metric_tensors([circuit], [values])  # (every column: the scratch grows)
    assert dev.metric_stats()["n_allocations"] > allocations


def test_the_solver_reports_the_best_individuals_metric():
    from queasars_amd.evqe import EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration, NaturalGradient

    n = 4
    operator = helpers.random_ising_operator(n, seed=5)

    def config(optimizer):
        return EVQEMinimumEigensolverConfiguration(
            optimizer=optimizer, population_size=4, max_generations=2, random_seed=3, n_initial_layers=2,
            randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2, use_tournament_selection=True,
            tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1, parameter_search_probability=0.3,
            topological_search_probability=0.4, layer_removal_probability=0.05,
        )

    from queasars_amd.evqe import SPSA

    spsa = lambda: SPSA(maxiter=5, learning_rate=0.4, perturbation=0.3)  # noqa: E731
    plain = EVQEMinimumEigensolver(config(spsa())).compute_minimum_eigenvalue(OperatorCircuitEvaluator(operator))
    assert plain.parameter_metric is None and plain.parameter_metric_rank is None
    evaluator = OperatorCircuitEvaluator(operator)
    asked = EVQEMinimumEigensolver(config(spsa())).compute_minimum_eigenvalue(evaluator, parameter_metric=True)
    assert asked.eigenvalue == plain.eigenvalue and asked.circuit_evaluations == plain.circuit_evaluations
    best = asked.best_individual
    circuit = best.get_parameterized_quantum_circuit()
    want = mr.backward(circuit, list(best.parameter_values))
    check("result.parameter_metric", asked.parameter_metric, want, allowed(circuit))
    assert asked.parameter_metric_rank == int((np.linalg.eigvalsh(want) > 1e-10).sum())
    assert 0 < asked.parameter_metric_rank <= circuit.num_parameters
    # a search by natural gradient runs on the device's gradients and metrics and lowers the energy
    searched = EVQEMinimumEigensolver(config(NaturalGradient(maxiter=5, learning_rate=0.2, regularization=1e-2))).compute_minimum_eigenvalue(
        OperatorCircuitEvaluator(operator, gradient_method="adjoint"))
    assert np.isfinite(searched.eigenvalue) and searched.eigenvalue <= searched.best_expectation_values[0]


def test_gpu_qfi():
    from queasars_amd.primitives import GpuQFI

    cases = [family_circuits(6)[0], family_circuits(6)[4], family_circuits(3)[-1]]
    circuits, values = [c for _, c, _ in cases], [v for _, _, v in cases]
    qfi = GpuQFI()
    result = qfi.run(circuits, values).result()
    assert len(result.qfis) == len(result.metadata) == 3
    for (name, c, v), got in zip(cases, result.qfis):
        check(f"QFI {name}", got, 4.0 * mr.backward(c, v), 4.0 * allowed(c))
    some = qfi.run(circuits, values, parameters=[[2, 0], None, [1]]).result().qfis
    assert np.array_equal(some[0], result.qfis[0][np.ix_([2, 0], [2, 0])]) and np.array_equal(some[1], result.qfis[1])
    assert np.array_equal(some[2], result.qfis[2][np.ix_([1], [1])])
    single = qfi.run(circuits[0], values[0]).result().qfis
    assert len(single) == 1 and np.array_equal(single[0], result.qfis[0])
    with pytest.raises(ValueError, match="values were given"):
        qfi.run(circuits[0], values[0][:-1])
