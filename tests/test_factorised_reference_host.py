"""tests/factorised_reference.py held to the references the project already trusts, at sizes where both run (n = 9 .. 12 in three
interleaved blocks, the full state from the NumPy oracle on the merged circuit), and -- for every case and seed of
tests/test_gpu_large_registers.py, at its own size -- the conditions that keep those device tests from hiding a failure.  No GPU."""

from __future__ import annotations

import numpy as np
import pytest

import adjoint_reference
import covariance_reference as cr
import dense_gradient
import factorised_reference as fr
import helpers
import overlap_reference as ovr
import top_states_reference as tsr
import variance_reference as vr
from oracle import statevector_oracle as so

# (n, block sizes): three blocks each; 12 = 4 + 4 + 4 and the uneven ones
SMALL = [(9, (3, 3, 3)), (10, (4, 3, 3)), (11, (3, 5, 3)), (12, (4, 4, 4))]
REL = 1e-12  # agreement, times the references' own scale


class _Small:
    def __init__(self, n, sizes):
        self.n = n
        self.blocks = fr.interleaved_blocks(n, sizes, seed=n)
        self.pcs = [fr.product_circuit(n, self.blocks, [fr.FAMILIES[(i + b) % 3] for b in range(3)], 10 * n + i) for i in range(3)]
        self.points = [pc.params for pc in self.pcs] + [fr.perturbed(self.pcs[0], n)]
        self.pcs.append(self.pcs[0])
        self.full = [helpers.oracle_state(pc.circuit, p) for pc, p in zip(self.pcs, self.points)]
        self.fact = [fr.Factorised(self.blocks, pc.states(p)) for pc, p in zip(self.pcs, self.points)]
        self.ops = {"general": fr.general_operator(n, self.blocks, n), "ising": fr.ising_operator(n, self.blocks, n, n_pairs=12)}


_small: dict = {}


def small(n, sizes) -> _Small:
    if n not in _small:
        _small[n] = _Small(n, sizes)
    return _small[n]


@pytest.mark.parametrize("n,sizes", SMALL)
def test_the_merged_circuit_prepares_the_product_of_the_block_states(n, sizes):
    s = small(n, sizes)
    for pc, p, full, fact in zip(s.pcs, s.points, s.full, s.fact):
        assert len(pc.circuit) == sum(len(local) for local, _, _ in pc.parts) and pc.circuit.num_parameters == len(p)
        assert np.abs(fr.full_state(fact) - full).max() <= REL
    kinds = {int(row["kind"]) for pc in s.pcs for row in pc.circuit.packed()}
    assert kinds >= {1, 2}  # (a generic block of this few ops may draw no id)
    packed = s.pcs[0].circuit.packed()
    assert (packed["p_theta"] < 0).any() and len(set(packed["p_theta"].tolist())) < len(packed)  # literals and shared ParamRefs


@pytest.mark.parametrize("n,sizes", SMALL)
def test_operators_hold_the_terms_the_device_tests_need(n, sizes):
    s = small(n, sizes)
    op = s.ops["general"]
    top = 1 << (n - 1)
    x, z = [int(v) for v in op.x_mask], [int(v) for v in op.z_mask]
    owner = {q: i for i, b in enumerate(s.blocks) for q in b}
    assert any(a & top and not b & top for a, b in zip(x, z)) and any(a & top and b & top for a, b in zip(x, z))
    assert any(not a & top and b & top for a, b in zip(x, z))
    assert any(len({owner[q] for q in range(n) if (a >> q) & 1}) >= 3 for a in x)
    assert any((a | b) == 1 for a, b in zip(x, z))
    assert len(op) <= 40 and len({a for a in x if a}) <= 12
    assert s.ops["ising"].is_diagonal()
    for m in (17, 33):
        ops = fr.observable_set(n, s.blocks, m, n)
        assert len(ops) == m and ops[1].is_diagonal() and sum(len(o) for o in ops) <= 40 * 3


@pytest.mark.parametrize("n,sizes", SMALL)
def test_moments_against_the_variance_reference(n, sizes):
    s = small(n, sizes)
    for name, op in s.ops.items():
        scale = max(1.0, vr.spread(op)) ** 2
        for full, fact in zip(s.full, s.fact):
            want, got = vr.moments(op, full), fr.moments(op, fact)
            assert abs(got[0] - want[0]) <= REL * scale and abs(got[1] - want[1]) <= REL * scale, (name, got, want)


@pytest.mark.parametrize("n,sizes", SMALL)
@pytest.mark.parametrize("m", [17, 33])
def test_covariances_against_the_covariance_reference(n, sizes, m):
    s = small(n, sizes)
    ops = fr.observable_set(n, s.blocks, m, n)
    scale = np.maximum(1.0, cr.spreads(ops))
    for full, fact in zip(s.full[:2], s.fact[:2]):
        want_values, want_cov = cr.moments(ops, full)
        values, cov = fr.covariance(ops, fact)
        assert np.all(np.abs(values - want_values) <= REL * scale)
        assert np.all(np.abs(cov - want_cov) <= REL * np.outer(scale, scale))


@pytest.mark.parametrize("n,sizes", SMALL)
def test_overlaps_and_elements_against_the_overlap_reference(n, sizes):
    s = small(n, sizes)
    want_s = ovr.overlaps(s.full, s.full)
    got_s = np.asarray([[fr.overlap(k, e) for k in s.fact] for e in s.fact])
    assert ovr.max_component_error(got_s, want_s) <= REL
    assert abs(want_s[3, 0]) >= 0.5  # (the perturbed copy against its original)
    for name, op in s.ops.items():
        want_t = ovr.elements(op, s.full, s.full, dense=False)
        got_t = np.asarray([[fr.element(op, k, e) for k in s.fact] for e in s.fact])
        assert ovr.max_component_error(got_t, want_t) <= REL * max(1.0, ovr.spread(op)), name


@pytest.mark.parametrize("n,sizes", SMALL)
def test_gradients_against_the_full_sweep(n, sizes):
    s = small(n, sizes)
    for name, op in s.ops.items():
        for pc, p in zip(s.pcs[:2], s.points[:2]):
            want = adjoint_reference.gradient(pc.circuit, p, op)
            got = fr.gradient(op, pc, p)
            assert np.abs(want).max() > 1e-2
            assert np.abs(got - want).max() <= REL * max(1.0, vr.spread(op)), name


def test_a_block_gradient_is_the_dense_derivative():
    """On eight qubits in two blocks the whole register fits tests/dense_gradient.py."""
    n = 8
    blocks = [[0, 2, 5, 6], [1, 3, 4, 7]]
    pc = fr.product_circuit(n, blocks, ["generic", "ladder"], 3)
    op = fr.general_operator(n, blocks, 8, n_terms=16)
    want = dense_gradient.gradient(pc.circuit, pc.params, dense_gradient.dense_operator(op))
    assert np.abs(fr.gradient(op, pc) - want).max() <= REL * max(1.0, vr.spread(op))


def test_a_block_of_nine_qubits_takes_the_numpy_sweep():
    """Blocks above eight qubits (n = 25 and 28 need them: only three blocks can reach the top three qubits) leave
    tests/dense_gradient.py for the sweep of tests/adjoint_reference.py: held here to the same sweep over the whole register."""
    n = 13
    blocks = fr.interleaved_blocks(n, (9, 2, 2), seed=n)
    pc = fr.product_circuit(n, blocks, ["all_pairs", "ladder", "generic"], 13)
    for op in (fr.general_operator(n, blocks, n), fr.ising_operator(n, blocks, n, n_pairs=12)):
        want = adjoint_reference.gradient(pc.circuit, pc.params, op)
        assert np.abs(want).max() > 1e-2
        assert np.abs(fr.gradient(op, pc) - want).max() <= REL * max(1.0, vr.spread(op))


@pytest.mark.parametrize("n,sizes", SMALL)
@pytest.mark.parametrize("k", [1, 16, 200])
def test_top_states_against_the_sorted_probabilities(n, sizes, k):
    s = small(n, sizes)
    for full, fact in zip(s.full, s.fact):
        probs = so.probabilities(full)
        states, got, gap = fr.top_states(fact, k)
        want_states, want = tsr.expected_top(probs, k + 1)
        assert gap >= 1e-9  # (or the two roundings may order a pair differently: another seed then)
        assert states.tolist() == want_states[:k].tolist()
        assert np.abs(got - want[:k]).max() <= REL
        tsr.check_top(states, got, probs, k, tsr.TOL_FP64)
        assert abs(gap - float(((want[:k] - want[1:]) / want[:k]).min())) <= 1e-6 * max(gap, 1e-9) + 1e-9


def test_top_states_break_exact_ties_by_the_lower_index():
    """Two blocks in |+>^m: every probability equal, so the tie rule alone decides, across the fold."""
    blocks = [[0, 2, 5], [1, 3, 4]]
    plus = np.full(8, 1 / np.sqrt(8), dtype=np.complex128)
    states, probs, gap = fr.top_states(fr.Factorised(blocks, [plus, plus]), 10)
    assert states.tolist() == list(range(10)) and gap == 0.0 and np.all(probs == probs[0])


# ---- the device tests' own cases -------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module", params=list(fr.LARGE_CASES))
def case(request):
    return fr.large_case(request.param)


def test_large_cases_use_interleaved_blocks_that_reach_every_range(case):
    fr.check_blocks(case.n, case.blocks)
    for b in case.blocks:
        assert any(q < 6 for q in b) and any(10 <= q <= 13 for q in b) and any(q >= case.n - 3 for q in b)
        assert len(b) <= 10
    for pc, _ in case.evals:
        assert {int(t) for t in pc.circuit.packed()["target"]} >= {0, case.n - 1}


def test_large_cases_have_sizeable_variances(case):
    """Every variance and every diagonal covariance entry at least 1e-3 (sum |c|)^2."""
    for i in range(len(case.evals)):
        f = case.factorised(i)
        for op in (case.general, case.ising):
            assert fr.moments(op, f)[1] >= 1e-3 * fr.spread(op) ** 2, (case.name, i)
        for m, ops in case.observables.items():
            cov = fr.covariance(ops, f)[1]
            assert np.all(np.diagonal(cov) >= 1e-3 * np.asarray([fr.spread(o) for o in ops]) ** 2), (case.name, i, m)


def test_large_cases_have_large_and_small_overlaps(case):
    if not case.kept:
        return  # (the batch of 20 runs no overlaps)
    s = np.abs([[fr.overlap(case.kept_factorised(j), case.factorised(i)) for j in range(len(case.kept))] for i in range(len(case.evals))])
    assert s.max() >= 0.5 and s.min() <= 0.1, (case.name, s.max(), s.min())
    own = (len(case.evals) + 1) // 2
    assert all(s[i].max() >= 0.5 for i in range(own, len(case.evals)))  # (every perturbed copy against its original)


def test_large_cases_have_top_states_apart(case):
    for i in range(len(case.evals)):
        assert fr.top_states(case.factorised(i), fr.TOP_K)[2] >= fr.gap_floor(case.name), (case.name, i)


def test_large_cases_have_sizeable_gradients(case):
    """At least a quarter of the gradient entries exceed 1e-3 sum |c| in magnitude."""
    pc, p = case.evals[0]
    for op in (case.general, case.ising):
        g = fr.gradient(op, pc, p)
        assert np.mean(np.abs(g) > 1e-3 * fr.spread(op)) >= 0.25, (case.name, float(np.mean(np.abs(g) > 1e-3 * fr.spread(op))))
