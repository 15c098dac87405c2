"""The deflated (VQD) cost at n = 20, where no NumPy sweep holds the state: product circuits of
tests/factorised_reference.py, for which cost and gradient factorise block by block.

With S_k = prod_b s_kb, s_kb = <phi_kb|psi_b>, the penalty beta_k |S_k|^2 = beta_k prod_b <psi_b| |phi_kb><phi_kb| |psi_b>, so the
gradient by a parameter of block b is the gradient, on the block alone, of the expectation value of
    H_eff,b + sum_k beta_k (prod_(b' != b) |s_kb'|^2) |phi_kb><phi_kb|
-- factorised_reference.effective_operator's Pauli sum plus a dense rank-K term -- by tests/dense_gradient.py (blocks of at most
eight qubits).  The factorised gradient is what was done; the C oracle's full states are not used.  The first test holds the
helper to tests/deflation_reference.py on a 10-qubit register, on the host."""

import numpy as np
import pytest

import deflation_reference as dr
import dense_gradient
import factorised_reference as fr
from queasars_amd.circuit_evaluation import StatevectorDevice

EXP_TOL = 1e-10


def factorised_terms(op, f: fr.Factorised, kept, betas):
    """(C, E, c) of one evaluation against kept product states over the same partition."""
    energy, _ = fr.moments(op, f)
    c = np.asarray([fr.overlap(k, f) for k in kept], dtype=np.complex128)
    penalty = 0.0
    for beta, ck in zip(betas, c):
        penalty += beta * (ck.real * ck.real + ck.imag * ck.imag)
    return energy + penalty, energy, c


def factorised_gradient(op, pc: fr.ProductCircuit, params, kept, betas) -> np.ndarray:
    """dC / d params[p] for every parameter of the product circuit, block by block."""
    f = fr.Factorised(pc.blocks, pc.states(params))
    # |s_kb|^2 per kept state and block
    s2 = np.asarray([[abs(np.vdot(phi, psi)) ** 2 for phi, psi in zip(k.states, f.states)] for k in kept]).reshape(len(kept), len(pc.blocks))
    out = np.zeros(pc.circuit.num_parameters)
    for b, ((local, sl, qubits), values) in enumerate(zip(pc.parts, pc.local_params(params))):
        assert len(qubits) <= 8
        h = dense_gradient.dense_operator(fr.effective_operator(op, f, b)).copy()
        for k, (beta, state) in enumerate(zip(betas, kept)):
            others = float(np.prod(np.delete(s2[k], b)))
            h += beta * others * np.outer(state.states[b], state.states[b].conj())
        out[sl] = dense_gradient.gradient(local, values, h)
    return out


def _case(n: int, sizes, seed: int, n_kept: int = 3):
    """(partition, kept product circuits, evaluations [(product circuit, point)], operator, betas): two circuits of their own and one
    perturbed copy of each kept circuit, so that overlaps of order one occur."""
    blocks = fr.interleaved_blocks(n, sizes, seed)
    families = lambda i: [fr.FAMILIES[(i + b) % len(fr.FAMILIES)] for b in range(len(sizes))]  # noqa: E731
    kept = [fr.product_circuit(n, blocks, families(j), 100 * seed + 50 + j) for j in range(n_kept)]
    evals = [(pc, pc.params) for pc in (fr.product_circuit(n, blocks, families(i), 100 * seed + i) for i in range(2))]
    evals += [(pc, fr.perturbed(pc, 100 * seed + j)) for j, pc in enumerate(kept)]
    return blocks, kept, evals, fr.general_operator(n, blocks, seed), [6.5, -2.25, 0.8][:n_kept]


def test_the_factorised_deflated_cost_is_the_full_state_one_at_ten_qubits():
    n = 10
    blocks, kept, evals, op, betas = _case(n, (4, 3, 3), 3)
    kept_f = [fr.Factorised(blocks, pc.states()) for pc in kept]
    kept_full = [fr.full_state(k) for k in kept_f]
    largest = 0.0
    for pc, p in evals:
        want_g, want_c, want_e, want_s = dr.gradient_and_terms(pc.circuit, p, op, kept_full, betas)
        got_c, got_e, got_s = factorised_terms(op, fr.Factorised(blocks, pc.states(p)), kept_f, betas)
        largest = max(largest, float(np.abs(got_s).max()))
        scale = dr.scale(op, betas)
        assert abs(got_c - want_c) < 1e-12 * scale and abs(got_e - want_e) < 1e-12 * scale and float(np.abs(got_s - want_s).max()) < 1e-12
        got_g = factorised_gradient(op, pc, p, kept_f, betas)
        assert float(np.abs(got_g - want_g).max()) < 1e-11 * scale and float(np.abs(want_g).max()) > 1e-3
    assert largest > 0.5  # (the perturbed copies: overlaps of order one)


@pytest.mark.gpu
def test_n20_against_the_factorised_reference():
    n = 20
    blocks, kept, evals, op, betas = _case(n, (7, 7, 6), 7)
    kept_f = [fr.Factorised(blocks, pc.states()) for pc in kept]
    dev = StatevectorDevice(n)
    dev.set_operator(op)
    states = dev.keep_states([pc.circuit for pc in kept], [pc.params for pc in kept])
    circuits, params = [pc.circuit for pc, _ in evals], [list(p) for _, p in evals]
    gradients, costs, energies, overlaps = dev.deflated_gradients(circuits, params, states, betas, with_values=True, with_overlaps=True)
    scale = dr.scale(op, betas)
    worst = {"g": 0.0, "c": 0.0, "e": 0.0, "s": 0.0}
    for i, (pc, p) in enumerate(evals):
        want_c, want_e, want_s = factorised_terms(op, fr.Factorised(blocks, pc.states(p)), kept_f, betas)
        want_g = factorised_gradient(op, pc, p, kept_f, betas)
        assert float(np.abs(want_g).max()) > 1e-3
        worst["g"] = max(worst["g"], float(np.abs(gradients[i] - want_g).max()))
        worst["c"] = max(worst["c"], abs(costs[i] - want_c))
        worst["e"] = max(worst["e"], abs(energies[i] - want_e))
        worst["s"] = max(worst["s"], float(np.abs(overlaps[i] - want_s).max()))
    print(f"n = 20, K = 3: |dgrad| {worst['g']:.3e}, |dC| {worst['c']:.3e}, |dE| {worst['e']:.3e}, |dc| {worst['s']:.3e}; scale {scale:.1f}")
    assert worst["g"] < EXP_TOL * max(1.0, float(np.abs(betas).sum()))
    assert worst["c"] < 1e-12 * scale and worst["e"] < 1e-12 * scale and worst["s"] < 1e-12 * scale
    assert float(np.abs(overlaps[2:]).max()) > 0.5  # (the perturbed copies: overlaps of order one)
    # the bit contracts hold here too: the overlaps are the overlap call's, a row alone is the row of the batch
    assert np.array_equal(np.ascontiguousarray(overlaps).view(np.uint64), np.ascontiguousarray(dev.overlaps(circuits, params, states)).view(np.uint64))
    alone = dev.deflated_gradients(circuits[3:4], params[3:4], states, betas, with_values=True)
    assert np.array_equal(alone[0][0].view(np.uint64), gradients[3].view(np.uint64)) and alone[1][0] == costs[3]
    dev.close()
