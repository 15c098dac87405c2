"""Reduced density matrices at 24 qubits, where every workgroup of the 64 walks 256 blocks or more and no host
holds the state: one product circuit on three interleaved blocks of eight qubits (tests/factorised_reference.py), for which the
matrix of a subset is the Kronecker product of the blocks' own matrices over their share of the subset, rows and columns
reordered (rdm_reference.kron_reordered, held to the full state by tests/test_rdm_host.py).  One circuit, three subsets: inside
one block of the partition, across two, and the four top qubits."""

from __future__ import annotations

import numpy as np
import pytest

import factorised_reference as fr
import rdm_reference as rr
from queasars_amd.circuit_evaluation import StatevectorDevice

pytestmark = pytest.mark.gpu


def test_twenty_four_qubits_against_the_factorised_reference():
    n, seed = 24, 7
    blocks = fr.interleaved_blocks(n, (8, 8, 8), seed)
    pc = fr.product_circuit(n, blocks, ["generic", "ladder", "all_pairs"], seed)
    states = pc.states()
    owner = {q: b for b, qubits in enumerate(blocks) for q in qubits}
    inside = (blocks[0][5], blocks[0][0], blocks[0][7])
    across = (blocks[1][6], blocks[0][1], blocks[1][0], blocks[0][6])
    top = (20, 21, 22, 23)
    assert len({owner[q] for q in top}) >= 2
    subsets = [inside, across, top]

    def reference(subset):
        factors = []
        for b in sorted({owner[q] for q in subset}):
            mine = [q for q in subset if owner[q] == b]
            factors.append((rr.reduced_density_matrix(states[b], [blocks[b].index(q) for q in mine]), mine))
        return rr.kron_reordered(factors, subset)

    want = [reference(s)[None] for s in subsets]
    assert all(abs(np.trace(w[0]) - 1.0) <= 1e-13 for w in want)
    assert max(np.abs(w[0] - np.diag(np.diagonal(w[0]))).max() for w in want) > 1e-2  # (coherences an index error would move)
    dev = StatevectorDevice(n)
    got = dev.reduced_density_matrices([pc.circuit], [pc.params], subsets)
    err = rr.largest_error(got, want)
    print(f"rho n=24: largest component error {err:.3e} (allowed {rr.TOL:.3e})")
    assert err <= rr.TOL
    for m in got:
        assert np.array_equal(m, m.conj().transpose(0, 2, 1)) and not np.diagonal(m, axis1=1, axis2=2).imag.any()
