"""The Fubini-Study metric at 20 and 24 qubits, where no host holds the derivative states: product circuits on
interleaved blocks (tests/factorised_reference.py).  A tangent by a parameter of block b is (d psi_b) times the other blocks'
states, so G is block diagonal: inside a block it is the block's own metric (tests/metric_reference.py on the local circuit),
between blocks <d_i psi|d_j psi> = <d_i psi_a|psi_a><psi_b|d_j psi_b> cancels against the second term exactly -- zero in the
reference.  At 24 qubits the 17 columns and psi's two buffers are 19 states of 256 MiB: offsets into the scratch pass 4 GiB."""

from __future__ import annotations

import numpy as np
import pytest

import factorised_reference as fr
import metric_reference as mr
from queasars_amd.circuit_evaluation import StatevectorDevice

pytestmark = pytest.mark.gpu

TOL64 = 1e-10


def block_diagonal_reference(pc: fr.ProductCircuit, wrt) -> tuple[np.ndarray, np.ndarray]:
    """(G over ``wrt``, slots that read each of them) from the blocks' own metrics."""
    home = {}
    for b, (local, sl, _) in enumerate(pc.parts):
        for p in range(sl.start, sl.stop):
            home[p] = (b, p - sl.start)
    want = np.zeros((len(wrt), len(wrt)))
    slots = np.zeros(len(wrt))
    for b, ((local, sl, _), values) in enumerate(zip(pc.parts, pc.local_params())):
        mine = [(k, home[p][1]) for k, p in enumerate(wrt) if home[p][0] == b]
        if not mine:
            continue
        rows, local_wrt = [k for k, _ in mine], [j for _, j in mine]
        want[np.ix_(rows, rows)] = mr.backward(local, values, local_wrt)
        slots[rows] = mr.slot_counts(local)[local_wrt]
    return want, slots


def run_case(n, sizes, families, seed, count):
    blocks = fr.interleaved_blocks(n, sizes, seed)
    pc = fr.product_circuit(n, blocks, families, seed)
    total = pc.circuit.num_parameters
    # parameters no slot shares, spread over every block, the first and the last of the circuit among them: one column each
    single = np.flatnonzero(mr.slot_counts(pc.circuit) == 1)
    rng = np.random.default_rng(seed)
    wrt = sorted({int(single[0]), int(single[-1])} | {int(p) for p in rng.choice(single[1:-1], size=count - 2, replace=False)})
    rng.shuffle(wrt)
    wrt = [int(p) for p in wrt]
    want, slots = block_diagonal_reference(pc, wrt)
    assert len(wrt) == count and (slots == 1).all() and total > count
    assert len({next(b for b, (_, sl, _) in enumerate(pc.parts) if sl.start <= p < sl.stop) for p in wrt}) == len(blocks)
    assert np.count_nonzero(want) > count and np.count_nonzero(want == 0.0) > count  # (both kinds of entry are there)
    dev = StatevectorDevice(n)
    got = dev.metric_tensors([pc.circuit], [pc.params], wrt)[0]
    stats = dev.metric_stats()
    assert stats["n_columns"] == count and stats["scratch_bytes"] >= (count + 2) * (16 << n)
    err = np.abs(got - want)
    print(f"n={n}, {count} columns, {stats['n_run_launches']} runs: largest |G - ref| {err.max():.3e} (allowed {TOL64:.1e}); "
          f"largest coupling between blocks {np.abs(got[want == 0.0]).max():.3e}")
    assert err.max() <= TOL64
    assert np.array_equal(got, got.T)
    return stats


def test_twenty_qubits_twenty_columns():
    run_case(20, (7, 7, 6), ["generic", "ladder", "all_pairs"], seed=3, count=20)


def test_twenty_four_qubits_offsets_past_four_gib():
    stats = run_case(24, (8, 8, 8), ["ladder", "generic", "all_pairs"], seed=7, count=17)
    assert stats["scratch_bytes"] > 1 << 32
