"""The live entries of a three-key evaluation's Gram tables (csrc/kernels.hpp ``live_entry``, ``qsv_live_entries``; option
``"live_entries"``) on the CPU.  On the reduced split form an entry (kappa, kappa') of a side's 8 x 8 Hermitian table is exactly
zero where the rows differ in a final-control key of that side, and the combination multiplies the sides' tables entry by entry:
only the entries whose rows agree on every such key of either side are handed off and paired.  Checked here: the set and its
order against a plain restatement of the entry numbering, and that the compact pairing over the live entries, in the order the
kernel states, has the bits of the full 64-term pairing."""
import ctypes as C

import numpy as np
import pytest

from queasars_amd import _lib

J = 8


def split_entry_of(pi: int):
    """Entry pi of a J x J Hermitian form: (ja, jb, part) -- part 0 the diagonal entry ja, 1 / 2 the real / imaginary part of the
    pair ja < jb; the pairs in lexicographic order behind the J diagonal entries."""
    if pi < J:
        return pi, pi, 0
    o, part = (pi - J) >> 1, 1 + ((pi - J) & 1)
    ja = 0
    while o >= J - 1 - ja:
        o -= J - 1 - ja
        ja += 1
    return ja, ja + 1 + o, part


def live_entries(key_mask: int):
    out = np.full(64, -7, dtype=np.int32)
    count = _lib.load().qsv_live_entries(3, key_mask, out.ctypes.data_as(C.POINTER(C.c_int)))
    assert count >= 0, count
    assert (out[count:] == -1).all()
    return [int(pi) for pi in out[:count]]


def test_the_numbering_is_the_pairs_in_order():
    seen = [split_entry_of(pi) for pi in range(J * J)]
    assert seen[:J] == [(j, j, 0) for j in range(J)]
    pairs = [(a, b) for a in range(J) for b in range(a + 1, J)]
    assert seen[J:] == [(a, b, part) for a, b in pairs for part in (1, 2)]


@pytest.mark.parametrize("key_mask", range(8))
def test_live_set(key_mask):
    want = [pi for pi in range(J * J) if (split_entry_of(pi)[0] ^ split_entry_of(pi)[1]) & key_mask == 0]
    got = live_entries(key_mask)
    assert got == want and got == sorted(got)
    assert len(got) == 64 >> bin(key_mask).count("1")
    assert got[:J] == list(range(J))  # (the diagonal entries, always)
    # both parts of a pair or neither, next to each other: the compact pairing walks them two at a time
    assert all(split_entry_of(a)[:2] == split_entry_of(b)[:2] and (split_entry_of(a)[2], split_entry_of(b)[2]) == (1, 2)
               for a, b in zip(got[J::2], got[J + 1::2]))


def test_arguments():
    out = np.zeros(64, dtype=np.int32)
    ptr = out.ctypes.data_as(C.POINTER(C.c_int))
    lib = _lib.load()
    assert lib.qsv_live_entries(2, 1, ptr) < 0 and lib.qsv_live_entries(3, 8, ptr) < 0 and lib.qsv_live_entries(3, 1, None) < 0


def entries_of(m: np.ndarray) -> np.ndarray:
    """The entry representation of a Hermitian matrix: m[ja, ja], then Re and Im of m[ja, jb] for every pair."""
    out = np.zeros(J * J)
    for pi in range(J * J):
        ja, jb, part = split_entry_of(pi)
        out[pi] = m[ja, jb].imag if part == 2 else m[ja, jb].real
    return out


def fma(a, b, c):
    """a * b + c rounded once: with exact rational arithmetic (the operands are doubles, so the sum is a rational number)."""
    from fractions import Fraction

    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return float(exact)  # (Fraction -> float rounds to nearest, ties to even)


def pairing_full(a, b):
    """kernels.hip factor_pairing_unrolled<8>: the diagonal entries by fused multiply-add, then twice every pair's real part."""
    t = 0.0
    for j in range(J):
        t = fma(a[j], b[j], t)
    for e in range(J, J * J, 2):
        t = t + 2.0 * fma(a[e], b[e], -(a[e + 1] * b[e + 1]))
    return t


def pairing_live(a, b, count):
    """kernels.hip factor_pairing_live<L> over the compact tables."""
    t = 0.0
    for j in range(J):
        t = fma(a[j], b[j], t)
    for e in range(J, count, 2):
        t = t + 2.0 * fma(a[e], b[e], -(a[e + 1] * b[e + 1]))
    return t


def random_hermitian(rng):
    m = rng.standard_normal((J, J)) + 1j * rng.standard_normal((J, J))
    return m + m.conj().T


@pytest.mark.parametrize("key_mask", range(1, 8))
@pytest.mark.parametrize("zeroed", ["A", "B", "both"])
def test_compact_pairing_has_the_bits_of_the_full_one(key_mask, zeroed):
    rng = np.random.default_rng(100 + key_mask)
    rows = np.arange(J)
    dead = ((rows[:, None] ^ rows[None, :]) & key_mask) != 0
    live = live_entries(key_mask)
    for _ in range(20):
        a, b = random_hermitian(rng), random_hermitian(rng)
        if zeroed in ("A", "both"):
            a = np.where(dead, 0.0, a)
        if zeroed in ("B", "both"):
            b = np.where(dead, 0.0, b)
        ea, eb = entries_of(a), entries_of(b)
        full = pairing_full(ea, eb)
        compact = pairing_live(ea[live], eb[live], len(live))
        assert np.float64(full).tobytes() == np.float64(compact).tobytes()
        # ... and it is sum_{j'j} A[j'j] B[j'j], as far as doubles say
        assert abs(full - np.sum(a * b).real) < 1e-12 * (1.0 + np.abs(a * b).sum())
