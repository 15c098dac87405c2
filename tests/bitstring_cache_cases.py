"""Inputs the value-cache tests share (tests only): the dyadic operator, the nonlinear scoring function and its vectorised form."""

from __future__ import annotations

import numpy as np

from queasars_amd.ir import PauliOperator


def dyadic_ising_operator(n: int, seed: int) -> PauliOperator:
    """A diagonal Ising operator whose coefficients are nonzero integers in [-16, 16] divided by 8: every partial sum of its
    terms is a multiple of 1/8 far below 2^53 / 8, so it is exact in fp64 in any order."""
    rng = np.random.default_rng(seed)

    def coefficient() -> float:
        k = int(rng.integers(1, 17))
        return (k if rng.integers(0, 2) else -k) / 8.0

    terms = [("ZZ", [i, j], coefficient()) for i in range(n) for j in range(i + 1, n)]
    terms += [("Z", [i], coefficient()) for i in range(n)]
    return PauliOperator.from_sparse_list(terms, n)


def nonlinear(bitstring: str) -> float:
    """A value no linear or quadratic table reproduces; exact in fp64 (an integer minus a multiple of one half)."""
    return float(int(bitstring, 2) % 97) - 0.5 * bitstring.count("1")


def popcount(states: np.ndarray) -> np.ndarray:
    v = np.asarray(states, dtype=np.uint64).copy()
    count = np.zeros(v.shape, dtype=np.int64)
    while v.any():
        count += (v & np.uint64(1)).astype(np.int64)
        v >>= np.uint64(1)
    return count


def nonlinear_of_states(states: np.ndarray) -> np.ndarray:
    """:func:`nonlinear` of every entry of an integer array."""
    states = np.asarray(states, dtype=np.uint64)
    return (states % np.uint64(97)).astype(np.float64) - 0.5 * popcount(states)


def score_states(states: np.ndarray, n: int, function) -> np.ndarray:
    """``function`` of every state's bitstring (qubit 0 is the last character), one Python call each."""
    return np.asarray([function(format(int(s), f"0{n}b")) for s in np.asarray(states).reshape(-1)], dtype=np.float64)
