"""References for the operator's variance, tests only: Var = <psi|H_h^2|psi> - <psi|H_h|psi>^2 with H_h the
Hermitian part of the operator (the real parts of the coefficients), raw -- no division by <psi|psi> --, on the NumPy oracle's
state.  Two forms: the dense matrix of tests/dense_gradient.py (n <= 8), which holds the Hermitian-part convention, and a
matrix-free application of the strings for larger registers; tests/test_variance_host.py holds them to each other."""

from __future__ import annotations

import functools

import numpy as np

import helpers
from dense_gradient import dense_operator
from oracle.statevector_oracle import _popcount_parity
from queasars_amd.ir import PauliOperator

#: |E - evaluate_circuits| in fp64: the project's own figure
TOL_VALUES = 1e-10
#: the project's fp32 floor, relative to sum |c_k| squared
FP32_FLOOR = 2e-6


def spread(op: PauliOperator) -> float:
    """sum |c_k|: a bound of |H|."""
    return float(np.abs(op.coeffs).sum())


def tol_fp64(op: PauliOperator) -> float:
    """|Var - reference| in fp64: amplitudes after at most ~150 gates carry about 2e-14 relative error, lambda = H psi is bounded
    by sum |c_k| times that, so m2 and m1^2 are each off by at most about 1e-13 (sum |c_k|)^2, the fixed-order sums of 2^13 to
    2^17 terms included; a hundred times that."""
    return 1e-11 * max(1.0, spread(op)) ** 2


def apply_strings(op: PauliOperator, state: np.ndarray) -> np.ndarray:
    """H_h |state>, string by string: (P psi)_i = (-i)^ny (-1)^popcount(i & z) psi_(i ^ x) for P = i^ny X^x Z^z, the oracle's
    reading of a label (pauli_term_expectation)."""
    idx = np.arange(state.shape[0], dtype=np.int64)
    out = np.zeros(state.shape[0], dtype=np.complex128)
    for x, z, c in zip(op.x_mask.tolist(), op.z_mask.tolist(), op.coeffs.tolist()):
        c = complex(c).real
        if c == 0.0:
            continue
        n_y = bin(int(x) & int(z)).count("1")
        sign = 1.0 - 2.0 * _popcount_parity(idx & int(z))
        out += (c * (-1j) ** (n_y % 4)) * (sign * state[idx ^ int(x)])
    return out


def _moments(state: np.ndarray, lam: np.ndarray) -> tuple[float, float]:
    value = float(np.real(np.vdot(state, lam)))
    return value, float(np.real(np.vdot(lam, lam))) - value * value


def moments(op: PauliOperator, state: np.ndarray) -> tuple[float, float]:
    """(E, Var) of `op` in `state`, matrix-free."""
    return _moments(state, apply_strings(op, state))


def dense_moments(op: PauliOperator, state: np.ndarray) -> tuple[float, float]:
    """(E, Var) from the dense Hermitian part (n <= 8)."""
    assert op.num_qubits <= 8
    return _moments(state, dense_operator(op) @ state)


@functools.lru_cache(maxsize=None)
def population(n: int, layers: int, count: int, seed: int):
    """helpers.population_circuits with the oracle's states, computed once: (circuits, parameter values, states)."""
    _, circuits, params = helpers.population_circuits(n, layers, count, seed=seed)
    return circuits, params, [helpers.oracle_state(c, p) for c, p in zip(circuits, params)]


def reference(op: PauliOperator, states) -> tuple[np.ndarray, np.ndarray]:
    """(values, variances) over `states`: dense for n <= 8, matrix-free above."""
    form = dense_moments if op.num_qubits <= 8 else moments
    pairs = [form(op, s) for s in states]
    return np.asarray([p[0] for p in pairs]), np.asarray([p[1] for p in pairs])
