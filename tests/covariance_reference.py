"""References for the covariance matrix of an observable set, tests only: with lambda_m = O_m psi for the
Hermitian part O_m of each observable (the real parts of the coefficients), E_m = Re<psi|lambda_m> and C_ab = Re<lambda_a|lambda_b> -
E_a E_b, raw -- no division by <psi|psi> --, on the NumPy oracle's state.  Two forms, as tests/variance_reference.py has them: the
dense matrices of tests/dense_gradient.py (n <= 8) and a matrix-free application of the strings for larger registers;
tests/test_covariance_host.py holds them to each other."""

from __future__ import annotations

import numpy as np

from dense_gradient import dense_operator
from queasars_amd.ir import PauliOperator
from variance_reference import FP32_FLOOR, TOL_VALUES, apply_strings, population, spread  # noqa: F401  (shared with the variance tests)


def _from_panel(state: np.ndarray, panel: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(E, C) from the columns lambda_m of `panel` (amplitudes x M)."""
    values = np.real(state.conj() @ panel)
    gram = np.real(panel.conj().T @ panel)
    return values, gram - np.outer(values, values)


def moments(ops, state: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(E (M), C (M, M)) of `ops` in `state`, matrix-free."""
    return _from_panel(state, np.stack([apply_strings(op, state) for op in ops], axis=1))


def dense_moments(ops, state: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(E, C) from the dense Hermitian parts (n <= 8)."""
    assert all(op.num_qubits <= 8 for op in ops)
    return _from_panel(state, np.stack([dense_operator(op) @ state for op in ops], axis=1))


def reference(ops, states) -> tuple[np.ndarray, np.ndarray]:
    """(values (n, M), covariances (n, M, M)) over `states`: dense for n <= 8, matrix-free above."""
    form = dense_moments if ops[0].num_qubits <= 8 else moments
    pairs = [form(ops, s) for s in states]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def spreads(ops) -> np.ndarray:
    """S_m = sum |c_mk| per observable: a bound of |O_m|."""
    return np.asarray([spread(op) if len(op) else 0.0 for op in ops])


def tol_fp64(ops) -> np.ndarray:
    """|C_ab - reference| in fp64, an (M, M) array: the bound of variance_reference.tol_fp64 with the two operators' norms in
    place of one squared -- lambda_a and lambda_b are each off by at most about 2e-14 S, so Re<lambda_a|lambda_b> and E_a E_b by
    about 1e-13 S_a S_b, the fixed-order sums included; a hundred times that."""
    s = np.maximum(1.0, spreads(ops))
    return 1e-11 * np.outer(s, s)


def combined(ops, weights) -> PauliOperator:
    """sum_m w_m O_m as one operator (terms concatenated, duplicates kept)."""
    labels = [label for op in ops for label in op.labels]
    return PauliOperator(labels, np.concatenate([float(w) * np.asarray(op.coeffs, dtype=complex) for op, w in zip(ops, weights)]))
