"""Subspace refinement of a set of states from their overlap and operator matrices (host only, NumPy).

With ``S[i, j] = <psi_i|psi_j>`` and ``H[i, j] = <psi_i|H|psi_j>`` over k states (``OperatorCircuitEvaluator.
evaluate_subspace_matrices``) the lowest generalised eigenvalue of ``H c = E S c`` is the lowest energy any
linear combination of the states reaches: a variational upper bound of the ground energy that is never above the best single
state's energy.  The states of a population are far from orthogonal and some nearly repeat each other, so S is close to
singular: the generalised problem is solved by canonical orthogonalisation, which drops the directions of S that are noise."""

from __future__ import annotations

import numpy as np


def lowest_subspace_eigenvalue(S, H, rcond: float = 1e-8):
    """``(eigenvalue, coefficients, rank, s_min_kept)`` of the pencil (H, S).

    Both matrices are Hermitised (``(A + A^H) / 2``: the device returns them raw).  S is eigendecomposed and the eigenvectors
    with eigenvalues above ``rcond * s_max`` are kept; ``rank`` is their number and ``s_min_kept`` the smallest of the kept
    eigenvalues.  H is projected on them, scaled by ``1 / sqrt(s)``, and the lowest eigenvalue of the projection is returned
    with its vector as coefficients over the ORIGINAL states, normalised to ``c^H S c = 1``.  A state that repeats another one
    adds a zero eigenvalue to S and is dropped this way: the rank falls by one, the eigenvalue stays.

    The eigenvalue's error grows as (entry error) * sum_k|c_k| / s_min_kept, c_k the operator's coefficients: the entries of
    H are as large as the operator's norm, and the scaling by ``1 / sqrt(s)`` on both sides multiplies their error by up to
    ``1 / s_min_kept``.  Choose ``rcond`` so that ``rcond * s_max`` stays well above the entries' error times the size of S."""
    S = np.asarray(S, dtype=np.complex128)
    H = np.asarray(H, dtype=np.complex128)
    if S.ndim != 2 or S.shape[0] != S.shape[1] or S.shape != H.shape or S.shape[0] == 0:
        raise ValueError("S and H must be square matrices of the same, non-zero size")
    if not rcond > 0:
        raise ValueError("rcond must be positive")
    if not (np.all(np.isfinite(S)) and np.all(np.isfinite(H))):
        raise ValueError("S and H must be finite")
    S = (S + S.conj().T) / 2
    H = (H + H.conj().T) / 2
    s, u = np.linalg.eigh(S)
    s_max = float(s[-1])
    if not s_max > 0:
        raise ValueError("S has no positive eigenvalue: these are not overlaps of states")
    keep = s > rcond * s_max
    x = u[:, keep] / np.sqrt(s[keep])
    projected = x.conj().T @ H @ x
    projected = (projected + projected.conj().T) / 2
    e, y = np.linalg.eigh(projected)
    return float(e[0]), x @ y[:, 0], int(np.count_nonzero(keep)), float(s[keep][0])
