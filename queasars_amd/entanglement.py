"""What a state looks like on a few qubits: entropies, mutual information, marginal distributions and local expectation values
from reduced density matrices.  NumPy only: the matrices come from an evaluator's
``reduced_density_matrices`` (``OperatorCircuitEvaluator``; anything with that method will do), everything here is host work on
arrays of at most 16 x 16.

A subset's row index carries the subset's j-th qubit in bit j, as the device returns it."""

from __future__ import annotations

from itertools import combinations
from typing import Sequence

import numpy as np


def von_neumann_entropy(rho: np.ndarray, base: float = 2) -> float:
    """``-Tr rho log rho`` of a density matrix, in units of ``log(base)`` (bits by default).  The matrix is Hermitised and
    divided by its trace, so a raw matrix of a state that is normalised to rounding only will do; eigenvalues at or below zero
    contribute nothing (0 log 0 = 0)."""
    rho = np.asarray(rho, dtype=np.complex128)
    if rho.ndim != 2 or rho.shape[0] != rho.shape[1]:
        raise ValueError(f"a density matrix is square, not of shape {rho.shape}")
    values = np.linalg.eigvalsh((rho + rho.conj().T) / 2)
    trace = values.sum()
    if not trace > 0:
        raise ValueError("a density matrix has a positive trace")
    values = values / trace
    values = values[values > 0]
    return float(-(values * np.log(values)).sum() / np.log(base))


def marginal_distribution(rho: np.ndarray) -> np.ndarray:
    """The distribution of the subset's qubits in the computational basis: the real diagonal, entry a the probability of
    the setting whose bit j is the subset's j-th qubit."""
    return np.real(np.diagonal(np.asarray(rho), axis1=-2, axis2=-1)).copy()


def local_expectation(rho: np.ndarray, matrix: np.ndarray) -> complex:
    """``Tr(rho O)`` for an operator ``O`` on the subset's qubits, a ``2**k x 2**k`` matrix in the same index convention (bit j
    of an index: the subset's j-th qubit) -- so ``np.kron(O_1, O_0)`` for ``O_0`` on the subset's first qubit."""
    rho, matrix = np.asarray(rho), np.asarray(matrix)
    if rho.shape != matrix.shape:
        raise ValueError(f"the operator's matrix has shape {matrix.shape}, the density matrix {rho.shape}")
    return complex(np.einsum("ab,ba->", rho, matrix))


def _single_entropies(singles: Sequence[np.ndarray], base: float) -> np.ndarray:
    """(n, n_qubits) entropies from the single-qubit matrices, one (n, 2, 2) array per qubit."""
    n = singles[0].shape[0]
    return np.asarray([[von_neumann_entropy(rho[e], base) for rho in singles] for e in range(n)], dtype=np.float64).reshape(n, len(singles))


def qubit_entropies(evaluator, circuits: Sequence, parameter_values: Sequence, base: float = 2) -> np.ndarray:
    """The entanglement entropy of every qubit with the rest of the register, per circuit: an ``(n, n_qubits)`` array, from
    one ``reduced_density_matrices`` call over the single qubits."""
    n_qubits = int(evaluator.n_qubits)
    return _single_entropies(evaluator.reduced_density_matrices(circuits, parameter_values, [(q,) for q in range(n_qubits)]), base)


def mutual_information(evaluator, circuits: Sequence, parameter_values: Sequence, base: float = 2, with_entropies: bool = False):
    """The quantum mutual information ``I_ij = S_i + S_j - S_ij`` between every two qubits, per circuit: an ``(n, n_qubits,
    n_qubits)`` array, symmetric with a zero diagonal, from ONE ``reduced_density_matrices`` call over all single qubits and
    pairs.  With ``with_entropies`` the pair ``(qubit entropies, mutual information)``."""
    n_qubits = int(evaluator.n_qubits)
    pairs = list(combinations(range(n_qubits), 2))
    matrices = evaluator.reduced_density_matrices(circuits, parameter_values, [(q,) for q in range(n_qubits)] + pairs)
    single = _single_entropies(matrices[:n_qubits], base)
    n = single.shape[0]
    information = np.zeros((n, n_qubits, n_qubits), dtype=np.float64)
    for rho, (i, j) in zip(matrices[n_qubits:], pairs):
        for e in range(n):
            information[e, i, j] = information[e, j, i] = single[e, i] + single[e, j] - von_neumann_entropy(rho[e], base)
    return (single, information) if with_entropies else information


def marginal_distributions(evaluator, circuits: Sequence, parameter_values: Sequence, subsets: Sequence[Sequence[int]]) -> list[list[dict[str, float]]]:
    """Per circuit and subset ``{bitstring: probability}`` over all ``2**k`` settings of the subset's qubits, the subset's first
    qubit LAST in the bitstring, as ``most_probable_states`` spells the whole register."""
    subsets = [tuple(subset) for subset in subsets]
    matrices = evaluator.reduced_density_matrices(circuits, parameter_values, subsets)
    n = matrices[0].shape[0] if matrices else 0
    result = []
    for e in range(n):
        row = []
        for subset, rho in zip(subsets, matrices):
            k = len(subset)
            row.append({format(a, f"0{k}b"): float(p) for a, p in enumerate(marginal_distribution(rho[e]))})
        result.append(row)
    return result
