"""References for overlaps and operator matrix elements between states, tests only: S = <phi|psi> = vdot(phi,
psi) and T = <phi|H_h|psi> = vdot(phi, H_h psi), raw, on the NumPy oracle's states, H_h the Hermitian part of the operator -- the
dense matrix of tests/dense_gradient.py up to eight qubits, the matrix-free strings of tests/variance_reference.py above;
tests/test_overlap_host.py holds the two to each other."""

from __future__ import annotations

import functools

import numpy as np

import helpers
import variance_reference as vr
from dense_gradient import dense_operator
from queasars_amd.ir import PauliOperator

#: |S - reference| per component in fp64: amplitudes after at most ~150 gates carry about 2e-14, the fixed-order sums included;
#: a hundred times that, rounded up
TOL_S = 1e-11
#: the project's fp32 floor
FP32_FLOOR = 2e-6


def spread(op: PauliOperator) -> float:
    return vr.spread(op)


def tol_t(op: PauliOperator) -> float:
    """|T - reference| per component in fp64: the bound of S with one operator norm."""
    return TOL_S * max(1.0, spread(op))


def tol_fp32(e_s: float) -> float:
    """|dS| on an fp32 handle, e_s the largest |psi_32 - psi_ref|_2 of the handle's statevector() over the test's own circuits:
    two state errors enter, with a factor two of room, and the project's fp32 floor."""
    return max(FP32_FLOOR, 4.0 * e_s)


def apply_operator(op: PauliOperator, state: np.ndarray, dense: bool | None = None) -> np.ndarray:
    """H_h |state>: dense up to eight qubits, matrix-free above (`dense` forces one form)."""
    if dense is None:
        dense = op.num_qubits <= 8
    return dense_operator(op) @ state if dense else vr.apply_strings(op, state)


def overlaps(kept_states, states) -> np.ndarray:
    """S[e, k] = <phi_k|psi_e>, an (n, K) complex array."""
    return np.asarray([[np.vdot(phi, psi) for phi in kept_states] for psi in states], dtype=np.complex128).reshape(len(states), len(kept_states))


def elements(op: PauliOperator, kept_states, states, dense: bool | None = None) -> np.ndarray:
    """T[e, k] = <phi_k|H_h|psi_e>."""
    if dense is None:
        dense = op.num_qubits <= 8
    if dense:
        matrix = dense_operator(op)  # (built once for all states)
        applied = [matrix @ psi for psi in states]
    else:
        applied = [vr.apply_strings(op, psi) for psi in states]
    return overlaps(kept_states, applied)


def max_component_error(got: np.ndarray, want: np.ndarray) -> float:
    d = np.asarray(got) - np.asarray(want)
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max())) if d.size else 0.0


@functools.lru_cache(maxsize=None)
def population(n: int, layers: int, count: int, seed: int, perturbed: bool = False):
    """(circuits, parameter values, oracle states) of `count` evaluations, computed once.  `perturbed`: the second half repeats
    the first half's circuits at slightly perturbed parameters, so that overlaps of order 1 occur (the overlaps of unrelated
    circuits fall with the register: the largest is 0.39 at n = 4 and 0.11 at n = 11)."""
    if not perturbed:
        return vr.population(n, layers, count, seed)
    first = (count + 1) // 2
    _, circuits, params = helpers.population_circuits(n, layers, first, seed=seed)
    rng = np.random.default_rng(77 + seed)
    circuits = list(circuits) + list(circuits[: count - first])
    params = [list(p) for p in params] + [[float(v + rng.normal(0.0, 0.05)) for v in p] for p in params[: count - first]]
    return circuits, params, [helpers.oracle_state(c, p) for c, p in zip(circuits, params)]
