"""Dense NumPy derivatives of expectation values, for small registers (tests only): the gate matrix itself is differentiated,
dE/da = 2 Re <psi|H|d psi/da>, so nothing here knows about shift rules.  n <= 8."""

from __future__ import annotations

import cmath
import math

import numpy as np

from oracle import statevector_oracle as so
from queasars_amd.ir import OP_CU3, OP_ID, CircuitIR, PauliOperator


def du_matrix(theta: float, phi: float, lam: float, slot: int) -> np.ndarray:
    """d U(theta, phi, lam) / d (theta, phi, lam)[slot], U as Qiskit's UGate (oracle.statevector_oracle.u_matrix)."""
    c, s = math.cos(theta / 2.0), math.sin(theta / 2.0)
    ep, el, epl = cmath.exp(1j * phi), cmath.exp(1j * lam), cmath.exp(1j * (phi + lam))
    if slot == 0:
        return np.array([[-s / 2, -el * c / 2], [ep * c / 2, -epl * s / 2]], dtype=np.complex128)
    if slot == 1:
        return np.array([[0, 0], [1j * ep * s, 1j * epl * c]], dtype=np.complex128)
    return np.array([[0, -1j * el * s], [0, 1j * epl * c]], dtype=np.complex128)


def _apply(state: np.ndarray, n: int, target: int, control: int, m: np.ndarray, controlled_derivative: bool = False) -> np.ndarray:
    """m on `target` (where bit `control` is 1, if control >= 0).  controlled_derivative: the control = 0 block is the
    derivative of the identity, i.e. 0."""
    idx = np.arange(1 << n)
    low = idx[(idx >> target) & 1 == 0]
    high = low | (1 << target)
    out = state.copy()
    new_low = m[0, 0] * state[low] + m[0, 1] * state[high]
    new_high = m[1, 0] * state[low] + m[1, 1] * state[high]
    if control < 0:
        out[low], out[high] = new_low, new_high
        return out
    on = (low >> control) & 1 == 1
    out[low[on]], out[high[on]] = new_low[on], new_high[on]
    if controlled_derivative:
        out[low[~on]] = 0.0
        out[high[~on]] = 0.0
    return out


def dense_operator(operator: PauliOperator) -> np.ndarray:
    n = operator.num_qubits
    h = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for label, coeff in zip(operator.labels, operator.coeffs):
        h += coeff * so.dense_pauli(label)
    return 0.5 * (h + h.conj().T)  # (the evaluators return the real part: the Hermitian part's expectation)


def expectation(circuit: CircuitIR, params, h: np.ndarray) -> float:
    psi = so.simulate(circuit.n_qubits, circuit.bound_ops(params))
    return float(np.real(np.vdot(psi, h @ psi)))


def gradient(circuit: CircuitIR, params, h: np.ndarray) -> np.ndarray:
    """d real(<psi|H|psi>) / d params[p] for every parameter, summed over every angle slot that reads it."""
    assert circuit.n_qubits <= 8
    n = circuit.n_qubits
    ops = circuit.bound_ops(params)
    slots = [(int(row["p_theta"]), int(row["p_phi"]), int(row["p_lambda"])) for row in circuit.packed()]
    psi = so.simulate(n, ops)
    h_psi = h @ psi
    out = np.zeros(circuit.num_parameters)
    for k, (op, refs) in enumerate(zip(ops, slots)):
        kind, target, control, theta, phi, lam = op
        if kind == OP_ID:
            continue
        for slot, p in enumerate(refs):
            if p < 0:
                continue
            d = so.simulate(n, ops[:k])
            d = _apply(d, n, int(target), int(control) if kind == OP_CU3 else -1, du_matrix(theta, phi, lam, slot), kind == OP_CU3)
            d = so.simulate(n, ops[k + 1:], initial_state=d)
            out[p] += 2.0 * float(np.real(np.vdot(h_psi, d)))
    return out
