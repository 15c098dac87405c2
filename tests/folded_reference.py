"""The folded-spectrum and variance costs of DESIGN.md 4.21 in NumPy (test helper, no tests), usable up to n = 16.

F = <psi|(H_h - c)^2|psi> with psi the oracle's state of the circuit, H_h the Hermitian part of the operator applied term by
term (tests/adjoint_reference.py::apply_hermitian_part) and c the centre: a target, or (``target=None``) E = Re<psi|H_h psi>.
r = H_h psi - c psi, cost = |r|^2, and the gradient is tests/adjoint_reference.py's sweep started from lambda_G =
H_h r - c r, c held fixed."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import adjoint_reference as ar
import dense_gradient
from oracle import statevector_oracle as so
from queasars_amd.ir import OP_CU3, OP_ID, CircuitIR, PauliOperator


def spread(operator: PauliOperator) -> float:
    return float(np.abs(operator.coeffs.real).sum())


def seed_norm(operator: PauliOperator, centre: float) -> float:
    """(sum |c_k| + |c|)^2: a bound of |(H_h - c)^2|, what the sweep's errors are measured in."""
    return (spread(operator) + abs(float(centre))) ** 2


@dataclass
class FoldedCase:
    gradient: np.ndarray
    cost: float      # |r|^2
    energy: float    # E
    centre: float    # c


def state(circuit: CircuitIR, params) -> np.ndarray:
    return np.array(so.simulate(circuit.n_qubits, circuit.bound_ops(params)), dtype=np.complex128)


def cost_and_energy(circuit: CircuitIR, params, operator: PauliOperator, target=None) -> tuple[float, float]:
    psi = state(circuit, params)
    lam = ar.apply_hermitian_part(operator, psi)
    energy = float(np.real(np.vdot(psi, lam)))
    c = energy if target is None else float(target)
    r = lam - c * psi
    return float(np.real(np.vdot(r, r))), energy


def cost(circuit: CircuitIR, params, operator: PauliOperator, target=None) -> float:
    return cost_and_energy(circuit, params, operator, target)[0]


def folded(circuit: CircuitIR, params, operator: PauliOperator, target=None) -> FoldedCase:
    n = circuit.n_qubits
    assert n <= 16
    ops = circuit.bound_ops(params)
    slots = [(int(row["p_theta"]), int(row["p_phi"]), int(row["p_lambda"])) for row in circuit.packed()]
    psi = np.array(so.simulate(n, ops), dtype=np.complex128)
    lam1 = ar.apply_hermitian_part(operator, psi)
    energy = float(np.real(np.vdot(psi, lam1)))
    c = energy if target is None else float(target)
    r = lam1 - c * psi
    value = float(np.real(np.vdot(r, r)))
    lam = ar.apply_hermitian_part(operator, r) - c * r
    out = np.zeros(circuit.num_parameters)
    for (kind, tgt, control, theta, phi, lamb), refs in zip(reversed(ops), reversed(slots)):
        if kind == OP_ID:
            continue
        tgt, control = int(tgt), int(control) if kind == OP_CU3 else -1
        inverse = so.u_matrix(theta, phi, lamb).conj().T
        ar._apply_in_place(psi, n, tgt, control, inverse)
        for slot, p in enumerate(refs):
            if p >= 0:
                out[p] += ar._derivative_term(lam, psi, n, tgt, control, dense_gradient.du_matrix(theta, phi, lamb, slot))
        ar._apply_in_place(lam, n, tgt, control, inverse)
    return FoldedCase(out, value, energy, c)


def finite_differences(circuit: CircuitIR, params, operator: PauliOperator, target=None, h: float = 1e-6) -> np.ndarray:
    """Central differences of :func:`cost`, one entry per parameter; ``target=None``: of the variance itself, its centre moving
    with the point."""
    params = [float(p) for p in params]
    out = np.zeros(len(params))
    for p in range(len(params)):
        up, down = list(params), list(params)
        up[p] += h
        down[p] -= h
        out[p] = (cost(circuit, up, operator, target) - cost(circuit, down, operator, target)) / (2.0 * h)
    return out


def folded_matrix(operator: PauliOperator, centre: float) -> np.ndarray:
    """(H_h - c)^2, dense (n <= 8)."""
    m = dense_gradient.dense_operator(operator) - float(centre) * np.eye(1 << operator.num_qubits)
    return m @ m
