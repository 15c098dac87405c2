"""The deflated (VQD) cost of DESIGN.md 4.18 in NumPy (test helper, no tests), usable up to n = 16.

C = <psi|H_h|psi> + sum_k beta_k |c_k|^2 with c_k = <phi_k|psi>, psi the oracle's state of the circuit, H_h the Hermitian part of
the operator (tests/dense_gradient.py::dense_operator's convention, applied term by term by tests/adjoint_reference.py) and
phi_k the kept states as dense vectors.  The gradient is tests/adjoint_reference.py's sweep started from the deflated seed
lambda_G = H_h psi + sum_k beta_k c_k phi_k, for which Re<psi|lambda_G> = C."""

from __future__ import annotations

import numpy as np

import adjoint_reference as ar
import dense_gradient
from oracle import statevector_oracle as so
from queasars_amd.ir import OP_CU3, OP_ID, CircuitIR, PauliOperator


def spread(operator: PauliOperator) -> float:
    return float(np.abs(operator.coeffs.real).sum())


def scale(operator: PauliOperator, betas) -> float:
    """sum |c| + sum |beta|: what the cost's absolute errors are measured in."""
    return spread(operator) + float(np.abs(np.asarray(betas, dtype=np.float64)).sum())


def terms(circuit: CircuitIR, params, operator: PauliOperator, kept, betas):
    """(C, E, c): the cost, the energy alone and the overlaps <phi_k|psi> as a complex (K,) array."""
    psi = np.array(so.simulate(circuit.n_qubits, circuit.bound_ops(params)), dtype=np.complex128)
    energy = float(np.real(np.vdot(psi, ar.apply_hermitian_part(operator, psi))))
    c = np.asarray([np.vdot(phi, psi) for phi in kept], dtype=np.complex128).reshape(len(kept))
    penalty = 0.0
    for beta, ck in zip(betas, c):
        penalty += float(beta) * (ck.real * ck.real + ck.imag * ck.imag)
    return energy + penalty, energy, c


def cost(circuit: CircuitIR, params, operator: PauliOperator, kept, betas) -> float:
    return terms(circuit, params, operator, kept, betas)[0]


def gradient_and_terms(circuit: CircuitIR, params, operator: PauliOperator, kept, betas):
    """(dC / d params[p] for every parameter, C, E, c)."""
    n = circuit.n_qubits
    assert n <= 16
    ops = circuit.bound_ops(params)
    slots = [(int(row["p_theta"]), int(row["p_phi"]), int(row["p_lambda"])) for row in circuit.packed()]
    psi = np.array(so.simulate(n, ops), dtype=np.complex128)
    lam = ar.apply_hermitian_part(operator, psi)
    energy = float(np.real(np.vdot(psi, lam)))
    c = np.asarray([np.vdot(phi, psi) for phi in kept], dtype=np.complex128).reshape(len(kept))
    for beta, ck, phi in zip(betas, c, kept):
        lam = lam + (float(beta) * ck) * np.asarray(phi, dtype=np.complex128)
    value = float(np.real(np.vdot(psi, lam)))
    out = np.zeros(circuit.num_parameters)
    for (kind, target, control, theta, phi_angle, lamb), refs in zip(reversed(ops), reversed(slots)):
        if kind == OP_ID:
            continue
        target, control = int(target), int(control) if kind == OP_CU3 else -1
        inverse = so.u_matrix(theta, phi_angle, lamb).conj().T
        ar._apply_in_place(psi, n, target, control, inverse)
        for slot, p in enumerate(refs):
            if p >= 0:
                out[p] += ar._derivative_term(lam, psi, n, target, control, dense_gradient.du_matrix(theta, phi_angle, lamb, slot))
        ar._apply_in_place(lam, n, target, control, inverse)
    return out, value, energy, c


def gradient(circuit: CircuitIR, params, operator: PauliOperator, kept, betas) -> np.ndarray:
    return gradient_and_terms(circuit, params, operator, kept, betas)[0]


def finite_differences(circuit: CircuitIR, params, operator: PauliOperator, kept, betas, h: float = 1e-6) -> np.ndarray:
    """Central differences of :func:`cost`, one entry per parameter."""
    params = [float(p) for p in params]
    out = np.zeros(len(params))
    for p in range(len(params)):
        up, down = list(params), list(params)
        up[p] += h
        down[p] -= h
        out[p] = (cost(circuit, up, operator, kept, betas) - cost(circuit, down, operator, kept, betas)) / (2.0 * h)
    return out


def deflated_matrix(operator: PauliOperator, kept, betas) -> np.ndarray:
    """H_h + sum_k beta_k |phi_k><phi_k|, dense (n <= 8): the cost of ANY normalised state is at least its lowest eigenvalue."""
    m = dense_gradient.dense_operator(operator).copy()
    for beta, phi in zip(betas, kept):
        phi = np.asarray(phi, dtype=np.complex128)
        m += float(beta) * np.outer(phi, phi.conj())
    return m
