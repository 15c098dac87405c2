"""The exact CVaR's gradient of DESIGN.md 4.20 in vectorised NumPy (test helper, no tests), usable up to n = 16.

The documented rule, restated: the basis states sorted ascending by (value, index) -- a stable ``argsort`` of the values --,
``target = alpha - (1e-8 + 1e-5 |alpha|)``, ``b`` the first rank whose cumulative mass ``cum_b >= target`` (the last rank where
none has), ``t = v_b`` and ``s = max(alpha - cum_b, 0)``; the seed ``lambda = diag(w) psi`` with ``w_i = -max(t - v_i, 0) / alpha``;
the reverse sweep of tests/adjoint_reference.py from that seed; the value ``t (1 - s / alpha) + Re<psi|lambda>``.

Two margins say how far a case is from where the rule itself is discontinuous: the KINK margin ``min(alpha - cum_(b-1),
cum_b - alpha)`` (positive: the CVaR is differentiable there and the gradient is its derivative) and the IDENTIFICATION margin
``min(target - cum_(b-1), cum_b - target)`` (how much rounding of the cumulative mass it takes to move the boundary)."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import dense_gradient
from adjoint_reference import _apply_in_place, _derivative_term
from oracle import statevector_oracle as so
from queasars_amd.circuit_evaluation.expectation_calculation import basis_state_values
from queasars_amd.ir import OP_CU3, OP_ID, CircuitIR, PauliOperator


@dataclass
class CVaRCase:
    gradient: np.ndarray
    value: float
    threshold: float
    left_out: float  # s
    boundary: int  # b, a rank
    weights: np.ndarray  # w, by basis state
    kink_margin: float
    identification_margin: float

    @property
    def weight_norm(self) -> float:
        return float(np.max(np.abs(self.weights)))


def diagonal_values(operator: PauliOperator) -> np.ndarray:
    """The operator's value on every basis state: the terms added in their order, as the device's table adds them."""
    assert operator.is_diagonal()
    return basis_state_values(np.arange(1 << operator.num_qubits, dtype=np.uint64), operator)


def boundary(probabilities: np.ndarray, values: np.ndarray, alpha: float):
    """(b, t, s, kink margin, identification margin) of a distribution over the basis states."""
    order = np.argsort(values, kind="stable")
    cum = np.cumsum(probabilities[order])
    target = alpha - (1e-8 + 1e-5 * abs(alpha))
    reached = np.nonzero(cum >= target)[0]
    b = int(reached[0]) if reached.size else len(cum) - 1
    before = float(cum[b - 1]) if b > 0 else 0.0
    at = float(cum[b])
    return (b, float(values[order[b]]), max(alpha - at, 0.0), min(alpha - before, at - alpha), min(target - before, at - target))


def state_and_values(circuit: CircuitIR, params, operator: PauliOperator):
    psi = np.array(so.simulate(circuit.n_qubits, circuit.bound_ops(params)), dtype=np.complex128)
    return psi, diagonal_values(operator)


def cvar_gradient(circuit: CircuitIR, params, operator: PauliOperator, alpha: float, state_type=np.complex128) -> CVaRCase:
    """``state_type=numpy.complex64``: the boundary from the probabilities of the state rounded to single precision, as a handle
    of that type finds it; everything else in double precision from the unrounded state."""
    n = circuit.n_qubits
    assert n <= 16
    ops = circuit.bound_ops(params)
    slots = [(int(row["p_theta"]), int(row["p_phi"]), int(row["p_lambda"])) for row in circuit.packed()]
    psi, values = state_and_values(circuit, params, operator)
    seen = psi.astype(state_type).astype(np.complex128)
    b, t, s, kink, identification = boundary(seen.real ** 2 + seen.imag ** 2, values, alpha)
    w = -np.maximum(t - values, 0.0) / alpha
    lam = w * psi
    value = t * (1.0 - s / alpha) + float(np.real(np.vdot(psi, lam)))
    out = np.zeros(circuit.num_parameters)
    for (kind, target, control, theta, phi, lamb), refs in zip(reversed(ops), reversed(slots)):
        if kind == OP_ID:
            continue
        target, control = int(target), int(control) if kind == OP_CU3 else -1
        inverse = so.u_matrix(theta, phi, lamb).conj().T
        _apply_in_place(psi, n, target, control, inverse)
        for slot, p in enumerate(refs):
            if p >= 0:
                out[p] += _derivative_term(lam, psi, n, target, control, dense_gradient.du_matrix(theta, phi, lamb, slot))
        _apply_in_place(lam, n, target, control, inverse)
    return CVaRCase(out, value, t, s, b, w, kink, identification)


def numpy_cvar(circuit: CircuitIR, params, operator: PauliOperator, alpha: float) -> float:
    """``_get_expectation`` on the oracle state's distribution: the reference's accumulation."""
    from queasars_amd.circuit_evaluation.expectation_calculation import _get_expectation

    psi, values = state_and_values(circuit, params, operator)
    p = psi.real ** 2 + psi.imag ** 2
    return _get_expectation([(i, float(p[i]), float(values[i])) for i in range(len(p))], alpha)
