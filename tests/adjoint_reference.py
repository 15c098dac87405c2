"""The adjoint sweep of DESIGN.md 4.12 in vectorised NumPy (test helper, no tests), usable up to n = 16, and
``qsv_adjoint_describe`` read back as Python values.

E = Re<psi|H|psi>, psi = U_G .. U_1 |0..0> (oracle.statevector_oracle.simulate), H_h the Hermitian part of H applied term by
term.  psi_G = psi, lambda_G = H_h psi; for g = G .. 1: psi_(g-1) = U_g^dagger psi_g, every angle slot of gate g that reads a
parameter adds 2 Re<lambda_g| dU_g/d(slot) |psi_(g-1)> to that parameter's entry (cu3: the derivative's control-0 block is
zero), then lambda_(g-1) = U_g^dagger lambda_g.  id gates and literal angles add nothing.

For larger registers see tests/factorised_reference.py: product circuits whose gradients factorise block by block."""

from __future__ import annotations

import ctypes as C

import numpy as np

import dense_gradient
from oracle import statevector_oracle as so
from queasars_amd import _lib
from queasars_amd.ir import OP_CU3, OP_ID, CircuitIR, PauliOperator


def apply_hermitian_part(operator: PauliOperator, state: np.ndarray) -> np.ndarray:
    """sum_k real(c_k) P_k |state>, P = i^ny X^x Z^z: (P psi)_i = (-i)^ny (-1)^popcount(i & z) psi_(i ^ x)."""
    idx = np.arange(state.shape[0], dtype=np.int64)
    out = np.zeros_like(state)
    for x, z, c in zip(operator.x_mask, operator.z_mask, operator.coeffs):
        x, z = int(x), int(z)
        parity = np.zeros_like(idx)
        for q in range(operator.num_qubits):
            if (z >> q) & 1:
                parity ^= (idx >> q) & 1
        ny = bin(x & z).count("1")
        out += (complex(c).real * (-1j) ** (ny % 4)) * ((1.0 - 2.0 * parity) * state[idx ^ x])
    return out


def _pairs(state: np.ndarray, n: int, target: int, control: int):
    """Views of the lower and upper elements of every target pair, and the pairs the gate acts on (control bit 1)."""
    v = state.reshape(1 << (n - target - 1), 2, 1 << target)
    if control < 0:
        return v[:, 0, :], v[:, 1, :], None
    low = np.arange(1 << n, dtype=np.int64).reshape(v.shape)[:, 0, :]
    return v[:, 0, :], v[:, 1, :], ((low >> control) & 1) == 1


def _apply_in_place(state: np.ndarray, n: int, target: int, control: int, m: np.ndarray) -> None:
    a0, a1, on = _pairs(state, n, target, control)
    b0 = m[0, 0] * a0 + m[0, 1] * a1
    b1 = m[1, 0] * a0 + m[1, 1] * a1
    if on is None:
        a0[...], a1[...] = b0, b1
    else:
        a0[on], a1[on] = b0[on], b1[on]


def _derivative_term(lam: np.ndarray, psi: np.ndarray, n: int, target: int, control: int, d: np.ndarray) -> float:
    a0, a1, on = _pairs(psi, n, target, control)
    l0, l1, _ = _pairs(lam, n, target, control)
    w0 = d[0, 0] * a0 + d[0, 1] * a1
    w1 = d[1, 0] * a0 + d[1, 1] * a1
    terms = np.conj(l0) * w0 + np.conj(l1) * w1
    if on is not None:
        terms = terms[on]
    return 2.0 * float(np.real(terms.sum()))


def gradient_and_value(circuit: CircuitIR, params, operator: PauliOperator) -> tuple[np.ndarray, float]:
    """(dE / d params[p] for every parameter, E)."""
    n = circuit.n_qubits
    assert n <= 16
    ops = circuit.bound_ops(params)
    slots = [(int(row["p_theta"]), int(row["p_phi"]), int(row["p_lambda"])) for row in circuit.packed()]
    psi = np.array(so.simulate(n, ops), dtype=np.complex128)
    lam = apply_hermitian_part(operator, psi)
    value = float(np.real(np.vdot(psi, lam)))
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
    return out, value


def gradient(circuit: CircuitIR, params, operator: PauliOperator) -> np.ndarray:
    return gradient_and_value(circuit, params, operator)[0]


def describe(circuit: CircuitIR, wrt=None) -> dict:
    """``qsv_adjoint_describe``: {"runs": [(mask, first_op, last_op)], "n_gates", "tile_bits", "low_bits"}; ``wrt`` None: by every
    parameter."""
    lib = _lib.load()
    ops = circuit.packed()
    capacity = max(1, len(ops))
    masks = np.zeros(capacity, dtype=np.uint64)
    first, last = np.zeros(capacity, dtype=np.int32), np.zeros(capacity, dtype=np.int32)
    n_gates, tile_bits, low_bits = C.c_int64(-1), C.c_int32(-1), C.c_int32(-1)
    wrt_array = None if wrt is None else np.asarray(list(wrt) + [0], dtype=np.int32)  # (never an empty array: a null pointer)
    n_runs = lib.qsv_adjoint_describe(
        circuit.n_qubits, len(ops), _lib.as_ptr(ops), circuit.num_parameters, -1 if wrt is None else len(wrt),
        None if wrt is None else _lib.as_ptr(wrt_array), capacity, _lib.as_ptr(masks), _lib.as_ptr(first), _lib.as_ptr(last),
        C.byref(n_gates), C.byref(tile_bits), C.byref(low_bits))
    assert 0 <= n_runs <= capacity, n_runs
    return {"runs": [(int(masks[r]), int(first[r]), int(last[r])) for r in range(n_runs)], "n_gates": int(n_gates.value),
            "tile_bits": int(tile_bits.value), "low_bits": int(low_bits.value)}
