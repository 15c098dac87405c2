"""The Fubini-Study metric of DESIGN.md 4.17 in NumPy (test helper, no tests), two ways.

G_ij = Re<d_i psi|d_j psi> - <d_i psi|psi><psi|d_j psi>, psi = U_G .. U_1 |0..0> (oracle.statevector_oracle.simulate).

``backward``: the sweep the device runs.  Every tangent is multiplied by (U_G .. U_1)^dagger, which changes no inner product:
for g = G .. 1, psi_(g-1) = U_g^dagger psi_g, every angle slot of gate g that reads a requested parameter gives birth to a column
dU_g/d(slot) psi_(g-1) (cu3: the derivative's control-0 block is zero), and every living column, the new ones included, is
multiplied by U_g^dagger; the sweep ends at the earliest gate that reads a requested parameter.  Then T = Re<xi_a|xi_b>,
b = Im<psi|xi_a>, per slot T - b b^T, per parameter the sum over its slots.
Vectorised over the columns; usable up to n = 17 with a few columns.

``forward``: independent of it -- each slot's derivative state U_G .. dU_k .. U_1 |0..0> built forwards with
dense_gradient._apply, summed into d_i psi, and the definition evaluated as it stands.  n <= 12.

For larger registers see tests/factorised_reference.py: product circuits whose metric is block diagonal."""

from __future__ import annotations

import numpy as np

import dense_gradient
from oracle import statevector_oracle as so
from queasars_amd.ir import OP_CU3, OP_ID, CircuitIR


def _slots(circuit: CircuitIR) -> list:
    return [(int(row["p_theta"]), int(row["p_phi"]), int(row["p_lambda"])) for row in circuit.packed()]


def slot_counts(circuit: CircuitIR) -> np.ndarray:
    """How many angle slots read each parameter (id gates read none)."""
    counts = np.zeros(circuit.num_parameters, dtype=np.int64)
    for row, refs in zip(circuit.packed(), _slots(circuit)):
        if int(row["kind"]) == OP_ID:
            continue
        for p in refs:
            if p >= 0:
                counts[p] += 1
    return counts


def _apply_rows(rows: np.ndarray, n: int, target: int, control: int, m: np.ndarray, derivative: bool = False) -> None:
    """m on `target` of every row of `rows` (shape (k, 2^n)), in place, where bit `control` is 1 (control >= 0); with
    ``derivative`` the control-0 block becomes zero."""
    v = rows.reshape(rows.shape[0], 1 << (n - target - 1), 2, 1 << target)
    a0, a1 = v[:, :, 0, :], v[:, :, 1, :]
    b0 = m[0, 0] * a0 + m[0, 1] * a1
    b1 = m[1, 0] * a0 + m[1, 1] * a1
    if control >= 0:
        low = np.arange(1 << n, dtype=np.int64).reshape(v.shape[1:])[:, 0, :]
        on = (((low >> control) & 1) == 1)[None, :, :]
        keep = 0.0 if derivative else 1.0
        b0 = np.where(on, b0, keep * a0)
        b1 = np.where(on, b1, keep * a1)
    a0[...], a1[...] = b0, b1


def _requested(circuit: CircuitIR, wrt) -> list:
    return list(range(circuit.num_parameters)) if wrt is None else [int(p) for p in wrt]


def backward(circuit: CircuitIR, params, wrt=None) -> np.ndarray:
    """G over the parameters ``wrt`` names (None: all), by the backward sweep."""
    n = circuit.n_qubits
    assert n <= 17
    wanted = _requested(circuit, wrt)
    ops = circuit.bound_ops(params)
    psi = np.array(so.simulate(n, ops), dtype=np.complex128).reshape(1, -1)
    columns = np.zeros((0, 1 << n), dtype=np.complex128)
    owner = []  # the parameter each column's slot reads
    slots = _slots(circuit)
    # the sweep may end at the earliest gate that reads a requested parameter: psi and the columns are then all at that gate's
    # time, and no inner product depends on the time
    readers = [k for k, (op, refs) in enumerate(zip(ops, slots)) if op[0] != OP_ID and any(p >= 0 and p in wanted for p in refs)]
    stop = min(readers, default=len(ops))
    for k in range(len(ops) - 1, stop - 1, -1):
        (kind, target, control, theta, phi, lamb), refs = ops[k], slots[k]
        if kind == OP_ID:
            continue
        target, control = int(target), int(control) if kind == OP_CU3 else -1
        inverse = so.u_matrix(theta, phi, lamb).conj().T
        _apply_rows(psi, n, target, control, inverse)
        born = [slot for slot, p in enumerate(refs) if p >= 0 and p in wanted]
        if born:
            new = np.repeat(psi, len(born), axis=0)
            for j, slot in enumerate(born):
                _apply_rows(new[j:j + 1], n, target, control, dense_gradient.du_matrix(theta, phi, lamb, slot), derivative=True)
                owner.append(refs[slot])
            columns = np.concatenate([columns, new], axis=0)
        if columns.shape[0]:
            _apply_rows(columns, n, target, control, inverse)
    t = np.real(columns.conj() @ columns.T)
    b = np.imag(columns @ psi[0].conj())
    per_slot = t - np.outer(b, b)
    owner = np.asarray(owner, dtype=np.int64)
    select = np.array([[1.0 if owner[c] == p else 0.0 for c in range(len(owner))] for p in wanted]).reshape(len(wanted), len(owner))
    return select @ per_slot @ select.T


def forward(circuit: CircuitIR, params, wrt=None) -> np.ndarray:
    """G over the parameters ``wrt`` names (None: all), from derivative states built forwards."""
    n = circuit.n_qubits
    assert n <= 12
    wanted = _requested(circuit, wrt)
    ops = circuit.bound_ops(params)
    psi = np.asarray(so.simulate(n, ops), dtype=np.complex128)
    tangents = np.zeros((circuit.num_parameters, 1 << n), dtype=np.complex128)
    for k, (op, refs) in enumerate(zip(ops, _slots(circuit))):
        kind, target, control, theta, phi, lamb = op
        if kind == OP_ID:
            continue
        before = None
        for slot, p in enumerate(refs):
            if p < 0 or p not in wanted:
                continue
            if before is None:
                before = np.asarray(so.simulate(n, ops[:k]), dtype=np.complex128)
            d = dense_gradient._apply(before, n, int(target), int(control) if kind == OP_CU3 else -1,
                                      dense_gradient.du_matrix(theta, phi, lamb, slot), kind == OP_CU3)
            tangents[p] += np.asarray(so.simulate(n, ops[k + 1:], initial_state=d), dtype=np.complex128)
    d = tangents[wanted]
    overlaps = d.conj() @ psi  # <d_i psi|psi>
    return np.real(d.conj() @ d.T) - np.real(np.outer(overlaps, overlaps.conj()))


def fidelity_second_difference(circuit: CircuitIR, params, v, eps: float = 1e-3) -> float:
    """(2 - F(x + eps v) - F(x - eps v)) / (2 eps^2) with F = |<psi(x)|psi(y)>|^2: v^T G v up to O(eps^2)."""
    n = circuit.n_qubits
    x, v = np.asarray(params, dtype=np.float64), np.asarray(v, dtype=np.float64)
    psi = np.asarray(so.simulate(n, circuit.bound_ops(x)))

    def fidelity(y):
        return abs(np.vdot(psi, np.asarray(so.simulate(n, circuit.bound_ops(y))))) ** 2

    return (2.0 - fidelity(x + eps * v) - fidelity(x - eps * v)) / (2.0 * eps * eps)
