"""References for operator-weighted reduced density matrices, tests only: W_A = Tr_rest(H_h |psi><psi|) of a
NumPy oracle state from lambda = H_h psi (overlap_reference.apply_operator) by the reshape of rdm_reference.reduced_density_matrix,
raw; the derivatives at identity of the gates a layer can hold, written down here on their own (queasars_amd/evqe/growth.py is held
to them, not used); the gradients of appended gates and of Pauli generators; and, for product circuits, the factorised form.  Bit j
of a row index is the value of the subset's j-th qubit.  tests/test_operator_density_host.py holds this to facts."""

from __future__ import annotations

import functools

import numpy as np

import factorised_reference as fr
import overlap_reference as ovr
import rdm_reference as rr
from operator_families import from_masks
from queasars_amd.ir import PauliOperator

#: dV/ds at 0 of Qiskit's u(theta, phi, lambda) = [[cos(theta/2), -e^(i lambda) sin(theta/2)], [e^(i phi) sin(theta/2),
#: e^(i (phi + lambda)) cos(theta/2)]] by theta, phi and lambda
D_THETA = np.array([[0.0, -0.5], [0.5, 0.0]], dtype=np.complex128)
D_PHI = np.array([[0.0, 0.0], [0.0, 1.0j]], dtype=np.complex128)
D_LAMBDA = np.array([[0.0, 0.0], [0.0, 1.0j]], dtype=np.complex128)
DERIVATIVES = (D_THETA, D_PHI, D_LAMBDA)

PAULI = {"I": np.eye(2, dtype=np.complex128), "X": np.array([[0, 1], [1, 0]], dtype=np.complex128),
         "Y": np.array([[0, -1j], [1j, 0]], dtype=np.complex128), "Z": np.array([[1, 0], [0, -1]], dtype=np.complex128)}


def tol(op: PauliOperator) -> float:
    """|W - reference| per component in fp64: the project's bound for <phi|H|psi>, the same kind of sum."""
    return ovr.tol_t(op)


def _panel(state: np.ndarray, subset) -> np.ndarray:
    """The state as a 2^k x 2^(n-k) matrix, rows indexed by the subset's bits (rdm_reference.reduced_density_matrix's reshape)."""
    state = np.asarray(state, dtype=np.complex128)
    n = int(state.size).bit_length() - 1
    assert state.size == 1 << n
    subset = [int(q) for q in subset]
    k = len(subset)
    assert 1 <= k <= n and len(set(subset)) == k and all(0 <= q < n for q in subset)
    rest = [q for q in range(n - 1, -1, -1) if q not in subset]
    axes = [n - 1 - q for q in reversed(subset)] + [n - 1 - q for q in rest]
    return state.reshape((2,) * n).transpose(axes).reshape(1 << k, 1 << (n - k))


def cross_matrix(lam: np.ndarray, psi: np.ndarray, subset) -> np.ndarray:
    """sum_b lam(a, b) conj psi(a', b)."""
    return np.einsum("ab,cb->ac", _panel(lam, subset), _panel(psi, subset).conj())


def operator_density_matrix(op: PauliOperator, state: np.ndarray, subset, lam=None) -> np.ndarray:
    lam = ovr.apply_operator(op, state) if lam is None else lam
    return cross_matrix(lam, state, subset)


def operator_density_matrices(op: PauliOperator, states, subsets) -> list[np.ndarray]:
    """One (len(states), 2^k, 2^k) array per subset, as the device method returns them."""
    lams = [ovr.apply_operator(op, s) for s in states]
    return [np.stack([cross_matrix(lam, s, subset) for lam, s in zip(lams, states)]) for subset in subsets]


def values(op: PauliOperator, states) -> np.ndarray:
    return np.asarray([float(np.real(np.vdot(s, ovr.apply_operator(op, s)))) for s in states])


def largest_error(got_list, want_list) -> float:
    return rr.largest_error(got_list, want_list)


# ---- gradients of what is appended at identity ----------------------------------------------------------------------------------


def rate(derivative: np.ndarray, w: np.ndarray) -> float:
    """dE/ds = 2 Re sum D[a][a'] conj W[a][a']."""
    return float(2.0 * np.real(np.sum(derivative * np.conj(w))))


def controlled(derivative: np.ndarray, control_bit: int) -> np.ndarray:
    """The derivative of the controlled gate on an ordered pair: `derivative` on the target at the rows and columns whose control
    bit (bit `control_bit` of the row index) is 1, zero elsewhere."""
    out = np.zeros((4, 4), dtype=np.complex128)
    t_bit = 1 - control_bit
    for a in range(4):
        for b in range(4):
            if (a >> control_bit) & 1 and (b >> control_bit) & 1:
                out[a, b] = derivative[(a >> t_bit) & 1, (b >> t_bit) & 1]
    return out


def u_gradients(op: PauliOperator, state: np.ndarray) -> np.ndarray:
    """(Q, 3): u appended on qubit q, by theta, phi, lambda."""
    n = op.num_qubits
    lam = ovr.apply_operator(op, state)
    return np.asarray([[rate(d, cross_matrix(lam, state, (q,))) for d in DERIVATIVES] for q in range(n)]).reshape(n, 3)


def cu3_gradients(op: PauliOperator, state: np.ndarray) -> np.ndarray:
    """(Q, Q, 3): cu3 appended with control c and target t at [c, t]; zeros on the diagonal."""
    n = op.num_qubits
    lam = ovr.apply_operator(op, state)
    out = np.zeros((n, n, 3))
    for c in range(n):
        for t in range(n):
            if c != t:
                w = cross_matrix(lam, state, (c, t))  # (the control is bit 0 of the row index)
                out[c, t] = [rate(controlled(d, 0), w) for d in DERIVATIVES]
    return out


def pauli_on(label: str) -> np.ndarray:
    """The matrix of a string whose j-th letter acts on the subset's j-th qubit."""
    m = np.ones((1, 1), dtype=np.complex128)
    for letter in label:
        m = np.kron(PAULI[letter], m)
    return m


def pool_gradient(op: PauliOperator, state: np.ndarray, label: str, qubits, lam=None) -> float:
    """dE/dtheta at 0 of exp(-i theta P / 2) appended: D = -i P / 2."""
    return rate(-0.5j * pauli_on(label), operator_density_matrix(op, state, qubits, lam))


def random_generators(n: int, count: int, seed: int) -> list[tuple[str, tuple[int, ...]]]:
    """`count` generators of weight 1 to min(4, n), no identity letters, qubits in random order."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        k = int(rng.integers(1, min(4, n) + 1))
        qubits = tuple(int(q) for q in rng.choice(n, size=k, replace=False))
        out.append(("".join(rng.choice(list("XYZ"), size=k)), qubits))
    return out


# ---- operators --------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def general_operator(n: int, seed: int = 0, n_terms: int = 14) -> PauliOperator:
    """Strings of every kind over the register with COMPLEX coefficients, so that H_h != H: X, Y and Z on the top qubit and on
    qubit 0, x masks of weight up to three, a constant."""
    rng = np.random.default_rng(4190 + 31 * n + seed)
    top = 1 << (n - 1)
    terms = {(0, 0): 0.25 + 0.5j, (top, 0): 0.7 - 0.2j, (top, top): -0.6 + 0.3j, (0, top): 0.8 + 0.1j, (1, 0): -0.5 + 0.4j, (0, 1): 0.9 - 0.7j}
    for _ in range(20 * n_terms):
        if len(terms) >= n_terms:
            break
        x = sum(1 << int(q) for q in rng.choice(n, size=int(rng.integers(0, min(3, n) + 1)), replace=False))
        z = sum(1 << int(q) for q in rng.choice(n, size=int(rng.integers(0, min(3, n) + 1)), replace=False))
        terms.setdefault((x, z), complex(rng.uniform(-1, 1), rng.uniform(-1, 1)))
    return from_masks(n, [(x, z, c) for (x, z), c in terms.items()])


# ---- the factorised form ------------------------------------------------------------------------------------------------------------


def factorised_matrix(op: PauliOperator, f: fr.Factorised, subset) -> np.ndarray:
    """W_A of a state factorised over blocks: W_A = sum_t c_t [prod over the blocks b outside A of <psi_b|P_t^b|psi_b>] times the
    reordered Kronecker product over the blocks touching A of Tr_rest (P_t^b psi_b) psi_b^H."""
    subset = tuple(int(q) for q in subset)
    owner = {q: b for b, qubits in enumerate(f.blocks) for q in qubits}
    touching = sorted({owner[q] for q in subset})
    outside = [b for b in range(len(f.blocks)) if b not in touching]
    terms = fr._terms(op)
    factors = f.factors(terms)  # (terms, blocks): <psi_b|P_t^b|psi_b>
    out = np.zeros((1 << len(subset),) * 2, dtype=np.complex128)
    for t, (x, z, c) in enumerate(terms):
        weight = c * np.prod(factors[t, outside]) if outside else c
        parts = []
        for b in touching:
            mine = [q for q in subset if owner[q] == b]
            local = [f.blocks[b].index(q) for q in mine]
            parts.append((cross_matrix(f.applied(b, x, z), f.states[b], local), mine))
        out += weight * rr.kron_reordered(parts, subset)
    return out
