"""Operator families outside the benchmark's shapes (test helpers, no tests): seeded, pure generators of ``PauliOperator``s that
are not "all pairs of Z" or "uniform over IXYZ" -- strings of weight one and two, long Z runs between two X or Y factors, hundreds
of strings under one x mask (pauli_groups_kernel's chunks of kChunk, an observable set's rows of kObsChunk), every Z string on
ten qubits, the all-X / all-Y / all-Z strings and the lowest and highest pivots, terms placed relative to a split circuit's two
sides and its keys, unweighted cuts whose values tie by the thousand, and untidy lists (repeated strings, a zero, imaginary
parts, coefficients over nine decades).

The same arguments give the same operator (``circuit_families._rng``).  ``groups_of`` and ``rows_of`` restate the grouping of
qsv_set_operator and the row cutting of qsv_observables_create, so that a test can say which regime an operator reaches.
"""

from __future__ import annotations

import numpy as np

from circuit_families import _rng
from queasars_amd.ir import PauliOperator

# pauli_groups_kernel's chunk of one group's terms (kernels.hip kChunk), pauli_terms_kernel's row (kernels.hpp kObsChunk)
K_CHUNK, K_OBS_CHUNK = 256, 512
# the sizes one_group is asked for: both sides of a chunk, a third (partial) chunk, both sides of a row; and 2^10, every z mask
GROUP_COUNTS = (K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 2 * K_CHUNK + 1, K_OBS_CHUNK, K_OBS_CHUNK + 1)
X_MASK_NAMES = ("low", "high", "ones", "random")


def from_masks(n: int, terms) -> PauliOperator:
    """The operator of [(x mask, z mask, coefficient)] (bit q of a mask = qubit q; x and z both set: Y)."""
    chars = "IZXY"
    labels = ["".join(chars[2 * ((int(x) >> q) & 1) + ((int(z) >> q) & 1)] for q in range(n - 1, -1, -1)) for x, z, _ in terms]
    return PauliOperator(labels, [c for _, _, c in terms])


def masks_of(op: PauliOperator):
    return [(int(x), int(z), complex(c)) for x, z, c in zip(op.x_mask, op.z_mask, op.coeffs)]


def _bits(mask: int) -> list[int]:
    return [q for q in range(mask.bit_length()) if (mask >> q) & 1]


def _string(qubits, kinds) -> tuple[int, int]:
    x = z = 0
    for q, kind in zip(qubits, kinds):
        x |= (kind in "XY") << int(q)
        z |= (kind in "ZY") << int(q)
    return x, z


def _bonds(n: int, periodic: bool):
    return [(q, q + 1) for q in range(n - 1)] + ([(n - 1, 0)] if periodic and n > 2 else [])


def transverse_ising(n: int, periodic: bool = False) -> PauliOperator:
    """ZZ on neighbours, an X field on every qubit: a diagonal part and n groups of one weight-1 string, every pivot 0 .. n-1."""
    rng = _rng("transverse_ising", n, periodic)
    terms = [(0, (1 << a) | (1 << b), float(rng.normal())) for a, b in _bonds(n, periodic)]
    terms += [(1 << q, 0, float(rng.normal())) for q in range(n)]
    return from_masks(n, terms)


def heisenberg(n: int, periodic: bool = False) -> PauliOperator:
    """XX + YY + ZZ on neighbours (a coupling of its own each) and Z fields: XX and YY share an x mask, ny = 0 and 2."""
    rng = _rng("heisenberg", n, periodic)
    terms = []
    for a, b in _bonds(n, periodic):
        pair = (1 << a) | (1 << b)
        terms += [(pair, 0, float(rng.normal())), (pair, pair, float(rng.normal())), (0, pair, float(rng.normal()))]
    terms += [(0, 1 << q, float(rng.normal())) for q in range(n)]
    return from_masks(n, terms)


def hopping(n: int, n_terms: int) -> PauliOperator:
    """Jordan-Wigner-like: for n_terms random pairs i < j the strings X_i Z_{i+1..j-1} X_j and Y_i Z.. Y_j (one x mask, ny = 0
    and 2, a Z run of any length) and the number terms Z_i Z_j; Z_i on every qubit."""
    rng = _rng("hopping", n, n_terms)
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    chosen = [pairs[int(k)] for k in rng.choice(len(pairs), size=min(n_terms, len(pairs)), replace=False)]
    terms = []
    for a, b in chosen:
        ends = (1 << a) | (1 << b)
        run = ((1 << b) - 1) & ~((1 << (a + 1)) - 1)
        terms += [(ends, run, float(rng.normal())), (ends, run | ends, float(rng.normal())), (0, ends, float(rng.normal()))]
    terms += [(0, 1 << q, float(rng.normal())) for q in range(n)]
    return from_masks(n, terms)


def x_mask_of(n: int, name) -> int:
    """The x masks one_group is asked for: qubit 0 alone (pivot 0, no bit below it), qubit n - 1 alone (every bit below the
    pivot), all ones, a random one; an int is taken as it is."""
    if not isinstance(name, str):
        return int(name)
    if name == "random":
        rng = _rng("x mask", n)
        return int(rng.integers(2, 1 << (n - 1))) | int(rng.integers(0, 2)) << (n - 1)
    return {"low": 1, "high": 1 << (n - 1), "ones": (1 << n) - 1}[name]


def one_group(n: int, count: int, x="random") -> PauliOperator:
    """`count` distinct strings that share the x mask `x` (a name of x_mask_of, or the mask), their z masks drawn without
    replacement; both parities of the number of Y factors occur (asserted)."""
    x = x_mask_of(n, x)
    assert 0 < x < (1 << n) and 2 <= count <= (1 << n)
    for attempt in range(64):  # (a handful of strings on a few qubits may all have one parity: the next stream then)
        rng = _rng("one_group", n, count, x, attempt)
        zs = rng.choice(1 << n, size=count, replace=False)
        if {bin(x & int(z)).count("1") & 1 for z in zs} == {0, 1}:
            break
    assert {bin(x & int(z)).count("1") & 1 for z in zs} == {0, 1}
    return from_masks(n, [(x, int(z), float(c)) for z, c in zip(zs, rng.uniform(-1.0, 1.0, size=count))])


def all_z_strings(k: int, n: int) -> PauliOperator:
    """All 2^k Z strings on the lowest k qubits of n (the identity among them): diagonal, not quadratic."""
    rng = _rng("all_z_strings", k, n)
    return from_masks(n, [(0, z, float(c)) for z, c in zip(range(1 << k), rng.uniform(-1.0, 1.0, size=1 << k))])


def parities(n: int) -> PauliOperator:
    """X, Y and Z on every qubit at once (ny = n: every residue mod 4 over four consecutive sizes), the identity, and X, Y, Z
    on qubit 0 and on qubit n - 1."""
    rng = _rng("parities", n)
    ones, top = (1 << n) - 1, 1 << (n - 1)
    strings = [(ones, 0), (ones, ones), (0, ones), (0, 0), (1, 0), (1, 1), (0, 1), (top, 0), (top, top), (0, top)]
    strings = list(dict.fromkeys(strings))  # (n = 1: qubit 0 is qubit n - 1)
    return from_masks(n, [(x, z, float(c)) for (x, z), c in zip(strings, rng.uniform(-1.0, 1.0, size=len(strings)))])


def placed(n: int, mask_a: int, mask_b: int, where: str, kind: str, part: str | None = None, n_terms: int = 24) -> PauliOperator:
    """Terms placed relative to two disjoint sets of qubits (a split circuit's sides): every support inside mask_a ("a"),
    inside mask_b ("b"), with qubits of both and of nothing else ("across"), or on the qubits of neither ("rest": the keys).

    kind "quadratic": a constant, Z on every qubit of the place, ZZ on its pairs (across: one end in each mask).
    kind "general": n_terms strings of weight 1 .. 4 with random X / Y / Z factors; ``part`` confines their support to the six
    lowest qubits of a mask ("low6") or to its remaining ones ("high").  ValueError where the place holds no qubit."""
    assert mask_a & mask_b == 0 and where in ("a", "b", "across", "rest") and kind in ("quadratic", "general")
    assert part in (None, "low6", "high") and (part is None or kind == "general")
    rng = _rng("placed", n, mask_a, mask_b, where, kind, part, n_terms)

    def confined(mask):
        qubits = _bits(mask)
        return qubits if part is None else qubits[:6] if part == "low6" else qubits[6:]

    if where == "across":
        sets = [confined(mask_a), confined(mask_b)]
    else:
        sets = [confined({"a": mask_a, "b": mask_b, "rest": ((1 << n) - 1) & ~(mask_a | mask_b)}[where])]
    if any(not s for s in sets):
        raise ValueError(f"no qubit to place a term on: {where}, {part}")
    terms = []
    if kind == "quadratic":
        terms.append((0, 0, 0.75))
        if where == "across":
            pairs = [(a, b) for a in sets[0] for b in sets[1]]
        else:
            terms += [(0, 1 << q, float(rng.normal())) for q in sets[0]]
            pairs = [(a, b) for i, a in enumerate(sets[0]) for b in sets[0][i + 1:]]
        terms += [(0, (1 << a) | (1 << b), float(rng.normal())) for a, b in pairs]
        return from_masks(n, terms)
    seen = set()
    for _ in range(20 * n_terms):
        if len(terms) == n_terms:
            break
        if where == "across":
            na = int(rng.integers(1, min(3, len(sets[0])) + 1))
            nb = int(rng.integers(1, min(4 - na, len(sets[1])) + 1))
            qubits = list(rng.choice(sets[0], size=na, replace=False)) + list(rng.choice(sets[1], size=nb, replace=False))
        else:
            qubits = list(rng.choice(sets[0], size=int(rng.integers(1, min(4, len(sets[0])) + 1)), replace=False))
        string = _string(qubits, rng.choice(list("XYZ"), size=len(qubits)))
        if string not in seen:
            seen.add(string)
            terms.append((*string, float(rng.uniform(-1.0, 1.0))))
    return from_masks(n, terms)


def unweighted_cut(n: int, degree: int = 3) -> PauliOperator:
    """MaxCut-like: ZZ with coefficient exactly 0.5 on a ring and on chords from qubit 0 that bring it to the given degree, and
    the constant -edges / 2: D = -(edges cut), an integer of at most n + degree - 1 values, tied by the thousand."""
    assert n >= 4 and 2 <= degree <= n - 1
    edges = {(q, (q + 1) % n) for q in range(n)} | {(0, 2 + j * (n - 3) // max(1, degree - 2)) for j in range(degree - 2)}
    edges = sorted({(min(a, b), max(a, b)) for a, b in edges})
    assert len(edges) == n + degree - 2
    return from_masks(n, [(0, 0, -0.5 * len(edges))] + [(0, (1 << a) | (1 << b), 0.5) for a, b in edges])


def untidy(op: PauliOperator) -> PauliOperator:
    """`op` as a careless caller hands it over: the coefficients spread over 1e-6 .. 1e3, an imaginary part on every third
    (the evaluators return real(<H>): the library ignores it, the oracles drop it at the end), one coefficient zero, every
    fifth term once more with another coefficient."""
    rng = _rng("untidy", op.labels, op.coeffs.tolist())
    terms = masks_of(op)
    out = []
    for k, (x, z, c) in enumerate(terms):
        c = c.real * 10.0 ** float(rng.uniform(-6.0, 3.0))
        if k % 3 == 1:
            c = complex(c, float(rng.normal()))
        out.append((x, z, c))
    out[len(out) // 2] = (*out[len(out) // 2][:2], 0.0)
    out += [(x, z, float(rng.normal())) for x, z, _ in out[::5]]
    return from_masks(op.num_qubits, out)


# ---- which regime an operator reaches -----------------------------------------------------------------------------------------


def groups_of(op: PauliOperator) -> tuple[int, list[tuple[int, int]]]:
    """qsv_set_operator's grouping: the terms with x = 0 split off (their number), the rest in a stable sort by x mask,
    [(x, terms of the group)]."""
    order = sorted((k for k in range(len(op)) if int(op.x_mask[k])), key=lambda k: int(op.x_mask[k]))
    groups: list[tuple[int, int]] = []
    for k in order:
        x = int(op.x_mask[k])
        if groups and groups[-1][0] == x:
            groups[-1] = (x, groups[-1][1] + 1)
        else:
            groups.append((x, 1))
    return len(op) - len(order), groups


def chunks_of(count: int) -> list[int]:
    """The chunks pauli_groups_kernel stages a group of `count` terms in."""
    return [min(K_CHUNK, count - c0) for c0 in range(0, count, K_CHUNK)]


def rows_of(operators) -> list[tuple[int, int, int]]:
    """qsv_observables_create's rows for a set of operators: the distinct strings sorted by (x, z), cut where the x mask changes
    and after kObsChunk strings; [(x, strings of the row, parts)] with parts bit 0 / 1: a string of even / odd ny."""
    strings = sorted({(int(x), int(z)) for op in operators for x, z in zip(op.x_mask, op.z_mask)})
    rows: list[list[int]] = []
    for x, z in strings:
        if not rows or rows[-1][0] != x or rows[-1][1] == K_OBS_CHUNK:
            rows.append([x, 0, 0])
        rows[-1][1] += 1
        rows[-1][2] |= 2 if bin(x & z).count("1") & 1 else 1
    return [tuple(r) for r in rows]


def mean_weight(op: PauliOperator) -> float:
    return float(np.mean([bin(int(x) | int(z)).count("1") for x, z in zip(op.x_mask, op.z_mask)]))


def single_strings(op: PauliOperator) -> list[PauliOperator]:
    """Each string of `op` as an operator of its own with coefficient 1 (an observable set's per-string values)."""
    return [PauliOperator([label], [1.0]) for label in op.labels]


# ---- references that need no 2^n x 2^n matrix ----------------------------------------------------------------------------------


def apply_operator(op: PauliOperator, state: np.ndarray) -> np.ndarray:
    """(sum_k real(c_k) P_k) |state>, P = i^ny X^x Z^z as the oracle's pauli_term_expectation reads it: the Hermitian part of
    the operator, whose expectation value the evaluators return."""
    idx = np.arange(state.shape[0], dtype=np.int64)
    out = np.zeros_like(state)
    for x, z, c in masks_of(op):
        src = idx ^ x
        parity = np.zeros_like(idx)
        for q in _bits(z):
            parity ^= (src >> q) & 1
        out += (c.real * 1j ** (bin(x & z).count("1") % 4)) * ((1.0 - 2.0 * parity) * state[src])
    return out


def adjoint_gradient(circuit, params, op: PauliOperator) -> np.ndarray:
    """d real(<psi|H|psi>) / d params[p], as dense_gradient.gradient computes it -- the gate matrix itself differentiated,
    dE/da = 2 Re <H psi|d psi/da>, summed over the angle slots that read a parameter -- but in one sweep back through the
    circuit, so that it reaches the registers a split circuit needs: with psi_k the state in front of gate k and
    chi_k = U_k^+ .. U_N^+ H psi, the slot's derivative is 2 Re <chi_{k+1}|dU_k|psi_k>."""
    import dense_gradient as dg
    from oracle import statevector_oracle as so
    from queasars_amd.ir import OP_CU3, OP_ID

    n = circuit.n_qubits
    ops = circuit.bound_ops(params)
    slots = [(int(row["p_theta"]), int(row["p_phi"]), int(row["p_lambda"])) for row in circuit.packed()]
    psi = so.simulate(n, ops)
    chi = apply_operator(op, psi)
    out = np.zeros(circuit.num_parameters)
    for (kind, target, control, theta, phi, lam), refs in zip(reversed(ops), reversed(slots)):
        if kind == OP_ID:
            continue
        control = int(control) if kind == OP_CU3 else -1
        inverse = so.u_matrix(theta, phi, lam).conj().T
        psi = dg._apply(psi, n, int(target), control, inverse)  # (psi_k: the gate undone)
        for slot, p in enumerate(refs):
            if p >= 0:
                d = dg._apply(psi, n, int(target), control, dg.du_matrix(theta, phi, lam, slot), kind == OP_CU3)
                out[p] += 2.0 * float(np.real(np.vdot(chi, d)))
        chi = dg._apply(chi, n, int(target), control, inverse)
    return out
