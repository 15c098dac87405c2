"""The reduced split form (csrc/split.hpp, reduce_final_controls) on the CPU: a key whose control is FINAL -- nothing targets it
after the key's first gate -- needs no key qubit on the control's side, a_kappa(x) = a(x) [x_c = kappa_j].  The reduced virtual
circuits, simulated with the oracle's own gate application and combined in NumPy, reproduce the oracle's state; the sizes are
what the identity promises; and the weighted Gram table a reduced side hands off, in the full form's layout, is the full
form's table (entries whose final-key bits differ: exactly zero)."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
from queasars_amd import _lib
from queasars_amd.ir import QSV_OP_DTYPE, CircuitIR
from test_split import describe, run_virtual

MAX_KEYS = 8  # QSV_SPLIT_MAX_KEYS


def describe_reduced(circuit: CircuitIR, max_side: int):
    lib = _lib.load()
    ops = circuit.packed()
    cap = 4 * len(ops) + 64
    out = [np.zeros(cap, dtype=QSV_OP_DTYPE), np.zeros(cap, dtype=QSV_OP_DTYPE)]
    na, nb, mask = C.c_int(0), C.c_int(0), C.c_uint64(0)
    simulated, final = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    key_bits, qubits = np.zeros((2, MAX_KEYS), dtype=np.int32), np.zeros((2, 32), dtype=np.int32)
    k = lib.qsv_split_describe_reduced(circuit.n_qubits, len(ops), _lib.as_ptr(ops), max_side, C.byref(mask), _lib.as_ptr(out[0]), cap,
                                       C.byref(na), _lib.as_ptr(out[1]), cap, C.byref(nb), _lib.as_ptr(simulated), _lib.as_ptr(final),
                                       _lib.as_ptr(key_bits), _lib.as_ptr(qubits))
    assert k >= -1, k
    if k < 0:
        return None
    sides = []
    for s, count in enumerate((na.value, nb.value)):
        real = [int(q) for q in qubits[s] if q >= 0]
        sides.append({"ops": out[s][:count], "simulated": int(simulated[s]), "final": int(final[s]), "key_bits": [int(b) for b in key_bits[s][:k]],
                      "qubits": real, "n_virtual": len(real) + bin(int(simulated[s])).count("1")})
    return k, int(mask.value), sides


def first_split(circuit: CircuitIR, limits):
    for max_side in limits:
        got = describe_reduced(circuit, max_side)
        if got is not None:
            return max_side, got
    return None, None


def check_layout(n: int, k: int, mask_a: int, sides):
    """What the header promises of a reduced side's index: other real qubits ascending, final controls by key, simulated keys."""
    for s, side in enumerate(sides):
        own = [q for q in range(n) if ((mask_a >> q) & 1) == (1 - s)]
        assert sorted(side["qubits"]) == own
        assert side["simulated"] | side["final"] == (1 << k) - 1 and side["simulated"] & side["final"] == 0
        n_final = bin(side["final"]).count("1")
        others = side["qubits"][: len(own) - n_final]
        assert others == sorted(others)
        finals = [j for j in range(k) if (side["final"] >> j) & 1]
        assert [side["key_bits"][j] for j in finals] == list(range(len(own) - n_final, len(own)))
        sims = [j for j in range(k) if (side["simulated"] >> j) & 1]
        assert [side["key_bits"][j] for j in sims] == list(range(len(own), len(own) + len(sims)))
    assert sides[0]["final"] & sides[1]["final"] == 0  # (a key has one control)


def reduced_state(n: int, k: int, sides, states) -> np.ndarray:
    """psi[i] = sum_kappa prod_{j in F_A} [i_cj = kappa_j] a[e_A(kappa, i)] * prod_{j in F_B} [...] b[e_B(kappa, i)]"""
    idx = np.arange(1 << n, dtype=np.int64)
    real = []
    for side in sides:
        r = np.zeros_like(idx)
        for p, q in enumerate(side["qubits"]):
            r |= ((idx >> q) & 1) << p
        real.append(r)
    psi = np.zeros(1 << n, dtype=np.complex128)
    for kappa in range(1 << k):
        term = np.ones(1 << n, dtype=np.complex128)
        for side, r, state in zip(sides, real, states):
            e = r.copy()
            keep = np.ones(1 << n, dtype=bool)
            for j in range(k):
                kj = (kappa >> j) & 1
                if (side["final"] >> j) & 1:
                    keep &= ((r >> side["key_bits"][j]) & 1) == kj
                else:
                    e |= kj << side["key_bits"][j]
            term *= np.where(keep, state[e], 0.0)
        psi += term
    return psi


def check_state(circuit: CircuitIR, params, limits):
    max_side, got = first_split(circuit, limits)
    if got is None:
        return None
    k, mask_a, sides = got
    check_layout(circuit.n_qubits, k, mask_a, sides)
    full = describe(circuit, max_side)
    assert full[0] == k and full[1] == mask_a
    for side, full_ops in zip(sides, full[2:]):
        assert side["n_virtual"] <= max_side
        if not side["final"]:  # (a side without a final control is the full form's, gate for gate)
            assert side["ops"].tobytes() == full_ops.tobytes()
    states = [run_virtual(side["n_virtual"], side["ops"], params) for side in sides]
    psi = reduced_state(circuit.n_qubits, k, sides, states)
    ref = helpers.oracle_state(circuit, params)
    assert np.abs(psi - ref).max() < 1e-13
    return k, sum(bin(side["final"]).count("1") for side in sides)


@pytest.mark.parametrize("n,layers", [(12, 3), (12, 4), (12, 5), (14, 3), (14, 4), (14, 5)])
def test_reduced_circuits_reproduce_the_state(n, layers):
    _, circuits, params = helpers.population_circuits(n, layers, 24, seed=0)
    seen = [check_state(c, p, (n // 2 + 2, n // 2 + 4)) for c, p in zip(circuits, params)]
    seen = [s for s in seen if s is not None]
    assert seen, "no circuit of the population was split"
    if layers >= 4:
        assert any(k >= 1 and f >= 1 for k, f in seen), f"no final control in the population: {seen}"
        assert any(k >= 1 and f < k for k, f in seen), f"no key that stays simulated on both sides: {seen}"


@functools.lru_cache(maxsize=None)
def headline_population():
    _, circuits, params = helpers.population_circuits(20, 4, 64, seed=0)
    return circuits, params


@pytest.mark.parametrize("index", [1, 22, 38, 41, 42])
def test_reduced_circuits_of_the_headline_population(index):
    circuits, params = headline_population()
    assert check_state(circuits[index], params[index], (12, 13)) is not None


def test_sizes_of_the_headline_circuits():
    circuits, _ = headline_population()
    # circuit 41, the population's one three-key circuit (10 + 10): two of its three controls are final, one on each side
    max_side, (k, mask_a, sides) = first_split(circuits[41], (12, 13))
    assert k == 3 and bin(mask_a).count("1") == 10 and max_side == 13
    assert [side["n_virtual"] for side in sides] == [12, 12]
    assert [bin(side["final"]).count("1") for side in sides] == [1, 1]
    # circuit 38: two keys, neither final -- the full form, gate for gate
    max_side, (k, mask_a, sides) = first_split(circuits[38], (12, 13))
    full = describe(circuits[38], max_side)
    assert k == 2 and [side["final"] for side in sides] == [0, 0]
    for s, side in enumerate(sides):
        assert side["ops"].tobytes() == full[2 + s].tobytes()
        assert side["n_virtual"] == len(side["qubits"]) + 2 and side["qubits"] == sorted(side["qubits"])


def two_triangles() -> CircuitIR:
    """Qubits 0 1 2 and 3 4 5, each triple held together by two keys per qubit: only cross gates can be cut at three a side."""
    c = CircuitIR(6)
    for q in range(6):
        c.u(0.3 + 0.1 * q, 0.2 * q, -0.1 * q, q)
    c.cu3(0.7, 0.1, 0.2, 0, 1).cu3(0.5, -0.3, 0.4, 0, 2).cu3(0.9, 0.8, -0.7, 1, 2)
    c.cu3(0.4, 0.5, 0.6, 3, 4).cu3(0.3, 0.2, 0.1, 3, 5).cu3(0.6, 0.1, 0.1, 4, 5)
    return c


def test_a_control_that_is_targeted_again_is_not_reduced():
    final = two_triangles().cu3(1.1, 0.2, 0.3, 2, 3)
    k, mask_a, sides = describe_reduced(final, 4)
    assert (k, mask_a) == (1, 0b000111)
    assert (sides[0]["final"], sides[0]["simulated"], sides[0]["n_virtual"]) == (1, 0, 3)  # every key final: no key qubit on A
    assert (sides[1]["final"], sides[1]["simulated"], sides[1]["n_virtual"]) == (0, 1, 4)
    assert sides[0]["qubits"] == [0, 1, 2] and all(int(o["p_theta"]) >= -1 for o in sides[0]["ops"])
    assert check_state(final, [], (4,)) == (1, 1)
    again = two_triangles().cu3(1.1, 0.2, 0.3, 2, 3).u(0.2, 0.1, 0.0, 2)
    k, mask_a, sides = describe_reduced(again, 4)
    assert (k, mask_a) == (1, 0b000111) and [side["final"] for side in sides] == [0, 0]
    assert [side["n_virtual"] for side in sides] == [4, 4]
    assert check_state(again, [], (4,)) == (1, 0)
    # ... also when the later gate that targets the control is a controlled one from the other side (a second key)
    back = two_triangles().cu3(1.1, 0.2, 0.3, 2, 3).cu3(0.2, 0.1, 0.0, 4, 2)
    k, mask_a, sides = describe_reduced(back, 5)
    assert (k, mask_a) == (2, 0b000111)
    # (keys count in the order of their first gates: key 0 is qubit 4's -- 4 -> 5, then 4 -> 2 in the same epoch --, final on B;
    # key 1 is 2 -> 3, not final on A: 2 is targeted afterwards)
    assert [side["final"] for side in sides] == [0, 0b01]
    assert check_state(back, [], (5,)) == (2, 1)


def test_a_control_of_two_epochs_reduces_only_the_last():
    c = two_triangles().cu3(1.1, 0.2, 0.3, 2, 3).u(0.2, 0.1, 0.0, 2).cu3(0.8, -0.2, 0.5, 2, 4)
    k, mask_a, sides = describe_reduced(c, 5)
    assert (k, mask_a) == (2, 0b000111)
    assert (sides[0]["final"], sides[0]["simulated"], sides[0]["n_virtual"]) == (0b10, 0b01, 4)
    assert (sides[1]["final"], sides[1]["simulated"], sides[1]["n_virtual"]) == (0, 0b11, 5)
    assert sides[0]["qubits"] == [0, 1, 2] and sides[0]["key_bits"] == [3, 2]
    assert check_state(c, [], (5,)) == (2, 1)


def test_every_key_final_on_one_side_leaves_it_without_a_key_qubit():
    c = two_triangles().cu3(1.1, 0.2, 0.3, 1, 3).cu3(0.8, -0.2, 0.5, 2, 4)
    k, mask_a, sides = describe_reduced(c, 5)
    assert (k, mask_a) == (2, 0b000111)
    assert (sides[0]["final"], sides[0]["simulated"], sides[0]["n_virtual"]) == (0b11, 0, 3)
    assert (sides[1]["final"], sides[1]["simulated"], sides[1]["n_virtual"]) == (0, 0b11, 5)
    assert sides[0]["qubits"] == [0, 1, 2] and sides[0]["key_bits"] == [1, 2]
    assert all(int(o["p_theta"]) >= -1 and int(o["target"]) < 3 for o in sides[0]["ops"])
    assert check_state(c, [], (5,)) == (2, 2)
    # final controls that are not the side's highest qubits move there: the others keep their order
    low = two_triangles().cu3(1.1, 0.2, 0.3, 0, 3).cu3(0.8, -0.2, 0.5, 1, 4)
    k, mask_a, sides = describe_reduced(low, 5)
    assert k == 2 and sides[0]["final"] == 0b11 and sides[0]["qubits"][0] == 2 and sorted(sides[0]["qubits"][1:]) == [0, 1]
    assert check_state(low, [], (5,)) == (2, 2)


# ---- the table a side hands off: 2 + n_side weights x 4^K entries, the full form's layout -------------------------------
def gram_tables(rows: np.ndarray, weights: np.ndarray) -> np.ndarray:
    """G[w, kappa, kappa'] = sum_x weights[w, x] conj(rows[kappa, x]) rows[kappa', x]"""
    return np.einsum("wx,kx,lx->wkl", weights, rows.conj(), rows)


def side_weights(n_side: int, d: np.ndarray) -> np.ndarray:
    x = np.arange(1 << n_side)
    return np.stack([np.ones(1 << n_side), d] + [((x >> q) & 1).astype(np.float64) for q in range(n_side)])


def reduced_gram(k: int, side, own, state: np.ndarray, d: np.ndarray) -> np.ndarray:
    """The full-layout table from a reduced side's state: entries whose final-key bits differ are written as zeros, the others
    are sums over the rows' block of x; D is the side's own table in the reduced order of its qubits, the weight of a final
    control's bit is a constant per block."""
    n_side = len(own)
    finals = [j for j in range(k) if (side["final"] >> j) & 1]
    low_bits = n_side - len(finals)
    local = [own.index(q) for q in side["qubits"]]  # the full form's local number of each reduced position
    xr = np.arange(1 << n_side)
    x_full = np.zeros_like(xr)
    for p, q in enumerate(local):
        x_full |= ((xr >> p) & 1) << q
    d_reduced = d[x_full]  # (what the side's own table of D holds in the reduced order)
    table = np.zeros((2 + n_side, 1 << k, 1 << k), dtype=np.complex128)
    xl = np.arange(1 << low_bits)
    for ka in range(1 << k):
        for kb in range(1 << k):
            if any(((ka ^ kb) >> j) & 1 for j in finals):
                continue  # exactly zero
            block = sum((((ka >> j) & 1) << t) for t, j in enumerate(finals))
            x = (block << low_bits) | xl
            ea, eb = x.copy(), x.copy()
            for j in range(k):
                if (side["simulated"] >> j) & 1:
                    ea |= ((ka >> j) & 1) << side["key_bits"][j]
                    eb |= ((kb >> j) & 1) << side["key_bits"][j]
            p = state[ea].conj() * state[eb]
            table[0, ka, kb] = p.sum()
            table[1, ka, kb] = (d_reduced[x] * p).sum()
            for pos, q in enumerate(local):
                if pos < low_bits:
                    table[2 + q, ka, kb] = (((xl >> pos) & 1) * p).sum()
                else:
                    table[2 + q, ka, kb] = p.sum() if (block >> (pos - low_bits)) & 1 else 0.0
    return table


def check_gram(circuit: CircuitIR, params, limits) -> int:
    max_side, got = first_split(circuit, limits)
    k, mask_a, sides = got
    full = describe(circuit, max_side)
    n, checked = circuit.n_qubits, 0
    rng = np.random.default_rng(7)
    for s, side in enumerate(sides):
        if not side["final"]:
            continue
        own = [q for q in range(n) if ((mask_a >> q) & 1) == (1 - s)]
        n_side = len(own)
        d = rng.normal(size=1 << n_side)
        rows = run_virtual(n_side + k, full[2 + s], params).reshape(1 << k, 1 << n_side)
        want = gram_tables(rows, side_weights(n_side, d))
        state = run_virtual(side["n_virtual"], side["ops"], params)
        have = reduced_gram(k, side, own, state, d)
        assert np.abs(have - want).max() < 1e-13
        differ = np.array([[any(((ka ^ kb) >> j) & 1 for j in range(k) if (side["final"] >> j) & 1) for kb in range(1 << k)] for ka in range(1 << k)])
        assert differ.any() and np.all(have[:, differ] == 0.0) and np.abs(want[:, differ]).max() < 1e-13
        checked += 1
    return checked


def test_gram_table_of_a_reduced_side_is_the_full_forms():
    circuits, params = headline_population()
    assert check_gram(circuits[41], params[41], (12, 13)) == 2  # both sides of the three-key circuit
    assert check_gram(circuits[22], params[22], (12, 13)) >= 1
    c = two_triangles().cu3(1.1, 0.2, 0.3, 0, 3).cu3(0.8, -0.2, 0.5, 1, 4)  # every key final, controls moved up
    assert check_gram(c, [], (5,)) == 1
    c = two_triangles().cu3(1.1, 0.2, 0.3, 2, 3).u(0.2, 0.1, 0.0, 2).cu3(0.8, -0.2, 0.5, 2, 4)  # one of two
    assert check_gram(c, [], (5,)) == 1
