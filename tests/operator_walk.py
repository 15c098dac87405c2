"""A live handle walked through operators of every kind (test helpers, no tests).

One ``StatevectorDevice`` is shared by evaluators with different operators, and ``qsv_set_operator`` is a state transition on a
handle that already holds registered circuits, uploaded plans, side tables and a sort order of D, recorded launches, kept states,
gradient plans and observable sets.  What a circuit does afterwards depends on the operator set NOW.  This module names the five
kinds of operator ``qsv_set_operator`` tells apart (``kinds``), restates its classification from the masks alone (``flags_of``)
and gives a fixed walk that makes every ordered pair of distinct kinds adjacent once (``walk``: an Euler circuit of the complete
digraph on five nodes).  The same arguments give the same operators, circuits and parameter sets on every machine.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

import circuit_families as cf
import helpers
import operator_families as of
from queasars_amd.ir import PauliOperator

KINDS = ("ising", "fields", "cubic", "mixed", "offdiag")
DIAGONAL_KINDS = ("ising", "fields", "cubic")
SIZES = (10, 14, 20)
SEED = 2020


class Flags(NamedTuple):
    """What qsv_set_operator derives from the masks: ``diagonal`` (no term with an x mask), ``quadratic`` (diagonal and no Z
    string of weight above two: the couplings go to a dense matrix), ``has_diag_part`` (some I/Z term: the table of D is
    rebuilt), the number of x-mask groups -- and whether the coupling matrix has an entry at all, which is all that tells
    single-Z fields from an Ising operator."""

    all_diag: bool
    quadratic: bool
    has_diag_part: bool
    n_groups: int
    coupled: bool


def flags_of(op: PauliOperator) -> Flags:
    n_diag, groups = of.groups_of(op)
    all_diag = not groups
    weights = [bin(z).count("1") for x, z, _ in of.masks_of(op) if x == 0]
    quadratic = all_diag and max(weights, default=0) <= 2
    coupled = quadratic and any(x == 0 and bin(z).count("1") == 2 and c.real != 0.0 for x, z, c in of.masks_of(op))
    return Flags(all_diag, quadratic, n_diag > 0, len(groups), coupled)


def _cubic(n: int) -> PauliOperator:
    """2 n distinct Z strings of weight three drawn over the whole register (both sides of any cut and across it), seeded."""
    rng = cf._rng("operator_walk cubic", n)
    masks: dict[int, float] = {}
    while len(masks) < 2 * n:
        a, b, c = (int(q) for q in rng.choice(n, size=3, replace=False))
        masks.setdefault((1 << a) | (1 << b) | (1 << c), float(rng.uniform(-1.0, 1.0)))
    return of.from_masks(n, [(0, z, c) for z, c in masks.items()])


def _fields(n: int) -> PauliOperator:
    rng = cf._rng("operator_walk fields", n)
    return of.from_masks(n, [(0, 0, 0.375)] + [(0, 1 << q, float(rng.normal())) for q in range(n)])


def _offdiag(n: int) -> PauliOperator:
    """of.hopping's X Z..Z X and Y Z..Z Y strings without its number terms and fields: no I/Z term at all, several x-mask
    groups, Y phases, Z runs of every length."""
    return of.from_masks(n, [term for term in of.masks_of(of.hopping(n, 8)) if term[0]])


_KINDS: dict = {}


def kinds(n: int) -> dict:
    """{kind: operator} on n qubits: the same five objects at every call (a handle's evaluators compare by identity)."""
    if n not in _KINDS:
        _KINDS[n] = {"ising": helpers.random_ising_operator(n, seed=SEED), "fields": _fields(n), "cubic": _cubic(n),
                     "mixed": of.heisenberg(n), "offdiag": _offdiag(n)}
    return _KINDS[n]


def intended_flags(n: int) -> dict:
    """What each kind is meant to be, written down by hand: heisenberg(n) has one x mask per bond (XX and YY share it), the
    hopping strings of 8 distinct pairs have 8."""
    return {"ising": Flags(True, True, True, 0, True), "fields": Flags(True, True, True, 0, False),
            "cubic": Flags(True, False, True, 0, False), "mixed": Flags(False, False, True, n - 1, False),
            "offdiag": Flags(False, False, False, 8, False)}


def walk() -> list[str]:
    """21 stops over the five kinds, every ordered pair of distinct kinds adjacent exactly once: for each difference
    d = 1 .. 4 the cycle 0, d, 2d, .. (mod 5) back to 0 -- five is prime, so each is a cycle through all five nodes, and the
    arc a -> b lies on the cycle of d = b - a alone.  Starts and ends at "ising"; "offdiag", "ising", "cubic" follow each other
    (a stale table or sort order of D, last written two operators ago)."""
    stops = [0]
    for d in (1, 2, 3, 4):
        stops += [(d * k) % 5 for k in range(1, 6)]
    return [KINDS[s] for s in stops]


def transitions(stops=None) -> list[tuple[str, str]]:
    stops = walk() if stops is None else stops
    return list(zip(stops[:-1], stops[1:]))


# ---- what is evaluated at every stop --------------------------------------------------------------------------------------------

FOUR_KEYS = "two_blocks 4"
# (layers, individuals drawn, the ones taken) of helpers.population_circuits(n, .., seed=n).  At 14 qubits the three-layer
# genome circuits split without a key and the eight-layer ones not at all: of eight six-layer individuals these three cut
# with two, one and two keys.  At 20 the headline's four layers: both cut with one key, the second into a reduced side.
GENOME = {10: (3, 4, (0, 1, 2, 3)), 14: (6, 8, (0, 2, 3)), 20: (4, 6, (1, 5))}


def population(n: int):
    """(the EVQE individuals the genome circuits come from, [(name, circuit, parameters)]): fresh objects at every call (a
    circuit on a kept state belongs to one device).  10: the one-tile route.  14: genome circuits, a two-key circuit and a
    ladder that split, a four-key circuit that splits under a quadratic operator only, all pairs, which never split.  20: the
    headline's shape, for the one-launch route and its reduced sides."""
    layers, count, picks = GENOME[n]
    pop, circuits, params = helpers.population_circuits(n, layers, count, seed=n)
    made = [(f"individual {i}", circuits[k], list(params[k])) for i, k in enumerate(picks)]
    # (at 14 qubits two_blocks(14, 4) with seed 0 cuts with three keys and ladder(14, 2) splits with two: seed 1 has four
    # keys, all pairs of qubits have no cut at all)
    extra = {10: [("ladder", cf.ladder(10)), ("all_pairs", cf.all_pairs(10))],
             14: [("two_blocks 2", cf.two_blocks(14, 2)), (FOUR_KEYS, cf.two_blocks(14, 4, seed=1)), ("ladder", cf.ladder(14, 2)),
                  ("all_pairs", cf.all_pairs(14))],
             20: [("two_blocks 2", cf.two_blocks(20, 2))]}[n]
    return [pop.individuals[k] for k in picks], made + [(name, c, list(p)) for name, (c, p) in extra]


def parameter_sets(params, seed: int, count: int = 3):
    """The parameters and count - 1 perturbed copies: the same batch again with other values (tests/test_gpu_replay.py)."""
    rng = np.random.default_rng(seed)
    return [params] + [[[float(v + rng.normal(0.0, 0.3)) for v in p] for p in params] for _ in range(count - 1)]


def observable_set(n: int) -> list[PauliOperator]:
    """One diagonal, one mixed and one off-diagonal operator, none of them a kind of the walk: an observable set does not use the
    handle's operator."""
    return [of.unweighted_cut(n, 3), of.transverse_ising(n), of.one_group(n, 24)]


def spread(op: PauliOperator) -> float:
    return float(np.abs(op.coeffs.real).sum())


def diagonal_moments(table: np.ndarray, state: np.ndarray) -> tuple[float, float]:
    """(E, Var) of a diagonal operator with the values ``table`` in ``state``: variance_reference.moments with lambda = D psi
    written out (tests/test_operator_walk.py holds the two together)."""
    probs = np.abs(state) ** 2
    value = float(np.dot(probs, table))
    return value, float(np.dot(probs, table * table)) - value * value


def grouped_moments(op: PauliOperator, state: np.ndarray) -> tuple[float, float]:
    """(E, Var) of `op` in `state`: variance_reference.moments' quantity with the strings grouped by x mask.  The state is
    seen as a tensor with one axis per qubit; the strings of a group share psi_(i ^ x) (the tensor flipped along the axes of x,
    a view) and differ in their factor c (-i)^ny (-1)^popcount(i & z), which is a product of [1, -1] along the axes of z: the
    group's factors are summed as small broadcast arrays, and the state is passed over once per group, not once per string.
    (77 strings of heisenberg(20): 20 passes.)  tests/test_operator_walk.py holds it to variance_reference.moments."""
    n = op.num_qubits
    tensor = np.asarray(state).reshape((2,) * n)  # (axis n - 1 - q is qubit q)
    groups: dict[int, list] = {}
    for x, z, c in of.masks_of(op):
        if c.real != 0.0:
            groups.setdefault(x, []).append((z, c.real * (-1j) ** (bin(x & z).count("1") % 4)))
    lam = np.zeros_like(tensor)
    for x, strings in groups.items():
        factor = np.zeros((1,) * n, dtype=np.complex128)
        for z, c in strings:
            sign = np.ones((1,) * n)
            for q in of._bits(z):
                shape = [1] * n
                shape[n - 1 - q] = 2
                sign = sign * np.array([1.0, -1.0]).reshape(shape)
            factor = factor + c * sign
        lam += factor * np.flip(tensor, axis=tuple(n - 1 - q for q in of._bits(x)))
    flat, lam = tensor.reshape(-1), lam.reshape(-1)
    value = float(np.real(np.vdot(flat, lam)))
    return value, float(np.real(np.vdot(lam, lam))) - value * value


def same_bits(got, want) -> bool:
    """Bit for bit: the same shape and bytes (a list of arrays as their concatenation; anything else by ==)."""
    if isinstance(got, (str, tuple, int)) or isinstance(want, (str, tuple, int)):
        return type(got) is type(want) and got == want
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
