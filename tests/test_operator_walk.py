"""CPU half of the operator walk (tests/operator_walk.py): the five kinds are five different classifications as
qsv_set_operator makes them, the intended ones, and the walk makes every ordered pair of distinct kinds adjacent."""

from __future__ import annotations

import numpy as np
import pytest

import helpers
import operator_walk as ow
import variance_reference as vr
from queasars_amd.ir import PauliOperator


@pytest.mark.parametrize("n", ow.SIZES)
def test_the_five_kinds_are_five_different_classifications(n):
    ops = ow.kinds(n)
    assert tuple(ops) == ow.KINDS and all(isinstance(op, PauliOperator) and op.num_qubits == n for op in ops.values())
    assert ow.kinds(n)["mixed"] is ops["mixed"]  # (the same objects at every visit)
    flags = {kind: ow.flags_of(op) for kind, op in ops.items()}
    assert len(set(flags.values())) == 5, flags
    assert flags == ow.intended_flags(n)
    # what the table of kinds says about their content, from the masks
    assert not ops["ising"].x_mask.any() and {bin(int(z)).count("1") for z in ops["ising"].z_mask} == {1, 2}
    assert not ops["fields"].x_mask.any() and {bin(int(z)).count("1") for z in ops["fields"].z_mask} == {0, 1}
    assert not ops["cubic"].x_mask.any() and {bin(int(z)).count("1") for z in ops["cubic"].z_mask} == {3}
    mixed = [(bool(x), bin(int(x) & int(z)).count("1")) for x, z in zip(ops["mixed"].x_mask, ops["mixed"].z_mask)]
    assert {(False, 0), (True, 0), (True, 2)} == set(mixed)  # (ZZ and Z; XX; YY)
    assert ops["offdiag"].x_mask.all() and len(ops["offdiag"]) == 16
    # cubic reaches both halves of the register and crosses between them: no side of a split circuit holds all of it
    half = (1 << (n // 2)) - 1
    where = {(bool(int(z) & half), bool(int(z) & ~half)) for z in ops["cubic"].z_mask}
    assert (True, True) in where and len(where) >= 2


@pytest.mark.parametrize("n", ow.SIZES)
def test_the_walk_covers_all_twenty_ordered_pairs(n):
    stops = ow.walk()
    assert len(stops) == 21 and stops[0] == stops[-1] == "ising" and set(stops) == set(ow.kinds(n))
    pairs = ow.transitions(stops)
    assert len(pairs) == len(set(pairs)) == 20 and all(a != b for a, b in pairs)
    assert set(pairs) == {(a, b) for a in ow.KINDS for b in ow.KINDS if a != b}
    assert any(stops[i:i + 3] == ["offdiag", "ising", "cubic"] for i in range(len(stops)))
    assert ow.walk() == stops


def test_the_populations_and_their_parameter_sets_are_the_same_at_every_call():
    for n in (10, 14):
        _, first = ow.population(n)
        _, again = ow.population(n)
        assert [name for name, _, _ in first] == [name for name, _, _ in again] and len(first) == {10: 6, 14: 7}[n]
        for (_, c, p), (_, c2, p2) in zip(first, again):
            assert c is not c2 and c._bytes == c2._bytes and p == p2 and len(p) == c.num_parameters
            assert min(c.gradient_terms(), default=0) >= 0  # (every parameter has a shift rule)
        sets = ow.parameter_sets([p for _, _, p in first], seed=n)
        assert len(sets) == 3 and sets[0][0] == first[0][2] and sets[1] != sets[2]
        assert sets[1] == ow.parameter_sets([p for _, _, p in again], seed=n)[1]
    kinds = [ow.flags_of(op) for op in ow.observable_set(10)]
    assert kinds[0].all_diag and not kinds[1].all_diag and kinds[1].has_diag_part and not kinds[2].has_diag_part


@pytest.mark.parametrize("n", [5, 10, 13])
def test_moments_grouped_by_x_mask_are_the_references(n):
    """ow.grouped_moments is variance_reference.moments' quantity, string for string: the five kinds, the observable set's
    operators, an operator of many x masks with every number of Y factors, the parities (X, Y, Z on every qubit at once) and an
    untidy list (imaginary parts, a zero coefficient, repeated strings) -- within 1e-12 (sum |c_k|)^2, the rounding of two
    orders of summation."""
    import operator_families as of

    made = ow.population(10)[1][:2] if n == 10 else [("ladder", *ow.cf.ladder(n)), ("generic", *ow.cf.generic(n, 60))]
    states = [helpers.oracle_state(c, p) for _, c, p in made]
    ops = {**ow.kinds(n), **{f"observable {m}": op for m, op in enumerate(ow.observable_set(n))},
           "random": helpers.random_pauli_operator(n, 40, seed=n), "parities": of.parities(n), "untidy": of.untidy(of.heisenberg(n))}
    for name, op in ops.items():
        for state in states:
            got, want = ow.grouped_moments(op, state), vr.moments(op, state)
            scale = max(1.0, float(np.abs(op.coeffs.real).sum())) ** 2
            assert abs(got[0] - want[0]) < 1e-12 * scale and abs(got[1] - want[1]) < 1e-12 * scale, (n, name, got, want)
    assert max(abs(vr.moments(op, states[0])[1]) for op in ops.values()) > 1e-2  # (not variances of zero)


def test_the_table_form_of_a_diagonal_operators_moments_is_the_references(c_oracle):
    """ow.diagonal_moments (D from the plain-C oracle's table, lambda = D psi) is variance_reference.moments' quantity: the
    20-qubit arm of the GPU walk uses it where the matrix-free reference takes ten seconds per circuit."""
    n = 10
    _, made = ow.population(n)
    for kind in ow.DIAGONAL_KINDS:
        op = ow.kinds(n)[kind]
        table = c_oracle.diagonal_table(op)
        for _, c, p in made[:2]:
            state = helpers.oracle_state(c, p)
            got, want = ow.diagonal_moments(table, state), vr.moments(op, state)
            assert np.abs(np.asarray(got) - np.asarray(want)).max() < 1e-12 * max(1.0, ow.spread(op)) ** 2, (kind, got, want)
