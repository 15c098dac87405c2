"""The operator families of tests/operator_families.py on the CPU: both oracles against Kronecker products of the 2 x 2 Pauli
matrices on every family (which pins the i^ny convention for every ny up to n), the families in the regimes they are here for
-- groups on both sides of pauli_groups_kernel's chunk, observable rows on both sides of kObsChunk, supports where ``placed``
says, tied values of D -- and the counts read off the kernels' own constants.  The GPU half is
tests/test_gpu_operator_families.py."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import circuit_families as cf
import helpers
import operator_families as of
from oracle import statevector_oracle as so

DENSE_REL = 1e-13  # per unit of sum |c_k|

_PAULI = {"I": np.eye(2, dtype=complex), "X": np.array([[0, 1], [1, 0]], dtype=complex),
          "Y": np.array([[0, -1j], [1j, 0]], dtype=complex), "Z": np.array([[1, 0], [0, -1]], dtype=complex)}


def small_families(n: int):
    """Every family at n <= 6 qubits (the lower half of the register and the upper half without its last qubit as the two sides
    of ``placed``: the last qubit is the "rest")."""
    lower, upper = (1 << (n // 2)) - 1, ((1 << (n - 1)) - 1) & ~((1 << (n // 2)) - 1)
    made = {"transverse_ising": of.transverse_ising(n, False), "transverse_ising periodic": of.transverse_ising(n, True),
            "heisenberg": of.heisenberg(n, True), "hopping": of.hopping(n, 5), "all_z_strings": of.all_z_strings(n - 1, n),
            "parities": of.parities(n), "unweighted_cut": of.unweighted_cut(n, 3) if n >= 4 else of.all_z_strings(2, n)}
    for name in of.X_MASK_NAMES:
        made[f"one_group {name}"] = of.one_group(n, 1 << (n - 1), name)
    made["one_group of every z"] = of.one_group(n, 1 << n, "ones")
    for where in ("a", "b", "across", "rest"):
        for kind in ("quadratic", "general"):
            made[f"placed {where} {kind}"] = of.placed(n, lower, upper, where, kind, n_terms=8)
    made.update({f"untidy {name}": of.untidy(made[name]) for name in ("heisenberg", "all_z_strings", "placed across general")})
    return made


def dense_expectation(state: np.ndarray, op) -> complex:
    total = 0.0j
    for label, c in zip(op.labels, op.coeffs):
        matrix = np.array([[1.0 + 0.0j]])
        for ch in label:  # (the leftmost character is the highest qubit: the most significant factor)
            matrix = np.kron(matrix, _PAULI[ch])
        total += c * np.vdot(state, matrix @ state)
    return total


def c_expectation(c_oracle, state: np.ndarray, op) -> float:
    flat = np.ascontiguousarray(state).view(np.float64)
    x, z = np.ascontiguousarray(op.x_mask), np.ascontiguousarray(op.z_mask)
    cre, cim = np.ascontiguousarray(op.coeffs.real), np.ascontiguousarray(op.coeffs.imag)
    out = np.zeros(2)
    c_oracle.lib.qsvo_expectation.restype = C.c_int
    assert c_oracle.lib.qsvo_expectation(op.num_qubits, flat.ctypes, len(op), x.ctypes, z.ctypes, cre.ctypes, cim.ctypes, out.ctypes) == 0
    return float(out[0])


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_both_oracles_against_kronecker_products(n, c_oracle):
    """real(<psi|H|psi>) from Kronecker products of the 2 x 2 matrices, for every family and two states of generic circuits:
    so.pauli_expectation and the plain-C oracle within 1e-13 per unit of sum |c_k|."""
    states = [helpers.oracle_state(*cf.generic(n, 40, seed=seed)) for seed in (0, 1)]
    worst = 0.0
    for name, op in small_families(n).items():
        scale = float(np.abs(op.coeffs).sum())
        for state in states:
            want = dense_expectation(state, op).real
            got = so.pauli_expectation(state, op.x_mask.tolist(), op.z_mask.tolist(), op.coeffs.tolist()).real
            got_c = c_expectation(c_oracle, state, op)
            worst = max(worst, abs(got - want) / scale, abs(got_c - want) / scale)
            assert abs(got - want) < DENSE_REL * scale and abs(got_c - want) < DENSE_REL * scale, (name, got, got_c, want)
    print(f"\nn = {n}: largest |oracle - dense| / sum |c_k| = {worst:.2e}")


def test_the_y_convention_on_strings_of_many_y():
    """YYYYY (ny = 5), XYZYX (ny = 2) and YYYYI (ny = 4) on a generic state: the oracle is the dense value."""
    state = helpers.oracle_state(*cf.generic(5, 40))
    for label in ("YYYYY", "XYZYX", "YYYYI", "YYYII", "IYIII"):
        x, z = so.label_to_masks(label)
        op = of.from_masks(5, [(x, z, 1.0)])
        assert op.labels == [label]
        assert abs(so.pauli_term_expectation(state, x, z) - dense_expectation(state, op)) < 1e-15, label


def test_one_group_reaches_both_sides_of_a_chunk_and_of_a_row():
    """qsv_set_operator's grouping and qsv_observables_create's row cutting, restated: one_group gives one group of exactly the
    count asked for -- 255, 256, 257 (a second chunk of one term), 513 (a third, partial chunk), 512, 513 and every z mask of ten
    qubits -- under each x mask, with strings of even and of odd ny; as an observable set one full row, or a full row and a row
    of one that carries its own `parts`."""
    for n in (10, 14):
        for count in of.GROUP_COUNTS + ((1 << n,) if n == 10 else ()):
            for name in of.X_MASK_NAMES:
                op = of.one_group(n, count, name)
                x = of.x_mask_of(n, name)
                assert of.groups_of(op) == (0, [(x, count)]), (n, count, name)
                chunks = of.chunks_of(count)
                assert sum(chunks) == count and all(c == of.K_CHUNK for c in chunks[:-1]) and 1 <= chunks[-1] <= of.K_CHUNK
                rows = of.rows_of(of.single_strings(op))
                assert [r[1] for r in rows] == [min(of.K_OBS_CHUNK, count - r0) for r0 in range(0, count, of.K_OBS_CHUNK)]
                assert all(r[0] == x and r[2] in (1, 2, 3) for r in rows) and rows[0][2] | rows[-1][2] == 3
    assert of.chunks_of(of.K_CHUNK - 1) == [255] and of.chunks_of(of.K_CHUNK) == [256] and of.chunks_of(of.K_CHUNK + 1) == [256, 1]
    assert of.chunks_of(2 * of.K_CHUNK + 1) == [256, 256, 1]
    pivots = {of.x_mask_of(14, name).bit_length() - 1 for name in of.X_MASK_NAMES}
    assert {0, 13} <= pivots
    for n in (10, 14):
        assert of.rows_of(of.single_strings(of.all_z_strings(10, n))) == [(0, 512, 1), (0, 512, 1)]
        rows = of.rows_of([of.one_group(n, of.K_OBS_CHUNK + 1, "high")])
        assert [r[1] for r in rows] == [of.K_OBS_CHUNK, 1] and rows[1][2] in (1, 2)
        assert [r[1] for r in of.rows_of([of.one_group(n, of.K_OBS_CHUNK, "ones")])] == [of.K_OBS_CHUNK]
    # the same rows whether a set holds each string as an observable of its own or two observables of many strings
    op = of.one_group(14, of.K_OBS_CHUNK + 1, "random")
    halves = [of.from_masks(14, of.masks_of(op)[:300]), of.from_masks(14, of.masks_of(op)[300:])]
    assert of.rows_of(halves) == of.rows_of(of.single_strings(op))


def test_the_physical_families_have_the_groups_they_are_here_for():
    for n in (10, 14, 17, 20):
        diag, groups = of.groups_of(of.transverse_ising(n, True))
        assert diag == n and groups == [(1 << q, 1) for q in range(n)]  # every pivot, one weight-1 string each
        op = of.heisenberg(n, False)
        diag, groups = of.groups_of(op)
        assert diag == 2 * n - 1 and len(groups) == n - 1 and all(count == 2 for _, count in groups)
        assert sorted({bin(int(x) & int(z)).count("1") for x, z in zip(op.x_mask, op.z_mask)}) == [0, 2]
        op = of.hopping(n, 12)
        diag, groups = of.groups_of(op)
        assert all(count == 2 and bin(x).count("1") == 2 for x, count in groups) and len(groups) == 12
        runs = [bin(int(z) & ~int(x)).count("1") for x, z in zip(op.x_mask, op.z_mask) if int(x)]
        assert max(runs) >= n // 2 and of.mean_weight(of.transverse_ising(n)) < 2
        op = of.parities(n)
        assert len(op) == 10 and n in {bin(int(x) & int(z)).count("1") for x, z in zip(op.x_mask, op.z_mask)}
        assert not of.all_z_strings(10, n).x_mask.any() and max(bin(int(z)).count("1") for z in of.all_z_strings(10, n).z_mask) == 10
    # Y on every qubit has ny = n: residues 2, 2, 1, 0 mod 4 at these sizes; every residue under one_group's x mask of all ones
    op = of.one_group(10, of.K_CHUNK + 1, "ones")
    assert {bin(int(x) & int(z)).count("1") & 3 for x, z in zip(op.x_mask, op.z_mask)} == {0, 1, 2, 3}


def test_placed_keeps_every_support_where_it_says():
    n, mask_a, mask_b = 16, 0x007f, 0x7f80  # (seven and eight qubits; qubit 15 is in neither)
    rest = ((1 << n) - 1) & ~(mask_a | mask_b)
    low6 = lambda mask: sum(1 << q for q in of._bits(mask)[:6])  # noqa: E731
    for kind in ("quadratic", "general"):
        for where, inside in (("a", mask_a), ("b", mask_b), ("rest", rest)):
            op = of.placed(n, mask_a, mask_b, where, kind)
            support = [int(x) | int(z) for x, z in zip(op.x_mask, op.z_mask)]
            assert all(s & ~inside == 0 for s in support) and any(support), (kind, where)
        op = of.placed(n, mask_a, mask_b, "across", kind)
        support = [int(x) | int(z) for x, z in zip(op.x_mask, op.z_mask)]
        assert all((s & mask_a and s & mask_b and not s & rest) or s == 0 for s in support), kind
        assert (not op.x_mask.any()) == (kind == "quadratic")
    for part in ("low6", "high"):
        for where, masks in (("a", [mask_a]), ("b", [mask_b]), ("across", [mask_a, mask_b])):
            op = of.placed(n, mask_a, mask_b, where, "general", part)
            allowed = sum(low6(m) if part == "low6" else m & ~low6(m) for m in masks)
            for x, z in zip(op.x_mask, op.z_mask):
                s = int(x) | int(z)
                assert s and s & ~allowed == 0 and all(s & m for m in masks) and 1 <= bin(s).count("1") <= 4, (part, where)
    with pytest.raises(ValueError):
        of.placed(n, mask_a, mask_b | rest, "rest", "general")
    # weight-1 and weight-2 strings, and strings with no X or Y on one side (fx = 0 there: a weighted norm)
    op = of.placed(n, mask_a, mask_b, "across", "general", n_terms=60)
    weights = {bin(int(x) | int(z)).count("1") for x, z in zip(op.x_mask, op.z_mask)}
    assert {2, 3, 4} <= weights and any(int(x) & mask_a == 0 and int(x) for x in op.x_mask)


def test_unweighted_cut_has_few_distinct_values():
    op = of.unweighted_cut(10, 3)
    values = so.diagonal_values(10, op.z_mask.tolist(), op.coeffs.real.tolist())
    distinct = sorted(set(values.tolist()))
    assert len(distinct) <= 10 + 2 and all(v == round(v) for v in distinct) and max(distinct) == 0.0
    assert set(np.abs(op.coeffs[1:]).tolist()) == {0.5}
    print(f"\nunweighted_cut(10, 3): {len(distinct)} values of D over 1024 states, the most common {np.unique(values, return_counts=True)[1].max()} times")


def test_untidy_keeps_the_real_part_of_the_expectation_meaningful():
    op = of.heisenberg(6, True)
    wild = of.untidy(op)
    assert len(wild) == len(op) + len(range(0, len(op), 5)) and 0.0 in wild.coeffs.tolist() and np.abs(wild.coeffs.imag).max() > 0
    mags = np.abs(wild.coeffs.real[wild.coeffs.real != 0])
    assert mags.min() < 1e-3 and mags.max() > 10.0
    assert len({(int(x), int(z)) for x, z in zip(wild.x_mask, wild.z_mask)}) == len(op)  # (repeated strings)
    assert of.untidy(op).labels == wild.labels and of.untidy(op).coeffs.tolist() == wild.coeffs.tolist()


def test_the_counts_are_the_kernels():
    """kChunk of pauli_groups_kernel (kernels.hip) and kObsChunk (kernels.hpp), read from the source."""
    csrc = Path(of.__file__).resolve().parent.parent / "queasars_amd" / "csrc"
    chunk = re.search(r"constexpr uint32_t kChunk = (\d+);", (csrc / "kernels.hip").read_text())
    obs = re.search(r"constexpr uint32_t kObsChunk = (\d+);", (csrc / "kernels.hpp").read_text())
    assert chunk and obs and (int(chunk.group(1)), int(obs.group(1))) == (of.K_CHUNK, of.K_OBS_CHUNK)
    k, r = of.K_CHUNK, of.K_OBS_CHUNK
    assert set(of.GROUP_COUNTS) == {k - 1, k, k + 1, 2 * k + 1, r, r + 1} and r - 1 != k
    assert 1 << 10 == 2 * r  # (all_z_strings(10, n): exactly two rows)


def test_the_families_leave_the_benchmarks_operators():
    """Printed: the largest x-mask group, the number of groups and the mean string weight of the suite's operators next to the
    families'.  Conditions: the suite's general operator has no group beyond a handful of terms and weight about 3n / 4; the
    families hold groups of hundreds and strings of weight below 2."""
    n = 20
    rows = [("random_ising_operator(20)", helpers.random_ising_operator(n, seed=1)),
            ("random_pauli_operator(20, 500)", helpers.random_pauli_operator(n, 500, seed=1)),
            ("transverse_ising", of.transverse_ising(n, True)), ("heisenberg", of.heisenberg(n, True)), ("hopping", of.hopping(n, 40)),
            ("one_group 257", of.one_group(n, of.K_CHUNK + 1, "random")), ("one_group 513", of.one_group(n, of.K_OBS_CHUNK + 1, "high")),
            ("all_z_strings(10)", of.all_z_strings(10, n)), ("parities", of.parities(n)), ("unweighted_cut", of.unweighted_cut(n, 3)),
            ("placed across general", of.placed(n, (1 << 10) - 1, ((1 << 10) - 1) << 10, "across", "general"))]
    print()
    stats = {}
    for name, op in rows:
        diag, groups = of.groups_of(op)
        stats[name] = (diag, len(groups), max((c for _, c in groups), default=0), of.mean_weight(op))
        print(f"{name:32s} terms {len(op):4d} diagonal {diag:4d} groups {len(groups):3d} largest group {stats[name][2]:3d} "
              f"mean weight {stats[name][3]:5.2f}")
    assert stats["random_pauli_operator(20, 500)"][2] <= 8 and stats["random_pauli_operator(20, 500)"][3] > 13
    assert stats["one_group 257"][2] == 257 and stats["one_group 513"][2] == 513 and stats["all_z_strings(10)"][0] == 1024
    assert stats["transverse_ising"][3] < 2 and stats["heisenberg"][3] < 2


@pytest.mark.parametrize("n", [5, 7])
def test_the_adjoint_gradient_is_the_dense_gradient(n):
    """operator_families.adjoint_gradient (the reference of the GPU half's gradients at 14 qubits, where dense_gradient's
    2^n x 2^n matrix does not fit) against dense_gradient.gradient: shared parameters, literals, cu3 in both directions."""
    import dense_gradient

    for c, p in (cf.generic(n, 40, share=0.3, literal=0.3, seed=n), cf.two_blocks(n, 2)):
        for op in (of.heisenberg(n, True), of.untidy(of.hopping(n, 4)), of.unweighted_cut(n, 3), of.parities(n)):
            want = dense_gradient.gradient(c, p, dense_gradient.dense_operator(op))
            got = of.adjoint_gradient(c, p, op)
            assert got.shape == want.shape and np.abs(got - want).max() < 1e-12 * max(1.0, float(np.abs(op.coeffs).sum()))
