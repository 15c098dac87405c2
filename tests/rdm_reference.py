"""References for reduced density matrices of qubit subsets, tests only: rho_A of a NumPy oracle state by
reshape, transpose and einsum, raw (not divided by the norm), and the subset lists the GPU tests use.  Bit j of a row index is the
value of the subset's j-th qubit.  tests/test_rdm_host.py holds this to facts."""

from __future__ import annotations

import functools
from itertools import combinations

import numpy as np

import helpers
import overlap_reference as ovr

#: |rho - reference| per component in fp64: the bound of an overlap (overlap_reference.TOL_S) for the same kind of sum, 2^n
#: products of amplitudes with |entry| <= 1
TOL = 1e-11


def tol_fp32(e_s: float) -> float:
    """On an fp32 handle, e_s the largest |psi_32 - psi_ref|_2 of the handle's statevector() over the test's own circuits: as
    overlap_reference.tol_fp32."""
    return ovr.tol_fp32(e_s)


def reduced_density_matrix(state: np.ndarray, subset) -> np.ndarray:
    """rho_A[a][a'] = sum_b psi(a, b) conj psi(a', b) for A = subset, in the caller's order."""
    state = np.asarray(state, dtype=np.complex128)
    n = int(state.size).bit_length() - 1
    assert state.size == 1 << n
    subset = [int(q) for q in subset]
    k = len(subset)
    assert 1 <= k <= n and len(set(subset)) == k and all(0 <= q < n for q in subset)
    # (axis i of the reshaped state is qubit n - 1 - i; the subset's LAST qubit is the row index's highest bit, so it goes first)
    rest = [q for q in range(n - 1, -1, -1) if q not in subset]
    axes = [n - 1 - q for q in reversed(subset)] + [n - 1 - q for q in rest]
    m = state.reshape((2,) * n).transpose(axes).reshape(1 << k, 1 << (n - k))
    return np.einsum("ab,cb->ac", m, m.conj())


def reduced_density_matrices(states, subsets) -> list[np.ndarray]:
    """One (len(states), 2^k, 2^k) array per subset, as the device method returns them."""
    return [np.stack([reduced_density_matrix(s, subset) for s in states]) for subset in subsets]


def max_component_error(got, want) -> float:
    return ovr.max_component_error(np.asarray(got), np.asarray(want))


def largest_error(got_list, want_list) -> float:
    return max(max_component_error(g, w) for g, w in zip(got_list, want_list))


def subsets_for(n: int) -> list[tuple[int, ...]]:
    """The subsets a register of n qubits is asked for, where they exist: single qubits 0, 5, 6 and n - 1; two, three and four
    qubits on the lowest, on the highest, across the boundary between qubit 5 and qubit 6, and in non-ascending order; the whole
    register up to four qubits."""
    wanted: list[tuple[int, ...]] = [(0,), (5,), (6,), (n - 1,)]
    for k in (2, 3, 4):
        wanted.append(tuple(range(k)))                     # the lowest
        wanted.append(tuple(range(n - k, n)))              # the highest
    wanted += [(5, 6), (0, 6, 5), (0, 5, 6, n - 1), (4, 5, 6, 7)]   # across qubit 5 | 6
    wanted += [(n - 1, 0), (2, 0, 1), (7, 2, 9, 0), (n - 1, 3, 0), (3, 2, 1, 0), (n - 1, 1, n - 2, 0)]  # non-ascending
    if n <= 4:
        wanted.append(tuple(range(n)))                     # k = n: rho = |psi><psi|
        wanted.append(tuple(reversed(range(n))))
    seen, out = set(), []
    for subset in wanted:
        if len(subset) <= n and len(set(subset)) == len(subset) and all(0 <= q < n for q in subset) and subset not in seen:
            seen.add(subset)
            out.append(subset)
    return out


def all_pairs(n: int) -> list[tuple[int, int]]:
    return list(combinations(range(n), 2))


def singles_and_pairs(n: int) -> list[tuple[int, ...]]:
    return [(q,) for q in range(n)] + all_pairs(n)


@functools.lru_cache(maxsize=None)
def population(n: int, layers: int, count: int, seed: int, perturbed: bool = False):
    """(circuits, parameter values, oracle states), computed once (overlap_reference.population)."""
    return ovr.population(n, layers, count, seed, perturbed)


@functools.lru_cache(maxsize=None)
def case(n: int, count: int):
    """(circuits, parameter values, oracle states) of `count` evaluations of a register, computed once: the benchmark's
    population and, where there is room, one ladder and one all-pairs circuit of tests/circuit_families.py behind it.  From
    n = 11 on these are the first half, and the second half runs the same circuits again at slightly perturbed parameters (as
    overlap_reference.population perturbs)."""
    import circuit_families as cf

    half = (count + 1) // 2 if n >= 11 else count
    extra = ([cf.ladder(n, seed=n), cf.all_pairs(n, seed=n)] if n >= 2 else [])[: max(0, half - 1)]
    circuits, params, states = population(n, 3, half - len(extra), n)
    circuits, params, states = list(circuits), [list(p) for p in params], list(states)
    for circuit, values in extra:
        circuits.append(circuit)
        params.append(list(values))
        states.append(helpers.oracle_state(circuit, values))
    rng = np.random.default_rng(77 + n)
    for i in range(count - half):
        circuits.append(circuits[i])
        params.append([float(v + rng.normal(0.0, 0.05)) for v in params[i]])
        states.append(helpers.oracle_state(circuits[i], params[-1]))
    return circuits, params, states


def kron_reordered(factors, subset) -> np.ndarray:
    """rho of a product state over `subset` from its blocks' matrices: factors = [(rho_b, qubits_b)], the qubits_b disjoint and
    together the subset; the Kronecker product, with rows and columns reordered so that bit j is subset[j]."""
    order = [q for _, qubits in factors for q in qubits]
    assert sorted(order) == sorted(subset)
    rho = np.ones((1, 1), dtype=np.complex128)
    for block, _ in factors:  # (the first factor's bits lowest: kron(later, earlier))
        rho = np.kron(block, rho)
    k = len(subset)
    index = np.arange(1 << k)
    source = np.zeros_like(index)  # the place in `order`'s convention of the setting a in `subset`'s convention
    for j, q in enumerate(subset):
        source |= ((index >> j) & 1) << order.index(q)
    return rho[np.ix_(source, source)]
