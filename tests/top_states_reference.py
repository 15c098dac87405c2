"""The k most probable basis states restated on the host (test infrastructure, NumPy only): what ``qsv_top_states`` must
return for given probabilities, and the checks of a device answer against an oracle's probabilities.

The order is total -- probability descending, basis-state index ascending -- so for ONE array of probabilities the answer
is unique (``expected_top``).  The device and an oracle round differently, so near ties they may disagree about which of two
states comes first or is the last one in; ``check_top`` therefore does not ask for set equality but for

1. distinct states below 2^n,
2. every returned probability within ``tol`` of the oracle's at that state,
3. the returned probabilities in non-increasing order, equal neighbours in ascending index (exact: the device's own order),
4. completeness: no state left out whose oracle probability exceeds the smallest returned one by more than ``2 tol``
   (one ``tol`` for each of the two probabilities the device compared).

tol: fp64 ``TOL_FP64`` = 1e-13, the bound tests/test_gpu_parity.py holds device probabilities to; fp32 (n <= 16)
``FP32_REL`` = 2e-6 -- a probability is the expectation value of a projector of norm 1 (tests/sampler_draws.py).
"""

from __future__ import annotations

import numpy as np

TOL_FP64 = 1e-13
FP32_REL = 2e-6  # (tests/test_gpu_configs.py's fp32 bound per unit of sum |c_k|)


def expected_top(probs: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """(states, probabilities) of the first ``k`` entries of ``probs`` by probability descending, index ascending."""
    probs = np.asarray(probs, dtype=np.float64)
    if not 1 <= k <= probs.size:
        raise ValueError("k must be between 1 and the number of states")
    index = np.arange(probs.size)
    order = np.lexsort((index, -probs))[:k]
    return order.astype(np.uint64), probs[order]


def check_top(states: np.ndarray, probs_got: np.ndarray, oracle_probs: np.ndarray, k: int, tol: float) -> None:
    states = np.asarray(states)
    probs_got = np.asarray(probs_got, dtype=np.float64)
    oracle_probs = np.asarray(oracle_probs, dtype=np.float64)
    assert states.shape == (k,) and probs_got.shape == (k,), (states.shape, probs_got.shape, k)
    # 1. distinct, in range
    assert int(states.max()) < oracle_probs.size, int(states.max())
    index = states.astype(np.int64)
    assert np.unique(index).size == k, "a state was returned twice"
    # 2. the probabilities are the oracle's at those states
    worst = float(np.abs(probs_got - oracle_probs[index]).max())
    assert worst <= tol, f"a returned probability is {worst} off the oracle (tol {tol})"
    # 3. the device's own order
    assert np.all(probs_got[:-1] >= probs_got[1:]), "probabilities are not in non-increasing order"
    equal = probs_got[:-1] == probs_got[1:]
    assert np.all(index[:-1][equal] < index[1:][equal]), "equal probabilities are not in ascending index order"
    # 4. completeness
    left_out = np.ones(oracle_probs.size, dtype=bool)
    left_out[index] = False
    if left_out.any():
        best_left_out = float(oracle_probs[left_out].max())
        assert best_left_out <= float(probs_got.min()) + 2 * tol, (
            f"a state of probability {best_left_out} was left out, the smallest returned one is {float(probs_got.min())}"
        )
