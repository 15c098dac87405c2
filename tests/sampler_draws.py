"""The samplers' draws restated on the host (test infrastructure): every shot of ``qsv_sample_batch`` is a deterministic
function of (seed, evaluation, shot) and of the probabilities, so the host can say which state each shot must be.

* ``shot_uniform`` is ``kernels.hip``'s: SplitMix64 of the seed and the evaluation gives a stream, SplitMix64 of the stream
  and the shot gives 64 bits, their top 53 bits the uniform number u in [0, 1).
* The plain sampler (``sample_kernel``) walks the states in index order and takes the first whose inclusive running sum
  exceeds u * total.
* The split sampler (``split_sample_body``) walks them x-major: x over the states of side x (``circuit_form``'s mask_x),
  y over side y inside it, the state index deposit(x, mask_x) | deposit(y, mask_y).

A device draw s of uniform u is *accepted* if p(s) > 0 and u * total lies within ``delta`` of s's interval
[C(s), C(s) + p(s)) of the CDF in the sampler's order (C from the exact probabilities, summed in extended precision).
The device sums its own (rounded) probabilities in its own order, so a shot that falls within rounding of a boundary
may take the neighbour; any other difference is a wrong draw.

delta:

* fp64: ``DELTA_FP64`` = 1e-9 -- a million times the rounding of a running sum over 2^20 doubles, a thousandth of
  what a draw moved by a state of probability 1e-6 is off.
* fp32 (n <= 16): ``DELTA_FP32`` = 2 * FP32_REL = 4e-6.  C(s) is the expectation value of a projector (norm 1), held to
  FP32_REL like every fp32 expectation value per unit of sum |c|; the device's total (the identity's expectation) once
  more.
"""

from __future__ import annotations

import numpy as np

FP32_REL = 2e-6  # (tests/test_gpu_configs.py's fp32 bound per unit of sum |c_k|)
DELTA_FP64 = 1e-9
DELTA_FP32 = 2 * FP32_REL

_M64 = (1 << 64) - 1


def splitmix64(x) -> np.ndarray:
    """SplitMix64's output function (kernels.hip ``splitmix64``: the state advanced by the golden gamma, then mixed) on
    uint64 arrays, wrapping like the device's 64-bit arithmetic."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def shot_uniform(seed: int, evaluation, shot) -> np.ndarray:
    """kernels.hip ``shot_uniform``: the uniform number in [0, 1) of shot ``shot`` of evaluation ``evaluation`` (both may
    be arrays; they broadcast)."""
    evaluation = np.asarray(evaluation, dtype=np.uint64)
    shot = np.asarray(shot, dtype=np.uint64)
    with np.errstate(over="ignore"):
        stream = splitmix64(np.uint64(seed & _M64) + np.uint64(0xD1B54A32D192ED03) * (evaluation + np.uint64(1)))
        bits = splitmix64(stream ^ splitmix64(shot + np.uint64(1)))
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def deposit(values, mask: int) -> np.ndarray:
    """pdep: the bits of ``values`` (low first) placed at the set bits of ``mask``."""
    values = np.asarray(values, dtype=np.uint64)
    out = np.zeros_like(values)
    src = 0
    for q in range(64):
        if mask >> q & 1:
            out |= ((values >> np.uint64(src)) & np.uint64(1)) << np.uint64(q)
            src += 1
    return out


def plain_order(n: int) -> np.ndarray:
    """The plain sampler's order of states: index order."""
    return np.arange(1 << n, dtype=np.uint64)


def split_order(mask_x: int, mask_y: int) -> np.ndarray:
    """The split sampler's order of states: x-major, state = deposit(x, mask_x) | deposit(y, mask_y)."""
    bx, by = bin(mask_x).count("1"), bin(mask_y).count("1")
    if mask_x & mask_y:
        raise ValueError("the two sides' masks overlap")
    xs = deposit(np.arange(1 << bx, dtype=np.uint64), mask_x)
    ys = deposit(np.arange(1 << by, dtype=np.uint64), mask_y)
    return (xs[:, None] | ys[None, :]).reshape(-1)


class DrawCheck:
    """The CDF of ``probs`` (indexed by state) in the order ``order`` (a permutation of the states), and the checks of
    device draws against it."""

    def __init__(self, probs: np.ndarray, order: np.ndarray, delta: float):
        probs = np.asarray(probs, dtype=np.float64)
        order = np.asarray(order, dtype=np.int64)
        if order.shape != probs.shape or not np.array_equal(np.sort(order), np.arange(probs.size)):
            raise ValueError("order must be a permutation of the states")
        self.probs = probs
        self.order = order
        self.delta = float(delta)
        p = probs[order].astype(np.longdouble)
        inclusive = np.cumsum(p)
        self.inclusive = inclusive
        self.total = inclusive[-1]
        self.position = np.empty(probs.size, dtype=np.int64)
        self.position[order] = np.arange(probs.size)
        self.before = inclusive - p  # C(s) at position k

    def targets(self, u: np.ndarray) -> np.ndarray:
        return np.asarray(u, dtype=np.longdouble) * self.total

    def exact(self, u: np.ndarray) -> np.ndarray:
        """The state an exact inverse CDF draws for each u: the first in order whose inclusive sum exceeds u * total (never
        a state of probability zero)."""
        k = np.searchsorted(self.inclusive, self.targets(u), side="right")
        k = np.minimum(k, self.probs.size - 1)
        while True:  # (only at the very end can the clip land on a state of probability zero)
            zero = self.probs[self.order[k]] == 0.0
            if not zero.any():
                break
            k = np.where(zero, k - 1, k)
        return self.order[k].astype(np.uint64)

    def distance(self, u: np.ndarray, states: np.ndarray) -> np.ndarray:
        """How far u * total lies outside each drawn state's interval [C(s), C(s) + p(s)) (0 inside); inf for a state of
        probability zero or out of range."""
        states = np.asarray(states, dtype=np.int64)
        ok = (states >= 0) & (states < self.probs.size)
        s = np.where(ok, states, 0)
        k = self.position[s]
        t = self.targets(u)
        lo, hi = self.before[k], self.inclusive[k]
        d = np.maximum(np.maximum(lo - t, t - hi), np.longdouble(0)).astype(np.float64)
        return np.where(ok & (self.probs[s] > 0.0), d, np.inf)

    def accepted(self, u: np.ndarray, states: np.ndarray) -> np.ndarray:
        return self.distance(u, states) <= self.delta

    def report(self, u: np.ndarray, states: np.ndarray) -> dict:
        """Accepted shots, shots that differ from the exact draw, and the worst distance."""
        d = self.distance(u, states)
        differ = np.asarray(states, dtype=np.uint64) != self.exact(u)
        return {"shots": int(d.size), "rejected": int((d > self.delta).sum()), "differ": int(differ.sum()),
                "differ_fraction": float(differ.mean()) if d.size else 0.0, "worst": float(d.max()) if d.size else 0.0}
