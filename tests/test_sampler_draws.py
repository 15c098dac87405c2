"""The host restatement of the samplers' draws (tests/sampler_draws.py) on known values and hand-made distributions: the
GPU tests that hold every shot to it are only as good as it is."""

import numpy as np
import pytest

from sampler_draws import DELTA_FP64, DrawCheck, deposit, plain_order, shot_uniform, split_order, splitmix64


def test_splitmix64_published_values():
    # SplitMix64 seeded with 0: its first outputs (the state advanced by the golden gamma once, twice, three times)
    assert int(splitmix64(0)) == 0xE220A8397B1DCDAF
    assert int(splitmix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    assert int(splitmix64((2 * 0x9E3779B97F4A7C15) % 2**64)) == 0x06C45D188009454F
    # vectorised the same as one by one, wrapping at 2^64
    xs = np.asarray([0, 1, 2**63, 2**64 - 1], dtype=np.uint64)
    assert [int(v) for v in splitmix64(xs)] == [int(splitmix64(int(x))) for x in xs]


def test_uniforms_lie_in_the_unit_interval_with_53_bits():
    u = shot_uniform(12345, np.arange(64)[:, None], np.arange(4096)[None, :])
    assert u.shape == (64, 4096)
    assert (u >= 0.0).all() and (u < 1.0).all()
    scaled = u * 2.0**53
    assert np.array_equal(scaled, np.floor(scaled))  # multiples of 2^-53
    assert (scaled % 2 == 1).any() and u.min() < 1e-3 and u.max() > 1 - 1e-3  # the lowest bit is used, the range covered
    assert abs(float(u.mean()) - 0.5) < 0.01
    # a stream per evaluation, a counter per shot: the seed, the evaluation and the shot each change the number
    assert shot_uniform(1, 0, 0) != shot_uniform(2, 0, 0)
    assert shot_uniform(1, 0, 0) != shot_uniform(1, 1, 0) != shot_uniform(1, 1, 1)
    # the function itself, restated by hand for one shot
    m = 2**64 - 1
    stream = int(splitmix64((7 + 0xD1B54A32D192ED03 * 4) & m))
    bits = int(splitmix64(stream ^ int(splitmix64(5 + 1))))
    assert float(shot_uniform(7, 3, 5)) == (bits >> 11) / 2.0**53


def test_deposit_and_the_split_order():
    assert [int(v) for v in deposit(np.arange(4), 0b1010)] == [0b0000, 0b0010, 0b1000, 0b1010]
    order = split_order(0b0101, 0b1010)  # x-major: x over qubits 0 and 2, y over 1 and 3
    assert [int(v) for v in order[:4]] == [0b0000, 0b0010, 0b1000, 0b1010]
    assert [int(v) for v in order[4:8]] == [0b0001, 0b0011, 0b1001, 0b1011]
    assert sorted(int(v) for v in order) == list(range(16))
    with pytest.raises(ValueError):
        split_order(0b11, 0b10)


def test_inverse_cdf_on_hand_made_distributions():
    # a single state
    one = np.zeros(8)
    one[5] = 1.0
    check = DrawCheck(one, plain_order(3), DELTA_FP64)
    u = np.asarray([0.0, 0.25, 0.999999])
    assert [int(s) for s in check.exact(u)] == [5, 5, 5]
    assert check.accepted(u, np.asarray([5, 5, 5])).all()
    assert not check.accepted(u, np.asarray([4, 6, 0])).any()  # (probability zero: never)
    # zero-probability states interleaved
    probs = np.asarray([0.0, 0.25, 0.0, 0.0, 0.5, 0.0, 0.25, 0.0])
    check = DrawCheck(probs, plain_order(3), DELTA_FP64)
    u = np.asarray([0.0, 0.1, 0.3, 0.7, 0.8, 0.99])
    assert [int(s) for s in check.exact(u)] == [1, 1, 4, 4, 6, 6]
    # u exactly on a boundary: the state above it (the first inclusive sum that EXCEEDS u)
    assert [int(s) for s in check.exact(np.asarray([0.25, 0.75]))] == [4, 6]
    # in another order the same probabilities give other states
    order = np.asarray([6, 5, 4, 3, 2, 1, 0, 7])
    rev = DrawCheck(probs, order, DELTA_FP64)
    assert [int(s) for s in rev.exact(np.asarray([0.1, 0.3, 0.8]))] == [6, 4, 1]


def test_the_acceptance_rule():
    probs = np.asarray([0.1, 0.2, 0.3, 0.4])
    check = DrawCheck(probs, plain_order(2), DELTA_FP64)
    u = np.asarray([0.05, 0.2, 0.45, 0.8])
    exact = check.exact(u)
    assert [int(s) for s in exact] == [0, 1, 2, 3]
    assert check.accepted(u, exact).all()
    # a draw moved by one state, either way, is rejected
    assert not check.accepted(u[:3], exact[:3] + np.uint64(1)).any()
    assert not check.accepted(u[1:], exact[1:] - np.uint64(1)).any()
    # a tie at a boundary: u * total = C(2) -- the state below (its interval's closed end) and the one above are both right
    tie = np.asarray([0.3, 0.3])
    assert check.accepted(tie, np.asarray([1, 2])).all()
    # ... and within delta of it, too; beyond delta, no
    near = np.asarray([0.3 + 0.5 * DELTA_FP64])
    assert check.accepted(near, np.asarray([1])).all()
    far = np.asarray([0.3 + 4 * DELTA_FP64])
    assert not check.accepted(far, np.asarray([1])).any()
    # (the tie counts as accepted but may differ from the exact draw; the moved one is both)
    rep = check.report(np.asarray([0.05, 0.3, 0.45]), np.asarray([0, 2, 3]))
    assert rep["rejected"] == 1 and rep["differ"] == 2 and rep["shots"] == 3
    # a state out of range is a rejection, not an error
    assert not check.accepted(np.asarray([0.5]), np.asarray([99])).any()


def test_a_kernel_that_moves_every_draw_slightly_is_caught():
    """What a chi-square over 4096 shots cannot see: every u scaled by (1 - 1e-6) before the inverse CDF.  The draws then
    differ from the exact ones only for the few shots near a boundary, but each of those lies beyond delta."""
    rng = np.random.default_rng(3)
    n = 14
    probs = rng.exponential(size=1 << n)
    probs /= probs.sum()
    order = split_order(0b10110100101101, 0b01001011010010)
    check = DrawCheck(probs, order, DELTA_FP64)
    u = shot_uniform(9, 0, np.arange(1 << 16))
    moved = check.exact(u * (1 - 1e-6))
    assert not check.accepted(u, moved).all()
    assert check.accepted(u, check.exact(u)).all()
