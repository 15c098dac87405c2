"""Three-key evaluations of the one-launch route with a side on the reduced form hand off and combine only the LIVE entries of
their Gram tables (option ``"live_entries"``, csrc/kernels.hpp ``live_entry``; kernels.hip ``fused_factor_tail``): the terms left
out are exact zeros and the others keep their order, so the option must not move a bit.  Asked here of every three-key shape
of final controls -- one on each side, two and one, one on either side beside a thirteen-qubit side on two halves, two on one
side, none (the untouched path) -- : option on == option off bit for bit, both within ``EXP_TOL`` of the C oracle, the same bits
on every repetition; and of one launch that holds them all beside a two-key reduced, a zero-key and a one-key circuit: together
== alone == reversed, on == off, from host lists and from a device matrix (replayed pushes), and after the option was flipped.

Shapes: the route exists only where the handle's geometry is k = 12, r = 4, and 20 qubits is the smallest such register."""

import numpy as np
import pytest

import helpers
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator
from test_final_controls import first_split
from test_gpu_reduced_handoff import EXP_TOL, N, two_blocks

pytestmark = pytest.mark.gpu

CROSS = [(1, 12), (3, 14), (17, 6)]  # keys 0 and 1 controlled from the first block, key 2 from the second
# name: (cross gates, qubits rotated afterwards -- such a control is not final --, keys, final keys on (first block's side, the other),
#        virtual qubits of the two sides as the route launches them)
THREE_KEYS = {
    "finals (1, 1)": (CROSS, (3,), 3, (1, 1), (12, 12)),
    "finals (2, 1)": (CROSS, (), 3, (2, 1), (11, 12)),
    "finals (1, 0), the other side on two halves": (CROSS, (1, 17), 3, (1, 0), (12, 13)),
    "finals (0, 1), the other side on two halves": (CROSS, (1, 3), 3, (0, 1), (13, 12)),
    "finals (2, 0), the other side on two halves": (CROSS, (17,), 3, (2, 0), (11, 13)),
    "finals (0, 0), the untouched path": (CROSS, (1, 3, 17), 3, (0, 0), (13, 13)),
}
OTHERS = {
    "two keys, one final a side": ([(3, 13), (17, 6)], (), 2, (1, 1), (11, 11)),
    "no key": ([], (), 0, (0, 0), (10, 10)),
    "one key, not final": ([(2, 15)], (2,), 1, (0, 0), (11, 11)),
}
SHAPES = {**THREE_KEYS, **OTHERS}


class _Setup:
    def __init__(self, c_oracle):
        self.op = helpers.random_ising_operator(N, seed=2121)
        self.on = OperatorCircuitEvaluator(self.op)
        self.off = OperatorCircuitEvaluator(self.op)
        self.off.statevector_device.set_option("live_entries", 0)
        self.cases = {name: two_blocks(10, spec[0], spec[1], seed=70 + i) for i, (name, spec) in enumerate(SHAPES.items())}
        table, scratch = c_oracle.diagonal_table(self.op), np.zeros(2 << N)
        self.ref = {name: c_oracle.evaluate(c, p, self.op, table, scratch) for name, (c, p) in self.cases.items()}
        self.alone = {}  # name -> the value of the circuit alone, option on (test_shapes; shared with the launch of all)

    def close(self):
        self.on.statevector_device.close()
        self.off.statevector_device.close()


@pytest.fixture(scope="module")
def setup(c_oracle):
    s = _Setup(c_oracle)
    yield s
    s.close()


def _alone(s, name):
    if name not in s.alone:
        s.alone[name] = s.on.evaluate_circuits([s.cases[name][0]], [s.cases[name][1]])[0]
    return s.alone[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(setup, name):
    s = setup
    _, _, keys, finals, launched_sizes = SHAPES[name]
    circuit, values = s.cases[name]
    _, (k, mask_a, sides) = first_split(circuit, (12, 13))
    assert k == keys and mask_a == (1 << 10) - 1
    assert tuple(bin(side["final"]).count("1") for side in sides) == finals
    s.on.circuit_costs([circuit])
    dev = s.on.statevector_device
    form, launched = dev.circuit_form(circuit), dev.circuit_launch_form(circuit)
    print(name, "form:", form, "launched:", launched)
    assert form["one_launch"] and form["n_keys"] == keys
    assert tuple(side["n_virtual"] for side in sides) == launched_sizes
    assert sorted(launched["n_virtual"]) == sorted(launched_sizes) and (launched != form) == (sum(finals) > 0)
    assert bool(launched["halves"]) == (13 in launched_sizes)  # (a thirteen-qubit side: two halves)
    on = _alone(s, name)
    for rep in range(20):
        assert s.on.evaluate_circuits([circuit], [values]) == [on], rep
    off = s.off.evaluate_circuits([circuit], [values])[0]
    for rep in range(20):
        assert s.off.evaluate_circuits([circuit], [values]) == [off], rep
    print(f"on {on!r} off {off!r}  |on - oracle| = {abs(on - s.ref[name]):.3e}  |off - oracle| = {abs(off - s.ref[name]):.3e}")
    assert on == off
    assert abs(on - s.ref[name]) < EXP_TOL and abs(off - s.ref[name]) < EXP_TOL


def test_all_shapes_in_one_launch(setup):
    """Together == alone == reversed, on == off, host lists and a device matrix (replayed pushes), and the option flipped
    between calls of one handle."""
    import torch

    s = setup
    names = list(SHAPES)
    cs, ps = [s.cases[name][0] for name in names], [s.cases[name][1] for name in names]
    alone = [_alone(s, name) for name in names]
    together = s.on.evaluate_circuits(cs, ps)
    assert together == alone
    assert s.on.evaluate_circuits(cs[::-1], ps[::-1]) == together[::-1]
    assert s.off.evaluate_circuits(cs, ps) == together
    assert s.off.evaluate_circuits(cs[::-1], ps[::-1]) == together[::-1]
    worst = max(abs(v - s.ref[name]) for v, name in zip(together, names))
    print(f"worst against the oracle: {worst:.3e}")
    assert worst < EXP_TOL

    width = max(len(p) for p in ps) + 3
    host = np.full((len(cs), width), 1e300)
    for row, p in enumerate(ps):
        host[row, : len(p)] = p
    matrix = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()

    def to_device(ev, feed):
        buf = torch.full((len(cs),), float("nan"), dtype=torch.float64, device="cuda")
        assert ev.evaluate_circuits_to_device(cs, feed, buf.data_ptr())
        torch.cuda.synchronize()
        return buf.cpu().tolist()

    for ev in (s.on, s.off):
        dev = ev.statevector_device
        assert to_device(ev, ps) == together and to_device(ev, matrix) == together
        before = dev.replayed_pushes()
        for _ in range(4):
            assert to_device(ev, matrix) == together
        assert dev.replayed_pushes() > before
        before = dev.replayed_pushes()
        for _ in range(4):
            assert ev.evaluate_circuits(cs, ps) == together
        assert dev.replayed_pushes() > before

    # the option flipped between calls of one handle: the recorded launch is dropped, the next call has the first one's bits
    dev = s.on.statevector_device
    try:
        for value in (0, 1, 0):
            dev.set_option("live_entries", value)
            before = dev.replayed_pushes()
            assert s.on.evaluate_circuits(cs, ps) == together  # (laid out anew: no replay of a launch of the other mode)
            assert dev.replayed_pushes() == before
            assert to_device(s.on, matrix) == together and to_device(s.on, matrix) == together
            assert s.on.evaluate_circuits(cs, ps) == together
    finally:
        dev.set_option("live_entries", 1)
    assert s.on.evaluate_circuits(cs, ps) == together
