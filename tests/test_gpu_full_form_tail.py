"""The stretch between a side's Gram sums and the result on the one-launch route, for sides on the FULL form (kernels.hip
``fused_factor_tail``, ``factor_side_body``: only the weights a side has are added across the lanes and written, and nothing
else is read; ``factor_sum_partials``, the hand-off, the combination).  Work on that stretch may not move a bit: every sum keeps
its order.  Asked here of every shape the stretch takes -- zero keys (one entry a weight; 10 + 10 and 8 + 12: sides of four and of
eight Gram waves, of two, four and six block bits out of the ten accumulators), one key (11 + 11), two keys with
``"final_controls"`` off (12 + 12, sixteen entries), three keys with it off (13 + 13: half sides, four partial tables an
evaluation), and one launch that holds a reduced three-key circuit beside zero- and one-key ones (the full form inside the
instantiation of reduced sides) -- : the value against the C oracle within ``EXP_TOL``, the same bits alone, together, reversed
and on every repetition, with launches replayed and not, and the bits the commit before
profiles/r27_full_form_tail.txt gave on the GPU (``golden/full_form_tail_parent.json``, hex doubles).

Shapes: the route exists only where the handle's geometry is k = 12, r = 4, and 20 qubits is the smallest such register."""

import json
from pathlib import Path

import numpy as np
import pytest

import helpers
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator
from test_gpu_reduced_handoff import EXP_TOL, N, two_blocks

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "full_form_tail_parent.json"
CROSS3 = [(1, 12), (3, 14), (17, 6)]
# name: (qubits of the first block, cross gates, qubits rotated afterwards, "final_controls", keys, the sides as launched, halves)
SHAPES = {
    "zero keys, 10 + 10": (10, [], (), 1, 0, (10, 10), False),
    "zero keys, 8 + 12": (8, [], (), 1, 0, (8, 12), False),
    "one key, 11 + 11": (10, [(2, 15)], (2,), 1, 1, (11, 11), False),
    "two keys, 12 + 12, full form": (10, [(3, 13), (17, 6)], (), 0, 2, (12, 12), False),
    "three keys, 13 + 13 half sides, full form": (10, CROSS3, (), 0, 3, (13, 13), True),
    "three keys, reduced (1, 1)": (10, CROSS3, (3,), 1, 3, (12, 12), False),
}
FULL_FORM = [name for name in SHAPES if "reduced" not in name]
BESIDE_REDUCED = ["three keys, reduced (1, 1)", "zero keys, 10 + 10", "zero keys, 8 + 12", "one key, 11 + 11"]


def make_cases():
    return {name: two_blocks(spec[0], spec[1], spec[2], seed=90 + i) for i, (name, spec) in enumerate(SHAPES.items())}


def make_operator():
    return helpers.random_ising_operator(N, seed=2020)


def make_evaluators(op):
    """(final_controls, replay_launches) -> evaluator"""
    made = {}
    for final_controls in (1, 0):
        for replay in (1, 0):
            ev = OperatorCircuitEvaluator(op)
            ev.statevector_device.set_option("final_controls", final_controls)  # (read when a circuit is registered: none yet)
            ev.statevector_device.set_option("replay_launches", replay)
            made[final_controls, replay] = ev
    return made


class _Setup:
    def __init__(self, c_oracle):
        self.op = make_operator()
        self.ev = make_evaluators(self.op)
        self.cases = make_cases()
        table, scratch = c_oracle.diagonal_table(self.op), np.zeros(2 << N)
        self.ref = {name: c_oracle.evaluate(c, p, self.op, table, scratch) for name, (c, p) in self.cases.items()}
        self.golden = {name: float.fromhex(text) for name, text in json.loads(GOLDEN.read_text()).items()}
        self.alone = {}  # (name, final_controls) -> the value of the circuit alone, launches replayed

    def value_alone(self, name, final_controls):
        if (name, final_controls) not in self.alone:
            circuit, values = self.cases[name]
            self.alone[name, final_controls] = self.ev[final_controls, 1].evaluate_circuits([circuit], [values])[0]
        return self.alone[name, final_controls]

    def close(self):
        for ev in self.ev.values():
            ev.statevector_device.close()


@pytest.fixture(scope="module")
def setup(c_oracle):
    s = _Setup(c_oracle)
    yield s
    s.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(setup, name):
    s = setup
    _, _, _, final_controls, keys, sizes, halves = SHAPES[name]
    circuit, values = s.cases[name]
    ev, plain = s.ev[final_controls, 1], s.ev[final_controls, 0]
    ev.circuit_costs([circuit])
    dev = ev.statevector_device
    form, launched = dev.circuit_form(circuit), dev.circuit_launch_form(circuit)
    print(name, "form:", form, "launched:", launched)
    assert form["one_launch"] and form["n_keys"] == keys
    assert sorted(launched["n_virtual"]) == sorted(sizes) and bool(launched["halves"]) == halves
    assert (launched != form) == ("reduced" in name)
    got = s.value_alone(name, final_controls)
    for rep in range(10):
        assert ev.evaluate_circuits([circuit], [values]) == [got], rep
        assert plain.evaluate_circuits([circuit], [values]) == [got], rep
    print(f"{got!r} ({got.hex()})  parent {s.golden[name].hex()}  |value - oracle| = {abs(got - s.ref[name]):.3e}")
    assert abs(got - s.ref[name]) < EXP_TOL
    assert got.hex() == s.golden[name].hex()


def _launch_of(s, names, final_controls):
    """One launch holding ``names``: each circuit's bits alone, in either order, on every repetition, replayed or not."""
    cs, ps = [s.cases[name][0] for name in names], [s.cases[name][1] for name in names]
    alone = [s.value_alone(name, final_controls) for name in names]
    ev, plain = s.ev[final_controls, 1], s.ev[final_controls, 0]
    together = ev.evaluate_circuits(cs, ps)
    assert together == alone
    assert ev.evaluate_circuits(cs[::-1], ps[::-1]) == together[::-1]
    assert plain.evaluate_circuits(cs, ps) == together
    assert plain.evaluate_circuits(cs[::-1], ps[::-1]) == together[::-1]
    before = ev.statevector_device.replayed_pushes()
    for rep in range(5):
        assert ev.evaluate_circuits(cs, ps) == together, rep
        assert plain.evaluate_circuits(cs, ps) == together, rep
    assert ev.statevector_device.replayed_pushes() > before
    worst = max(abs(v - s.ref[name]) for v, name in zip(together, names))
    print(f"worst against the oracle: {worst:.3e}")
    assert worst < EXP_TOL
    return together


def test_full_forms_in_one_launch(setup):
    """Every full-form shape in one launch (no reduced side: the tail's other instantiation).  With final controls off the zero-
    and one-key circuits are what they are with them on: the parent's bits again."""
    s = setup
    together = _launch_of(s, FULL_FORM, 0)
    assert [v.hex() for v in together] == [s.golden[name].hex() for name in FULL_FORM]


def test_full_forms_beside_a_reduced_side(setup):
    """A reduced three-key circuit beside zero- and one-key circuits: the launch's tail is the one of reduced sides, and the
    others take its full-form branch."""
    s = setup
    names = BESIDE_REDUCED
    dev = s.ev[1, 1].statevector_device
    s.ev[1, 1].circuit_costs([s.cases[name][0] for name in names])
    assert dev.circuit_launch_form(s.cases[names[0]][0]) != dev.circuit_form(s.cases[names[0]][0])
    together = _launch_of(s, names, 1)
    assert [v.hex() for v in together] == [s.golden[name].hex() for name in names]
