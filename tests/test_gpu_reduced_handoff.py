"""The table a reduced side hands off on the one-launch route (kernels.hip ``factor_reduced_rows`` / ``factor_reduced_value``):
what a thread's entry alone decides is worked out once per thread, the weight's slot and the sum once per value.  Asked here of
every shape of that table -- one, two and three keys (4, 16 and 64 entries a weight: sixteen, four and one weight per wave of
the store loop), final controls on one side or both, and sides of nine and eleven real qubits beside the benchmark's ten (the
weight slots of positions 8 .. 10 lie in the second slot word) -- : the value against the C oracle and against the full form
(option ``"final_controls"`` off) within ``EXP_TOL``, and the same bits alone, together, reversed and on every repetition.

Shapes: the route exists only where the handle's geometry is k = 12, r = 4, and 20 qubits is the smallest such register."""

import numpy as np
import pytest

import helpers
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator
from queasars_amd.ir import CircuitIR, ParamRef
from test_final_controls import first_split

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10
N = 20


def two_blocks(first, cross, rotate=(), seed=0):
    """Blocks [0, first) and [first, N), each held together by a chain and a star of cu3, then the cross gates (control, target)
    in order and a last u on every qubit of ``rotate`` (a control that is rotated afterwards is not final)."""
    rng = np.random.default_rng(seed)
    c = CircuitIR(N)
    k = 0

    def angle():
        nonlocal k
        k += 1
        return ParamRef(k - 1)

    for q in range(N):
        c.u(angle(), angle(), angle(), q)
    for block in (list(range(0, first)), list(range(first, N))):
        for a, b in zip(block, block[1:]):
            c.cu3(angle(), angle(), angle(), a, b)
        for b in block[2:]:
            c.cu3(angle(), angle(), angle(), block[0], b)
        for a, b in zip(block[1:], block[2:]):
            c.cu3(angle(), angle(), angle(), b, a)
    for control, target in cross:
        c.cu3(angle(), angle(), angle(), control, target)
    for q in rotate:
        c.u(angle(), angle(), angle(), q)
    assert c.num_parameters == k
    return c, list(rng.uniform(-np.pi, np.pi, size=k))


# name: (qubits of the first block, cross gates, qubits rotated afterwards, keys, final keys on (first block's side, the other))
SHAPES = {
    "9 + 11, one key final on the side of eleven": (9, [(15, 2)], (), 1, (0, 1)),
    "9 + 11, one key final on the side of nine": (9, [(2, 15)], (), 1, (1, 0)),
    "9 + 11, two keys final on the side of eleven": (9, [(12, 2), (16, 4)], (), 2, (0, 2)),
    "9 + 11, two keys, one final a side": (9, [(3, 13), (17, 6)], (), 2, (1, 1)),
    "11 + 9, two keys, one final, one simulated on its control's side": (11, [(2, 13), (4, 15)], (4,), 2, (1, 0)),
    "10 + 10, three keys, every key final": (10, [(1, 12), (3, 14), (17, 6)], (), 3, (2, 1)),
    "10 + 10, three keys, one final": (10, [(1, 12), (3, 14), (17, 6)], (1, 17), 3, (1, 0)),
    "10 + 10, three keys, one final a side": (10, [(1, 12), (3, 14), (17, 6)], (3,), 3, (1, 1)),
}


class _Setup:
    def __init__(self, c_oracle):
        self.op = helpers.random_ising_operator(N, seed=2020)
        self.on = OperatorCircuitEvaluator(self.op)
        self.off = OperatorCircuitEvaluator(self.op)
        self.off.statevector_device.set_option("final_controls", 0)  # (read when a circuit is registered: none yet)
        self.cases = {name: two_blocks(spec[0], spec[1], spec[2], seed=40 + i) for i, (name, spec) in enumerate(SHAPES.items())}
        table, scratch = c_oracle.diagonal_table(self.op), np.zeros(2 << N)
        self.ref = {name: c_oracle.evaluate(c, p, self.op, table, scratch) for name, (c, p) in self.cases.items()}

    def close(self):
        self.on.statevector_device.close()
        self.off.statevector_device.close()


@pytest.fixture(scope="module")
def setup(c_oracle):
    s = _Setup(c_oracle)
    yield s
    s.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(setup, name):
    s = setup
    first, _, _, keys, finals = SHAPES[name]
    circuit, values = s.cases[name]
    _, (k, mask_a, sides) = first_split(circuit, (12, 13))
    assert k == keys and mask_a == (1 << first) - 1
    assert tuple(bin(side["final"]).count("1") for side in sides) == finals
    s.on.circuit_costs([circuit])
    dev = s.on.statevector_device
    form, launched = dev.circuit_form(circuit), dev.circuit_launch_form(circuit)
    print(name, "form:", form, "launched:", launched)
    assert form["one_launch"] and form["n_keys"] == keys
    # (every reduced side here is at most twelve virtual qubits, one tile: the route runs it, and says so)
    assert sorted(launched["n_virtual"]) == sorted(side["n_virtual"] for side in sides) and launched != form
    on = s.on.evaluate_circuits([circuit], [values])
    for rep in range(20):
        assert s.on.evaluate_circuits([circuit], [values]) == on, rep
    off = s.off.evaluate_circuits([circuit], [values])
    print(f"|on - off| = {abs(on[0] - off[0]):.3e}  |on - oracle| = {abs(on[0] - s.ref[name]):.3e}  |off - oracle| = {abs(off[0] - s.ref[name]):.3e}")
    assert abs(on[0] - off[0]) < EXP_TOL and abs(on[0] - s.ref[name]) < EXP_TOL and abs(off[0] - s.ref[name]) < EXP_TOL


def test_shapes_together(setup):
    """One launch holding every shape: each circuit's bits alone, in either order, on every repetition."""
    s = setup
    cs, ps = [s.cases[name][0] for name in SHAPES], [s.cases[name][1] for name in SHAPES]
    together = s.on.evaluate_circuits(cs, ps)
    assert [s.on.evaluate_circuits([c], [p])[0] for c, p in zip(cs, ps)] == together
    assert s.on.evaluate_circuits(cs[::-1], ps[::-1]) == together[::-1]
    for rep in range(10):
        assert s.on.evaluate_circuits(cs, ps) == together, rep
    worst = max(abs(v - s.ref[name]) for v, name in zip(together, SHAPES))
    print(f"worst against the oracle: {worst:.3e}")
    assert worst < EXP_TOL
