"""The one-launch route on the reduced split form (option ``"final_controls"``, csrc/split.hpp ``reduce_final_controls``): a
side simulates no key qubit for a key whose control on it is final, its Gram sums run over the blocks of x the final controls
name and the table it hands off keeps the full form's layout.  Asked here: the route (``circuit_form``, which describes the
full form) and the reduced sizes (``qsv_split_describe_reduced``); option on against off and each against an oracle at ``EXP_TOL``; the same bits on every
repetition, alone, together, reversed, from either parameter feed, with ``side_prepare`` on or off, under replay and in a mixed
batch; single precision; and the routes that keep the full form (a general operator, the split sampler) on the same handle.

Shapes: the route exists only where the handle's geometry is k = 12, r = 4, and 20 qubits is the smallest such register: two
dense blocks of 10 + 10 qubits joined by one to three cross gates, every pattern of final and simulated keys one at a time, and
circuits 41 (three keys, a final control on each side: 13 + 13 virtual qubits become 12 + 12) and 22 of the benchmark's
population.
"""

import numpy as np
import pytest

import helpers
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator
from queasars_amd.ir import CircuitIR, ParamRef
from test_final_controls import first_split

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10
FP32_REL = 2e-6  # (per unit of sum |c_k|: tests/test_gpu_configs.py)


def bridged(n, cross, rotate=(), seed=0):
    """Two blocks [0, n/2) and [n/2, n), each held together by a chain and a star of cu3 (no single key cuts a block in two),
    then the cross gates ``cross`` = [(control, target)] in order and a last u on every qubit of ``rotate``.  A cross gate's
    control is final unless something targets it afterwards."""
    rng = np.random.default_rng(seed)
    c = CircuitIR(n)
    k = 0

    def angle():
        nonlocal k
        k += 1
        return ParamRef(k - 1)

    for q in range(n):
        c.u(angle(), angle(), angle(), q)
    for block in (range(0, n // 2), range(n // 2, n)):
        block = list(block)
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


# name: (cross gates, qubits rotated afterwards, keys, final keys on (the side of qubit 0, the other side))
SMALL = {
    "one key, final on one side": ([(2, 13)], (), 1, (1, 0)),
    "two keys, one final, one side": ([(2, 13), (4, 15)], (4,), 2, (1, 0)),
    "two keys, final on both sides": ([(2, 13), (17, 5)], (), 2, (1, 1)),
    "two keys, both final on one side": ([(2, 13), (4, 15)], (), 2, (2, 0)),
    "three keys, every key final": ([(1, 12), (3, 14), (17, 6)], (), 3, (2, 1)),
    "three keys, one final": ([(1, 12), (3, 14), (17, 6)], (1, 17), 3, (1, 0)),
    "two keys, none final": ([(2, 13), (17, 5)], (2, 17), 2, (0, 0)),
}
N = 20


def _forms(ev, circuits):
    ev.circuit_costs(circuits)
    return [ev.statevector_device.circuit_form(c) for c in circuits]


def _launch_forms(ev, circuits):
    """What the one-launch route runs for each circuit on this handle (``qsv_circuit_launch_form``)."""
    ev.circuit_costs(circuits)
    return [ev.statevector_device.circuit_launch_form(c) for c in circuits]


class _Setup:
    def __init__(self, c_oracle):
        self.small = {name: bridged(N, spec[0], spec[1], seed=i) for i, (name, spec) in enumerate(SMALL.items())}
        self.ops, self.on, self.off = {}, {}, {}
        for n in (N,):
            self.ops[n] = helpers.random_ising_operator(n, seed=2020)
            self.on[n] = OperatorCircuitEvaluator(self.ops[n])
            self.off[n] = OperatorCircuitEvaluator(self.ops[n])
            self.off[n].statevector_device.set_option("final_controls", 0)  # (read when a circuit is registered: none yet)
        _, self.circuits, self.params = helpers.population_circuits(20, 4, 64, seed=0)
        _, self.circuits5, self.params5 = helpers.population_circuits(20, 5, 64, seed=0)
        self.oracle = c_oracle
        self.table = c_oracle.diagonal_table(self.ops[20])
        self.scratch = np.zeros(2 << 20)
        self._ref = {}

    def reference(self, i):
        if i not in self._ref:
            self._ref[i] = self.oracle.evaluate(self.circuits[i], self.params[i], self.ops[20], self.table, self.scratch)
        return self._ref[i]

    def close(self):
        for evs in (self.on, self.off):
            for ev in evs.values():
                ev.statevector_device.close()


@pytest.fixture(scope="module")
def setup(c_oracle):
    s = _Setup(c_oracle)
    yield s
    s.close()


def _bits(ev, cs, ps, repetitions=50):
    """The values of the circuits together; the same bits alone, reversed and on every repetition."""
    together = ev.evaluate_circuits(cs, ps)
    assert [ev.evaluate_circuits([c], [p])[0] for c, p in zip(cs, ps)] == together
    assert ev.evaluate_circuits(cs[::-1], ps[::-1]) == together[::-1]
    for rep in range(repetitions):
        assert ev.evaluate_circuits(cs, ps) == together, rep
    return together


@pytest.mark.parametrize("name", list(SMALL))
def test_small_shapes(setup, name):
    """The route, the reduced sizes, on against off against the C oracle, and the bits."""
    s = setup
    n = N
    _, _, keys, finals = SMALL[name]
    circuit, values = s.small[name]
    _, (k, mask_a, sides) = first_split(circuit, (12, 13))
    assert k == keys and mask_a == (1 << (n // 2)) - 1
    assert tuple(bin(side["final"]).count("1") for side in sides) == finals
    form_on, form_off = _forms(s.on[n], [circuit])[0], _forms(s.off[n], [circuit])[0]
    print(name, "on:", form_on, "off:", form_off)
    assert form_on["one_launch"] and form_off["one_launch"] and form_on["n_keys"] == form_off["n_keys"] == keys
    # (circuit_form describes the full form, which every other consumer of the side states runs: the reduced sizes are the
    # describe call's -- twelve virtual qubits at most, so every reduced side here is taken -- and a reduced side shows in the bits)
    full = sorted(len(side["qubits"]) + keys for side in sides)
    assert sorted(form_off["n_virtual"]) == sorted(form_on["n_virtual"]) == full, full
    assert all(side["n_virtual"] <= 12 and side["n_virtual"] == len(side["qubits"]) + keys - bin(side["final"]).count("1") for side in sides if side["final"])
    # (... and the handle says what it launches: every reduced side with the option on, the full form with it off)
    launch_on, launch_off = _launch_forms(s.on[n], [circuit])[0], _launch_forms(s.off[n], [circuit])[0]
    print(name, "launched on:", launch_on, "off:", launch_off)
    assert launch_off == form_off
    assert sorted(launch_on["n_virtual"]) == sorted(side["n_virtual"] for side in sides)
    assert launch_on["outer"] == tuple(int(v == 13) for v in launch_on["n_virtual"])  # (one tile -- but for a side that stays a half side)
    assert (launch_on != form_on) == (sum(finals) > 0)
    assert launch_on["halves"] == (keys == 3 and 13 in launch_on["n_virtual"])  # (a thirteen-qubit side that stays: a half side, as ever)
    on = _bits(s.on[n], [circuit], [values])
    off = _bits(s.off[n], [circuit], [values], repetitions=3)
    ref = s.oracle.evaluate(circuit, values, s.ops[n], s.table, s.scratch)
    print(f"|on - off| = {abs(on[0] - off[0]):.3e}  |on - oracle| = {abs(on[0] - ref):.3e}  |off - oracle| = {abs(off[0] - ref):.3e}")
    assert abs(on[0] - off[0]) < EXP_TOL and abs(on[0] - ref) < EXP_TOL and abs(off[0] - ref) < EXP_TOL
    if sum(finals) == 0:
        assert on == off  # (no key final: the full form, the same bits)
    else:
        print("same bits with the option off" if on == off else "other bits with the option off")  # (either may be: other orders of the sums)


def test_small_shapes_together(setup):
    """Every shape in one batch, reduced and not: the bits of each alone."""
    s = setup
    cs, ps = [s.small[name][0] for name in SMALL], [s.small[name][1] for name in SMALL]
    together = _bits(s.on[N], cs, ps, repetitions=10)
    off = s.off[N].evaluate_circuits(cs, ps)
    assert np.abs(np.asarray(together) - np.asarray(off)).max() < EXP_TOL


def test_benchmark_circuits_against_the_c_oracle(setup):
    """Circuits 41 and 22 of the headline population: the forms the issue names, on and off against the C oracle."""
    s = setup
    idx = [41, 22]
    cs, ps = [s.circuits[i] for i in idx], [s.params[i] for i in idx]
    on_forms, off_forms = _forms(s.on[20], cs), _forms(s.off[20], cs)
    print("on:", on_forms, "off:", off_forms)
    assert on_forms == off_forms and on_forms[0]["n_keys"] == 3 and sorted(on_forms[0]["n_virtual"]) == [13, 13] and on_forms[1]["n_keys"] == 2
    for i, sizes in zip(idx, ([12, 12], [11, 12])):  # (what the one-launch route runs with the option on)
        _, (_, _, sides) = first_split(s.circuits[i], (12, 13))
        assert sorted(side["n_virtual"] for side in sides) == sizes
    launched_on, launched_off = _launch_forms(s.on[20], cs), _launch_forms(s.off[20], cs)
    print("launched on:", launched_on, "off:", launched_off)
    assert launched_off == off_forms and off_forms[0]["halves"]
    assert [sorted(f["n_virtual"]) for f in launched_on] == [[12, 12], [11, 12]] and not any(f["halves"] for f in launched_on)
    assert all(f["one_launch"] and f["amps_per_thread"] == 8 for f in on_forms + off_forms)
    on = _bits(s.on[20], cs, ps)
    off = _bits(s.off[20], cs, ps, repetitions=3)
    for i, a, b in zip(idx, on, off):
        print(f"circuit {i}: |on - off| = {abs(a - b):.3e}  |on - oracle| = {abs(a - s.reference(i)):.3e}  |off - oracle| = {abs(b - s.reference(i)):.3e}")
        assert abs(a - b) < EXP_TOL and abs(a - s.reference(i)) < EXP_TOL and abs(b - s.reference(i)) < EXP_TOL


def test_whole_populations_on_against_off(setup):
    """The four- and five-layer populations: circuits without a final control keep their bits, the others stay within
    EXP_TOL; a reduced side next to a half side (a three-key circuit with one final control) among the five-layer ones."""
    s = setup
    for cs, ps in ((s.circuits, s.params), (s.circuits5, s.params5)):
        on_forms, off_forms = _forms(s.on[20], cs), _forms(s.off[20], cs)
        on, off = s.on[20].evaluate_circuits(cs, ps), s.off[20].evaluate_circuits(cs, ps)
        assert on_forms == off_forms
        finals = [first_split(c, (12, 13))[1] for c in cs]
        changed = [i for i, got in enumerate(finals) if got is not None and any(side["final"] for side in got[2])]
        assert changed and all(on[i] == off[i] for i in range(len(cs)) if i not in changed)
        assert sum(on[i] != off[i] for i in changed) >= len(changed) // 2
        assert np.abs(np.asarray(on) - np.asarray(off)).max() < EXP_TOL
        assert s.on[20].evaluate_circuits(cs[::-1], ps[::-1]) == on[::-1]
    beside = [i for i in changed if finals[i][0] == 3 and sorted(side["n_virtual"] for side in finals[i][2]) == [12, 13] and on_forms[i]["halves"]]
    assert beside and all(on[i] != off[i] for i in beside), "a reduced side beside a half side"
    launched = _launch_forms(s.on[20], [cs[i] for i in beside])
    assert all(sorted(f["n_virtual"]) == [12, 13] and f["halves"] for f in launched), launched


def test_feeds_side_prepare_and_replay(setup):
    """Host lists against a device matrix, ``side_prepare`` on and off, and a replayed push: the same bits."""
    import torch

    s = setup
    ev, dev = s.on[20], s.on[20].statevector_device
    idx = [41, 22, 1, 8]
    cs, ps = [s.circuits[i] for i in idx], [s.params[i] for i in idx]
    want = ev.evaluate_circuits(cs, ps)
    width = max(len(p) for p in ps) + 3
    host = np.full((len(cs), width), 1e300)
    for row, p in enumerate(ps):
        host[row, : len(p)] = p
    matrix = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()

    def to_device(feed):
        buf = torch.full((len(cs),), float("nan"), dtype=torch.float64, device="cuda")
        assert ev.evaluate_circuits_to_device(cs, feed, buf.data_ptr())
        torch.cuda.synchronize()
        return buf.cpu().tolist()

    assert to_device(ps) == want and to_device(matrix) == want
    before = dev.replayed_pushes()
    for _ in range(4):
        assert to_device(matrix) == want
    assert dev.replayed_pushes() > before
    try:
        dev.set_option("side_prepare", 0)
        assert ev.evaluate_circuits(cs, ps) == want and to_device(matrix) == want
    finally:
        dev.set_option("side_prepare", 1)
    assert ev.evaluate_circuits(cs, ps) == want


def test_mixed_batch(setup):
    """Reduced circuits between circuits on the ordinary plan (nine layers: not split) and a half-sided three-key circuit of
    the five-layer population: the bits of each one by one."""
    s = setup
    ev = s.on[20]
    _, deep, pd = helpers.population_circuits(20, 9, 2, seed=8)
    forms5 = _forms(ev, s.circuits5)
    half = next(i for i, f in enumerate(forms5) if f["halves"] and f["n_keys"] == 3
                and not any(side["final"] for side in first_split(s.circuits5[i], (12, 13))[1][2]))
    cs = [deep[0], s.circuits[41], s.circuits5[half], s.circuits[22], deep[1], s.circuits[8]]
    ps = [pd[0], s.params[41], s.params5[half], s.params[22], pd[1], s.params[8]]
    forms = _forms(ev, cs)
    assert not forms[0]["one_launch"] and forms[2]["halves"] and forms[1]["n_keys"] == 3
    alone = [ev.evaluate_circuits([c], [p])[0] for c, p in zip(cs, ps)]
    for _ in range(5):
        assert ev.evaluate_circuits(cs, ps) == alone


def test_single_precision(setup):
    s = setup
    ev32 = OperatorCircuitEvaluator(s.ops[20], dtype="fp32")
    off32 = OperatorCircuitEvaluator(s.ops[20], dtype="fp32")
    try:
        off32.statevector_device.set_option("final_controls", 0)
        idx = [41, 22, 1, 4]
        cs, ps = [s.circuits[i] for i in idx], [s.params[i] for i in idx]
        forms, forms_off = _forms(ev32, cs), _forms(off32, cs)
        print("fp32 forms:", forms, forms_off)
        launched, launched_off = _launch_forms(ev32, cs), _launch_forms(off32, cs)
        assert launched_off == forms_off and sorted(launched[0]["n_virtual"]) == [12, 12] and launched[0] != forms[0], launched
        got = _bits(ev32, cs, ps, repetitions=5)
        want = s.on[20].evaluate_circuits(cs, ps)
        bound = FP32_REL * float(np.abs(s.ops[20].coeffs).sum())
        worst = float(np.abs(np.asarray(got) - np.asarray(want)).max())
        worst_off = float(np.abs(np.asarray(off32.evaluate_circuits(cs, ps)) - np.asarray(want)).max())
        print(f"fp32 against fp64: on {worst:.3e}, off {worst_off:.3e}, bound {bound:.3e}")
        assert worst < bound and worst_off < bound
        assert got != off32.evaluate_circuits(cs, ps), "no reduced side in single precision"
    finally:
        ev32.statevector_device.close()
        off32.statevector_device.close()


def test_other_routes_keep_the_full_form(setup, c_oracle):
    """A general operator and a sampled batch on the handle that runs circuits 41 and 22 reduced: both read the full form's
    side states and agree with a device that does not split."""
    from sampler_draws import DELTA_FP64, DrawCheck, plain_order, shot_uniform, split_order

    s = setup
    n = 20
    idx = [41, 22]
    cs, ps = [s.circuits[i] for i in idx], [s.params[i] for i in idx]
    dev = s.on[20].statevector_device
    reduced = s.on[20].evaluate_circuits(cs, ps)
    general = helpers.random_pauli_operator(n, 6, seed=4)
    split = OperatorCircuitEvaluator(general, statevector_device=dev).evaluate_circuits(cs, ps)
    plain = OperatorCircuitEvaluator(general)
    try:
        plain.statevector_device.set_option("split", 0)
        assert np.abs(np.asarray(split) - np.asarray(plain.evaluate_circuits(cs, ps))).max() < EXP_TOL
    finally:
        plain.statevector_device.close()
    dev.set_operator(s.ops[20])
    forms = [dev.circuit_form(c) for c in cs]
    assert all(f["split_sampled"] for f in forms), forms
    shots = 2048
    states, values = dev.sample_batch(cs, ps, shots, seed=29, with_values=True)
    for i, f in enumerate(forms):
        probs = np.abs(c_oracle.simulate(cs[i], ps[i])) ** 2
        order = split_order(f["mask_x"], f["mask_y"]) if f["split_sampled"] else plain_order(n)
        rep = DrawCheck(probs, order, DELTA_FP64).report(shot_uniform(29, i, np.arange(shots)), states[i])
        assert rep["rejected"] == 0 and rep["differ_fraction"] <= 0.01, (i, f, rep)
        assert np.abs(values[i] - s.table[states[i].astype(np.int64)]).max() <= 1e-12 * float(np.abs(s.ops[20].coeffs).sum()), i
    assert s.on[20].evaluate_circuits(cs, ps) == reduced  # (and the one-launch route again afterwards: the same bits)
