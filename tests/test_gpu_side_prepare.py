"""The one-launch route's staged preparation (option ``"side_prepare"``, kernels.hip ``side_prepare``): a side whose plan
qualifies is prepared from one staged read of its plan and parameters and keeps its threads' and tiles' factors in registers;
every other side goes through ``prepare_eval`` as before.  Both form every matrix, factor and product by the same expressions
in the same order, so the option must not change a single bit -- that, and the C oracle within ``EXP_TOL``, is what every
test here asks, for each form a side can take (read through ``circuit_form``), both parameter feeds, literal angles, the plans
that fall back, single precision and batches mixed with circuits on the ordinary plan.

The route exists only where the handle's geometry is k = 12, r = 4: n = 20 is the smallest size.  Every case is a handful of
circuits; the populations, their forms and the oracle's diagonal table are made once per module.
"""

import os

import numpy as np
import pytest

import helpers
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator
from queasars_amd.evqe import EVQEPopulation
from queasars_amd.ir import CircuitIR, ParamRef

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10
FP32_REL = 2e-6  # (per unit of sum |c_k|: tests/test_gpu_configs.py)
N = 20


def _forms(ev, circuits):
    ev.circuit_costs(circuits)  # (registers them under the evaluator's operator, several at once)
    return [ev.statevector_device.circuit_form(c) for c in circuits]


def _picked(forms):
    """{name: index}: one one-launch circuit per number of keys 0 .. 3 and a half-sided circuit per number of keys where there
    is one."""
    picks = {}
    launched = [(i, f) for i, f in enumerate(forms) if f["one_launch"]]
    for one_tile_only in (True, False):  # (per number of keys: a circuit whose sides are one tile and one workgroup, if there is one)
        for i, f in launched:
            if not one_tile_only or (not f["halves"] and max(f["outer"]) == 0):
                picks.setdefault(f"{f['n_keys']} keys", i)
    for i, f in launched:
        if f["halves"]:
            picks.setdefault(f"half sides, {f['n_keys']} keys", i)
    return picks


class _Setup:
    def __init__(self, c_oracle):
        self.op = helpers.random_ising_operator(N, seed=2020)
        self.ev = OperatorCircuitEvaluator(self.op)
        self.dev = self.ev.statevector_device
        self.individuals, self.circuits, self.params = [], [], []
        for layers in (4, 5):
            pop = EVQEPopulation.random_population(N, layers, 64, True, 0)
            self.individuals += list(pop.individuals)
        # (helpers.population_circuits(N, layers, 64, seed=0) is these individuals' circuits and values)
        self.circuits = [ind.get_parameterized_quantum_circuit() for ind in self.individuals]
        self.params = [list(ind.parameter_values) for ind in self.individuals]
        _, c4, p4 = helpers.population_circuits(N, 4, 64, seed=0)
        assert p4 == self.params[:64] and [c.packed().tobytes() for c in c4[:4]] == [c.packed().tobytes() for c in self.circuits[:4]]
        self.forms = _forms(self.ev, self.circuits)
        self.picks = _picked(self.forms)
        # a thirteen-qubit side SWEPT as two tiles by its one workgroup: the form a half side's plan falls back to, here asked for
        # (read when a circuit is registered: an evaluator of its own) for the half-sided circuits of one and two keys
        self.swept_idx = sorted({i for name, i in self.picks.items() if name in ("half sides, 1 keys", "half sides, 2 keys")})
        os.environ["QSV_NO_HALF_SIDES"] = "1"
        try:
            self.swept_ev = OperatorCircuitEvaluator(self.op)
            self.swept_forms = _forms(self.swept_ev, [self.circuits[i] for i in self.swept_idx])
        finally:
            del os.environ["QSV_NO_HALF_SIDES"]
        self.oracle = c_oracle
        self.table = c_oracle.diagonal_table(self.op)
        self.scratch = np.zeros(2 << N)
        self._ref = {}

    def reference(self, circuit, params, key):
        if key not in self._ref:
            self._ref[key] = self.oracle.evaluate(circuit, params, self.op, self.table, self.scratch)
        return self._ref[key]


@pytest.fixture(scope="module")
def setup(c_oracle):
    s = _Setup(c_oracle)
    yield s
    s.swept_ev.statevector_device.close()
    s.dev.set_option("side_prepare", 1)


def _on_and_off(ev, evaluate):
    """evaluate() with the staged preparation, without it and with it again: the three must be the same bits."""
    dev = ev.statevector_device
    dev.set_option("side_prepare", 1)
    on = evaluate()
    dev.set_option("side_prepare", 0)
    off = evaluate()
    dev.set_option("side_prepare", 1)
    again = evaluate()
    assert on == off and again == on, (on, off, again)
    return on


def _check_group(s, ev, idx):
    """Option on == option off for each circuit alone, together, reversed and twenty times over (the first batch is fresh, the
    others repeat its layout); each value within EXP_TOL of the C oracle."""
    dev = ev.statevector_device
    cs, ps = [s.circuits[i] for i in idx], [s.params[i] for i in idx]
    alone = [_on_and_off(ev, lambda c=c, p=p: ev.evaluate_circuits([c], [p]))[0] for c, p in zip(cs, ps)]
    together = _on_and_off(ev, lambda: ev.evaluate_circuits(cs, ps))
    backwards = _on_and_off(ev, lambda: ev.evaluate_circuits(cs[::-1], ps[::-1]))
    assert together == alone and backwards == alone[::-1]
    for option in (1, 0, 1):
        dev.set_option("side_prepare", option)
        for rep in range(20):
            assert ev.evaluate_circuits(cs, ps) == alone, (option, rep)
    for i, value in zip(idx, alone):
        err = abs(value - s.reference(s.circuits[i], s.params[i], ("whole", i)))
        print(f"circuit {i}: |value - oracle| = {err:.3e}")
        assert err < EXP_TOL, i


def test_every_form_of_a_side(setup):
    """One circuit per number of keys 0 .. 3 and the half-sided circuits of one, two and three keys (two workgroups a side, one
    tile each), from the four- and five-layer populations."""
    s = setup
    picks = s.picks
    print("picked:", {name: (i, s.forms[i]) for name, i in picks.items()})
    for keys in range(4):
        assert f"{keys} keys" in picks, sorted(picks)
    assert "half sides, 3 keys" in picks, sorted(picks)
    for name, i in picks.items():
        f = s.forms[i]
        assert f["one_launch"] and f["amps_per_thread"] == 8, (name, f)
        assert f["halves"] or not name.startswith("half sides"), (name, f)
        assert f["halves"] == (max(f["outer"]) == 1 and max(f["n_virtual"]) == 13), (name, f)
    assert any(not s.forms[i]["halves"] for i in picks.values())
    _check_group(s, s.ev, sorted(set(picks.values())))


def test_a_thirteen_qubit_side_swept_as_two_tiles(setup):
    """The half-sided circuits of one and two keys planned without half sides: a thirteen-qubit side is then two tiles swept
    by the side's ONE workgroup, which keeps both tiles' factors and base indices."""
    s = setup
    print("swept:", list(zip(s.swept_idx, s.swept_forms)))
    assert s.swept_idx, sorted(s.picks)
    for f in s.swept_forms:
        assert f["one_launch"] and not f["halves"] and f["amps_per_thread"] == 8 and max(f["outer"]) == 1 and max(f["n_virtual"]) == 13, f
    _check_group(s, s.swept_ev, s.swept_idx)


def test_literal_angles(setup):
    """The same individuals with only their last layer parameterised: the other layers' angle entries carry literals, the
    vectors are short (a layer's worth) and of no particular length."""
    s = setup
    idx = sorted(set(s.picks.values()))
    cs = [s.individuals[i].get_partially_parameterized_quantum_circuit({-1}) for i in idx]
    ps = [list(s.individuals[i].get_layer_parameter_values(-1)) for i in idx]
    forms = _forms(s.ev, cs)
    print("forms:", forms, "vector lengths:", [len(p) for p in ps])
    assert sum(f["one_launch"] for f in forms) >= 4 and any(f["halves"] for f in forms), forms
    assert all(0 < len(p) < len(s.params[i]) for p, i in zip(ps, idx))
    together = _on_and_off(s.ev, lambda: s.ev.evaluate_circuits(cs, ps))
    alone = [_on_and_off(s.ev, lambda c=c, p=p: s.ev.evaluate_circuits([c], [p]))[0] for c, p in zip(cs, ps)]
    assert together == alone
    for i, c, p, value in zip(idx, cs, ps, together):
        err = abs(value - s.reference(c, p, ("last layer", i)))
        print(f"circuit {i}: |value - oracle| = {err:.3e}")
        assert err < EXP_TOL, i
        # (bound to the individual's own values it is the whole circuit's state: the same value up to rounding)
        assert abs(value - s.reference(s.circuits[i], s.params[i], ("whole", i))) < EXP_TOL


def test_both_parameter_feeds(setup):
    """Pinned host lists and a device matrix reach the preparation through the same pointer: the same bits from either, with
    the option on and off, values left on the device (evaluate_circuits_to_device)."""
    import torch

    s = setup
    idx = sorted(set(s.picks.values()))
    cs, ps = [s.circuits[i] for i in idx], [s.params[i] for i in idx]
    width = max(len(p) for p in ps) + 3
    host = np.full((len(cs), width), 1e300)  # (never read: a circuit takes the first num_parameters values of its row)
    for row, p in enumerate(ps):
        host[row, : len(p)] = p
    matrix = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()

    def to_device(feed):
        buf = torch.full((len(cs),), float("nan"), dtype=torch.float64, device="cuda")
        assert s.ev.evaluate_circuits_to_device(cs, feed, buf.data_ptr())
        torch.cuda.synchronize()
        return buf.cpu().tolist()

    from_lists = _on_and_off(s.ev, lambda: to_device(ps))
    from_matrix = _on_and_off(s.ev, lambda: to_device(matrix))
    assert from_lists == from_matrix
    assert from_lists == _on_and_off(s.ev, lambda: s.ev.evaluate_circuits(cs, ps))


def _layered(rounds_before, rounds_after):
    """u on every qubit `rounds_before` times before anything entangles (folded gates), cu3(q, q + 1) for even q, then
    `rounds_after` rounds of u: no gate joins qubits 0 .. 9 with 10 .. 19, the circuit splits 10 + 10 without a key."""
    c = CircuitIR(N)
    k = 0

    def angle():
        nonlocal k
        k += 1
        return ParamRef(k - 1)

    for _ in range(rounds_before):
        for q in range(N):
            c.u(angle(), angle(), angle(), q)
    for q in range(0, N - 1, 2):
        c.cu3(angle(), angle(), angle(), q, q + 1)
    for _ in range(rounds_after):
        for q in range(N):
            c.u(angle(), angle(), angle(), q)
    assert c.num_parameters == k
    return c


@pytest.mark.parametrize("rounds_before,rounds_after", [(13, 1), (1, 34)])
def test_plans_that_fall_back(setup, rounds_before, rounds_after):
    """Sides the staged preparation does not take run prepare_eval as before, with the option on: 130 folded gates a side
    (more than the 128 that are staged), and a parameter vector of more than 1024 values (2130: more than a side's share of
    1024 whichever way it is counted).  Zero keys, one launch; against the C oracle, and on == off."""
    s = setup
    c = _layered(rounds_before, rounds_after)
    if rounds_before == 13:
        assert rounds_before * (N // 2) > 128
    else:
        assert c.num_parameters // 2 > 1024
    rng = np.random.default_rng(rounds_before)
    vectors = [list(rng.uniform(-np.pi, np.pi, size=c.num_parameters)) for _ in range(2)]
    form = _forms(s.ev, [c])[0]
    print("form:", form)
    assert form["one_launch"] and form["n_keys"] == 0 and sorted(form["n_virtual"]) == [10, 10], form
    got = _on_and_off(s.ev, lambda: s.ev.evaluate_circuits([c, c], vectors))
    for p, value in zip(vectors, got):
        err = abs(value - s.oracle.evaluate(c, p, s.op, s.table, s.scratch))
        print(f"|value - oracle| = {err:.3e}")
        assert err < EXP_TOL


def test_single_precision_handle(setup):
    """An fp32 handle leaves the scheduled gates' matrices as floats (prepare_eval's float_mats) on either route: on == off,
    and within FP32_REL * sum |c_k| of the fp64 values."""
    s = setup
    ev32 = OperatorCircuitEvaluator(s.op, dtype="fp32")
    try:
        idx = sorted(set(s.picks.values()))
        cs, ps = [s.circuits[i] for i in idx], [s.params[i] for i in idx]
        forms = _forms(ev32, cs)
        print("fp32 forms:", forms)
        # (single precision has no sides of eight amplitudes per thread and no half sides: its thirteen-qubit sides may take
        # launches of their own, the others are the one-launch route's)
        assert sum(f["one_launch"] and f["amps_per_thread"] == 16 for f in forms) >= 3, forms
        got = _on_and_off(ev32, lambda: ev32.evaluate_circuits(cs, ps))
        assert got == [_on_and_off(ev32, lambda c=c, p=p: ev32.evaluate_circuits([c], [p]))[0] for c, p in zip(cs, ps)]
        s.dev.set_option("side_prepare", 1)
        want = s.ev.evaluate_circuits(cs, ps)
        worst = float(np.abs(np.asarray(got) - np.asarray(want)).max())
        print(f"fp32 against fp64: {worst:.3e}, bound {FP32_REL * float(np.abs(s.op.coeffs).sum()):.3e}")
        assert worst < FP32_REL * float(np.abs(s.op.coeffs).sum())
    finally:
        ev32.statevector_device.close()


def test_mixed_with_circuits_on_the_ordinary_plan(setup):
    """A batch that also holds nine-layer individuals, which are not split: the split ones keep their bits, the others do
    not depend on the option."""
    s = setup
    _, deep, pd = helpers.population_circuits(N, 9, 3, seed=8)
    assert all(f["route"] not in (1, 2) and not f["one_launch"] for f in _forms(s.ev, deep))
    idx = sorted(set(s.picks.values()))
    cs, ps = [s.circuits[i] for i in idx], [s.params[i] for i in idx]
    s.dev.set_option("side_prepare", 1)
    alone = s.ev.evaluate_circuits(cs, ps)
    mixed = _on_and_off(s.ev, lambda: s.ev.evaluate_circuits(deep[:2] + cs + deep[2:], pd[:2] + ps + pd[2:]))
    assert mixed[2:-1] == alone
    assert mixed[:2] + mixed[-1:] == _on_and_off(s.ev, lambda: s.ev.evaluate_circuits(deep, pd))
