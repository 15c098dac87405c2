"""The device-resident value cache (``qsv_value_cache_*``, ``qsv_sample_lookup`` / ``_finish``, ``StatevectorDevice.value_cache``)
and the ``device_value_cache=True`` path of the BitstringCircuitEvaluator on top of it.

Every comparison is exact.  Against the operator sampler that is possible because the operator is dyadic (its values are the same
doubles in any order of the sum: test_bitstring_cache_host.py), against the host because the scoring functions are exact in fp64 and,
where sums are compared, integer valued.  The state route runs the committed n = 6 population, the split route a 16-qubit
population that holds circuits the sampler draws from their side tables and circuits it draws from probabilities.
"""

import json
from pathlib import Path

import numpy as np
import pytest

import helpers
from bitstring_cache_cases import dyadic_ising_operator, nonlinear, nonlinear_of_states, score_states
from queasars_amd.circuit_evaluation import BitstringCircuitEvaluator, BitstringEvaluator, StatevectorDevice
from queasars_amd.circuit_evaluation.circuit_evaluation import _cvar_of_sample_matrix
from queasars_amd.circuit_evaluation.expectation_calculation import basis_state_values
from queasars_amd.ir import CircuitIR

pytestmark = pytest.mark.gpu

SPLIT_N, SPLIT_SEED = 16, 1
X = (np.pi, 0.0, np.pi)
H = (np.pi / 2, 0.0, np.pi)


def _population_n6():
    from queasars_amd.evqe.serialization import population_from_dict

    data = json.loads((Path(__file__).resolve().parent / "golden" / "population_n6.json").read_text())
    population = population_from_dict(data["population"])
    circuits = [ind.get_parameterized_quantum_circuit() for ind in population.individuals]
    return 6, circuits, [list(ind.parameter_values) for ind in population.individuals]


def _population_split():
    """``population_circuits(16, 4, 8, seed=1)`` plus two nine-layer circuits of the same register.  Four layers on sixteen
    qubits cut into two sides with at most two keys whatever the seed (none of the seeds 0 .. 399 holds a circuit that needs
    more than three, by ``qsv_split_describe``), so every circuit of such a population is drawn from its side tables and no
    seed gives both kinds; nine layers have no cut at all and are drawn from probabilities.  ``_batch`` asserts the mix."""
    _, circuits, params = helpers.population_circuits(SPLIT_N, 4, 8, seed=SPLIT_SEED)
    _, deep, deep_params = helpers.population_circuits(SPLIT_N, 9, 2, seed=SPLIT_SEED)
    return SPLIT_N, circuits + deep, params + deep_params


BATCHES = {"state": _population_n6, "split": _population_split}
_shared = {}


def _batch(name, dtype="fp64"):
    """(n, circuits, parameter values, device, dyadic operator, its value on every basis state) -- built once per batch and
    precision, the operator set on the device."""
    key = (name, dtype)
    if key not in _shared:
        n, circuits, params = BATCHES[name]()
        dev = StatevectorDevice(n, dtype=dtype)
        op = dyadic_ising_operator(n, seed=11)
        dev.set_operator(op)
        if name == "split":
            kinds = {bool(dev.circuit_form(c)["split_sampled"]) for c in circuits}
            assert kinds == {False, True}, f"population seed {SPLIT_SEED} holds one kind of circuit only: {kinds}"
        table = basis_state_values(np.arange(1 << n, dtype=np.uint64), op)
        _shared[key] = (n, circuits, params, dev, op, table)
    return _shared[key]


def _evaluator_seed(seed, call):
    """The sampling seed of call number ``call`` (from 0) of a BitstringCircuitEvaluator built with ``seed``: the evaluator draws
    from its generator, and measure_quasi_distributions samples with the first draw of a generator seeded with that draw."""
    rng = np.random.default_rng(seed)
    for _ in range(call + 1):
        draw = int(rng.integers(0, 2**63 - 1))
    return int(np.random.default_rng(draw).integers(0, 2**63 - 1))


class _Recorder:
    def __init__(self, function):
        self.function = function
        self.calls = []

    def __call__(self, bitstring):
        self.calls.append(bitstring)
        return self.function(bitstring)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["state", "split"])
def test_same_numbers_as_the_operator_sampler(name, dtype):
    """lookup + finish(alpha) with the operator's values supplied from the host == sample_cvar_batch: same draws, same values,
    same sort and sum -- the fractional boundary sample of alpha = 0.37 included."""
    n, circuits, params, dev, op, table = _batch(name, dtype)

    def callable_(bitstring):  # (basis_state_values restated for one bitstring: the table is that function of every state)
        return float(table[int(bitstring, 2)])

    cache = dev.value_cache()
    try:
        for shots in (1, 63, 65, 1000, 4096):
            for k, alpha in enumerate((1.0, 0.25, 0.37)):
                seed = 1000 * shots + k
                want = dev.sample_cvar_batch(circuits, params, shots, seed, alpha)
                missing = cache.lookup(circuits, params, shots, seed)
                got = cache.finish(score_states(missing, n, callable_), alpha)
                assert np.array_equal(np.asarray(got), np.asarray(want)), (shots, alpha)
    finally:
        cache.close()


@pytest.mark.parametrize("name", ["state", "split"])
def test_every_sample_gets_its_own_value(name):
    n, circuits, params, dev, _, _ = _batch(name)
    shots, seed = 1000, 77
    states, _ = dev.sample_batch(circuits, params, shots, seed)
    cache = dev.value_cache()
    try:
        missing = cache.lookup(circuits, params, shots, seed)
        values = cache.finish(score_states(missing, n, nonlinear), want_values=True)
    finally:
        cache.close()
    assert values.shape == states.shape and np.array_equal(values, nonlinear_of_states(states))
    # the evaluator: integer values, so that every sum is exact and (alpha * shots whole) host and device agree bit for bit
    scorer = BitstringEvaluator(n, lambda b: float(np.floor(nonlinear(b))))
    for alpha in (1.0, 0.25):
        ev = BitstringCircuitEvaluator(shots, scorer, alpha=alpha, seed=3, statevector_device=dev, device_value_cache=True)
        got = ev.evaluate_circuits(circuits, params)
        drawn, _ = dev.sample_batch(circuits, params, shots, _evaluator_seed(3, 0))
        assert got == _cvar_of_sample_matrix(np.floor(nonlinear_of_states(drawn)), alpha), alpha


def test_more_shots_than_the_device_sorts():
    """Beyond MAX_CVAR_SHOTS the evaluator asks for every sample's value and sorts on the host, as the operator sampler does."""
    n, circuits, params, dev, _, _ = _batch("state")
    shots = StatevectorDevice.MAX_CVAR_SHOTS + 4
    scorer = BitstringEvaluator(n, lambda b: float(np.floor(nonlinear(b))))
    ev = BitstringCircuitEvaluator(shots, scorer, alpha=0.25, seed=3, statevector_device=dev, device_value_cache=True)
    got = ev.evaluate_circuits(circuits[:3], params[:3])
    drawn, _ = dev.sample_batch(circuits[:3], params[:3], shots, _evaluator_seed(3, 0))
    assert got == _cvar_of_sample_matrix(np.floor(nonlinear_of_states(drawn)), 0.25)


@pytest.mark.parametrize("name", ["state", "split"])
def test_scoring_accounting(name):
    n, circuits, params, dev, _, _ = _batch(name)
    shots = 300
    recorder = _Recorder(nonlinear)
    ev = BitstringCircuitEvaluator(shots, BitstringEvaluator(n, recorder), alpha=0.5, seed=3, statevector_device=dev,
                                   device_value_cache=True)
    per_call = len(circuits) * shots
    # first call: once per distinct state of the WHOLE batch, in ascending order
    first = ev.evaluate_circuits(circuits, params)
    seen = np.unique(dev.sample_batch(circuits, params, shots, _evaluator_seed(3, 0))[0])
    assert recorder.calls == [format(int(s), f"0{n}b") for s in seen]
    assert ev.last_scored_bitstrings == len(seen)
    stats = ev.value_cache_stats
    assert stats["entries"] == len(seen) and stats["samples_looked_up"] == per_call
    assert stats["new_entries"] == len(seen) and stats["hits"] == per_call - len(seen)
    # the same seed again (the evaluator's generator put back): nothing is scored, the same results
    recorder.calls.clear()
    ev._rng = np.random.default_rng(3)
    assert ev.evaluate_circuits(circuits, params) == first
    assert recorder.calls == [] and ev.last_scored_bitstrings == 0
    stats = ev.value_cache_stats
    assert stats["entries"] == len(seen) and stats["new_entries"] == len(seen) and stats["hits"] == 2 * per_call - len(seen)
    # another seed: the distinct states not seen before
    ev.evaluate_circuits(circuits, params)
    fresh = np.setdiff1d(np.unique(dev.sample_batch(circuits, params, shots, _evaluator_seed(3, 1))[0]), seen)
    assert recorder.calls == [format(int(s), f"0{n}b") for s in fresh] and ev.last_scored_bitstrings == len(fresh)
    stats = ev.value_cache_stats
    assert stats["entries"] == len(seen) + len(fresh) == stats["new_entries"]
    assert stats["samples_looked_up"] == 3 * per_call and stats["hits"] + stats["new_entries"] == stats["samples_looked_up"]
    assert stats["rehashes"] == 0 and stats["clears"] == 0 and stats["slots"] == 1 << 16


def test_edge_keys():
    # no gates: every sample is state 0, an ordinary key
    n = 13
    dev = StatevectorDevice(n)
    recorder = _Recorder(lambda b: 3.5 if b == "0" * n else -1.0)
    ev = BitstringCircuitEvaluator(500, BitstringEvaluator(n, recorder), alpha=0.3, seed=1, statevector_device=dev, device_value_cache=True)
    assert ev.evaluate_circuits([CircuitIR(n)], [[]]) == [3.5]
    assert recorder.calls == ["0" * n]
    # one basis state (the circuit of test_basis_state_is_sampled_exactly): scored once
    state = (1 << 3) | (1 << 12)
    circuit = CircuitIR(n).u(*X, 3).u(*X, 12)
    recorder.calls.clear()
    recorder.function = lambda b: 7.25 if int(b, 2) == state else -1.0
    assert ev.evaluate_circuits([circuit, circuit], [[], []]) == [7.25, 7.25]
    assert recorder.calls == [format(state, f"0{n}b")]
    assert ev.value_cache_stats["entries"] == 2
    # every qubit flipped: the all-ones key of six qubits
    n6, _, _, dev6, _, _ = _batch("state")
    ones = CircuitIR(n6)
    for q in range(n6):
        ones.u(*X, q)
    recorder6 = _Recorder(lambda b: 0.125 if b == "1" * n6 else -1.0)
    ev6 = BitstringCircuitEvaluator(64, BitstringEvaluator(n6, recorder6), alpha=1.0, seed=1, statevector_device=dev6,
                                    device_value_cache=True)
    assert ev6.evaluate_circuits([ones], [[]]) == [0.125] and recorder6.calls == ["1" * n6]


def _uniform_circuits(n=13, copies=4):
    circuits = []
    for _ in range(copies):
        c = CircuitIR(n)
        for q in range(n):
            c.u(*H, q)
        circuits.append(c)
    return n, circuits, [[] for _ in range(copies)]


def _lookup_values(cache, dev, n, circuits, params, shots, seed, function=nonlinear):
    """One step through ``cache``: (the drawn states, every sample's value, the states the cache asked for)."""
    states, _ = dev.sample_batch(circuits, params, shots, seed)
    missing = cache.lookup(circuits, params, shots, seed)
    values = cache.finish(score_states(missing, n, function), want_values=True)
    return states, values, missing


def test_growth_under_collisions():
    """Sixteen slots to begin with and 16384 samples spread over 8192 states: the table grows before it is probed, and again
    with its entries in it."""
    n, circuits, params = _uniform_circuits()
    dev = StatevectorDevice(n)
    cache = dev.value_cache(log2_slots=4)
    shots = 4096
    states, values, missing = _lookup_values(cache, dev, n, circuits, params, shots, seed=21)
    assert np.array_equal(values, nonlinear_of_states(states))
    assert np.array_equal(np.sort(missing), np.unique(states))
    stats = cache.stats()
    assert stats["rehashes"] >= 1 and stats["entries"] == len(np.unique(states)) and stats["slots"] >= 2 * stats["entries"]
    assert stats["slots"] >= 2 * (len(circuits) * shots) and len(np.unique(states)) > 4096
    # another seed: old values through the rehash, new ones beside them
    states2, values2, missing2 = _lookup_values(cache, dev, n, circuits, params, shots, seed=22)
    assert np.array_equal(values2, nonlinear_of_states(states2))
    assert np.array_equal(np.sort(missing2), np.setdiff1d(np.unique(states2), np.unique(states)))
    after = cache.stats()
    assert after["rehashes"] > stats["rehashes"] and after["clears"] == 0
    assert after["entries"] == len(np.union1d(states, states2)) and after["slots"] >= 2 * after["entries"]
    assert after["hits"] + after["new_entries"] == after["samples_looked_up"] == 2 * len(circuits) * shots
    cache.close()


def test_clearing_at_the_cap():
    """2^14 slots at most and 6000 samples per call: the second call's samples do not fit beside the first call's more than 2192
    entries, so the table is cleared and the states come again."""
    n, circuits, params = _uniform_circuits()
    dev = StatevectorDevice(n)
    cache = dev.value_cache(log2_slots=4, log2_max_slots=14)
    shots = 1500
    states, values, missing = _lookup_values(cache, dev, n, circuits, params, shots, seed=31)
    assert np.array_equal(values, nonlinear_of_states(states))
    before = cache.stats()
    assert before["clears"] == 0 and 2 * (before["entries"] + len(circuits) * shots) > 1 << 14
    states2, values2, missing2 = _lookup_values(cache, dev, n, circuits, params, shots, seed=32)
    assert np.array_equal(values2, nonlinear_of_states(states2))
    after = cache.stats()
    assert after["clears"] >= 1 and after["slots"] <= 1 << 14 and after["entries"] == len(np.unique(states2))
    assert np.array_equal(np.sort(missing2), np.unique(states2))  # (asked again ...
    assert len(np.intersect1d(missing2, missing)) > 0             # ... also for states it had already been given)
    # one call of more than 2^13 samples cannot fit: refused before anything is launched
    with pytest.raises(ValueError, match="fit"):
        cache.lookup(circuits, params, 2049, 33)
    assert cache.stats() == after
    states3, values3, _ = _lookup_values(cache, dev, n, circuits, params, 2048, seed=34)  # (exactly 2^13 is fine)
    assert np.array_equal(values3, nonlinear_of_states(states3))
    cache.close()


def test_a_callable_that_raises():
    n, circuits, params, dev, _, _ = _batch("state")
    shots = 1000
    drawn, _ = dev.sample_batch(circuits, params, shots, _evaluator_seed(3, 0))
    seen = np.unique(drawn)
    bad = {"bitstring": format(int(seen[len(seen) // 2]), f"0{n}b")}

    def scorer(bitstring):
        if bitstring == bad["bitstring"]:
            raise KeyError(bitstring)
        return float(np.floor(nonlinear(bitstring)))

    ev = BitstringCircuitEvaluator(shots, BitstringEvaluator(n, scorer), alpha=0.25, seed=3, statevector_device=dev,
                                   device_value_cache=True)
    with pytest.raises(KeyError):
        ev.evaluate_circuits(circuits, params)
    assert ev.value_cache_stats["entries"] == 0
    bad["bitstring"] = None
    got = ev.evaluate_circuits(circuits, params)
    drawn, _ = dev.sample_batch(circuits, params, shots, _evaluator_seed(3, 1))
    assert got == _cvar_of_sample_matrix(np.floor(nonlinear_of_states(drawn)), 0.25)
    assert ev.value_cache_stats["entries"] == len(np.unique(drawn))
    # a second lookup before the finish is refused, a finish with the wrong number of values too; clear() recovers
    cache = dev.value_cache()
    missing = cache.lookup(circuits, params, shots, 5)
    assert len(missing) > 1
    with pytest.raises(RuntimeError):
        cache.lookup(circuits, params, shots, 6)
    with pytest.raises(RuntimeError):
        cache.finish(np.zeros(len(missing) - 1))
    cache.clear()
    assert cache.stats()["entries"] == 0
    states, values, _ = _lookup_values(cache, dev, n, circuits, params, shots, seed=5)
    assert np.array_equal(values, nonlinear_of_states(states))
    cache.close()


def test_the_default_is_untouched():
    n, circuits, params, dev, _, _ = _batch("state")
    scorer = BitstringEvaluator(n, nonlinear)
    plain = BitstringCircuitEvaluator(200, scorer, 0.4, seed=3, statevector_device=dev)
    named = BitstringCircuitEvaluator(200, scorer, 0.4, seed=3, statevector_device=dev, device_value_cache=False)
    cached = BitstringCircuitEvaluator(200, scorer, 0.4, seed=3, statevector_device=dev, device_value_cache=True)
    for _ in range(3):
        assert plain.evaluate_circuits(circuits, params) == named.evaluate_circuits(circuits, params)
        cached.evaluate_circuits(circuits, params)
    assert named.value_cache_stats is None and cached.value_cache_stats["samples_looked_up"] == 3 * len(circuits) * 200
    # the two modes consume the generator in step
    draws = {int(ev._rng.integers(0, 2**63 - 1)) for ev in (plain, named, cached)}
    assert len(draws) == 1
