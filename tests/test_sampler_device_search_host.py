"""What the device-resident sampler search decides and checks without a device: the rule that sends a search to the device
(``solver._device_search_wanted`` / ``_minimize_batched`` through one helper), the binding of ``qsv_cvar_device`` against the
header, and argument checks that come before anything touches a GPU."""

import ctypes as C
import re
from pathlib import Path

import pytest

from queasars_amd import _lib
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, OperatorSamplerCircuitEvaluator, StatevectorDevice
from queasars_amd.evqe import device_search
from queasars_amd.evqe import solver as S

ROOT = Path(__file__).resolve().parent.parent


class _Stub:
    """An evaluator as the gating rule sees it."""

    def __init__(self, by_default=None, possible=True):
        if by_default is not None:
            self.device_resident_search_by_default = by_default
        self._possible = possible

    def device_resident_search_possible(self):
        return self._possible

    def evaluate_device_to_device(self, circuits, matrix, out):
        raise AssertionError("the rule evaluates nothing")


class _MaskedStub(_Stub):
    def evaluate_device_to_device(self, circuits, matrix, out, active=None, active_stride=1):
        raise AssertionError("the rule evaluates nothing")


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for name in ("QSV_DEVICE_SEARCH", "QSV_SCALAR_SPSA", "QSV_DEVICE_SEARCH_MASK"):
        monkeypatch.delenv(name, raising=False)


def test_the_default_sends_only_an_estimator_to_the_device():
    spsa = S.SPSA(maxiter=5)
    sampling, estimator = _MaskedStub(by_default=False), _Stub(by_default=True)
    many = S._DEVICE_SEARCH_MIN_RUNS
    # a sampling evaluator: None is the host driver whatever the size of the search, True opts in
    for n_runs in (2, many, 4 * many):
        assert S._device_search_wanted(sampling, n_runs, None, spsa) is False
        assert S._device_search_wanted(sampling, n_runs, True, spsa) is True
        assert S._device_search_wanted(sampling, n_runs, False, spsa) is False
    # the estimator: unchanged -- None is "at least _DEVICE_SEARCH_MIN_RUNS runs"
    assert S._device_search_wanted(estimator, many, None, spsa) is True
    assert S._device_search_wanted(estimator, many - 1, None, spsa) is False
    assert S._device_search_wanted(estimator, 2, True, spsa) is True
    assert S._device_search_wanted(estimator, 4 * many, False, spsa) is False
    # an evaluator that says nothing about a default is treated as one that samples
    assert S._device_search_wanted(_Stub(), 4 * many, None, spsa) is False
    # one that cannot do it, a single run, another termination rule
    assert S._device_search_wanted(_Stub(by_default=True, possible=False), many, True, spsa) is False
    assert S._device_search_wanted(estimator, 1, True, spsa) is False
    assert S._device_search_wanted(estimator, many, True, S.SPSA(maxiter=0)) is False


def test_the_environment_overrides_both_ways(monkeypatch):
    spsa = S.SPSA(maxiter=5)
    sampling, estimator = _MaskedStub(by_default=False), _Stub(by_default=True)
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "1")
    assert S._device_search_wanted(sampling, 4, None, spsa) is True
    assert S._device_search_asked_for(sampling, 4, False) is True
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "0")
    assert S._device_search_wanted(sampling, 64, True, spsa) is False
    assert S._device_search_wanted(estimator, 64, None, spsa) is False


def test_both_places_ask_the_same_helper(monkeypatch):
    """``_minimize_batched`` resolves ``on_device=None`` through ``_device_search_asked_for``: with a sampling stub it runs the
    host driver, with the flag set it asks the device search."""
    asked = []
    monkeypatch.setattr(device_search, "supported", lambda evaluator, jobs: asked.append(len(jobs)) or False)
    ran = []
    monkeypatch.setattr(S, "_minimize_spsa_vectorised", lambda evaluator, jobs: ran.append(len(jobs)))
    cfg = S.SPSA(maxiter=3)
    jobs = [(object(), cfg.new_run([0.1, 0.2], seed=k)) for k in range(S._DEVICE_SEARCH_MIN_RUNS + 4)]
    S._minimize_batched(_MaskedStub(by_default=False), jobs, on_device=None)
    assert asked == [] and ran == [len(jobs)]
    S._minimize_batched(_MaskedStub(by_default=False), jobs, on_device=True)
    assert asked == [len(jobs)] and ran == [len(jobs)] * 2
    S._minimize_batched(_Stub(by_default=True), jobs, on_device=None)
    assert asked == [len(jobs)] * 2
    S._minimize_batched(_Stub(by_default=True), jobs[:4], on_device=None)
    assert asked == [len(jobs)] * 2


def test_the_evaluators_name_their_default():
    assert OperatorCircuitEvaluator.device_resident_search_by_default is True
    assert OperatorSamplerCircuitEvaluator.device_resident_search_by_default is False
    assert callable(OperatorSamplerCircuitEvaluator.evaluate_device_to_device)
    assert callable(OperatorSamplerCircuitEvaluator.device_resident_search_possible)


def test_the_search_hands_the_mask_only_to_a_method_that_takes_it(monkeypatch):
    assert device_search._takes_mask(_MaskedStub()) is True
    assert device_search._takes_mask(_Stub()) is False
    monkeypatch.setenv("QSV_DEVICE_SEARCH_MASK", "0")
    assert device_search._takes_mask(_MaskedStub()) is False


def test_the_binding_matches_the_header():
    """``qsv_cvar_device`` as include/qsv.h declares it, argument by argument."""
    text = (ROOT / "include" / "qsv.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    match = re.search(r"int\s+qsv_cvar_device\s*\((.*?)\)\s*;", text, flags=re.S)
    assert match, "include/qsv.h does not declare qsv_cvar_device"
    declared = [" ".join(a.split()) for a in match.group(1).split(",")]
    assert declared == ["qsv_t* h", "int n_evals", "const int* circuit_ids", "int width", "const double* device_values",
                        "void* ready_event", "int shots", "uint64_t seed", "double alpha", "const uint8_t* device_active",
                        "int active_stride", "double* device_out"]
    restype, argtypes = _lib.SIGNATURES["qsv_cvar_device"]
    kinds = {"int": C.c_int, "uint64_t": C.c_uint64, "double": C.c_double}
    want = [C.c_void_p if "*" in a else kinds[a.rsplit(" ", 1)[0]] for a in declared]
    assert restype is C.c_int and argtypes == want
    lib = _lib.load()
    assert hasattr(lib, "qsv_cvar_device")
    assert lib.qsv_cvar_device(None, 0, None, 0, None, None, 0, 0, 0.5, None, 1, None) == _lib.QSV_E_ARG  # (no handle)


def test_argument_checks_that_need_no_device():
    dev = StatevectorDevice.__new__(StatevectorDevice)  # (no handle: every check below comes before the library is called)
    circuits = [object()]
    with pytest.raises(ValueError, match="matrix"):
        StatevectorDevice.cvar_of_device_parameters(dev, circuits, 0, 3, 0, 16, 1, 0.5, 8)
    with pytest.raises(ValueError, match="matrix"):
        StatevectorDevice.cvar_of_device_parameters(dev, circuits, 8, 3, 0, 16, 1, 0.5, 0)
    with pytest.raises(ValueError, match="shots"):
        StatevectorDevice.cvar_of_device_parameters(dev, circuits, 8, 3, 0, StatevectorDevice.MAX_CVAR_SHOTS + 1, 1, 0.5, 8)
    with pytest.raises(ValueError, match="alpha"):
        StatevectorDevice.cvar_of_device_parameters(dev, circuits, 8, 3, 0, 16, 1, 0.0, 8)
    with pytest.raises(ValueError, match="active_stride"):
        StatevectorDevice.cvar_of_device_parameters(dev, circuits, 8, 3, 0, 16, 1, 0.5, 8, active_ptr=8, active_stride=0)
    assert StatevectorDevice.cvar_of_device_parameters(dev, [], 0, 0, 0, 16, 1, 0.5, 0) is None  # (an empty batch is no call)


def test_more_shots_than_the_device_sorts_stay_on_the_host():
    sampler = OperatorSamplerCircuitEvaluator.__new__(OperatorSamplerCircuitEvaluator)
    sampler._shots = StatevectorDevice.MAX_CVAR_SHOTS + 1
    assert sampler.device_resident_search_possible() is False
    with pytest.raises(ValueError, match="shots"):
        sampler.evaluate_device_to_device([], None, None)


# ---- the run layout -------------------------------------------------------------------------------------------------------


def _mixed_runs(cfg):
    """Five runs: two on a layer inside a longer vector -- base vectors of different lengths, positions that do not follow each
    other --, three on rows of their own, of sizes 1, 2 and 3."""
    import numpy as np

    rng = np.random.default_rng(11)
    runs = []
    for total, positions in ((9, [1, 4, 7]), (4, [0, 3])):
        base = rng.normal(size=total)
        run = cfg.new_run(rng.normal(size=len(positions)), seed=total)
        run.embed = (base, np.array(positions, dtype=np.int64))
        runs.append(run)
    runs[2:2] = [cfg.new_run(rng.normal(size=1), seed=1)]  # (embedded and own rows interleaved)
    runs += [cfg.new_run(rng.normal(size=size), seed=size) for size in (2, 3)]
    return runs


def test_the_run_layout_and_its_inverse():
    """One statement of the layout (``device_search._PackedRuns``): every row is ``_full_point(run, run.x)`` behind zeros,
    ``columns_host`` says where the run's variables are, and the way back hands every run exactly its own entries."""
    import numpy as np

    runs = _mixed_runs(S.SPSA(maxiter=3))
    assert S._full_point is device_search._full_point
    pack = device_search._PackedRuns(runs)
    assert pack.n_runs == 5 and pack.width == 9 and pack.stride == 3
    assert pack.x_host.shape == (5, 9) and pack.x_host.dtype == np.float64
    assert pack.columns_host.shape == (5, 3) and pack.columns_host.dtype == np.int32 and pack.sizes.dtype == np.int32
    assert pack.lengths.tolist() == [9, 4, 1, 2, 3] and pack.sizes.tolist() == [3, 2, 1, 2, 3]
    for i, run in enumerate(runs):
        row = S._full_point(run, run.x)
        assert row.size == pack.lengths[i]
        assert np.array_equal(pack.x_host[i], np.concatenate([row, np.zeros(9 - row.size)]))
        want = run.embed[1] if run.embed is not None else np.arange(run.x.size)
        assert np.array_equal(pack.where[i], want)
        assert np.array_equal(pack.columns_host[i, : run.x.size], want)
        assert not pack.columns_host[i, run.x.size :].any()
    bases = [None if run.embed is None else run.embed[0].copy() for run in runs]
    perturbed = pack.x_host + np.arange(1, 46, dtype=np.float64).reshape(5, 9)
    kept = perturbed.copy()
    pack.write_back(perturbed)
    for i, run in enumerate(runs):
        assert np.array_equal(run.x, kept[i, pack.where[i]]) and run.x.dtype == np.float64
        assert not np.shares_memory(run.x, perturbed)
        if run.embed is not None:
            assert np.array_equal(run.embed[0], bases[i])  # (the base vector is not the run's to move)
    assert np.array_equal(perturbed, kept)


def test_the_signs_are_the_draws_of_propose():
    """``draw_signs``: per run the numbers ``propose()`` would draw call by call, at the run's columns, zero elsewhere."""
    import numpy as np

    cfg = S.SPSA(maxiter=4)
    runs, twins = _mixed_runs(cfg), _mixed_runs(cfg)
    pack = device_search._PackedRuns(runs)
    signs = pack.draw_signs(4)
    assert signs.shape == (4, 5, 9) and signs.dtype == np.int8
    for i, twin in enumerate(twins):
        for k in range(4):
            twin.propose()
            assert np.array_equal(signs[k, i, pack.where[i]], twin._delta)
        others = np.setdiff1d(np.arange(9), pack.where[i])
        assert not signs[:, i, others].any()


# ---- one rule -------------------------------------------------------------------------------------------------------------


class _Capable:
    """An evaluator as both halves of the rule see it: with everything, or with one thing missing."""

    def __init__(self, possible=True, values=True, plans=True):
        self._possible = possible
        if values:
            self.evaluate_device_to_device = lambda circuits, matrix, out: pytest.fail("the rule evaluates nothing")
        if plans:
            self.gradient_plan = lambda *a, **k: pytest.fail("the rule plans nothing")

    def device_resident_search_possible(self):
        return self._possible


class _AnotherRule(S.SPSATerminationChecker):
    """A termination rule the device does not implement."""

    def fresh(self):
        return _AnotherRule(self.minimum_relative_change, self.allowed_consecutive_violations, self.maxfev)


def _rule_cases():
    evaluators = {"capable": dict(), "not possible": dict(possible=False), "no evaluate_device_to_device": dict(values=False),
                  "no gradient_plan": dict(plans=False)}
    optimisers = {
        "SPSA maxiter=0": lambda: S.SPSA(maxiter=0), "SPSA maxiter=5": lambda: S.SPSA(maxiter=5),
        "SPSA its own checker": lambda: S.SPSA(maxiter=5, termination_checker=S.SPSATerminationChecker(1e-3, 2)),
        "SPSA another checker": lambda: S.SPSA(maxiter=5, termination_checker=_AnotherRule(1e-3, 2)),
        "NFT maxfev=0": lambda: S.NFT(maxfev=0), "NFT maxfev=10": lambda: S.NFT(maxfev=10),
        "Adam maxiter=0": lambda: S.Adam(maxiter=0), "Adam maxiter=5": lambda: S.Adam(maxiter=5),
    }
    return [pytest.param(kwargs, make, id=f"{ev}-{opt}") for ev, kwargs in evaluators.items() for opt, make in optimisers.items()]


def _supported_for(optimiser):
    return {S.SPSA: device_search.supported, S.NFT: device_search.supported_nft, S.Adam: device_search.supported_adam}[type(optimiser)]


def _fresh_jobs(optimiser, n_runs):
    return [(object(), optimiser.new_run([0.1 * (k + 1)] * (1 + k % 3), seed=k)) for k in range(n_runs)]


@pytest.mark.parametrize("kwargs,make", _rule_cases())
def test_the_prediction_is_the_rule(kwargs, make):
    """What ``_device_search_wanted`` says before the runs exist is what ``supported*`` says of fresh runs, case by case."""
    optimiser = make()
    for n_runs in (1, 2, S._DEVICE_SEARCH_MIN_RUNS):
        wanted = S._device_search_wanted(_Capable(**kwargs), n_runs, True, optimiser)
        assert wanted is _supported_for(optimiser)(_Capable(**kwargs), _fresh_jobs(optimiser, n_runs))
        can = (n_runs >= 2 and kwargs.get("possible", True) and getattr(optimiser, "maxiter", None) != 0
               and getattr(optimiser, "maxfev", None) != 0 and not isinstance(getattr(optimiser, "termination_checker", None), _AnotherRule)
               and kwargs.get("plans" if isinstance(optimiser, S.Adam) else "values", True))
        assert wanted is can


def test_the_sign_ceiling_is_the_one_thing_the_prediction_cannot_know(monkeypatch):
    spsa = S.SPSA(maxiter=5)
    jobs = _fresh_jobs(spsa, 4)  # (rows of up to 3 entries: 5 iterations x 4 runs x 3 doubles = 480 bytes of signs)
    assert S._device_search_wanted(_Capable(), 4, True, spsa) is True
    monkeypatch.setattr(device_search, "_MAX_SIGN_BYTES", 480)
    assert device_search.supported(_Capable(), jobs) is True
    monkeypatch.setattr(device_search, "_MAX_SIGN_BYTES", 479)
    assert device_search.supported(_Capable(), jobs) is False
    assert S._device_search_wanted(_Capable(), 4, True, spsa) is True
