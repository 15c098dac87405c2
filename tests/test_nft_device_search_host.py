"""What the device-resident NFT search decides and checks without a device: the schedule the host computes ahead
(``device_search.nft_schedule``) against real ``_NFTRun`` objects, the rule that sends an NFT search to the device (opt-in:
``solver._device_search_wanted`` / ``_minimize_batched``), ``supported_nft``, and the binding of ``qsv_nft_step`` against the
header."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from queasars_amd import _lib
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


class _HostOnly:
    """An evaluator without ``evaluate_device_to_device``: a smooth function of the points, so that the generic loop has
    something to minimise."""

    def __init__(self):
        self.calls = 0

    def device_resident_search_possible(self):
        return True

    def evaluate_circuits(self, circuits, parameter_values):
        self.calls += 1
        return [float(np.sum(np.cos(np.asarray(p) - 0.3 * np.arange(1, len(p) + 1)))) for p in parameter_values]


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for name in ("QSV_DEVICE_SEARCH", "QSV_SCALAR_SPSA", "QSV_DEVICE_SEARCH_MASK"):
        monkeypatch.delenv(name, raising=False)


CONFIGURATIONS = [
    (dict(maxfev=40), 20, 41),
    (dict(maxfev=23, reset_interval=4), None, None),
    (dict(maxfev=5), None, None),
    (dict(maxfev=1), None, None),
    (dict(maxfev=100, maxiter=7), 7, None),
    (dict(maxfev=12, reset_interval=0), None, None),
]


@pytest.mark.parametrize("kwargs,n_iterations,nfev", CONFIGURATIONS, ids=[str(c[0]) for c in CONFIGURATIONS])
def test_the_schedule_is_what_a_run_does(kwargs, n_iterations, nfev):
    """``nft_schedule`` against a real ``_NFTRun`` stepped with arbitrary values: the same base flag per iteration, the same
    number of iterations, the same final ``nfev`` -- for runs of several sizes (the schedule does not depend on the size)."""
    cfg = S.NFT(**kwargs)
    flags, total = device_search.nft_schedule(cfg)
    rng = np.random.default_rng(1)
    for size in (1, 3, 7):
        run = cfg.new_run(rng.normal(size=size), seed=None)
        seen = []
        while not run.done:
            points = run.propose()
            seen.append(len(points) == 3)
            assert len(points) in (2, 3)
            run.accept(*rng.normal(size=len(points)).tolist())
        assert seen == flags
        assert run.iteration == len(flags) and run.nfev == total
    if n_iterations is not None:
        assert len(flags) == n_iterations
    if nfev is not None:
        assert total == nfev
    assert flags[0] is True and all(isinstance(f, bool) for f in flags)


def test_a_configuration_that_evaluates_nothing_has_an_empty_schedule():
    assert device_search.nft_schedule(S.NFT(maxfev=0)) == ([], 0)
    assert S.NFT(maxfev=0).new_run([0.1], None).done


def test_nft_searches_are_opt_in_with_every_evaluator(monkeypatch):
    nft = S.NFT()
    estimator, sampling = _Stub(by_default=True), _MaskedStub(by_default=False)
    many = S._DEVICE_SEARCH_MIN_RUNS
    for n_runs in (2, many, 4 * many):
        for ev in (estimator, sampling):
            assert S._device_search_wanted(ev, n_runs, None, nft) is False
            assert S._device_search_wanted(ev, n_runs, True, nft) is True
            assert S._device_search_wanted(ev, n_runs, False, nft) is False
    assert S._device_search_wanted(estimator, 1, True, nft) is False
    assert S._device_search_wanted(_Stub(by_default=True, possible=False), many, True, nft) is False
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "1")
    assert S._device_search_wanted(estimator, many, None, nft) is True
    assert S._device_search_wanted(sampling, 2, None, nft) is True
    assert S._device_search_wanted(estimator, 1, None, nft) is False
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "0")
    assert S._device_search_wanted(estimator, many, True, nft) is False
    assert S._device_search_wanted(sampling, many, None, nft) is False
    # the SPSA rule next to it is what it was
    monkeypatch.delenv("QSV_DEVICE_SEARCH")
    assert S._device_search_wanted(estimator, many, None, S.SPSA(maxiter=5)) is True
    assert S._device_search_wanted(sampling, many, None, S.SPSA(maxiter=5)) is False


def _nft_jobs(cfg, n_jobs=5):
    rng = np.random.default_rng(4)
    return [(object(), cfg.new_run(rng.normal(size=1 + k % 3), seed=None)) for k in range(n_jobs)]


def test_minimize_batched_asks_only_when_asked_to(monkeypatch):
    """NFT jobs with ``on_device=True``: the device search is asked, declines, and the generic loop runs to the result it
    reaches without being asked; ``on_device=None`` (and an estimator's default) does not ask at all."""
    asked = []
    monkeypatch.setattr(device_search, "supported_nft", lambda evaluator, jobs: asked.append(len(jobs)) or False)
    monkeypatch.setattr(device_search, "minimize_nft_on_device", lambda *a, **k: pytest.fail("declined searches do not run"))
    cfg = S.NFT(maxfev=23, reset_interval=4)

    class Both(_HostOnly, _Stub):
        device_resident_search_by_default = True

        def __init__(self):
            _HostOnly.__init__(self)
            self._possible = True

    plain = _nft_jobs(cfg, S._DEVICE_SEARCH_MIN_RUNS + 1)
    S._minimize_batched(Both(), plain)
    assert asked == []
    by_default = _nft_jobs(cfg, S._DEVICE_SEARCH_MIN_RUNS + 1)
    S._minimize_batched(Both(), by_default, on_device=None)
    assert asked == []
    declined = _nft_jobs(cfg, S._DEVICE_SEARCH_MIN_RUNS + 1)
    S._minimize_batched(Both(), declined, on_device=True)
    assert asked == [len(declined)]
    for (_, a), (_, b), (_, c) in zip(plain, by_default, declined):
        assert a.done and b.done and c.done
        assert a.x.tolist() == b.x.tolist() == c.x.tolist()
        assert a.nfev == b.nfev == c.nfev and a.iteration == b.iteration == c.iteration
        assert a._recycled == b._recycled == c._recycled
    S._minimize_batched(Both(), _nft_jobs(cfg), on_device=False)
    assert asked == [len(declined)]
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "1")
    S._minimize_batched(Both(), _nft_jobs(cfg), on_device=None)
    assert asked == [len(declined), 5]


def test_supported_nft():
    cfg = S.NFT(maxfev=10)
    ev = _Stub(by_default=True)
    assert device_search.supported_nft(ev, _nft_jobs(cfg)) is True
    assert device_search.supported_nft(ev, _nft_jobs(cfg)[:1]) is False
    assert device_search.supported_nft(_Stub(possible=False), _nft_jobs(cfg)) is False
    # a run that has already advanced
    advanced = _nft_jobs(cfg)
    run = advanced[2][1]
    run.accept(*[0.1 * k for k in range(len(run.propose()))])
    assert run.iteration == 1 and not run.done
    assert device_search.supported_nft(ev, advanced) is False
    # two configuration objects, equal or not
    assert device_search.supported_nft(ev, _nft_jobs(cfg, 3) + _nft_jobs(S.NFT(maxfev=10), 3)) is False
    # SPSA runs among them
    mixed = _nft_jobs(cfg, 3) + [(object(), S.SPSA(maxiter=3).new_run([0.1, 0.2], seed=1))]
    assert device_search.supported_nft(ev, mixed) is False
    assert device_search.supported(ev, mixed) is False
    # an evaluator that cannot leave values on the device
    assert device_search.supported_nft(_HostOnly(), _nft_jobs(cfg)) is False
    # nothing to do
    assert device_search.supported_nft(ev, _nft_jobs(S.NFT(maxfev=0))) is False


def _declared_fields(struct_body: str):
    """(type, name) of every member of a C struct body, in order ("int32_t a, b;" declares two)."""
    fields = []
    for declaration in struct_body.split(";"):
        declaration = " ".join(declaration.split())
        if not declaration:
            continue
        first, *more = [part.strip() for part in declaration.split(",")]
        kind, name = first.rsplit(" ", 1)
        if name.startswith("*"):
            kind, name = kind + "*", name[1:]
        fields.append((kind, name))
        fields += [(kind, other) for other in more]
    return fields


def test_the_binding_matches_the_header():
    """``qsv_nft_step`` and ``qsv_nft_step_args`` as include/qsv.h declares them, field by field: name, order, type."""
    text = (ROOT / "include" / "qsv.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    match = re.search(r"typedef\s+struct\s+qsv_nft_step_args\s*\{(.*?)\}\s*qsv_nft_step_args\s*;", text, flags=re.S)
    assert match, "include/qsv.h does not declare qsv_nft_step_args"
    declared = _declared_fields(match.group(1))
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    want = [(name, C.c_void_p if "*" in kind else kinds[kind]) for kind, name in declared]
    assert [name for name, _ in want] == ["n_runs", "width", "columns_stride", "reserved", "x", "sizes", "columns", "recycled", "accept",
                                          "accept_with_base", "accept_iteration", "propose", "propose_with_base",
                                          "propose_iteration", "values", "points"]
    assert list(_lib.QsvNftStepArgs._fields_) == want
    # (every member on its natural alignment, no padding the compiler could place differently)
    assert C.sizeof(_lib.QsvNftStepArgs) == sum(C.sizeof(kind) for _, kind in want) == 96
    prototype = re.search(r"int\s+qsv_nft_step\s*\((.*?)\)\s*;", text, flags=re.S)
    assert prototype, "include/qsv.h does not declare qsv_nft_step"
    assert [" ".join(a.split()) for a in prototype.group(1).split(",")] == ["qsv_t* h", "const qsv_nft_step_args* args"]
    assert _lib.SIGNATURES["qsv_nft_step"] == (C.c_int, [C.c_void_p, C.c_void_p])
    lib = _lib.load()
    assert hasattr(lib, "qsv_nft_step")
    assert lib.qsv_nft_step(None, None) == _lib.QSV_E_ARG  # (no handle)


# ---- the driver, on a library in host memory --------------------------------------------------------------------------------


def _array(pointer, kind, shape):
    return np.ctypeslib.as_array(C.cast(C.c_void_p(pointer), C.POINTER(kind)), shape=shape)


class _HostLibrary:
    """``qsv_nft_step`` on host memory, row by row through ``_NFTRun.propose`` / ``accept`` themselves: a scratch run is given
    the row's variables and the state the call names, and what it leaves goes back into the arrays."""

    def __init__(self):
        self.steps = 0

    def qsv_nft_step(self, handle, reference):
        a = reference._obj
        self.steps += 1
        if (a.n_runs < 0 or a.width < 0 or a.columns_stride < 1 or not all((a.x, a.sizes, a.columns, a.recycled))
                or (a.accept and not a.values) or (a.propose and not a.points)):
            return _lib.QSV_E_ARG
        x = _array(a.x, C.c_double, (a.n_runs, a.width))
        sizes = _array(a.sizes, C.c_int32, (a.n_runs,))
        columns = _array(a.columns, C.c_int32, (a.n_runs, a.columns_stride))
        recycled = _array(a.recycled, C.c_double, (a.n_runs,))
        never_resets = S.NFT(maxfev=1 << 30, reset_interval=0)  # (the call says which form an iteration has, not the run)
        for r in range(a.n_runs):
            where = columns[r, : sizes[r]].astype(np.int64)
            if a.accept:
                k = 3 if a.accept_with_base else 2
                run = never_resets.new_run(x[r, where], seed=None)
                run.iteration, run._needs_base, run._recycled = int(a.accept_iteration), bool(a.accept_with_base), float(recycled[r])
                run.accept(*_array(a.values, C.c_double, (k * a.n_runs,))[k * r : k * r + k].tolist())
                x[r, where] = run.x
                recycled[r] = run._recycled
            if a.propose:
                k = 3 if a.propose_with_base else 2
                run = never_resets.new_run(x[r, where], seed=None)
                run.iteration, run._recycled = int(a.propose_iteration), None if a.propose_with_base else float(recycled[r])
                run.embed = (x[r].copy(), where)
                proposed = run.propose()
                assert len(proposed) == k
                _array(a.points, C.c_double, (k * a.n_runs, a.width))[k * r : k * r + k] = [S._full_point(run, p) for p in proposed]
        return _lib.QSV_OK


class _HostDevice:
    device_index = None  # (host memory: the searches make their tensors there)
    _handle = None

    def __init__(self):
        self._lib = _HostLibrary()

    def _check(self, rc):
        assert rc == _lib.QSV_OK


class _Circuit:
    def __init__(self, n_parameters):
        self.num_parameters = n_parameters


def _smooth(point) -> float:
    p = np.asarray(point, dtype=np.float64)
    return float(np.sum(np.cos(p - 0.3 * np.arange(1, p.size + 1))) + 0.1 * np.sum(np.sin(p) * np.sin(np.roll(p, 1) + 0.2)))


class _BothWays:
    """The same smooth function of a circuit's parameter vector from lists (``evaluate_circuits``: the generic loop) and from
    rows of a matrix in host memory into a vector there (``evaluate_device_to_device``: the device driver)."""

    def __init__(self):
        self.statevector_device = _HostDevice()
        self.lists = []

    def device_resident_search_possible(self):
        return True

    def evaluate_circuits(self, circuits, parameter_values):
        return [_smooth(p) for p in parameter_values]

    def evaluate_device_to_device(self, circuits, matrix, out):
        if not any(circuits is seen for seen in self.lists):
            self.lists.append(circuits)
        rows, values = matrix.numpy(), out.numpy()
        assert rows.shape[0] == len(circuits) <= values.size
        for i, circuit in enumerate(circuits):
            values[i] = _smooth(rows[i, : circuit.num_parameters])


def _embedded_nft_jobs(cfg):
    """Five jobs, two of them on a layer inside a longer vector."""
    rng = np.random.default_rng(9)
    jobs = []
    for total, positions in ((7, [1, 2, 5]), (1, None), (4, [0, 3]), (2, None), (3, None)):
        if positions is None:
            jobs.append((_Circuit(total), cfg.new_run(rng.normal(size=total), seed=None)))
        else:
            base = rng.normal(size=total)
            run = cfg.new_run(base[positions], seed=None)
            run.embed = (base, np.array(positions, dtype=np.int64))
            jobs.append((_Circuit(total), run))
    return jobs


def test_the_driver_leaves_what_the_generic_loop_leaves():
    """``minimize_nft_on_device`` with its tensors in host memory and ``qsv_nft_step`` played by ``_NFTRun`` itself: every run is
    left, bit for bit, as ``_minimize_batched``'s loop leaves it, and the evaluator has seen two list objects throughout."""
    cfg = S.NFT(maxfev=23, reset_interval=4)
    host, device = _embedded_nft_jobs(cfg), _embedded_nft_jobs(cfg)
    S._minimize_batched(_BothWays(), host, on_device=False)
    ev = _BothWays()
    assert device_search.supported_nft(ev, device)
    device_search.minimize_nft_on_device(ev, device)
    flags, nfev = device_search.nft_schedule(cfg)
    assert ev.statevector_device._lib.steps == len(flags) + 1
    assert len(ev.lists) == 2 and sorted(len(seen) for seen in ev.lists) == [10, 15]
    for (_, a), (_, b) in zip(host, device):
        assert a.done is True and b.done is True
        assert np.array_equal(a.x, b.x) and a.x.dtype == b.x.dtype
        assert a.iteration == b.iteration == len(flags) and a.nfev == b.nfev == nfev
        assert a._recycled == b._recycled and type(b._recycled) is float
        assert a._needs_base == b._needs_base
    assert any(not np.array_equal(run.x, fresh.x) for (_, run), (_, fresh) in zip(device, _embedded_nft_jobs(cfg)))
