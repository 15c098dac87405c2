"""What the device-resident Adam search decides and checks without a device: the bindings of the gradient-plan functions and
``qsv_adam_step`` against the header, the rule that sends an Adam search to the device (opt-in: ``solver._device_search_wanted`` /
``_minimize_batched`` / ``device_search.supported_adam``), and the driver itself, ``minimize_adam_on_device``, against a stub
evaluator whose plan and step are NumPy emulations of the contracts include/qsv.h documents -- which must leave every run as
``solver._minimize_adam`` leaves it."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from queasars_amd import _lib
from queasars_amd.evqe import device_search
from queasars_amd.evqe import solver as S

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for name in ("QSV_DEVICE_SEARCH", "QSV_SCALAR_SPSA", "QSV_SHARE_CIRCUITS"):
        monkeypatch.delenv(name, raising=False)


# ---- the binding ----------------------------------------------------------------------------------------------------------


def _header() -> str:
    text = (ROOT / "include" / "qsv.h").read_text()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


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


def _struct(text: str, name: str):
    match = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", text, flags=re.S)
    assert match, f"include/qsv.h does not declare {name}"
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    return [(field, C.c_void_p if "*" in kind else kinds[kind]) for kind, field in _declared_fields(match.group(1))]


def _prototype(text: str, name: str):
    match = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert match, f"include/qsv.h does not declare {name}"
    return [" ".join(a.split()) for a in match.group(1).split(",")]


def test_the_adam_step_binding_matches_the_header():
    text = _header()
    want = _struct(text, "qsv_adam_step_args")
    assert [name for name, _ in want] == ["n_runs", "width", "columns_stride", "grad_width", "x", "sizes", "columns", "m", "v", "gradient",
                                          "active", "iterations", "lr", "beta_1", "beta_2", "one_minus_beta_1", "one_minus_beta_2",
                                          "eps", "tol", "bias_1", "bias_2", "maxiter"]
    assert list(_lib.QsvAdamStepArgs._fields_) == want
    # (every member on its natural alignment, no padding the compiler could place differently)
    assert C.sizeof(_lib.QsvAdamStepArgs) == sum(C.sizeof(kind) for _, kind in want) == 4 * 4 + 8 * 8 + 9 * 8 + 8
    assert _prototype(text, "qsv_adam_step") == ["qsv_t* h", "const qsv_adam_step_args* args"]
    assert _lib.SIGNATURES["qsv_adam_step"] == (C.c_int, [C.c_void_p, C.c_void_p])
    lib = _lib.load()
    assert lib.qsv_adam_step(None, None) == _lib.QSV_E_ARG  # (no handle)


def test_the_gradient_plan_bindings_match_the_header():
    text = _header()
    want = _struct(text, "qsv_gradient_plan_stats_t")
    assert [name for name, _ in want] == ["n_shifted", "n_chunks", "n_runs", "n_host_waits", "table_bytes"]
    assert list(_lib.QsvGradientPlanStats._fields_) == want
    assert C.sizeof(_lib.QsvGradientPlanStats) == 40
    # the struct the plans must not touch
    assert [name for name, _ in _struct(text, "qsv_gradient_stats_t")] == ["n_shifted", "n_chunks", "n_allocations", "scratch_bytes"]
    P = C.c_void_p
    assert _prototype(text, "qsv_gradient_plan_create") == [
        "qsv_t* h", "int n_evals", "const int* circuit_ids", "int width", "const int64_t* wrt_offsets", "const int32_t* wrt",
        "int out_width", "int* out_plan_id", "int64_t* out_n_shifted"]
    assert _lib.SIGNATURES["qsv_gradient_plan_create"] == (
        C.c_int, [P, C.c_int, P, C.c_int, P, P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)])
    assert _prototype(text, "qsv_gradient_plan_run") == [
        "qsv_t* h", "int plan_id", "const double* device_values", "void* ready_event", "double* device_out"]
    assert _lib.SIGNATURES["qsv_gradient_plan_run"] == (C.c_int, [P, C.c_int, P, P, P])
    assert _prototype(text, "qsv_gradient_plan_destroy") == ["qsv_t* h", "int plan_id"]
    assert _lib.SIGNATURES["qsv_gradient_plan_destroy"] == (C.c_int, [P, C.c_int])
    assert _prototype(text, "qsv_gradient_plan_stats") == ["const qsv_t* h", "int plan_id", "qsv_gradient_plan_stats_t* out"]
    assert _lib.SIGNATURES["qsv_gradient_plan_stats"] == (C.c_int, [P, C.c_int, C.POINTER(_lib.QsvGradientPlanStats)])
    lib = _lib.load()
    plan_id, n_shifted, stats = C.c_int(0), C.c_int64(0), _lib.QsvGradientPlanStats()
    assert lib.qsv_gradient_plan_create(None, 0, None, 0, None, None, 0, C.byref(plan_id), C.byref(n_shifted)) == _lib.QSV_E_ARG
    assert lib.qsv_gradient_plan_run(None, 1, None, None, None) == _lib.QSV_E_ARG
    assert lib.qsv_gradient_plan_destroy(None, 1) == _lib.QSV_E_ARG
    assert lib.qsv_gradient_plan_stats(None, 1, C.byref(stats)) == _lib.QSV_E_ARG


# ---- a library in host memory ---------------------------------------------------------------------------------------------


def _array(pointer, kind, shape):
    return np.ctypeslib.as_array(C.cast(C.c_void_p(pointer), C.POINTER(kind)), shape=shape)


class _HostLibrary:
    """``qsv_adam_step`` as include/qsv.h documents it, on host memory: one scalar operation at a time, in the documented order."""

    def __init__(self):
        self.steps = 0

    def qsv_adam_step(self, handle, reference):
        a = reference._obj
        self.steps += 1
        if (a.n_runs < 0 or a.width < 0 or a.grad_width < 0 or a.columns_stride < 1 or a.grad_width < a.columns_stride
                or not all((a.x, a.sizes, a.columns, a.m, a.v, a.gradient, a.active, a.iterations))):
            return _lib.QSV_E_ARG
        if a.n_runs == 0 or a.width == 0:
            return _lib.QSV_OK
        x = _array(a.x, C.c_double, (a.n_runs, a.width))
        sizes = _array(a.sizes, C.c_int32, (a.n_runs,))
        columns = _array(a.columns, C.c_int32, (a.n_runs, a.columns_stride))
        m, v, gradient = (_array(p, C.c_double, (a.n_runs, a.grad_width)) for p in (a.m, a.v, a.gradient))
        active = _array(a.active, C.c_uint8, (a.n_runs,))
        iterations = _array(a.iterations, C.c_int64, (a.n_runs,))
        f = np.float64
        for r in range(a.n_runs):
            if not active[r]:
                continue
            total = f(0.0)
            for j in range(int(sizes[r])):
                g = gradient[r, j]
                m[r, j] = f(a.beta_1) * m[r, j] + f(a.one_minus_beta_1) * g
                v[r, j] = f(a.beta_2) * v[r, j] + f(a.one_minus_beta_2) * (g * g)
                u = f(a.lr) * (m[r, j] / f(a.bias_1)) / (np.sqrt(v[r, j] / f(a.bias_2)) + f(a.eps))
                x[r, columns[r, j]] = x[r, columns[r, j]] - u
                total = total + u * u
            iterations[r] += 1
            if iterations[r] >= a.maxiter or (a.tol > 0 and np.sqrt(total) < a.tol):
                active[r] = 0
        return _lib.QSV_OK


class _HostDevice:
    device_index = None  # (host memory: minimize_adam_on_device makes its tensors there)
    _handle = None

    def __init__(self):
        self._lib = _HostLibrary()

    def _check(self, rc):
        assert rc == _lib.QSV_OK


class _Circuit:
    """What the drivers ask of a circuit: its parameter count and its shift plan (two evaluations per angle, four for every
    fifth -- a cu3's theta)."""

    def __init__(self, n_parameters):
        self.num_parameters = n_parameters

    def gradient_terms(self):
        return [4 if p % 5 == 4 else 2 for p in range(self.num_parameters)]


def _value_gradient(point: np.ndarray, wrt) -> np.ndarray:
    """d/dp of sum_k cos(p_k - 0.3 (k + 1)) + 0.1 sin(p_k) sin(p_(k+1 mod n)): smooth, coupled, no symmetry between entries."""
    p = np.asarray(point, dtype=np.float64)
    k = np.arange(1, p.size + 1)
    g = -np.sin(p - 0.3 * k) + 0.1 * np.cos(p) * (np.sin(np.roll(p, -1)) + np.sin(np.roll(p, 1)))
    return g[np.asarray(wrt, dtype=np.int64)].copy()


class _PlanEvaluator:
    """An evaluator with gradients on the host (``evaluate_gradients``, what ``_minimize_adam`` calls) and the same gradients
    as a plan over tensors in host memory (``gradient_plan``, what ``minimize_adam_on_device`` calls)."""

    def __init__(self):
        self.statevector_device = _HostDevice()
        self.plans, self.runs, self.closed = 0, 0, 0

    def device_resident_search_possible(self):
        return True

    def evaluate_gradients(self, circuits, parameter_values, wrt=None):
        self.last_gradient_evaluations = sum(sum(c.gradient_terms()[p] for p in w) for c, w in zip(circuits, wrt))
        return [_value_gradient(p, w) for p, w in zip(parameter_values, wrt)]

    def gradient_plan(self, circuits, matrix, out, wrt=None):
        owner = self
        assert matrix.shape[0] == out.shape[0] == len(circuits) == len(wrt)
        assert max(len(w) for w in wrt) <= out.shape[1]

        class Plan:
            n_shifted = sum(sum(c.gradient_terms()[p] for p in w) for c, w in zip(circuits, wrt))

            def run(self, matrix, out, ready=True):
                owner.runs += 1
                points, rows = matrix.numpy(), out.numpy()
                rows[:] = 0.0
                for i, (circuit, positions) in enumerate(zip(circuits, wrt)):
                    rows[i, : len(positions)] = _value_gradient(points[i, : circuit.num_parameters], positions)
                return self.n_shifted

            def close(self):
                owner.closed += 1

        self.plans += 1
        return Plan()


def _adam_jobs(cfg, embedded: bool, n_jobs: int = 5, seed: int = 3):
    """Runs of several sizes: on rows of their own, or (embedded) on a layer inside a longer vector, at scattered positions."""
    rng = np.random.default_rng(seed)
    jobs = []
    for k in range(n_jobs):
        size = 1 + (3 * k) % 7
        if embedded:
            total = size + 2 + k
            positions = np.sort(rng.choice(total, size=size, replace=False)).astype(np.int64)
            base = rng.normal(size=total)
            run = cfg.new_run(base[positions], seed=None)
            run.embed = (base, positions)
            jobs.append((_Circuit(total), run))
        else:
            jobs.append((_Circuit(size), cfg.new_run(rng.normal(size=size), seed=None)))
    return jobs


def _host_update_norms(cfg, embedded):
    """Every update norm ``_minimize_adam`` forms on these jobs (what ``tol`` is compared with), run by run."""
    norms = []
    ev = _PlanEvaluator()
    for circuit, run in _adam_jobs(S.Adam(maxiter=cfg.maxiter, lr=cfg.lr, tol=0.0), embedded):
        while not run.done:
            positions = list(range(run.x.size)) if run.embed is None else [int(p) for p in run.embed[1]]
            run.accept_gradient(ev.evaluate_gradients([circuit], [S._full_point(run, run.x)], [positions])[0], 0)
            t = run.iteration  # (the update once more, by accept_gradient's own expressions: the same bits)
            update = cfg.lr * (run.m / (1 - cfg.beta_1**t)) / (np.sqrt(run.v / (1 - cfg.beta_2**t)) + cfg.eps)
            norms.append(float(np.linalg.norm(update)))
    return np.array(norms)


@pytest.mark.parametrize("embedded", [False, True], ids=["own rows", "embedded"])
@pytest.mark.parametrize("tol", [0.0, 0.06], ids=["tol=0", "tol>0"])
def test_the_driver_leaves_what_the_host_driver_leaves(embedded, tol):
    cfg = S.Adam(maxiter=21, lr=0.1, tol=tol)
    if tol > 0:
        # (the norm is the one number the two drivers sum differently: no norm of the reference search may decide by rounding)
        norms = _host_update_norms(cfg, embedded)
        assert np.all(np.abs(norms - tol) > 1e-6 * tol)
    host, device = _adam_jobs(cfg, embedded), _adam_jobs(cfg, embedded)
    S._minimize_adam(_PlanEvaluator(), host)
    ev = _PlanEvaluator()
    assert device_search.supported_adam(ev, device)
    device_search.minimize_adam_on_device(ev, device, look_every=4)
    assert ev.plans == 1 and ev.closed == 1
    for (_, a), (_, b) in zip(host, device):
        assert a.done and b.done
        assert np.array_equal(a.x, b.x) and np.array_equal(a.m, b.m) and np.array_equal(a.v, b.v)
        assert a.iteration == b.iteration and a.nfev == b.nfev and b.nfev > 0
    stopped = [a.iteration for _, a in host]
    if tol > 0:
        assert min(stopped) < cfg.maxiter  # (the rule stopped someone)
        assert ev.runs == ev.statevector_device._lib.steps <= cfg.maxiter
        assert ev.runs % 4 == 0 or ev.runs == cfg.maxiter  # (the host looks every fourth iteration)
        assert ev.runs >= max(stopped)
    else:
        assert stopped == [cfg.maxiter] * len(host)
        assert ev.runs == ev.statevector_device._lib.steps == cfg.maxiter


def test_the_driver_checks_the_plan_against_the_shift_plans():
    cfg = S.Adam(maxiter=3)
    ev = _PlanEvaluator()
    jobs = _adam_jobs(cfg, False)
    original = ev.gradient_plan

    def off_by_some(circuits, matrix, out, wrt=None):
        plan = original(circuits, matrix, out, wrt)
        plan.n_shifted += 2
        return plan

    ev.gradient_plan = off_by_some
    with pytest.raises(RuntimeError, match="shifted evaluations"):
        device_search.minimize_adam_on_device(ev, jobs)
    assert ev.closed == 1 and ev.runs == 0


# ---- gating ---------------------------------------------------------------------------------------------------------------


class _Gate:
    """An evaluator as the gating rule sees it."""

    def __init__(self, by_default=True, possible=True, plans=True):
        self.device_resident_search_by_default = by_default
        self._possible = possible
        if plans:
            self.gradient_plan = lambda *a, **k: pytest.fail("the rule plans nothing")

    def device_resident_search_possible(self):
        return self._possible

    def evaluate_device_to_device(self, circuits, matrix, out):
        raise AssertionError("the rule evaluates nothing")


def test_adam_searches_are_opt_in(monkeypatch):
    adam = S.Adam(maxiter=5)
    many = S._DEVICE_SEARCH_MIN_RUNS
    for ev in (_Gate(by_default=True), _Gate(by_default=False)):
        for n_runs in (2, many, 4 * many):
            assert S._device_search_wanted(ev, n_runs, None, adam) is False
            assert S._device_search_wanted(ev, n_runs, True, adam) is True
            assert S._device_search_wanted(ev, n_runs, False, adam) is False
        assert S._device_search_wanted(ev, 1, True, adam) is False
    assert S._device_search_wanted(_Gate(possible=False), many, True, adam) is False
    assert S._device_search_wanted(_Gate(plans=False), many, True, adam) is False
    assert S._device_search_wanted(_Gate(), many, True, S.Adam(maxiter=0)) is False
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "1")
    assert S._device_search_wanted(_Gate(), many, None, adam) is True
    assert S._device_search_wanted(_Gate(by_default=False), 2, None, adam) is True
    assert S._device_search_wanted(_Gate(), 1, None, adam) is False
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "0")
    assert S._device_search_wanted(_Gate(), many, True, adam) is False
    assert S._device_search_wanted(_Gate(), many, None, adam) is False
    # the rules next to it are what they were
    monkeypatch.delenv("QSV_DEVICE_SEARCH")
    assert S._device_search_wanted(_Gate(), many, None, S.SPSA(maxiter=5)) is True
    assert S._device_search_wanted(_Gate(), many, None, S.NFT()) is False


def test_supported_adam():
    cfg = S.Adam(maxiter=4)
    ev = _PlanEvaluator()
    assert device_search.supported_adam(ev, _adam_jobs(cfg, False)) is True
    assert device_search.supported_adam(ev, _adam_jobs(cfg, True)) is True
    assert device_search.supported_adam(ev, _adam_jobs(cfg, False)[:1]) is False
    assert device_search.supported_adam(_Gate(possible=False), _adam_jobs(cfg, False)) is False
    assert device_search.supported_adam(_Gate(plans=False), _adam_jobs(cfg, False)) is False
    # a run that has already moved
    moved = _adam_jobs(cfg, False)
    moved[2][1].accept_gradient(np.full(moved[2][1].x.size, 0.25), 2)
    assert moved[2][1].iteration == 1 and not moved[2][1].done
    assert device_search.supported_adam(ev, moved) is False
    # ... and runs that all stand at the same later iteration, but with moments
    for _, run in moved:
        if run.iteration == 0:
            run.accept_gradient(np.full(run.x.size, 0.25), 2)
    assert device_search.supported_adam(ev, moved) is False
    # two configuration objects, equal or not
    assert device_search.supported_adam(ev, _adam_jobs(cfg, False, 3) + _adam_jobs(S.Adam(maxiter=4), False, 3)) is False
    # other optimisers' runs among them
    mixed = _adam_jobs(cfg, False, 3) + [(object(), S.SPSA(maxiter=3).new_run([0.1, 0.2], seed=1))]
    assert device_search.supported_adam(ev, mixed) is False
    # nothing to do
    assert device_search.supported_adam(ev, _adam_jobs(S.Adam(maxiter=0), False)) is False


def test_minimize_batched_asks_only_when_asked_to(monkeypatch):
    """Adam jobs go to the device driver with ``on_device=True`` or ``QSV_DEVICE_SEARCH=1`` only; a declined search and a search
    nobody asked about both run ``_minimize_adam`` to the same result; one run alone is never asked about."""
    asked = []
    monkeypatch.setattr(device_search, "supported_adam", lambda evaluator, jobs: asked.append(len(jobs)) or False)
    monkeypatch.setattr(device_search, "minimize_adam_on_device", lambda *a, **k: pytest.fail("declined searches do not run"))
    cfg = S.Adam(maxiter=6)
    n = S._DEVICE_SEARCH_MIN_RUNS + 1
    plain, by_default, declined = (_adam_jobs(cfg, False, n) for _ in range(3))
    S._minimize_batched(_PlanEvaluator(), plain)
    S._minimize_batched(_PlanEvaluator(), by_default, on_device=None)
    assert asked == []
    S._minimize_batched(_PlanEvaluator(), declined, on_device=True)
    assert asked == [n]
    for (_, a), (_, b), (_, c) in zip(plain, by_default, declined):
        assert a.done and b.done and c.done
        assert a.x.tolist() == b.x.tolist() == c.x.tolist() and a.nfev == b.nfev == c.nfev
    S._minimize_batched(_PlanEvaluator(), _adam_jobs(cfg, False)[:1], on_device=True)
    assert asked == [n]
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "1")
    S._minimize_batched(_PlanEvaluator(), _adam_jobs(cfg, False), on_device=None)
    assert asked == [n, 5]
    monkeypatch.setenv("QSV_DEVICE_SEARCH", "0")
    S._minimize_batched(_PlanEvaluator(), _adam_jobs(cfg, False), on_device=True)
    assert asked == [n, 5]


def test_minimize_batched_takes_the_device_driver_when_it_can(monkeypatch):
    taken = []
    real = device_search.minimize_adam_on_device
    monkeypatch.setattr(device_search, "minimize_adam_on_device", lambda ev, jobs, **k: taken.append(len(jobs)) or real(ev, jobs, **k))
    cfg = S.Adam(maxiter=5)
    host, device = _adam_jobs(cfg, True), _adam_jobs(cfg, True)
    S._minimize_batched(_PlanEvaluator(), host, on_device=None)
    assert taken == []
    S._minimize_batched(_PlanEvaluator(), device, on_device=True)
    assert taken == [5]
    for (_, a), (_, b) in zip(host, device):
        assert np.array_equal(a.x, b.x) and a.nfev == b.nfev and a.iteration == b.iteration == 5


def test_mixed_optimisers_still_raise():
    jobs = _adam_jobs(S.Adam(maxiter=3), False, 3) + [(object(), S.SPSA(maxiter=3).new_run([0.1, 0.2], seed=1))]
    for flag in (None, True, False):
        with pytest.raises(ValueError, match="cannot share a search"):
            S._minimize_batched(_PlanEvaluator(), jobs, on_device=flag)
