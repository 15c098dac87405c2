"""The host code that feeds the whole-state consumers (csrc/qsv_api.hip: the sweep tables of csrc/adjoint_plan.hpp, the table blob,
the wrt check, the span timer, the host forms' head and tail) may not move a bit of what the kernels compute: the adjoint
gradients and values, the deflated gradients, costs, energies and overlaps, and the metric of one batch, against the bits the
commit before profiles/r28_sweep_tables.txt gave on the GPU (``golden/sweep_tables_parent.json``: hex doubles; of a full metric,
thousands of entries, the diagonal in hex doubles and the SHA-256 of the upper triangle's bytes, which any changed bit changes --
the entries of the permuted subsets, which are entries of the full matrices, are there in hex).  The kernels sum
in a fixed order (tests/test_gpu_adjoint.py, test_gpu_deflation.py and test_gpu_metric.py assert the same bits across
repetitions and batch positions), so the bits are a property of the tables the host hands them.

The batch: three distinct circuits and the first of them a second time at another point, on a handle with launch groups of two --
the tables hold circuits at a non-zero gate_base / run_base, an entry is reused, and the second group starts at position 2.  One
circuit has a shared parameter and literals; at n = T + 2 (several tile masks) one has a run that kAdjointMaxRunGates cuts.
Registers 6 and T + 2, both operator kinds of tests/test_gpu_adjoint.py.

The fixture was recorded at commit faf701d ("Fused tail: sum across lanes and write only the weights a side has") by this module
itself, copied into that commit's tests/.  To record it again (on the GPU, in a checkout of the commit whose bits are wanted):
    QSV_RECORD_SWEEP_TABLES=<file to write> python -m pytest tests/test_gpu_sweep_tables.py -m gpu"""

import hashlib
import json
import os
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import adjoint_reference
import circuit_families as cf
import test_gpu_adjoint as tga
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.ir import OP_ID, CircuitIR, ParamRef

pytestmark = pytest.mark.gpu

P = ParamRef
T = tga.T
SIZES = (6, T + 2)
MAX_RUN_GATES = 64  # csrc/adjoint_plan.hpp: kAdjointMaxRunGates
BETAS = (17.5, -0.0625)  # weights of unlike size
GOLDEN = Path(__file__).resolve().parent / "golden" / "sweep_tables_parent.json"
RECORD = os.environ.get("QSV_RECORD_SWEEP_TABLES", "")
_recorded = {}


def long_runs(n: int):
    """More than 64 gates in a row on six qubits (two of them the register's highest: one tile holds them all), then a cu3 down
    the register: a run cut by the gate limit, and above T qubits runs cut by their tile masks.  Most angles are literals (the
    fixture holds an entry per parameter)."""
    rng = np.random.default_rng(7000 + n)
    circuit, values = CircuitIR(n), []

    def angle(share_of_parameters):
        if rng.random() < share_of_parameters:
            values.append(float(rng.uniform(-np.pi, np.pi)))
            return P(len(values) - 1)
        return float(rng.uniform(-np.pi, np.pi))

    for q in range(n):
        circuit.u(angle(1.0), angle(0.0), angle(0.0), q)
    qubits = sorted({0, 1, 2, 5, n - 2, n - 1})
    for i in range(80):
        a, b = (int(x) for x in rng.choice(qubits, size=2, replace=False))
        if i % 3:
            circuit.u(angle(0.15), angle(0.05), angle(0.0), a)
        else:
            circuit.cu3(angle(0.15), angle(0.0), angle(0.05), a, b)
    for q in range(n - 1):
        circuit.cu3(angle(0.3), angle(0.0), angle(0.0), q, q + 1)
    circuit.declare_parameters(len(values))
    return circuit, values


def hub(n: int):
    """A u on every qubit and one cu3 from the highest qubit to the lowest: few parameters, a control outside the target's tile."""
    rng = np.random.default_rng(7100 + n)
    circuit = CircuitIR(n)
    for q in range(n):
        circuit.u(P(q), 0.1 * q, -0.3, q)
    circuit.cu3(P(n), P(n + 1), P(n + 2), n - 1, 0)
    return circuit, rng.uniform(-np.pi, np.pi, n + 3).tolist()


def _gates_of_runs(circuit) -> list:
    kinds = circuit.packed()["kind"]
    return [int((kinds[first:last + 1] != OP_ID).sum()) for _, first, last in adjoint_reference.describe(circuit)["runs"]]


@lru_cache(maxsize=None)
def batch(n: int):
    """(circuits, points): generic (a shared parameter, literals), long_runs, hub, and generic again at another point."""
    generic, generic_values = cf.generic(n, 60, share=0.3, literal=0.2)
    long_, long_values = long_runs(n)
    small, small_values = hub(n)
    assert tga._has_shared(generic)
    runs = _gates_of_runs(long_)
    assert sum(runs) > MAX_RUN_GATES and MAX_RUN_GATES in runs  # (a run the gate limit cut)
    if n > T:
        assert len({mask for mask, _, _ in adjoint_reference.describe(long_)["runs"]}) > 1
    circuits = [generic, long_, small, generic]
    points = [list(generic_values), list(long_values), list(small_values), [0.5 * v - 0.2 for v in generic_values]]
    return circuits, [p[: c.num_parameters] for c, p in zip(circuits, points)]


@lru_cache(maxsize=None)
def requests(n: int):
    """wrt lists per circuit: the parameters of the last gates (the sweep stops early) and two permuted subsets."""
    circuits, _ = batch(n)
    rng = np.random.default_rng(n)
    last = [tga._last_gates_parameters(c, 3) for c in circuits]
    permuted = [rng.permutation(c.num_parameters)[: 9 - e].tolist() for e, c in enumerate(circuits)]
    subset = [rng.permutation(c.num_parameters)[: 5 + 2 * e].tolist() for e, c in enumerate(circuits)]
    assert all(len(w) > 0 for w in last)
    return last, permuted, subset


def _hex(array) -> str:
    flat = np.ascontiguousarray(np.asarray(array)).view(np.float64).reshape(-1)
    return " ".join(float(x).hex() for x in flat)


def _upper(matrices) -> list:
    """A metric is symmetric to the bit (tests/test_gpu_metric.py): its upper triangle is all of it."""
    for m in matrices:
        assert np.array_equal(m, m.T)
    return [m[np.triu_indices(m.shape[0])] for m in matrices]


def outputs(ev, n: int, kept) -> tuple:
    """({name: hex doubles (a full metric: see above) of everything the batch's calls return}, the device times the calls left behind)."""
    dev = ev.statevector_device
    circuits, points = batch(n)
    last, permuted, subset = requests(n)
    out = {}
    gradients, values = dev.adjoint_gradients(circuits, points, return_values=True)
    out["adjoint gradients"], out["adjoint values"] = [_hex(g) for g in gradients], _hex(values)
    out["adjoint gradients, wrt the last gates"] = [_hex(g) for g in dev.adjoint_gradients(circuits, points, last)]
    out["adjoint gradients, wrt permuted"] = [_hex(g) for g in dev.adjoint_gradients(circuits, points, permuted)]
    gradients, costs, energies, overlaps = dev.deflated_gradients(circuits, points, kept, list(BETAS), with_values=True, with_overlaps=True)
    out["deflated gradients"] = [_hex(g) for g in gradients]
    out["deflated costs"], out["deflated energies"], out["deflated overlaps"] = _hex(costs), _hex(energies), _hex(overlaps)
    expect_ms = float(dev.profile()["expect_ms"])
    full = dev.metric_tensors(circuits, points)
    out["metric, diagonal"] = [_hex(np.diag(m)) for m in full]
    out["metric, sha256 of the upper triangle"] = [hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest() for m in _upper(full)]
    out["metric, wrt a permuted subset"] = [_hex(m) for m in _upper(dev.metric_tensors(circuits, points, subset))]
    stats = dev.metric_stats()
    return out, {"expect_ms": expect_ms, "run_ms": float(stats["run_ms"]), "gram_ms": float(stats["gram_ms"])}


@lru_cache(maxsize=None)
def golden() -> dict:
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("kind", tga.OPERATORS)
@pytest.mark.parametrize("n", SIZES)
def test_the_batch_gives_the_parents_bits(n, kind):
    dev = StatevectorDevice(n, group=2)
    assert int(dev._lib.qsv_group_size(dev._handle)) == 2
    ev = OperatorCircuitEvaluator(tga.operator(n, kind), statevector_device=dev, gradient_method="adjoint")
    circuits, points = batch(n)
    kept = dev.keep_states([circuits[2], circuits[0]], [[0.9 * v for v in points[2]], [v + 0.05 for v in points[0]]])
    got, _ = outputs(ev, n, kept)
    assert dev.adjoint_stats()["n_runs"] >= 1 and dev.metric_stats()["n_run_launches"] >= 1
    # under "time_moments": the same bits, and device times where the parent has them
    dev.set_option("time_moments", 1)
    timed, times = outputs(ev, n, kept)
    dev.set_option("time_moments", 0)
    print(f"n = {n}, {kind}: under time_moments expect_ms {times['expect_ms']:.4f} (the deflated call), run_ms {times['run_ms']:.4f}, "
          f"gram_ms {times['gram_ms']:.4f}")
    assert timed == got
    assert times["gram_ms"] > 0.0 and times["run_ms"] > 0.0 and times["expect_ms"] > 0.0
    dev.close()
    if RECORD:
        _recorded[f"n = {n}, {kind}"] = got
        # the metric reads no operator: one copy serves both kinds
        first = _recorded[f"n = {n}, {tga.OPERATORS[0]}"]
        assert all(got[name] == first[name] for name in got if name.startswith("metric"))
        stored = {key: {name: v for name, v in value.items() if not (name.startswith("metric") and tga.OPERATORS[0] not in key)}
                  for key, value in _recorded.items()}
        Path(RECORD).write_text(json.dumps(stored, indent=0) + "\n")
        return
    want = dict(golden()[f"n = {n}, {tga.OPERATORS[0]}"])
    want.update(golden()[f"n = {n}, {kind}"])
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name] == want[name], name
