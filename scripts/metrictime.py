"""Time OperatorCircuitEvaluator.metric_tensors on one MI355X and write profiles/r25_metric_tensor.txt.

  subject    metric_tensors(circuits, points, wrt): the Fubini-Study metric of every circuit's requested parameters, from one
             reverse sweep that carries derivative states and a real Gram matrix of them (qsv_metric_circuits)
  baselines  statevector() per circuit (2^n amplitudes over PCIe) and the backward construction of tests/metric_reference.py
             in NumPy on the host -- only where the columns of a circuit stay within --host-gib (default 2) of host memory --, and
             evaluate_gradients by the adjoint sweep for the same batch and wrt: the metric's cost in units of a gradient

Shapes: n = 20, 4 layers, wrt = the last layer; n = 20, 4 layers, every parameter; n = 24, 8 layers, wrt = the last layer (its
columns pass the default scratch bound: "metric_scratch_mib" is raised for it).  All variants of a shape run in one process,
interleaved: --warm rounds first, then --rounds timed rounds of one call each; a time is host wall time around a call that
returns its results, behind a synchronise.  Reported: the medians, and minimum / maximum per variant.  The run launches' and the
Gram kernel's own times come from HIP events on the handle's stream (option "time_moments", read back from metric_stats()) in
calls of their own.  Beside them: the bytes the run launches must move -- every run reads and writes psi and the columns alive in
it --, the bytes the Gram kernel needs (every vector once) and reads (32 vectors per pair of blocks), and the matrix pipe's fp64
operations on padded 16 x 16 tiles, 2 instructions of 2 * 16 * 16 * 4 per four amplitudes and pair of blocks.  Every figure is
what this run measured."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import adjoint_reference  # noqa: E402
import dense_gradient  # noqa: E402
import metric_reference as mr  # noqa: E402
from oracle import statevector_oracle as so  # noqa: E402
from queasars_amd import workloads  # noqa: E402
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator  # noqa: E402
from queasars_amd.ir import OP_CU3, OP_ID  # noqa: E402

SHAPES = (
    {"name": "n=20 L=4 1 circuit, last layer", "n": 20, "layers": 4, "circuits": 1, "last_layer": True, "scratch_mib": 8192},
    {"name": "n=20 L=4 1 circuit, every parameter", "n": 20, "layers": 4, "circuits": 1, "last_layer": False, "scratch_mib": 8192},
    {"name": "n=24 L=8 1 circuit, last layer", "n": 24, "layers": 8, "circuits": 1, "last_layer": True, "scratch_mib": 65536},
)


def host_metric(psi: np.ndarray, circuit, params, wrt) -> np.ndarray:
    """tests/metric_reference.backward from a state the device handed over (the sweep ends at the earliest requested gate)."""
    n = circuit.n_qubits
    ops, slots = circuit.bound_ops(params), mr._slots(circuit)
    psi = np.array(psi, dtype=np.complex128).reshape(1, -1)
    columns, owner = np.zeros((0, 1 << n), dtype=np.complex128), []
    readers = [k for k, (op, refs) in enumerate(zip(ops, slots)) if op[0] != OP_ID and any(p in wrt for p in refs)]
    for k in range(len(ops) - 1, min(readers, default=len(ops)) - 1, -1):
        (kind, target, control, theta, phi, lamb), refs = ops[k], slots[k]
        if kind == OP_ID:
            continue
        target, control = int(target), int(control) if kind == OP_CU3 else -1
        inverse = so.u_matrix(theta, phi, lamb).conj().T
        mr._apply_rows(psi, n, target, control, inverse)
        for slot, p in enumerate(refs):
            if p >= 0 and p in wrt:
                new = psi.copy()
                mr._apply_rows(new, n, target, control, dense_gradient.du_matrix(theta, phi, lamb, slot), derivative=True)
                columns = np.concatenate([columns, new], axis=0)
                owner.append(p)
        if columns.shape[0]:
            mr._apply_rows(columns, n, target, control, inverse)
    b = np.imag(columns @ psi[0].conj())
    per_slot = np.real(columns.conj() @ columns.T) - np.outer(b, b)
    select = np.array([[1.0 if o == p else 0.0 for o in owner] for p in wrt]).reshape(len(wrt), len(owner))
    return select @ per_slot @ select.T


def run_bytes(circuit, wrt, state_bytes: int) -> tuple[int, int, int]:
    """(bytes the run launches move, runs, columns): run r reads and writes psi and every column born at or behind its first op."""
    runs = adjoint_reference.describe(circuit)["runs"]
    born = [k for k, (row, refs) in enumerate(zip(circuit.packed(), mr._slots(circuit))) if int(row["kind"]) != OP_ID
            for p in refs if p >= 0 and p in wrt]
    moved = sum((1 + sum(1 for k in born if k >= first)) * 2 * state_bytes for _, first, _ in runs)
    return moved, len(runs), len(born)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--host-gib", type=float, default=2.0, help="most host memory a circuit's columns may take for the NumPy baseline to run")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r25_metric_tensor.txt")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("metrictime.py measures on a GPU: none found")
    lines = [f"metric_tensors against statevector() + NumPy and against adjoint gradients; {args.warm} warm-up and {args.rounds} timed rounds per "
             "shape, variants interleaved in one process, host wall time per call; kernel times from HIP events (calls of their own)",
             f"{'shape':38s} {'variant':26s} {'median ms':>11s} {'min ms':>11s} {'max ms':>11s} {'vs the call':>12s}"]
    records = []
    for shape in (SHAPES[i] for i in args.shapes):
        n, count = shape["n"], shape["circuits"]
        pop, circuits, params = workloads.population_circuits(n, shape["layers"], count, seed=0)
        params = [list(p) for p in params]
        if shape["last_layer"]:
            wrt = [list(range(c.num_parameters - ind.layers[-1].n_parameters, c.num_parameters)) for c, ind in zip(circuits, pop.individuals)]
        else:
            wrt = [list(range(c.num_parameters)) for c in circuits]
        evaluator = OperatorCircuitEvaluator(workloads.random_ising_operator(n, seed=2020), gradient_method="adjoint")
        dev = evaluator.statevector_device
        dev.set_option("metric_scratch_mib", shape["scratch_mib"])
        state_bytes = 16 << n
        moved, n_runs, n_cols = 0, 0, []
        for c, w in zip(circuits, wrt):
            m, r, k = run_bytes(c, set(w), state_bytes)
            moved, n_runs = moved + m, max(n_runs, r)
            n_cols.append(k)
        with_host = max(n_cols) * state_bytes <= args.host_gib * (1 << 30)

        def baseline():
            out = []
            for c, p, w in zip(circuits, params, wrt):
                out.append(host_metric(dev.statevector(c, p), c, p, w))
            torch.zeros(1, device="cuda").item()
            return out

        variants = {"metric_tensors": lambda: evaluator.metric_tensors(circuits, params, wrt),
                    "adjoint gradients": lambda: evaluator.evaluate_gradients(circuits, params, wrt)}
        if with_host:
            variants["statevector+numpy"] = baseline
        times = {name: [] for name in variants}
        results = {}
        for rnd in range(args.warm + args.rounds):
            for name, call in variants.items():  # (interleaved: every round runs each variant once)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results[name] = call()
                torch.cuda.synchronize()
                seconds = time.perf_counter() - t0
                if rnd >= args.warm:
                    times[name].append(seconds)
                print(f"  {shape['name']} round {rnd} {name}: {seconds * 1e3:.3f} ms", flush=True)
        err = None
        if with_host:
            err = max(float(np.abs(g - w).max()) for g, w in zip(results["metric_tensors"], results["statevector+numpy"]))
            if err > 1e-10:
                raise SystemExit(f"{shape['name']}: the variants disagree ({err:.3e})")
        base = float(np.median(times["metric_tensors"]))
        for name, t in times.items():
            med = float(np.median(t))
            records.append({"shape": shape["name"], "variant": name, "median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                            "ratio_to_call": med / base})
            lines.append(f"{shape['name']:38s} {name:26s} {med * 1e3:11.3f} {min(t) * 1e3:11.3f} {max(t) * 1e3:11.3f} {med / base:12.2f}")
            print(lines[-1], flush=True)
        if not with_host:
            lines.append(f"{shape['name']:38s} statevector+numpy: not measured ({max(n_cols)} columns of {state_bytes >> 20} MiB on the host)")
        # the kernels' own times: events around them, in calls of their own
        dev.set_option("time_moments", 1)
        run_ms, gram_ms = [], []
        for _ in range(args.warm + args.rounds):
            evaluator.metric_tensors(circuits, params, wrt)
            stats = dev.metric_stats()
            run_ms.append(float(stats["run_ms"]))
            gram_ms.append(float(stats["gram_ms"]))
        dev.set_option("time_moments", 0)
        run_t, gram_t = float(np.median(run_ms[args.warm:])), float(np.median(gram_ms[args.warm:]))
        pairs = [(-(-(k + 1) // 16)) * (-(-(k + 1) // 16) + 1) // 2 for k in n_cols]
        needed = sum((k + 1) * state_bytes for k in n_cols)
        panel_reads = sum(p * 32 * state_bytes for p in pairs)
        flops = sum(p * float(1 << n) / 4 * 2 * 2 * 16 * 16 * 4 for p in pairs)
        records.append({"shape": shape["name"], "columns": n_cols, "runs": n_runs, "run_ms": run_t, "gram_ms": gram_t, "run_bytes": moved,
                        "run_bytes_per_second": moved / (run_t * 1e-3), "gram_needed_bytes": needed, "gram_panel_bytes": panel_reads,
                        "gram_panel_bytes_per_second": panel_reads / (gram_t * 1e-3), "matrix_flops_per_second": flops / (gram_t * 1e-3),
                        "max_difference": err, "stats": stats})
        lines.append(f"{shape['name']:38s} columns {n_cols}, {n_runs} runs; run launches {run_t:.3f} ms for {moved / 1e6:.0f} MB = "
                     f"{moved / (run_t * 1e-3) / 1e12:.3f} TB/s; Gram kernel {gram_t:.3f} ms: needs {needed / 1e6:.0f} MB = "
                     f"{needed / (gram_t * 1e-3) / 1e12:.3f} TB/s, panels read {panel_reads / 1e6:.0f} MB = "
                     f"{panel_reads / (gram_t * 1e-3) / 1e12:.3f} TB/s, matrix pipe {flops / (gram_t * 1e-3) / 1e12:.2f} TFLOP/s fp64 (padded tiles)"
                     + (f"; largest difference to NumPy {err:.2e}" if err is not None else ""))
        print(lines[-1], flush=True)
        del evaluator, dev
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(records))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
