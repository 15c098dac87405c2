"""Time several observables per evaluation (StatevectorDevice.observable_values, qsv_eval_observables) against one
OperatorCircuitEvaluator per observable, on the workloads DESIGN.md reports:

  corr20     the benchmark population (n = 20, four layers, 64 individuals) x the 210 one- and two-body Z correlators + Ising
  general20  the same population x the 500-string general operator (workloads.random_pauli_operator(20, 500, seed=7))
  corr20L8   an eight-layer population (n = 20, 64 individuals) x the correlators
  general20L8  the eight-layer population x the 500-string operator (state route, ~one string per x-mask group)
  corr24L8   an eight-layer population (n = 24, 16 individuals) x the correlators

Every time is host wall time around a call that ends in a device synchronisation, the median of --reps calls after one
warm-up call.  Prints one JSON line per workload (and writes them to --out).  --only NAME runs one workload; --no-baseline
skips the per-observable evaluators (for a profiler run)."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator  # noqa: E402
from queasars_amd.circuit_evaluation.circuit_evaluation import StatevectorDevice  # noqa: E402
from queasars_amd.ir import PauliOperator  # noqa: E402
from queasars_amd.workloads import population_circuits, random_ising_operator, random_pauli_operator  # noqa: E402


def correlators(n: int) -> list[PauliOperator]:
    ops = [PauliOperator.from_sparse_list([("Z", [a], 1.0)], n) for a in range(n)]
    ops += [PauliOperator.from_sparse_list([("ZZ", [a, b], 1.0)], n) for a in range(n) for b in range(a + 1, n)]
    return ops


WORKLOADS = {
    "corr20": (20, 4, 64, "corr"),
    "general20": (20, 4, 64, "general"),
    "corr20L8": (20, 8, 64, "corr"),
    "general20L8": (20, 8, 64, "general"),
    "corr24L8": (24, 8, 16, "corr"),
}


def median_time(fn, reps: int) -> float:
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def run(name: str, reps: int, baseline: bool) -> dict:
    n, layers, count, kind = WORKLOADS[name]
    _, circuits, params = population_circuits(n, layers, count, seed=0)
    ops = correlators(n) + [random_ising_operator(n, seed=2020)] if kind == "corr" else [random_pauli_operator(n, 500, seed=7)]
    dev = StatevectorDevice(n)
    values = dev.observable_values(circuits, params, ops)
    t_new = median_time(lambda: dev.observable_values(circuits, params, ops), reps)
    forms = [dev.circuit_form(c)["route"] for c in circuits]
    record = {"workload": name, "n": n, "layers": layers, "evaluations": count, "observables": len(ops),
              "distinct_strings": len({(int(x), int(z)) for op in ops for x, z in zip(op.x_mask, op.z_mask)}),
              "routes": {str(r): forms.count(r) for r in sorted(set(forms))},
              "observables_ms": t_new * 1e3, "observables_us_per_evaluation": t_new * 1e6 / count}
    if baseline:
        evaluators = [OperatorCircuitEvaluator(op, statevector_device=dev) for op in ops]
        t0 = time.perf_counter()
        want = np.stack([np.asarray(ev.evaluate_circuits(circuits, params)) for ev in evaluators], axis=1)
        t_old = time.perf_counter() - t0
        record.update({"per_observable_ms": t_old * 1e3, "speedup": t_old / t_new,
                       "max_abs_diff": float(np.abs(values - want).max())})
    dev.close()
    return record


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", type=Path)
    args = ap.parse_args()
    lines = []
    for name in ([args.only] if args.only else list(WORKLOADS)):
        record = run(name, args.reps, not args.no_baseline)
        line = json.dumps(record)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
