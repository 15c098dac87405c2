"""Time the parameter-shift gradients of the headline population -- n = 20, 64 individuals, four layers, the 210-term Ising
operator -- on one MI355X and write profiles/r07_gradients.txt.

  subject    the full gradient (every parameter of every circuit) and one searched layer (the last), each through
               host     OperatorCircuitEvaluator.evaluate_gradients (points as lists, gradients as arrays)
               device   OperatorCircuitEvaluator.evaluate_gradients_device_to_device (points and gradients in device memory)
  baseline   the same gradients from the public API without the gradient entry points: shifted parameter lists built in
             Python, one evaluate_circuits call, the NumPy combination (what a user had to write before)

All variants run in ONE process, interleaved: --warm rounds first, then --rounds rounds of one call each; a time is host wall
time around a call that ends with its results complete (a device synchronise for the device form).  Reported: median, minimum
and maximum per variant, the ratio of medians to the baseline, and the run-to-run spread (max - min) / median the condition
"not slower than the baseline beyond the spread" is judged against.  The expansion and combination kernels' own times come
from a `rocprofv3 --kernel-trace --stats` run of their own: a fresh child process (`--kernels`) that only makes gradient
calls.  Every figure is what this run measured; nothing is estimated."""

from __future__ import annotations

import argparse
import csv
import json
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from queasars_amd import workloads  # noqa: E402
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator  # noqa: E402
from queasars_amd.evqe import EVQEPopulation  # noqa: E402

S1 = np.pi / 2
SHIFTS = (S1, -S1, 3.0 * S1, -3.0 * S1)
CP = (np.sqrt(2.0) + 1.0) / (4.0 * np.sqrt(2.0))
CM = (np.sqrt(2.0) - 1.0) / (4.0 * np.sqrt(2.0))
HEADLINE_RATE = 1.35e6  # evaluations per second of the headline population


def workload(args):
    pop = EVQEPopulation.random_population(args.n, args.layers, args.individuals, True, 0)
    circuits = [ind.get_parameterized_quantum_circuit() for ind in pop.individuals]
    params = [list(ind.parameter_values) for ind in pop.individuals]
    last = args.layers - 1
    layer = [list(range(ind.circuit_parameter_offsets[last], ind.circuit_parameter_offsets[last] + ind.layers[last].n_parameters))
             for ind in pop.individuals]
    return circuits, params, {"full": [list(range(c.num_parameters)) for c in circuits], "layer": layer}


def baseline_gradients(evaluator, circuits, params, terms, wrt):
    """Public API of the parent commit only: Python-built shifted lists, evaluate_circuits, NumPy."""
    owners, points = [], []
    for c, t, p, w in zip(circuits, terms, params, wrt):
        for j in w:
            for s in SHIFTS[: t[j]]:
                q = list(p)
                q[j] = p[j] + s
                points.append(q)
                owners.append(c)
    v = np.asarray(evaluator.evaluate_circuits(owners, points))
    out, cur = [], 0
    for t, w in zip(terms, wrt):
        g = np.zeros(len(w))
        for k, j in enumerate(w):
            if t[j] == 2:
                g[k] = 0.5 * (v[cur] - v[cur + 1])
            elif t[j] == 4:
                g[k] = CP * (v[cur] - v[cur + 1]) - CM * (v[cur + 2] - v[cur + 3])
            cur += t[j]
        out.append(g)
    return out, len(points)


def kernels_only(args) -> None:
    """The child of the profiled run: a few gradient calls of both subjects, nothing else."""
    import torch

    circuits, params, subjects = workload(args)
    evaluator = OperatorCircuitEvaluator(workloads.random_ising_operator(args.n, seed=0))
    for _ in range(args.kernel_calls):
        for wrt in subjects.values():
            evaluator.evaluate_gradients(circuits, params, wrt)
    torch.cuda.synchronize()


def profiled_kernel_times(args) -> dict:
    rocprof = shutil.which("rocprofv3")
    if rocprof is None:
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory(dir=args.out.parent) as tmp:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, str(Path(__file__).resolve()),
               "--kernels", "--n", str(args.n), "--layers", str(args.layers), "--individuals", str(args.individuals),
               "--kernel-calls", str(args.kernel_calls)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.kernel_timeout)
        if res.returncode != 0:
            return {"error": f"rocprofv3 run failed ({res.returncode}): {res.stdout[-400:]}"}
        rows = {}
        try:
            for path in Path(tmp).rglob("*kernel_stats.csv"):
                with path.open() as f:
                    for row in csv.DictReader(f):
                        name = row.get("Name", "")
                        if "gradient_" in name or "pass_kernel" in name or "factor" in name:
                            rows[name.replace("(anonymous namespace)::", "").split("(")[0][-70:]] = {"calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3,
                                                             "average_us": float(row["AverageNs"]) / 1e3,
                                                             "share_percent": float(row.get("Percentage", "nan"))}
        except (KeyError, ValueError) as exc:
            return {"error": f"unexpected kernel statistics layout: {exc!r}"}
        return rows or {"error": "no kernel statistics found in " + ", ".join(p.name for p in Path(tmp).rglob("*"))[:300]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--individuals", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--kernels", action="store_true", help="(the profiled child: gradient calls only)")
    ap.add_argument("--kernel-calls", type=int, default=3)
    ap.add_argument("--kernel-timeout", type=int, default=300)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r07_gradients.txt")
    args = ap.parse_args()
    if args.kernels:
        kernels_only(args)
        return

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("gradtime.py measures on a GPU: none found")
    circuits, params, subjects = workload(args)
    terms = [c.gradient_terms() for c in circuits]
    evaluator = OperatorCircuitEvaluator(workloads.random_ising_operator(args.n, seed=0))
    width = max(c.num_parameters for c in circuits)
    matrix = torch.zeros((len(circuits), width), dtype=torch.float64, device="cuda")
    for e, p in enumerate(params):
        matrix[e, : len(p)] = torch.tensor(p, dtype=torch.float64)
    out = torch.zeros((len(circuits), width), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def run(variant, wrt):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if variant == "baseline":
            grads, count = baseline_gradients(evaluator, circuits, params, terms, wrt)
        elif variant == "host":
            grads = evaluator.evaluate_gradients(circuits, params, wrt)
            count = evaluator.last_gradient_evaluations
        else:
            evaluator.evaluate_gradients_device_to_device(circuits, matrix, out, wrt)
            torch.cuda.synchronize()
            grads, count = None, evaluator.last_gradient_evaluations
        return time.perf_counter() - t0, grads, count

    records, lines = [], []
    for subject, wrt in subjects.items():
        times = {v: [] for v in ("baseline", "host", "device")}
        reference = None
        for rnd in range(args.warm + args.rounds):
            for variant in times:  # (interleaved: every round runs each variant once)
                seconds, grads, count = run(variant, wrt)
                if variant == "baseline":
                    reference = grads
                elif variant == "host":
                    same = all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(grads, reference))
                    if not same:
                        raise SystemExit(f"{subject}: the host entry point and the baseline differ")
                else:
                    got = out.cpu().numpy()
                    if not all(np.array_equal(got[e, : len(r)].view(np.uint64), r.view(np.uint64)) for e, r in enumerate(reference)):
                        raise SystemExit(f"{subject}: the device entry point and the baseline differ")
                if rnd >= args.warm:
                    times[variant].append(seconds)
        base = float(np.median(times["baseline"]))
        for variant, t in times.items():
            med = float(np.median(t))
            records.append({"subject": subject, "variant": variant, "shifted_evaluations": count, "rounds": args.rounds,
                            "median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                            "spread": (max(t) - min(t)) / med, "ratio_to_baseline": med / base,
                            "evaluations_per_second": count / med, "share_of_headline_rate": count / med / HEADLINE_RATE})
    lines.append(f"parameter-shift gradients, n = {args.n}, {args.individuals} individuals, {args.layers} layers, 210-term Ising operator; "
                 f"{args.warm} warm-up and {args.rounds} timed rounds, variants interleaved in one process; results of all three bitwise equal")
    lines.append(f"{'subject':8s} {'variant':9s} {'shifted':>8s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'spread':>7s} "
                 f"{'vs baseline':>11s} {'evals/s':>10s} {'of 1.35 M/s':>11s}")
    for r in records:
        lines.append(f"{r['subject']:8s} {r['variant']:9s} {r['shifted_evaluations']:8d} {r['median_ms']:10.3f} {r['min_ms']:9.3f} "
                     f"{r['max_ms']:9.3f} {r['spread']:7.3f} {r['ratio_to_baseline']:11.3f} {r['evaluations_per_second']:10.0f} "
                     f"{r['share_of_headline_rate']:11.3f}")
    for subject in subjects:
        by = {r["variant"]: r for r in records if r["subject"] == subject}
        for variant in ("host", "device"):
            slower_by = by[variant]["median_ms"] / by["baseline"]["median_ms"] - 1.0
            allowed = max(by[variant]["spread"], by["baseline"]["spread"])
            verdict = "holds" if slower_by <= allowed else "FAILS"
            lines.append(f"condition ({subject}, {variant}): {slower_by:+.3f} of the baseline's median against a spread of {allowed:.3f}: {verdict}")
    stats = evaluator.statevector_device.gradient_stats()
    lines.append(f"gradient scratch in device memory after the runs: {stats['scratch_bytes'] / 1e6:.1f} MB in {stats['n_allocations']} allocations; "
                 f"the last call ran {stats['n_chunks']} chunk(s)")
    if not args.no_profile:
        del evaluator
        kernels = profiled_kernel_times(args)
        lines.append(f"kernel times (rocprofv3 --kernel-trace --stats, a run of its own: {args.kernel_calls} calls each of the full and the "
                     "layer gradient through the host entry point):")
        for name, row in sorted(kernels.items()) if "error" not in kernels else []:
            lines.append(f"  {name:70s} calls {row['calls']:6d}  total {row['total_us']:12.1f} us  average {row['average_us']:10.2f} us  "
                         f"{row['share_percent']:6.2f} %")
        if "error" in kernels:
            lines.append(f"  not measured: {kernels['error']}")
        records.append({"kernels": kernels})
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(records))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
