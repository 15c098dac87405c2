"""Time the BitstringCircuitEvaluator on the headline population -- n = 20, 64 individuals, four layers -- with 1024 shots and
alpha = 0.5 on one MI355X, with and without its device-resident value cache, and write profiles/r08_bitstring_cache.txt.

  callables  ones      b.count("1")
             makespan  a job-shop instance whose domain-wall encoding has n qubits (job_shop_scheduling.py): the bitstring is
                       translated into a schedule; a valid one scores its makespan, an invalid one the makespan limit plus its
                       number of unscheduled operations
  modes      default   device_value_cache=False: samples to the host, np.unique per circuit, every distinct state of every
                       circuit scored, CVaR in NumPy (the path before the cache existed; still the default)
             cache     device_value_cache=True
  cases      cold      the first call of a new evaluator (an empty cache)
             warm      the same seed again on the same evaluator (the evaluator's generator put back): every sample is a hit
             search    a 33-iteration SPSA search of every individual's last layer through the host driver
                       (solver._minimize_batched(..., on_device=False)), a new evaluator per search

Both modes run in ONE process on one StatevectorDevice, interleaved round by round; a time is host wall time around a call that
returns its results.  Reported per case and mode: median, minimum, maximum, spread (max - min) / median, the ratio of medians, the
callable's invocations per call (or per search), and the largest difference between the two modes' results (their CVaR sums
associate differently).  The four cache kernels' shares come from a `rocprofv3 --kernel-trace --stats` run of its own: a fresh
child process (`--kernels`) that only makes cached calls.  Every figure is what this run measured."""

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

from queasars_amd import job_shop_scheduling as jssp  # noqa: E402
from queasars_amd.circuit_evaluation import BitstringCircuitEvaluator, BitstringEvaluator, StatevectorDevice  # noqa: E402
from queasars_amd.evqe import EVQEPopulation  # noqa: E402
from queasars_amd.evqe import solver as S  # noqa: E402


class Counted:
    def __init__(self, function):
        self.function = function
        self.calls = 0

    def __call__(self, bitstring: str) -> float:
        self.calls += 1
        return self.function(bitstring)


def makespan_callable(n: int):
    """A random job-shop instance and makespan limit whose encoding has exactly n qubits, and its scoring function."""
    for seed in range(200):
        for n_jobs, n_machines in ((2, 2), (2, 3), (3, 2), (3, 3)):
            instance = jssp.random_job_shop_scheduling_instance("timing", n_jobs, n_machines, 1.0, {1: 0.5, 2: 0.5}, random_seed=seed)
            longest = max(sum(op.processing_duration for op in job.operations) for job in instance.jobs)
            for limit in range(longest, longest + 12):
                encoder = jssp.JSSPDomainWallHamiltonianEncoder(instance, limit)
                if encoder.n_qubits == n:
                    n_ops = sum(len(job.operations) for job in instance.jobs)

                    def score(bitstring: str, encoder=encoder, limit=limit) -> float:
                        result = encoder.translate_result_bitstring(bitstring)
                        if result.is_valid:
                            return float(result.makespan)
                        unscheduled = sum(1 for ops in result.schedule.values() for op in ops if not op.is_scheduled)
                        return float(limit + 1 + unscheduled)

                    return score, f"{n_jobs} jobs x {n_machines} machines (seed {seed}), {n_ops} operations, makespan limit {limit}"
                if encoder.n_qubits > n:
                    break
    raise SystemExit(f"no job-shop instance with a {n}-qubit encoding found")


def workload(args):
    pop = EVQEPopulation.random_population(args.n, args.layers, args.individuals, True, 0)
    circuits = [ind.get_parameterized_quantum_circuit() for ind in pop.individuals]
    params = [list(ind.parameter_values) for ind in pop.individuals]
    return pop, circuits, params


def kernels_only(args) -> None:
    """The child of the profiled run: cached calls only -- a cold one, the same seed again, further seeds."""
    import torch

    _, circuits, params = workload(args)
    ev = BitstringCircuitEvaluator(args.shots, BitstringEvaluator(args.n, lambda b: float(b.count("1"))), alpha=args.alpha, seed=0,
                                   device_value_cache=True)
    ev.evaluate_circuits(circuits, params)
    for _ in range(args.kernel_calls):
        ev._rng = np.random.default_rng(0)
        ev.evaluate_circuits(circuits, params)
    for _ in range(args.kernel_calls):
        ev.evaluate_circuits(circuits, params)
    torch.cuda.synchronize()
    print(json.dumps(ev.value_cache_stats))


def profiled_kernel_times(args) -> dict:
    rocprof = shutil.which("rocprofv3")
    if rocprof is None:
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory(dir=args.out.parent) as tmp:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, str(Path(__file__).resolve()),
               "--kernels", "--n", str(args.n), "--layers", str(args.layers), "--individuals", str(args.individuals),
               "--shots", str(args.shots), "--alpha", str(args.alpha), "--kernel-calls", str(args.kernel_calls)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.kernel_timeout)
        if res.returncode != 0:
            return {"error": f"rocprofv3 run failed ({res.returncode}): {res.stdout[-400:]}"}
        rows = {}
        try:
            for path in Path(tmp).rglob("*kernel_stats.csv"):
                with path.open() as f:
                    for row in csv.DictReader(f):
                        name = row.get("Name", "").replace("(anonymous namespace)::", "").split("(")[0][-60:]
                        rows[name] = {"calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3,
                                      "average_us": float(row["AverageNs"]) / 1e3, "share_percent": float(row.get("Percentage", "nan"))}
        except (KeyError, ValueError) as exc:
            return {"error": f"unexpected kernel statistics layout: {exc!r}"}
        return rows or {"error": "no kernel statistics found in " + ", ".join(p.name for p in Path(tmp).rglob("*"))[:300]}


def summarise(times):
    med = float(np.median(times))
    return {"median_ms": med * 1e3, "min_ms": min(times) * 1e3, "max_ms": max(times) * 1e3, "spread": (max(times) - min(times)) / med,
            "rounds": len(times)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--individuals", type=int, default=64)
    ap.add_argument("--shots", type=int, default=1024)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--search-rounds", type=int, default=3)
    ap.add_argument("--slow-search-rounds", type=int, default=1, help="searches per mode with the makespan callable")
    ap.add_argument("--callables", default="ones,makespan")
    ap.add_argument("--kernels", action="store_true", help="(the profiled child: cached calls only)")
    ap.add_argument("--kernel-calls", type=int, default=5)
    ap.add_argument("--kernel-timeout", type=int, default=300)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r08_bitstring_cache.txt")
    args = ap.parse_args()
    if args.kernels:
        kernels_only(args)
        return

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bitstringtime.py measures on a GPU: none found")
    pop, circuits, params = workload(args)
    makespan, instance_text = makespan_callable(args.n)
    functions = {"ones": lambda b: float(b.count("1")), "makespan": makespan}
    dev = StatevectorDevice(args.n)
    cfg = S.SPSA(termination_checker=S.SPSATerminationChecker(0.01, 2))  # (33 iterations, the notebooks' gains)
    modes = (("default", False), ("cache", True))

    def evaluator(counted, flag):
        return BitstringCircuitEvaluator(args.shots, BitstringEvaluator(args.n, counted), alpha=args.alpha, seed=0, statevector_device=dev,
                                         device_value_cache=flag)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        return time.perf_counter() - t0, out

    records = []
    for name in args.callables.split(","):
        counted = Counted(functions[name])
        # cold: a new evaluator per round and mode
        times = {m: [] for m, _ in modes}
        calls, results = {}, {}
        for rnd in range(args.warm + args.rounds):
            for mode, flag in modes:
                ev = evaluator(counted, flag)
                counted.calls = 0
                seconds, results[mode] = timed(lambda: ev.evaluate_circuits(circuits, params))
                calls[mode] = counted.calls
                if rnd >= args.warm:
                    times[mode].append(seconds)
        difference = float(np.abs(np.asarray(results["default"]) - np.asarray(results["cache"])).max())
        for mode, _ in modes:
            records.append({"callable": name, "case": "cold", "mode": mode, "invocations": calls[mode], "max_difference": difference,
                            **summarise(times[mode])})
        # warm: the same seed again on evaluators that have seen it
        kept = {mode: evaluator(counted, flag) for mode, flag in modes}
        for ev in kept.values():
            ev.evaluate_circuits(circuits, params)
        times = {m: [] for m, _ in modes}
        for rnd in range(args.warm + args.rounds):
            for mode, _ in modes:
                kept[mode]._rng = np.random.default_rng(0)
                counted.calls = 0
                seconds, results[mode] = timed(lambda: kept[mode].evaluate_circuits(circuits, params))
                calls[mode] = counted.calls
                if rnd >= args.warm:
                    times[mode].append(seconds)
        difference = float(np.abs(np.asarray(results["default"]) - np.asarray(results["cache"])).max())
        for mode, _ in modes:
            records.append({"callable": name, "case": "warm", "mode": mode, "invocations": calls[mode], "max_difference": difference,
                            **summarise(times[mode])})
        stats = kept["cache"].value_cache_stats
        del kept
        # search: 33 SPSA iterations over every individual's last layer, host driver, a new evaluator per search
        rounds = args.search_rounds if name == "ones" else args.slow_search_rounds
        times = {m: [] for m, _ in modes}
        checksum, search_stats = {}, None
        for rnd in range(rounds):
            for mode, flag in modes:
                ev = evaluator(counted, flag)
                batch = [(ind.get_partially_parameterized_quantum_circuit({-1}), cfg.new_run(ind.get_layer_parameter_values(-1), seed=k))
                         for k, ind in enumerate(pop.individuals)]
                counted.calls = 0
                seconds, _ = timed(lambda: S._minimize_batched(ev, batch, on_device=False))
                calls[mode] = counted.calls
                times[mode].append(seconds)
                checksum[mode] = float(sum(float(np.sum(run.x)) for _, run in batch))
                if flag:
                    search_stats = ev.value_cache_stats
        for mode, _ in modes:
            if times[mode]:
                records.append({"callable": name, "case": "search", "mode": mode, "invocations": calls[mode],
                                "max_difference": abs(checksum["default"] - checksum["cache"]), **summarise(times[mode])})
        records.append({"callable": name, "cache_after_warm_calls": stats, "cache_after_a_search": search_stats})

    lines = [f"BitstringCircuitEvaluator, n = {args.n}, {args.individuals} individuals, {args.layers} layers, {args.shots} shots, alpha = {args.alpha}; "
             f"{args.warm} warm-up and {args.rounds} timed rounds per call case, modes interleaved in one process on one device",
             f"makespan callable: {instance_text}",
             f"{'callable':9s} {'case':7s} {'mode':8s} {'rounds':>6s} {'median ms':>11s} {'min ms':>11s} {'max ms':>11s} {'spread':>7s} "
             f"{'vs default':>10s} {'invocations':>11s} {'max |difference|':>17s}"]
    timed_records = [r for r in records if "case" in r]
    for r in timed_records:
        base = next(b for b in timed_records if b["callable"] == r["callable"] and b["case"] == r["case"] and b["mode"] == "default")
        r["ratio_to_default"] = r["median_ms"] / base["median_ms"]
        lines.append(f"{r['callable']:9s} {r['case']:7s} {r['mode']:8s} {r['rounds']:6d} {r['median_ms']:11.3f} {r['min_ms']:11.3f} "
                     f"{r['max_ms']:11.3f} {r['spread']:7.3f} {r['ratio_to_default']:10.4f} {r['invocations']:11d} {r['max_difference']:17.3e}")
    lines.append("(search rows: invocations per search; the last column is the difference of the two modes' summed final points -- the "
                 "CVaR sums associate differently, so two searches may part ways)")
    for r in timed_records:
        if r["case"] == "warm" and r["mode"] == "cache":
            base = next(b for b in timed_records if b["callable"] == r["callable"] and b["case"] == "warm" and b["mode"] == "default")
            slower_by = r["median_ms"] / base["median_ms"] - 1.0
            lines.append(f"condition (warm, {r['callable']}): the cache path is {slower_by:+.3f} of the default path's median: "
                         f"{'holds' if slower_by <= 0 else 'FAILS'}")
    for r in records:
        if "cache_after_warm_calls" in r:
            lines.append(f"cache counters ({r['callable']}): after the warm calls {r['cache_after_warm_calls']}; after a search {r['cache_after_a_search']}")
    if not args.no_profile:
        del dev
        kernels = profiled_kernel_times(args)
        lines.append(f"kernel times (rocprofv3 --kernel-trace --stats, a run of its own: one cold call, {args.kernel_calls} calls with the same seed, "
                     f"{args.kernel_calls} with further seeds, callable ones):")
        for name, row in sorted(kernels.items(), key=lambda kv: -kv[1]["total_us"]) if "error" not in kernels else []:
            lines.append(f"  {name:60s} calls {row['calls']:6d}  total {row['total_us']:12.1f} us  average {row['average_us']:10.2f} us  "
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
