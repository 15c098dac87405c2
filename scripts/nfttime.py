"""Time one last-layer NFT search of the headline population -- n = 20, 64 individuals, four layers, the 210-term Ising
operator, fp64, ``NFT(maxfev=40)``: 20 iterations, 41 evaluations per run -- on one MI355X and write profiles/r09_nft_search.txt.

  evaluators  estimator   OperatorCircuitEvaluator (exact expectation values)
              sampler     OperatorSamplerCircuitEvaluator, 1024 shots, alpha = 0.5 (CVaR)
  variants    host        the solver's last-layer search with device_resident_search=False: the generic lock-step loop of
                          ``_minimize_batched`` (propose / accept per run in Python, one evaluate_circuits call per iteration) --
                          the only path an NFT search had before, and the yardstick
              device      the same search with device_resident_search=True: evqe/device_search.minimize_nft_on_device
                          (qsv_nft_step + evaluate_device_to_device per iteration, nothing waited for inside the search)

Both variants run through ``EVQEMinimumEigensolver._last_layer_search`` in ONE process per evaluator, interleaved: --warm rounds
first, then --rounds rounds of one search each; a time is host wall time around a search that ends with its results on the host.
For the device variant the time between two HIP events on the evaluator's stream, recorded right before and right after the
search, is reported too: what the device spent from the search's first operation to its last (idle gaps while the host queues
included, so an upper bound of its busy time).  Reported: median, minimum, maximum and the spread (max - min) / median per
variant, and the ratio of medians.  The claim checked: the device search is not slower than the host driver beyond the spread.

Each evaluator is measured by a child process of its own under ``timeout``; the second starts only if the first ended well.
Every figure is what this run measured; nothing is estimated."""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

KINDS = ("estimator", "sampler")


def measure(args, kind: str) -> dict:
    import torch

    from queasars_amd import workloads
    from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, OperatorSamplerCircuitEvaluator
    from queasars_amd.distributed import _chain_state
    from queasars_amd.evqe import EVQEPopulation, device_search
    from queasars_amd.evqe.solver import NFT, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    if not torch.cuda.is_available():
        raise SystemExit("nfttime.py measures on a GPU: none found")
    op = workloads.random_ising_operator(args.n, seed=0)
    if kind == "estimator":
        evaluator = OperatorCircuitEvaluator(op)
    else:
        evaluator = OperatorSamplerCircuitEvaluator(args.shots, op, alpha=args.alpha, seed=0)
    population = EVQEPopulation.random_population(args.n, args.layers, args.individuals, True, 0)
    optimizer = NFT(maxfev=args.maxfev)
    schedule, per_run = device_search.nft_schedule(optimizer)

    def solver(flag):
        return EVQEMinimumEigensolver(EVQEMinimumEigensolverConfiguration(
            optimizer=optimizer, population_size=args.individuals, max_generations=1, random_seed=0, n_initial_layers=args.layers,
            device_resident_search=flag))

    solvers = {"host": solver(False), "device": solver(True)}
    entered = []
    inner = device_search.minimize_nft_on_device

    def counting(ev, jobs, *a, **k):
        entered.append(len(jobs))
        return inner(ev, jobs, *a, **k)

    device_search.minimize_nft_on_device = counting
    stream = _chain_state(evaluator, torch.device("cuda", evaluator.statevector_device.device_index))["stream"]
    times = {"host": [], "device": []}
    between_events = []
    for rnd in range(args.warm + args.rounds):
        for variant, s in solvers.items():  # (interleaved: every round runs each variant once)
            torch.cuda.synchronize()
            before = len(entered)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            if variant == "device":
                start.record(stream)
            _, nfev = s._last_layer_search(evaluator, population)
            if variant == "device":
                end.record(stream)
            seconds = time.perf_counter() - t0
            torch.cuda.synchronize()
            if nfev != args.individuals * per_run:
                raise SystemExit(f"{kind} {variant}: {nfev} evaluations, the schedule says {args.individuals * per_run}")
            if (len(entered) - before) != (1 if variant == "device" else 0):
                raise SystemExit(f"{kind} {variant}: the search did not take the path it is timed as")
            if rnd >= args.warm:
                times[variant].append(seconds)
                if variant == "device":
                    between_events.append(start.elapsed_time(end) * 1e-3)
    out = {"kind": kind, "iterations": len(schedule), "evaluations_per_run": per_run, "rounds": args.rounds}
    for variant, t in list(times.items()) + [("device, between events", between_events)]:
        med = float(np.median(t))
        out[variant] = {"median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3, "spread": (max(t) - min(t)) / med}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--individuals", type=int, default=64)
    ap.add_argument("--maxfev", type=int, default=40)
    ap.add_argument("--shots", type=int, default=1024)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each evaluator's child process may take")
    ap.add_argument("--child", choices=KINDS, help="(one evaluator's measurement, as JSON on the last line)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r09_nft_search.txt")
    args = ap.parse_args()
    if args.rounds < 9:
        raise SystemExit("at least nine timed rounds")
    if args.child:
        print(json.dumps(measure(args, args.child)))
        return

    passed = [f"--{name.replace('_', '-')}={getattr(args, name)}" for name in ("n", "layers", "individuals", "maxfev", "shots", "alpha",
                                                                             "rounds", "warm")]
    results = []
    for kind in KINDS:  # (each under its own time limit; nothing more is started after one that did not end well)
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, str(Path(__file__).resolve()), "--child", kind] + passed
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            raise SystemExit(f"the {kind} measurement ended with status {res.returncode}; nothing further was started\n{res.stdout[-2000:]}")
        results.append(json.loads(res.stdout.strip().splitlines()[-1]))

    lines = [f"one last-layer NFT(maxfev={args.maxfev}) search, n = {args.n}, {args.individuals} individuals, {args.layers} layers, "
             f"210-term Ising operator, fp64: {results[0]['iterations']} iterations, {results[0]['evaluations_per_run']} evaluations per run; "
             f"{args.warm} warm-up and {args.rounds} timed rounds, variants interleaved in one process per evaluator",
             f"sampler: {args.shots} shots, alpha = {args.alpha}",
             f"{'evaluator':10s} {'variant':23s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'spread':>7s} {'vs host':>8s}"]
    for r in results:
        for variant in ("host", "device", "device, between events"):
            row = r[variant]
            lines.append(f"{r['kind']:10s} {variant:23s} {row['median_ms']:10.3f} {row['min_ms']:9.3f} {row['max_ms']:9.3f} "
                         f"{row['spread']:7.3f} {row['median_ms'] / r['host']['median_ms']:8.3f}")
    for r in results:
        slower_by = r["device"]["median_ms"] / r["host"]["median_ms"] - 1.0
        allowed = max(r["device"]["spread"], r["host"]["spread"])
        verdict = "holds" if slower_by <= allowed else "FAILS"
        lines.append(f"claim ({r['kind']}): the device search takes {slower_by:+.3f} of the host driver's median against a spread of "
                     f"{allowed:.3f}: not slower {verdict}")
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(results))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
