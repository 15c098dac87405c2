"""Time one last-layer Adam search of the headline population -- n = 20, 64 individuals, four layers, the 210-term Ising
operator, fp64, ``Adam(maxiter=33, tol=0)``: 33 iterations, each the parameter-shift gradient of every individual's last layer --
on one MI355X and write profiles/r10_adam_search.txt.

  variants    host        the solver's last-layer search with device_resident_search=False: ``solver._minimize_adam`` (per
                          iteration Python lists of the points, one ``evaluate_gradients`` call -- upload, shift tables, the
                          chunk, a wait, the download -- and ``_AdamRun.accept_gradient`` per run in NumPy): the yardstick
              device      the same search with device_resident_search=True: evqe/device_search.minimize_adam_on_device (one
                          gradient plan, then per iteration one run of it and one ``qsv_adam_step`` launch, nothing waited for;
                          ``x``, the moments and the counts read once at the end)

Both variants search the individuals' shared, fully parameterised circuits (``QSV_SHARE_CIRCUITS=2`` makes the host variant embed
its runs as the device variant does: registered once, the same circuits and shift tables), so the two differ in the driver alone.
Both run through ``EVQEMinimumEigensolver._last_layer_search`` in ONE process, interleaved: --warm rounds first, then
--rounds rounds of one search each; a time is host wall time around a search that ends with its results on the host.  For the
device variant the time between two HIP events on the evaluator's stream, recorded right before and right after the search, is
reported too (idle gaps while the host queues included: an upper bound of the device's busy time), and the plan's counters: its
runs, the host waits inside its first run and inside all the runs after it.  Reported: median, minimum, maximum and the spread
(max - min) / median per variant, and the ratio of medians.  No ratio is claimed in advance.

The measurement is a child process under ``timeout``.  Every figure is what this run measured; nothing is estimated."""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def measure(args) -> dict:
    import torch

    from queasars_amd import workloads
    from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator
    from queasars_amd.circuit_evaluation.circuit_evaluation import DeviceGradientPlan
    from queasars_amd.distributed import _chain_state
    from queasars_amd.evqe import EVQEPopulation, device_search
    from queasars_amd.evqe.solver import Adam, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    if not torch.cuda.is_available():
        raise SystemExit("adamtime.py measures on a GPU: none found")
    os.environ["QSV_SHARE_CIRCUITS"] = "2"
    evaluator = OperatorCircuitEvaluator(workloads.random_ising_operator(args.n, seed=0))
    population = EVQEPopulation.random_population(args.n, args.layers, args.individuals, True, 0)
    optimizer = Adam(maxiter=args.maxiter, tol=0.0)

    def solver(flag):
        return EVQEMinimumEigensolver(EVQEMinimumEigensolverConfiguration(
            optimizer=optimizer, population_size=args.individuals, max_generations=1, random_seed=0, n_initial_layers=args.layers,
            device_resident_search=flag))

    solvers = {"host": solver(False), "device": solver(True)}
    entered, plans = [], []
    inner = device_search.minimize_adam_on_device

    def counting(ev, jobs, *a, **k):
        entered.append(len(jobs))
        return inner(ev, jobs, *a, **k)

    device_search.minimize_adam_on_device = counting
    # a plan's counters after its first run and right before it is closed
    inner_run, inner_close = DeviceGradientPlan.run, DeviceGradientPlan.close

    def noting_run(self, *a, **k):
        out = inner_run(self, *a, **k)
        if not hasattr(self, "_first"):
            self._first = self.stats()
        return out

    def noting_close(self):
        if getattr(self, "_id", -1) >= 0 and hasattr(self, "_first"):
            plans.append((self._first, self.stats()))
        inner_close(self)

    DeviceGradientPlan.run, DeviceGradientPlan.close = noting_run, noting_close
    stream = _chain_state(evaluator, torch.device("cuda", evaluator.statevector_device.device_index))["stream"]
    times = {"host": [], "device": []}
    between_events, evaluations = [], {}
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
            if evaluations.setdefault("nfev", nfev) != nfev:
                raise SystemExit(f"{variant}: {nfev} evaluations, the other variant made {evaluations['nfev']}")
            if (len(entered) - before) != (1 if variant == "device" else 0):
                raise SystemExit(f"{variant}: the search did not take the path it is timed as")
            if rnd >= args.warm:
                times[variant].append(seconds)
                if variant == "device":
                    between_events.append(start.elapsed_time(end) * 1e-3)
    timed = plans[args.warm:]
    out = {"iterations": args.maxiter, "evaluations_per_search": evaluations["nfev"], "rounds": args.rounds,
           "shifted_per_iteration": timed[0][1]["n_shifted"], "chunks_per_iteration": timed[0][1]["n_chunks"],
           "plan_runs": sorted({last["n_runs"] for _, last in timed}),
           "host_waits_first_run": sorted({first["n_host_waits"] for first, _ in timed}),
           "host_waits_later_runs": sorted({last["n_host_waits"] - first["n_host_waits"] for first, last in timed})}
    for variant, t in list(times.items()) + [("device, between events", between_events)]:
        med = float(np.median(t))
        out[variant] = {"median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3, "spread": (max(t) - min(t)) / med}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--individuals", type=int, default=64)
    ap.add_argument("--maxiter", type=int, default=33)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help="(the measurement itself, as JSON on the last line)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r10_adam_search.txt")
    args = ap.parse_args()
    if args.rounds < 9:
        raise SystemExit("at least nine timed rounds")
    if args.child:
        print(json.dumps(measure(args)))
        return

    passed = [f"--{name}={getattr(args, name)}" for name in ("n", "layers", "individuals", "maxiter", "rounds", "warm")]
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, str(Path(__file__).resolve()), "--child"] + passed
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if res.returncode != 0:
        raise SystemExit(f"the measurement ended with status {res.returncode}\n{res.stdout[-2000:]}")
    r = json.loads(res.stdout.strip().splitlines()[-1])

    lines = [f"one last-layer Adam(maxiter={args.maxiter}, tol=0) search, n = {args.n}, {args.individuals} individuals, {args.layers} layers, "
             f"210-term Ising operator, fp64: {r['iterations']} iterations of {r['shifted_per_iteration']} shifted evaluations in "
             f"{r['chunks_per_iteration']} chunk(s), {r['evaluations_per_search']} evaluations per search; "
             f"{args.warm} warm-up and {args.rounds} timed rounds, variants interleaved in one process",
             f"{'variant':23s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'spread':>7s} {'vs host':>8s}"]
    for variant in ("host", "device", "device, between events"):
        row = r[variant]
        lines.append(f"{variant:23s} {row['median_ms']:10.3f} {row['min_ms']:9.3f} {row['max_ms']:9.3f} {row['spread']:7.3f} "
                     f"{row['median_ms'] / r['host']['median_ms']:8.3f}")
    lines.append(f"per iteration: host {r['host']['median_ms'] / r['iterations']:.3f} ms, device {r['device']['median_ms'] / r['iterations']:.3f} ms, "
                 f"device between events {r['device, between events']['median_ms'] / r['iterations']:.3f} ms")
    lines.append(f"the plan of a timed device search: runs {r['plan_runs']}, n_host_waits inside the first run {r['host_waits_first_run']}, "
                 f"inside all later runs together {r['host_waits_later_runs']} (sets over the {args.rounds} timed searches)")
    gain = 1.0 - r["device"]["median_ms"] / r["host"]["median_ms"]
    spread = max(r["device"]["spread"], r["host"]["spread"])
    lines.append(f"the device search takes {-gain:+.3f} of the host driver's median against a spread of {spread:.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(r))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
