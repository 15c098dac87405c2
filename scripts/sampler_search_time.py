"""Time one last-layer SPSA search of the benchmark population on the sampler (CVaR) branch -- n = 20, 64 individuals, four
layers, alpha 0.5, 33 iterations with the reference's termination checker as the notebooks configure it (runs stop at different
iterations) -- with 1024 shots and with the exact distribution (sampler_shots=None), through

  host         the host driver (solver._minimize_spsa_vectorised: points packed on the host, two waits per iteration)
  device       evqe/device_search.py on OperatorSamplerCircuitEvaluator.evaluate_device_to_device, the mask not handed over
  device+mask  the same with the runs' active flags handed to the evaluator (stopped runs cost a dispatch)

Every time is host wall time around a search that ends with its results on the host, one process, after --warm searches of
the same mode; --reps searches per mode, each from the same seeds (the evaluator's generator is reset), reported as median,
minimum and maximum.  On a checkout whose sampler evaluator has no evaluate_device_to_device only `host` is timed -- the
baseline for "the host path did not get slower".  Prints one JSON line per (shots, mode) and appends them to --out."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from queasars_amd import workloads  # noqa: E402
from queasars_amd.circuit_evaluation import OperatorSamplerCircuitEvaluator  # noqa: E402
from queasars_amd.evqe import EVQEPopulation  # noqa: E402
from queasars_amd.evqe import solver as S  # noqa: E402
from queasars_amd.ir import PauliOperator  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--individuals", type=int, default=64)
    ap.add_argument("--shots", type=int, default=1024)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--modes", default="host,device,device+mask")
    ap.add_argument("--only-shots", choices=("sampled", "exact"))
    ap.add_argument("--offset", type=float, default=0.0,
                    help="an identity term of this share of sum |c| added to the operator (the reference's termination rule divides "
                         "by the previous value: below zero -- the benchmark's Ising operator at alpha 0.5 -- it is met as soon as "
                         "its window is full; 0.3 lifts the CVaR above zero and the runs stop anywhere up to the last iteration)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", type=Path)
    args = ap.parse_args()

    import torch

    pop = EVQEPopulation.random_population(args.n, args.layers, args.individuals, True, 0)
    op = workloads.random_ising_operator(args.n, seed=2020)
    if args.offset:
        op = PauliOperator(list(op.labels) + ["I" * args.n], list(op.coeffs) + [args.offset * float(np.abs(op.coeffs).sum())])
    cfg = S.SPSA(termination_checker=S.SPSATerminationChecker(0.01, 2))  # (33 iterations, the notebooks' gains)

    def jobs():
        return [(ind.get_partially_parameterized_quantum_circuit({-1}), cfg.new_run(ind.get_layer_parameter_values(-1), seed=k))
                for k, ind in enumerate(pop.individuals)]

    lines = []
    for shots in (args.shots, None):
        if args.only_shots and (args.only_shots == "sampled") != (shots is not None):
            continue
        ev = OperatorSamplerCircuitEvaluator(shots, op, alpha=args.alpha, seed=0)
        on_device_possible = hasattr(ev, "evaluate_device_to_device")
        for mode in args.modes.split(","):
            if mode != "host" and not on_device_possible:
                continue
            os.environ.pop("QSV_DEVICE_SEARCH_MASK", None)
            if mode == "device":
                os.environ["QSV_DEVICE_SEARCH_MASK"] = "0"
            times, last = [], None
            for rep in range(args.warm + args.reps):
                ev._rng = np.random.default_rng(0)  # (every search draws the same seeds)
                batch = jobs()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S._minimize_batched(ev, batch, on_device=mode != "host")
                torch.cuda.synchronize()
                if rep >= args.warm:
                    times.append(time.perf_counter() - t0)
                last = batch
            iterations = [run.iteration for _, run in last]
            record = {"label": args.label, "mode": mode, "shots": shots, "n": args.n, "individuals": args.individuals,
                      "layers": args.layers, "alpha": args.alpha, "offset": args.offset, "reps": args.reps,
                      "median_ms": float(np.median(times)) * 1e3, "min_ms": min(times) * 1e3, "max_ms": max(times) * 1e3,
                      "all_ms": [round(t * 1e3, 3) for t in times],
                      "evaluations_used": int(sum(run.nfev for _, run in last)),
                      "stopping_iterations": {"min": min(iterations), "median": float(np.median(iterations)), "max": max(iterations)},
                      "x_checksum": float(sum(float(np.sum(run.x)) for _, run in last))}
            line = json.dumps(record)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        with args.out.open("a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
