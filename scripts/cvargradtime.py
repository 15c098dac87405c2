"""Time the exact CVaR gradient on one MI355X and write profiles/r30_cvar_gradient.txt.

  subject    StatevectorDevice.cvar_gradients (qsv_cvar_gradient_circuits): the adjoint sweep with the clipped
             seed, by every parameter and by the last layer's parameters alone, with values and thresholds
  against    StatevectorDevice.adjoint_gradients (qsv_adjoint_gradient_circuits) on the same inputs: the expectation value's
             gradient.  The difference is what the gathered threshold search costs (the seed pass stands where H psi stood);
             two StatevectorDevice.exact_cvar_batch evaluations of the same circuits: one SPSA iteration, the only way the CVaR was
             searched before;
             and the CVaR VALUE from StatevectorDevice.statevector() per circuit, then NumPy: the sorted order (taken once,
             outside the window), a cumulative sum and the clipped weights (no gradient existed on that route)

Workloads: the headline population (20 qubits, 64 individuals, four layers, the Ising operator, alpha = 0.5) and one 24-qubit
circuit of four layers.  All variants of a workload run in one process, interleaved: --warm rounds first (the first CVaR call also
sorts the operator's values), then --rounds timed rounds of one call each; a time is host wall time around a call that returns
its results, behind a synchronise.  The baseline moves gigabytes over PCIe and runs --baseline-rounds timed rounds.  Reported:
median, least and largest time per variant.  Every figure is what this run measured."""

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

from queasars_amd import workloads  # noqa: E402
from queasars_amd.circuit_evaluation import StatevectorDevice  # noqa: E402

WORKLOADS = ({"n": 20, "layers": 4, "circuits": 64}, {"n": 24, "layers": 4, "circuits": 1})
ALPHA = 0.5


def numpy_cvar(probabilities: np.ndarray, sorted_values: np.ndarray, order: np.ndarray, alpha: float) -> float:
    """The reference's accumulation on a whole distribution, with the sort taken out: up to the first state at which the gathered
    mass is within numpy.isclose of alpha, that state's mass clipped to what is missing."""
    p = probabilities[order]
    cum = np.cumsum(p)
    b = min(int(np.searchsorted(cum, alpha - (1e-8 + 1e-5 * alpha), side="left")), len(p) - 1)
    before = float(cum[b - 1]) if b else 0.0
    return float((np.dot(p[:b], sorted_values[:b]) + min(alpha - before, float(p[b])) * sorted_values[b]) / alpha)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--baseline-rounds", type=int, default=1)
    ap.add_argument("--workloads", type=int, nargs="*", default=list(range(len(WORKLOADS))), help="indices into WORKLOADS")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r30_cvar_gradient.txt")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("cvargradtime.py measures on a GPU: none found")
    import helpers

    c_oracle = helpers.load_c_oracle()
    lines = [f"exact CVaR gradient (alpha = {ALPHA}) against the plain adjoint gradient, two exact CVaR evaluations and statevector() + NumPy; "
             f"{args.warm} warm-up and {args.rounds} timed rounds per workload ({args.baseline_rounds} for the baseline), variants interleaved "
             "in one process, host wall time per call behind a synchronise",
             f"{'workload':28s} {'variant':36s} {'median ms':>11s} {'min ms':>11s} {'max ms':>11s}"]
    records = []
    for load in (WORKLOADS[i] for i in args.workloads):
        n, count = load["n"], load["circuits"]
        name = f"n={n} L={load['layers']} {count} circuit{'s' if count > 1 else ''}"
        op = workloads.random_ising_operator(n, seed=2020)
        table = c_oracle.diagonal_table(op)
        order = np.argsort(table, kind="stable")
        sorted_values = table[order]
        population, circuits, params = workloads.population_circuits(n, load["layers"], count, seed=0)
        last = [list(ind.layer_parameter_indices[len(ind.layers) - 1]) for ind in population.individuals]
        dev = StatevectorDevice(n)
        dev.set_operator(op)

        def baseline():
            values = np.zeros(count)
            for e, (c, p) in enumerate(zip(circuits, params)):
                psi = dev.statevector(c, p)
                values[e] = numpy_cvar(psi.real ** 2 + psi.imag ** 2, sorted_values, order, ALPHA)
            del psi
            torch.zeros(1, device="cuda").item()  # (the downloads are let go inside the baseline's own window)
            return values

        variants = {"cvar gradients, all parameters": lambda: dev.cvar_gradients(circuits, params, ALPHA, with_values=True, with_thresholds=True),
                    "plain adjoint, all parameters": lambda: dev.adjoint_gradients(circuits, params, return_values=True),
                    "cvar gradients, last layer": lambda: dev.cvar_gradients(circuits, params, ALPHA, last, with_values=True),
                    "plain adjoint, last layer": lambda: dev.adjoint_gradients(circuits, params, last, return_values=True),
                    "cvar value-only call": lambda: dev.cvar_gradients(circuits, params, ALPHA, [], with_values=True),
                    "two exact_cvar_batch (one SPSA step)": lambda: (dev.exact_cvar_batch(circuits, params, ALPHA), dev.exact_cvar_batch(circuits, params, ALPHA)),
                    "statevector+numpy (value)": baseline}
        times = {v: [] for v in variants}
        results = {}
        for rnd in range(args.warm + args.rounds):
            for v, call in variants.items():  # (interleaved: every round runs each variant once)
                if v.startswith("statevector") and not args.warm <= rnd < args.warm + args.baseline_rounds:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results[v] = call()
                torch.cuda.synchronize()
                seconds = time.perf_counter() - t0
                if rnd >= args.warm:
                    times[v].append(seconds)
        values = np.asarray(results["cvar gradients, all parameters"][1])
        thresholds = np.asarray(results["cvar gradients, all parameters"][2])
        weight_norm = float(np.max(thresholds - sorted_values[0]) / ALPHA)
        bound = 1e-10 * max(1.0, weight_norm)
        err_exact = float(np.abs(values - np.asarray(results["two exact_cvar_batch (one SPSA step)"][0])).max())
        err_numpy = float(np.abs(values - results["statevector+numpy (value)"]).max())
        if err_exact > bound or err_numpy > bound:
            raise SystemExit(f"{name}: the values disagree (exact_cvar_batch {err_exact:.3e}, NumPy {err_numpy:.3e}, bound {bound:.3e})")
        for v, t in times.items():
            med = float(np.median(t))
            records.append({"workload": name, "variant": v, "median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3, "rounds": len(t)})
            lines.append(f"{name:28s} {v:36s} {med * 1e3:11.3f} {min(t) * 1e3:11.3f} {max(t) * 1e3:11.3f}")
            print(lines[-1], flush=True)
        med = {v: float(np.median(t)) * 1e3 for v, t in times.items()}
        search_all = med["cvar gradients, all parameters"] - med["plain adjoint, all parameters"]
        search_last = med["cvar gradients, last layer"] - med["plain adjoint, last layer"]
        stats = dev.adjoint_stats()
        records.append({"workload": name, "search_over_plain_all_ms": search_all, "search_over_plain_last_ms": search_last,
                        "value_against_exact_cvar": err_exact, "value_against_numpy": err_numpy, "weight_norm": weight_norm,
                        "scratch_bytes": stats["scratch_bytes"]})
        parts = {"the sweep (what the plain adjoint call costs)": med["plain adjoint, all parameters"], "the gathered threshold search": search_all}
        lines.append(f"{name:28s} CVaR over plain adjoint: all parameters {search_all:+.3f} ms, last layer {search_last:+.3f} ms (the gathered threshold "
                     f"search; the seed pass stands where H psi stood); of the all-parameter call the larger part is {max(parts, key=parts.get)}; "
                     f"largest |dCVaR| to exact_cvar_batch {err_exact:.2e}, to NumPy {err_numpy:.2e} (|w|_inf = {weight_norm:.1f}); adjoint scratch "
                     f"{stats['scratch_bytes'] / 2**20:.0f} MiB")
        print(lines[-1], flush=True)
        dev.close()
        del dev
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(records))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
