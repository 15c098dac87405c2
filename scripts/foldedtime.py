"""Time the folded-spectrum and variance costs on one MI355X and write profiles/r31_folded_spectrum.txt.

  subject    StatevectorDevice.folded_gradients (qsv_folded_gradient_circuits) in mode *mean* (the variance): by
             every parameter and by the last layer's parameters alone, with costs and energies; and its value-only call
  against    StatevectorDevice.adjoint_gradients (qsv_adjoint_gradient_circuits) on the same inputs: the expectation value's
             gradient.  The difference is what the centre, the residual pass and the seed pass cost (an operator of its diagonal
             part alone: one fused pass);
             StatevectorDevice.variances (qsv_variance_circuits) against the value-only call;
             and the cost from StatevectorDevice.statevector() per circuit, then H applied twice in NumPy (a diagonal operator:
             its table, taken once outside the window; a general one: string by string) -- no gradient existed on that route

Workloads: the headline population (20 qubits, 64 individuals, four layers, the Ising operator), one 20-qubit circuit of four
layers under the 500-string general operator, and one 24-qubit circuit of four layers under the Ising operator.  All variants of
a workload run in one process, interleaved: --warm rounds first, then --rounds timed rounds of one call each; a time is host wall
time around a call that returns its results, behind a synchronise.  The baseline moves the states over PCIe and runs
--baseline-rounds timed rounds.  Reported: median, least and largest time per variant, what the extra passes cost over the plain
adjoint call, and their bytes over that time against the 8 TB/s of DESIGN.md 7.  Every figure is what this run measured."""

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

WORKLOADS = ({"n": 20, "layers": 4, "circuits": 64, "operator": "ising"}, {"n": 20, "layers": 4, "circuits": 1, "operator": "pauli500"},
             {"n": 24, "layers": 4, "circuits": 1, "operator": "ising"})
HBM_BYTES_PER_SECOND = 8e12


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--baseline-rounds", type=int, default=1)
    ap.add_argument("--workloads", type=int, nargs="*", default=list(range(len(WORKLOADS))), help="indices into WORKLOADS")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r31_folded_spectrum.txt")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("foldedtime.py measures on a GPU: none found")
    import helpers
    import variance_reference

    c_oracle = helpers.load_c_oracle()
    lines = ["folded-spectrum costs (mode mean: the variance) against the plain adjoint gradient, qsv_variance_circuits and statevector() + NumPy; "
             f"{args.warm} warm-up and {args.rounds} timed rounds per workload ({args.baseline_rounds} for the baseline), variants interleaved "
             "in one process, host wall time per call behind a synchronise",
             f"{'workload':34s} {'variant':36s} {'median ms':>11s} {'min ms':>11s} {'max ms':>11s}"]
    records = []
    for load in (WORKLOADS[i] for i in args.workloads):
        n, count, diagonal = load["n"], load["circuits"], load["operator"] == "ising"
        name = f"n={n} L={load['layers']} {count} circuit{'s' if count > 1 else ''} {load['operator']}"
        op = workloads.random_ising_operator(n, seed=2020) if diagonal else workloads.random_pauli_operator(n, 500, seed=7)
        table = c_oracle.diagonal_table(op) if diagonal else None
        population, circuits, params = workloads.population_circuits(n, load["layers"], count, seed=0)
        last = [list(ind.layer_parameter_indices[len(ind.layers) - 1]) for ind in population.individuals]
        dev = StatevectorDevice(n)
        dev.set_operator(op)

        def baseline():
            values = np.zeros(count)
            for e, (c, p) in enumerate(zip(circuits, params)):
                psi = dev.statevector(c, p)
                lam = table * psi if diagonal else variance_reference.apply_strings(op, psi)
                r = lam - float(np.real(np.vdot(psi, lam))) * psi
                values[e] = float(np.real(np.vdot(r, r)))
            del psi, lam, r
            torch.zeros(1, device="cuda").item()  # (the downloads are let go inside the baseline's own window)
            return values

        variants = {"folded gradients, all parameters": lambda: dev.folded_gradients(circuits, params, None, with_values=True, with_energies=True),
                    "plain adjoint, all parameters": lambda: dev.adjoint_gradients(circuits, params, return_values=True),
                    "folded gradients, last layer": lambda: dev.folded_gradients(circuits, params, None, last, with_values=True),
                    "plain adjoint, last layer": lambda: dev.adjoint_gradients(circuits, params, last, return_values=True),
                    "folded value-only call": lambda: dev.folded_gradients(circuits, params, None, [], with_values=True),
                    "variances (one pass)": lambda: dev.variances(circuits, params),
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
        costs = np.asarray(results["folded gradients, all parameters"][1])
        spread = float(np.abs(op.coeffs.real).sum())
        bound = 1e-10 * max(1.0, spread) ** 2
        err_one_pass = float(np.abs(costs - np.asarray(results["variances (one pass)"][1])).max())
        err_numpy = float(np.abs(costs - results["statevector+numpy (value)"]).max())
        if err_one_pass > bound or err_numpy > bound:
            raise SystemExit(f"{name}: the costs disagree (variances {err_one_pass:.3e}, NumPy {err_numpy:.3e}, bound {bound:.3e})")
        for v, t in times.items():
            med = float(np.median(t))
            records.append({"workload": name, "variant": v, "median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3, "rounds": len(t)})
            lines.append(f"{name:34s} {v:36s} {med * 1e3:11.3f} {min(t) * 1e3:11.3f} {max(t) * 1e3:11.3f}")
            print(lines[-1], flush=True)
        med = {v: float(np.median(t)) * 1e3 for v, t in times.items()}
        extra_all = med["folded gradients, all parameters"] - med["plain adjoint, all parameters"]
        extra_last = med["folded gradients, last layer"] - med["plain adjoint, last layer"]
        # what the extra passes must move per amplitude, 16-byte amplitudes: the fused pass reads psi and the diagonal table and writes
        # lambda; else the residual pass reads psi and lambda_1 and writes r, and the seed pass reads r and psi and writes lambda (its
        # gathers at i ^ x come on top; they are counted as one further read of r)
        per_amplitude = 16 + 8 + 16 if diagonal else (16 + 16 + 16) + (16 + 16 + 16 + 16)
        moved = per_amplitude * (1 << n) * count
        share = moved / (extra_all * 1e-3) / HBM_BYTES_PER_SECOND if extra_all > 0 else float("nan")
        stats = dev.adjoint_stats()
        records.append({"workload": name, "extra_over_plain_all_ms": extra_all, "extra_over_plain_last_ms": extra_last, "extra_bytes": moved,
                        "extra_share_of_hbm": share, "cost_against_variances": err_one_pass, "cost_against_numpy": err_numpy,
                        "scratch_bytes": stats["scratch_bytes"]})
        lines.append(f"{name:34s} folded over plain adjoint: all parameters {extra_all:+.3f} ms, last layer {extra_last:+.3f} ms "
                     f"({'one fused pass' if diagonal else 'the residual and the seed pass'}, {moved / 2**20:.0f} MiB: {share:.2f} of 8 TB/s); value-only call "
                     f"{med['folded value-only call']:.3f} ms against variances {med['variances (one pass)']:.3f} ms; largest |cost - variances| "
                     f"{err_one_pass:.2e}, to NumPy {err_numpy:.2e}; adjoint scratch {stats['scratch_bytes'] / 2**20:.0f} MiB")
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
