"""Time the deflated (VQD) cost evaluator on one MI355X and write profiles/r26_deflation.txt.

  subject    DeflatedOperatorCircuitEvaluator.evaluate_gradients (the adjoint sweep with the deflated seed) and
             .evaluate_circuits (the value-only call: forward run, H psi, overlaps) against K kept states
             (qsv_deflated_gradient_circuits)
  against    the plain adjoint gradient of the same circuits (OperatorCircuitEvaluator, gradient_method="adjoint"): the
             difference is what the overlaps and the deflate kernel cost;
             and the only route the public API had for the COST before: StatevectorDevice.statevector() per state, kept and
             evaluated alike, then np.vdot per pair and the diagonal operator's table times |psi|^2 (no gradient existed)

Shapes: n = 20 (16 circuits) and n = 24 (4 circuits), eight layers, the Ising operator, K = 1, 4, 16, 64.  The kept states are
kept once, outside the timed window.  All variants of a shape run in one process, interleaved: --warm rounds first, then
--rounds timed rounds of one call each; a time is host wall time around a call that returns its results, behind a synchronise.
The baseline moves gigabytes over PCIe and runs --baseline-rounds timed rounds (default one).  The deflate kernel's own time comes
from HIP events around it on the handle's stream (option "time_moments", read back as profile()["expect_ms"]) in calls of their
own; over it, the bytes the kernel moves: every kept state once per block of 16 evaluations, lambda of every evaluation read and
written, 16 bytes an amplitude.  Every figure is what this run measured."""

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
from queasars_amd.circuit_evaluation import DeflatedOperatorCircuitEvaluator, OperatorCircuitEvaluator  # noqa: E402

SIZES = ({"n": 20, "layers": 8, "circuits": 16}, {"n": 24, "layers": 8, "circuits": 4})
KEPT = (1, 4, 16, 64)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--baseline-rounds", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(range(len(SIZES))), help="indices into SIZES")
    ap.add_argument("--kept", type=int, nargs="*", default=list(KEPT))
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r26_deflation.txt")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("deflationtime.py measures on a GPU: none found")
    import helpers

    c_oracle = helpers.load_c_oracle()
    lines = [f"deflated cost evaluator against the plain adjoint gradient and against statevector() + NumPy; {args.warm} warm-up and "
             f"{args.rounds} timed rounds per shape ({args.baseline_rounds} for the baseline), variants interleaved in one process, host wall "
             "time per call; the deflate kernel's time from HIP events around it (calls of their own)",
             f"{'shape':28s} {'variant':30s} {'median ms':>11s} {'min ms':>11s} {'max ms':>11s}"]
    records = []
    for size in (SIZES[i] for i in args.sizes):
        n, count = size["n"], size["circuits"]
        op = workloads.random_ising_operator(n, seed=2020)
        table = c_oracle.diagonal_table(op)
        _, circuits, params = workloads.population_circuits(n, size["layers"], count, seed=0)
        _, kept_circuits, kept_params = workloads.population_circuits(n, size["layers"], max(args.kept), seed=1)
        plain = OperatorCircuitEvaluator(op, gradient_method="adjoint")
        dev = plain.statevector_device
        all_kept = plain.keep_states(kept_circuits, kept_params)
        for k in args.kept:
            name = f"n={n} L={size['layers']} {count} circuits K={k}"
            kept = all_kept[:k]
            deflated = DeflatedOperatorCircuitEvaluator(op, kept)
            betas = deflated.betas

            def baseline():
                phis = [dev.statevector(c, p) for c, p in zip(kept_circuits[:k], kept_params[:k])]
                costs = np.zeros(count)
                for e, (c, p) in enumerate(zip(circuits, params)):
                    psi = dev.statevector(c, p)
                    costs[e] = float(np.dot(table, psi.real ** 2 + psi.imag ** 2))
                    for beta, phi in zip(betas, phis):
                        costs[e] += beta * abs(np.vdot(phi, psi)) ** 2
                del phis, psi
                torch.zeros(1, device="cuda").item()  # (the downloads are let go inside the baseline's own window)
                return costs

            variants = {"deflated evaluate_gradients": lambda: deflated.evaluate_gradients(circuits, params),
                        "plain adjoint gradients": lambda: plain.evaluate_gradients(circuits, params),
                        "deflated evaluate_circuits": lambda: np.asarray(deflated.evaluate_circuits(circuits, params)),
                        "statevector+numpy (cost)": baseline}
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
            scale = float(np.abs(op.coeffs).sum()) + float(np.sum(np.abs(betas)))
            err = float(np.abs(results["deflated evaluate_circuits"] - results["statevector+numpy (cost)"]).max())
            if err > 1e-11 * scale:
                raise SystemExit(f"{name}: the cost and the baseline disagree ({err:.3e})")
            for v, t in times.items():
                med = float(np.median(t))
                records.append({"shape": name, "variant": v, "median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3, "rounds": len(t)})
                lines.append(f"{name:28s} {v:30s} {med * 1e3:11.3f} {min(t) * 1e3:11.3f} {max(t) * 1e3:11.3f}")
                print(lines[-1], flush=True)
            # the deflate kernel's own time: events around it, in calls of their own
            dev.set_option("time_moments", 1)
            kernel_ms = []
            for _ in range(args.warm + args.rounds):
                deflated.evaluate_gradients(circuits, params)
                kernel_ms.append(float(dev.profile()["expect_ms"]))
            dev.set_option("time_moments", 0)
            kernel = float(np.median(kernel_ms[args.warm:]))
            state_bytes = 16 << n
            moved = state_bytes * (k * ((count + 15) // 16) + 2 * count)
            flops = 8.0 * 16 * ((count + 15) // 16) * 4 * ((k + 3) // 4) * float(1 << n)
            overhead = (float(np.median(times["deflated evaluate_gradients"])) - float(np.median(times["plain adjoint gradients"]))) * 1e3
            records.append({"shape": name, "deflate_kernel_ms": kernel, "bytes_moved": moved, "bytes_per_second": moved / (kernel * 1e-3),
                            "matrix_flops_per_second": flops / (kernel * 1e-3), "overhead_ms": overhead, "max_cost_difference": err})
            lines.append(f"{name:28s} deflate kernel: {kernel:.3f} ms; moves {moved / 1e6:.0f} MB = {moved / (kernel * 1e-3) / 1e12:.3f} TB/s; matrix pipe "
                         f"{flops / (kernel * 1e-3) / 1e12:.2f} TFLOP/s fp64 (padded tiles); overlaps + deflate over the plain gradient {overhead:.3f} ms; "
                         f"largest |dC| to NumPy {err:.2e}")
            print(lines[-1], flush=True)
        for state in all_kept:
            state.release()
        del plain, dev, all_kept, deflated
    lines.append("a plain FMA loop in place of the matrix instructions was not built: no comparison was measured")
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(records))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
