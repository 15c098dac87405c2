"""Time OperatorCircuitEvaluator.evaluate_overlaps on one MI355X and write profiles/r21_overlaps.txt.

  subject    evaluate_overlaps(circuits, points, kept_states[, with_operator=True]): S = <phi_k|psi_e> (and T = <phi_k|H|psi_e>)
             of every circuit's final state against kept states, reduced on the device (qsv_overlap_circuits)
  baseline   the only route the public API had before: StatevectorDevice.statevector() per state (2^n amplitudes over PCIe each,
             kept states and evaluated ones alike), then np.vdot per pair; with the operator, H psi per evaluated state in NumPy
             first -- the diagonal table (built once, outside the timed window) times the state, plus
             tests/variance_reference.apply_strings for every other string, a sign vector times a gathered copy of the state

Shapes: n = 20, 4 layers, 16 circuits x 16 kept states; 64 x 64 with and without the Ising operator; 1 circuit x 16 kept states
with a general operator of 500 strings; n = 24, 8 layers, 4 x 4.  The kept states are kept once, outside the timed window (they
are what a user holds on to).  All variants of a shape run in one process, interleaved: --warm rounds first, then --rounds timed
rounds of one call each; a time is host wall time around a call that returns its results, behind a synchronise.  Reported: the
medians, and minimum / maximum per variant.  The two kernels' own time comes from HIP events around them on the handle's stream
(option "time_moments", read back as profile()["expect_ms"]) in calls of their own.  Over that time three figures: the bytes the
algorithm needs -- every state once, (circuits + kept states) * 16 * 2^n, against the HBM's bandwidth --, the bytes the tiles
read -- every pair of 16-state blocks reads its 32 states, plus one gathered read per x-mask group and evaluation of the pair
with the operator, which the caches serve --, and the matrix pipe's fp64 operations, 8 per amplitude and entry of a padded
tile (16 with the operator).  Every figure is what this run measured."""

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
sys.path.insert(0, str(ROOT / "scripts"))

from queasars_amd import workloads  # noqa: E402
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator  # noqa: E402

SHAPES = (
    {"name": "n=20 L=4 16 x 16", "n": 20, "layers": 4, "circuits": 16, "kept": 16, "operator": None},
    {"name": "n=20 L=4 64 x 64", "n": 20, "layers": 4, "circuits": 64, "kept": 64, "operator": None},
    {"name": "n=20 L=4 64 x 64, Ising", "n": 20, "layers": 4, "circuits": 64, "kept": 64, "operator": "ising"},
    {"name": "n=20 L=4 1 x 16, 500 Pauli strings", "n": 20, "layers": 4, "circuits": 1, "kept": 16, "operator": 500},
    {"name": "n=24 L=8 4 x 4", "n": 24, "layers": 8, "circuits": 4, "kept": 4, "operator": None},
)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r21_overlaps.txt")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("overlaptime.py measures on a GPU: none found")
    import helpers
    import variance_reference
    from variancetime import NumpyOperator

    c_oracle = helpers.load_c_oracle()
    lines = [f"evaluate_overlaps against statevector() + NumPy; {args.warm} warm-up and {args.rounds} timed rounds per shape, variants "
             "interleaved in one process, host wall time per call; kernel time from HIP events around the two kernels (calls of their own)",
             f"{'shape':36s} {'variant':20s} {'median ms':>11s} {'min ms':>11s} {'max ms':>11s} {'vs overlaps':>12s}"]
    records = []
    for shape in (SHAPES[i] for i in args.shapes):
        n, count, n_kept = shape["n"], shape["circuits"], shape["kept"]
        # the kept states: circuits of their own; the evaluated ones: another population
        _, kept_circuits, kept_params = workloads.population_circuits(n, shape["layers"], n_kept, seed=1)
        _, circuits, params = workloads.population_circuits(n, shape["layers"], count, seed=0)
        with_op = shape["operator"] is not None
        op = (workloads.random_pauli_operator(n, shape["operator"], seed=1234) if isinstance(shape["operator"], int)
              else workloads.random_ising_operator(n, seed=2020))
        host = NumpyOperator(op, c_oracle) if with_op else None  # (its diagonal table, and the count of x-mask groups)
        rest = None
        if with_op and host.strings:
            from queasars_amd.ir import PauliOperator

            off = (op.x_mask != 0) & (op.coeffs.real != 0.0)
            rest = PauliOperator([label for label, o in zip(op.labels, off) if o], op.coeffs.real[off])
        evaluator = OperatorCircuitEvaluator(op)
        dev = evaluator.statevector_device
        kept = evaluator.keep_states(kept_circuits, kept_params)

        def apply(state):
            lam = host.table * state if host.table is not None else np.zeros_like(state)
            return lam + variance_reference.apply_strings(rest, state) if rest is not None else lam

        def baseline():
            phis = [dev.statevector(c, p) for c, p in zip(kept_circuits, kept_params)]
            s = np.zeros((count, n_kept), dtype=np.complex128)
            t = np.zeros((count, n_kept), dtype=np.complex128) if with_op else None
            for e, (c, p) in enumerate(zip(circuits, params)):
                psi = dev.statevector(c, p)
                lam = apply(psi) if with_op else None
                for k, phi in enumerate(phis):
                    s[e, k] = np.vdot(phi, psi)
                    if with_op:
                        t[e, k] = np.vdot(phi, lam)
            # (the downloads are let go inside the baseline's own window, and one tiny device round trip follows: the next call
            # on the device otherwise pays for it -- about 10 ms per 16 MiB array freed, seen as 160 ms on the first call after
            # sixteen of them)
            del phis, psi, lam
            torch.zeros(1, device="cuda").item()
            return (s, t) if with_op else s

        variants = {"evaluate_overlaps": lambda: evaluator.evaluate_overlaps(circuits, params, kept, with_operator=with_op),
                    "statevector+numpy": baseline}
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
        got, want = results["evaluate_overlaps"], results["statevector+numpy"]
        spread = float(np.abs(op.coeffs).sum())
        err_s = float(np.abs((got[0] if with_op else got) - (want[0] if with_op else want)).max())
        err_t = float(np.abs(got[1] - want[1]).max()) if with_op else 0.0
        if err_s > 1e-11 or err_t > 1e-11 * max(1.0, spread):
            raise SystemExit(f"{shape['name']}: the variants disagree (S {err_s:.3e}, T {err_t:.3e})")
        base = float(np.median(times["evaluate_overlaps"]))
        for name, t in times.items():
            med = float(np.median(t))
            records.append({"shape": shape["name"], "variant": name, "median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                            "ratio_to_overlaps": med / base})
            lines.append(f"{shape['name']:36s} {name:20s} {med * 1e3:11.3f} {min(t) * 1e3:11.3f} {max(t) * 1e3:11.3f} {med / base:12.2f}")
            print(lines[-1], flush=True)
        # the kernels' own time: events around them, in calls of their own
        dev.set_option("time_moments", 1)
        kernel_ms = []
        for _ in range(args.warm + args.rounds):
            evaluator.evaluate_overlaps(circuits, params, kept, with_operator=with_op)
            kernel_ms.append(float(dev.profile()["expect_ms"]))
        dev.set_option("time_moments", 0)
        kernel = float(np.median(kernel_ms[args.warm:]))
        state_bytes = 16 << n
        blocks_e, blocks_k = (count + 15) // 16, (n_kept + 15) // 16
        groups = host.groups if with_op else 0
        needed = (count + n_kept) * state_bytes
        # (an evaluation is read once per block of kept states, a kept state once per block of evaluations)
        tile_reads = state_bytes * (blocks_k * count + blocks_e * n_kept) + state_bytes * blocks_k * count * groups
        if with_op and host.table is not None:
            tile_reads += (8 << n) * blocks_k * count
        flops = (16 if with_op else 8) * (16 * blocks_e) * (16 * blocks_k) * float(1 << n)
        records.append({"shape": shape["name"], "kernel_ms": kernel, "x_mask_groups": groups, "needed_bytes": needed,
                        "needed_bytes_per_second": needed / (kernel * 1e-3), "tile_read_bytes": tile_reads,
                        "tile_read_bytes_per_second": tile_reads / (kernel * 1e-3), "matrix_flops_per_second": flops / (kernel * 1e-3),
                        "max_s_difference": err_s, "max_t_difference": err_t})
        lines.append(f"{shape['name']:36s} the two kernels: {kernel:.3f} ms; needed {needed / 1e6:.0f} MB = {needed / (kernel * 1e-3) / 1e12:.3f} TB/s "
                     f"(against HBM bandwidth); tiles read {tile_reads / 1e6:.0f} MB = {tile_reads / (kernel * 1e-3) / 1e12:.3f} TB/s (caches); "
                     f"matrix pipe {flops / (kernel * 1e-3) / 1e12:.2f} TFLOP/s fp64 (padded tiles); {groups} x-mask groups; "
                     f"largest |dS| to NumPy {err_s:.2e}" + (f", |dT| {err_t:.2e}" if with_op else ""))
        for state in kept:
            state.release()
        del evaluator, dev, kept
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(records))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
