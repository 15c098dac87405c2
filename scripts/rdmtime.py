"""Time OperatorCircuitEvaluator.reduced_density_matrices on one MI355X and write profiles/r24_reduced_density.txt.

  subject    reduced_density_matrices(circuits, points, subsets): rho_A = Tr_rest |psi><psi| of every circuit's final state on
             every qubit subset, reduced on the device (qsv_reduced_density_circuits)
  baseline   the only route the public API had before: StatevectorDevice.statevector() per circuit (2^n amplitudes over PCIe),
             then per subset reshape, transpose and np.einsum on the host

Shapes: n = 20, 4 layers: 1 circuit x 210 subsets (all single qubits and pairs), 64 circuits x 20 single qubits, 16 circuits x 16
four-qubit subsets; n = 24, 8 layers: 4 circuits x 24 single qubits.  All variants of a shape run in one process, interleaved:
--warm rounds first, then --rounds timed rounds of one call each; a time is host wall time around a call that returns its results,
behind a synchronise.  Reported: the medians, and minimum / maximum per variant.  The two kernels' own time comes from HIP events
around them on the handle's stream (option "time_moments", read back as profile()["expect_ms"]) in calls of their own.  Over that
time three figures: the bytes the algorithm needs -- every state once, circuits * 16 * 2^n (fp64), against the HBM's bandwidth --,
the bytes the panels read -- every state once per subset, which the caches serve at 20 qubits --, and the matrix pipe's fp64
operations, 3 instructions of 2 * 16 * 16 * 4 per four columns of a padded 16 x 16 tile, 6 * 256 per amplitude column.  Every
figure is what this run measured."""

from __future__ import annotations

import argparse
import json
import sys
import time
from itertools import combinations
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from queasars_amd import workloads  # noqa: E402
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator  # noqa: E402


def _singles_and_pairs(n):
    return [(q,) for q in range(n)] + list(combinations(range(n), 2))


def _four_qubit_subsets(n, count):
    rng = np.random.default_rng(4)
    fixed = [(0, 1, 2, 3), (n - 4, n - 3, n - 2, n - 1), (0, 5, 6, n - 1), (7, 2, 9, 0)]
    return fixed + [tuple(int(q) for q in rng.choice(n, size=4, replace=False)) for _ in range(count - len(fixed))]


SHAPES = (
    {"name": "n=20 L=4 1 x 210 singles and pairs", "n": 20, "layers": 4, "circuits": 1, "subsets": _singles_and_pairs},
    {"name": "n=20 L=4 64 x 20 singles", "n": 20, "layers": 4, "circuits": 64, "subsets": lambda n: [(q,) for q in range(n)]},
    {"name": "n=20 L=4 16 x 16 four-qubit", "n": 20, "layers": 4, "circuits": 16, "subsets": lambda n: _four_qubit_subsets(n, 16)},
    {"name": "n=24 L=8 4 x 24 singles", "n": 24, "layers": 8, "circuits": 4, "subsets": lambda n: [(q,) for q in range(n)]},
)


def host_matrix(state: np.ndarray, subset) -> np.ndarray:
    """rho_A by reshape, transpose and einsum: bit j of a row index is the subset's j-th qubit."""
    n = int(state.size).bit_length() - 1
    k = len(subset)
    rest = [q for q in range(n - 1, -1, -1) if q not in subset]
    axes = [n - 1 - q for q in reversed(subset)] + [n - 1 - q for q in rest]
    m = state.reshape((2,) * n).transpose(axes).reshape(1 << k, 1 << (n - k))
    return np.einsum("ab,cb->ac", m, m.conj())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r24_reduced_density.txt")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rdmtime.py measures on a GPU: none found")
    lines = [f"reduced_density_matrices against statevector() + NumPy einsum; {args.warm} warm-up and {args.rounds} timed rounds per shape, "
             "variants interleaved in one process, host wall time per call; kernel time from HIP events around the two kernels (calls of their own)",
             f"{'shape':38s} {'variant':26s} {'median ms':>11s} {'min ms':>11s} {'max ms':>11s} {'vs the call':>12s}"]
    records = []
    for shape in (SHAPES[i] for i in args.shapes):
        n, count = shape["n"], shape["circuits"]
        subsets = shape["subsets"](n)
        _, circuits, params = workloads.population_circuits(n, shape["layers"], count, seed=0)
        evaluator = OperatorCircuitEvaluator(workloads.random_ising_operator(n, seed=2020))
        dev = evaluator.statevector_device

        def baseline():
            out = [np.zeros((count, 1 << len(s), 1 << len(s)), dtype=np.complex128) for s in subsets]
            for e, (c, p) in enumerate(zip(circuits, params)):
                psi = dev.statevector(c, p)
                for j, s in enumerate(subsets):
                    out[j][e] = host_matrix(psi, s)
            # (the download is let go inside the baseline's own window, with one tiny device round trip: scripts/overlaptime.py)
            del psi
            torch.zeros(1, device="cuda").item()
            return out

        variants = {"reduced_density_matrices": lambda: evaluator.reduced_density_matrices(circuits, params, subsets),
                    "statevector+einsum": baseline}
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
                print(f"  {shape['name']} round {rnd} {name}: {seconds * 1e3:.3f} ms", flush=True)
        err = max(float(max(np.abs((g - w).real).max(), np.abs((g - w).imag).max()))
                  for g, w in zip(results["reduced_density_matrices"], results["statevector+einsum"]))
        if err > 1e-11:
            raise SystemExit(f"{shape['name']}: the variants disagree ({err:.3e})")
        base = float(np.median(times["reduced_density_matrices"]))
        for name, t in times.items():
            med = float(np.median(t))
            records.append({"shape": shape["name"], "variant": name, "median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                            "ratio_to_call": med / base})
            lines.append(f"{shape['name']:38s} {name:26s} {med * 1e3:11.3f} {min(t) * 1e3:11.3f} {max(t) * 1e3:11.3f} {med / base:12.2f}")
            print(lines[-1], flush=True)
        # the kernels' own time: events around them, in calls of their own
        dev.set_option("time_moments", 1)
        kernel_ms = []
        for _ in range(args.warm + args.rounds):
            evaluator.reduced_density_matrices(circuits, params, subsets)
            kernel_ms.append(float(dev.profile()["expect_ms"]))
        dev.set_option("time_moments", 0)
        kernel = float(np.median(kernel_ms[args.warm:]))
        state_bytes = 16 << n
        needed = count * state_bytes
        panel_reads = count * len(subsets) * state_bytes
        # (a block of 2^(k+6) amplitudes is 16 steps of 3 instructions, each 2 * 16 * 16 * 4 operations, whatever k is)
        flops = sum(count * float(1 << n) / (1 << (len(s) + 6)) * 16 * 3 * 2 * 16 * 16 * 4 for s in subsets)
        records.append({"shape": shape["name"], "kernel_ms": kernel, "needed_bytes": needed, "needed_bytes_per_second": needed / (kernel * 1e-3),
                        "panel_read_bytes": panel_reads, "panel_read_bytes_per_second": panel_reads / (kernel * 1e-3),
                        "matrix_flops_per_second": flops / (kernel * 1e-3), "max_difference": err})
        lines.append(f"{shape['name']:38s} the two kernels: {kernel:.3f} ms; needed {needed / 1e6:.0f} MB = {needed / (kernel * 1e-3) / 1e12:.3f} TB/s "
                     f"(against HBM bandwidth); panels read {panel_reads / 1e6:.0f} MB = {panel_reads / (kernel * 1e-3) / 1e12:.3f} TB/s (caches); "
                     f"matrix pipe {flops / (kernel * 1e-3) / 1e12:.2f} TFLOP/s fp64 (padded tiles); largest difference to NumPy {err:.2e}")
        print(lines[-1], flush=True)
        del evaluator, dev
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(records))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
