"""Time OperatorCircuitEvaluator.operator_density_matrices on one MI355X and write profiles/r29_operator_density.txt.

  subject    operator_density_matrices(circuits, points, singles and pairs): W_A = Tr_rest(H |psi><psi|) of every circuit's final
             state on every single qubit and unordered pair, reduced on the device (qsv_operator_density_circuits)
             -- what evqe/growth.py turns into the gradient, at identity, of every gate a new EVQE layer could hold
  beside it  reduced_density_matrices with the same subsets on the same commit: half the bytes, three of the four matrix
             products, no operator sweep;
             k adjoint gradients of grown circuits per parent (k = 4 and 16 candidate layers appended at zeros): what screening
             k candidates cost without the call;
             statevector() + NumPy (download, H psi string by string, einsum per subset): the only other route to the numbers.
             A round of it takes seconds to a minute and the host does one circuit after the other, so it is timed apart from
             the interleaved rounds: 11 rounds behind an untimed one at 20 qubits and one circuit; ONE round, nothing in front
             of it, over the first 2 of the 64 circuits, reported per circuit and times 64 (scaled, and said so in the line);
             ONE round at 24 qubits.  Each line says its rounds

Shapes: n = 20 (4 layers) with 1 and 64 circuits, n = 24 (4 layers) with 1 circuit; operator: 20 random Pauli strings.  The device
variants of a shape run in one process, interleaved: --warm rounds first, then --rounds timed rounds of one call each; a time is
host wall time around a call that returns its results, behind a synchronise.  Reported: median, minimum and maximum per variant.
The call's own kernels (the operator sweep, the panels, the combine) are timed by HIP events around them on the handle's stream
(option "time_moments", profile()["expect_ms"]) in calls of their own, and so are the reduced density call's two kernels.  Against
that time: the bytes the algorithm needs (psi read and lambda written by the operator sweep, both read once by the panels:
circuits * 4 * 16 * 2^n) over the HBM's 8 TB/s, and the matrix pipe's fp64 operations on PADDED tiles (a block of 2^(k+6) amplitudes
is 16 steps of 4 instructions of 2 * 16 * 16 * 4 operations) over its 78.6 TFLOP/s; the larger of the two least times binds.  Every
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
from queasars_amd.evqe.genome import EVQEIndividual  # noqa: E402

HBM_BYTES_PER_SECOND = 8.0e12
MATRIX_FP64_PER_SECOND = 78.6e12
# host_circuits, host_rounds: the circuits a round of the host route takes and its timed rounds (behind one untimed round where
# host_warm is set: at 24 qubits a round takes most of a minute, and NumPy has nothing to warm but the page cache)
SHAPES = ({"name": "n=20 L=4 1 circuit", "n": 20, "layers": 4, "circuits": 1, "host_circuits": 1, "host_rounds": 11, "host_warm": 1},
          {"name": "n=20 L=4 64 circuits", "n": 20, "layers": 4, "circuits": 64, "host_circuits": 2, "host_rounds": 1, "host_warm": 0},
          {"name": "n=24 L=4 1 circuit", "n": 24, "layers": 4, "circuits": 1, "host_circuits": 1, "host_rounds": 1, "host_warm": 0})


def singles_and_pairs(n):
    return [(q,) for q in range(n)] + list(combinations(range(n), 2))


def host_panel(state: np.ndarray, subset) -> np.ndarray:
    """The state as a 2^k x 2^(n-k) matrix: bit j of a row index is the subset's j-th qubit."""
    n = int(state.size).bit_length() - 1
    k = len(subset)
    rest = [q for q in range(n - 1, -1, -1) if q not in subset]
    axes = [n - 1 - q for q in reversed(subset)] + [n - 1 - q for q in rest]
    return state.reshape((2,) * n).transpose(axes).reshape(1 << k, 1 << (n - k))


def host_apply(op, state: np.ndarray) -> np.ndarray:
    """H_h psi string by string: (P psi)_i = (-i)^ny (-1)^popcount(i & z) psi_(i ^ x), weighted by the coefficient's real part."""
    index = np.arange(state.size, dtype=np.int64)
    out = np.zeros_like(state)
    for x, z, c in zip(op.x_mask, op.z_mask, op.coeffs):
        x, z = int(x), int(z)
        parity = index & z
        for shift in (32, 16, 8, 4, 2, 1):
            parity ^= parity >> shift
        out += (complex(c).real * (-1j) ** (bin(x & z).count("1") % 4)) * ((1.0 - 2.0 * (parity & 1)) * state[index ^ x])
    return out


def summary(times):
    return float(np.median(times)) * 1e3, min(times) * 1e3, max(times) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r29_operator_density.txt")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("operatordensitytime.py measures on a GPU: none found")
    lines = [f"operator_density_matrices over all single qubits and unordered pairs; {args.warm} warm-up and {args.rounds} timed rounds per shape, "
             "device variants interleaved in one process, host wall time per call behind a synchronise; kernel time from HIP events (calls of their own)",
             f"{'shape':24s} {'variant':34s} {'median ms':>11s} {'min ms':>11s} {'max ms':>11s} {'vs the call':>12s}"]
    records = []
    for shape in (SHAPES[i] for i in args.shapes):
        n, count = shape["n"], shape["circuits"]
        subsets = singles_and_pairs(n)
        population, circuits, params = workloads.population_circuits(n, shape["layers"], count, seed=0)
        op = workloads.random_pauli_operator(n, 20, seed=1234)
        evaluator = OperatorCircuitEvaluator(op, gradient_method="adjoint")
        dev = evaluator.statevector_device
        grown = {}
        for k in (4, 16):
            individuals = [EVQEIndividual.add_random_layers(parent, 1, False, random_seed=1000 * k + 16 * e + c)
                           for e, parent in enumerate(population.individuals) for c in range(k)]
            grown[k] = ([i.get_parameterized_quantum_circuit() for i in individuals], [list(i.parameter_values) for i in individuals])
        variants = {"operator_density_matrices": lambda: evaluator.operator_density_matrices(circuits, params, subsets),
                    "reduced_density_matrices": lambda: evaluator.reduced_density_matrices(circuits, params, subsets),
                    "adjoint gradients, k=4 a parent": lambda: evaluator.evaluate_gradients(*grown[4]),
                    "adjoint gradients, k=16 a parent": lambda: evaluator.evaluate_gradients(*grown[16])}
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
            print(f"  {shape['name']} round {rnd} done", flush=True)
        base = float(np.median(times["operator_density_matrices"]))
        for name, t in times.items():
            med, low, high = summary(t)
            records.append({"shape": shape["name"], "variant": name, "median_ms": med, "min_ms": low, "max_ms": high, "ratio_to_call": med / (base * 1e3)})
            lines.append(f"{shape['name']:24s} {name:34s} {med:11.3f} {low:11.3f} {high:11.3f} {med / (base * 1e3):12.2f}")
            print(lines[-1], flush=True)
        host_count, host_times, parts, err = shape["host_circuits"], [], None, 0.0
        for rnd in range(shape["host_warm"] + shape["host_rounds"]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            spent = [0.0, 0.0, 0.0]
            for e in range(host_count):
                t1 = time.perf_counter()
                psi = dev.statevector(circuits[e], params[e])
                t2 = time.perf_counter()
                lam = host_apply(op, psi)
                t3 = time.perf_counter()
                host = [np.einsum("ab,cb->ac", host_panel(lam, s), host_panel(psi, s).conj()) for s in subsets]
                t4 = time.perf_counter()
                spent = [spent[0] + t2 - t1, spent[1] + t3 - t2, spent[2] + t4 - t3]
                if rnd == 0:  # (outside no timed round where there is a warm-up; inside the one timed round otherwise: microseconds)
                    err = max([err] + [float(max(np.abs((g[e] - w).real).max(), np.abs((g[e] - w).imag).max()))
                                       for g, w in zip(results["operator_density_matrices"], host)])
            if rnd >= shape["host_warm"]:
                host_times.append((time.perf_counter() - t0) / host_count * count)
                parts = [v / host_count for v in spent]
            print(f"  {shape['name']} host round {rnd} done", flush=True)
        scale = max(1.0, float(np.abs(op.coeffs.real).sum()))
        if err > 1e-10 * scale:
            raise SystemExit(f"{shape['name']}: the call and the host disagree ({err:.3e})")
        med, low, high = summary(host_times)
        how = f"{shape['host_rounds']} round(s)" + (f" over the first {host_count} circuits, per circuit x {count}: SCALED" if host_count < count else "")
        records.append({"shape": shape["name"], "variant": "statevector() + NumPy", "median_ms": med, "min_ms": low, "max_ms": high,
                        "ratio_to_call": med / (base * 1e3), "largest_difference": err, "rounds": shape["host_rounds"], "circuits_timed": host_count})
        lines.append(f"{shape['name']:24s} {'statevector() + NumPy':34s} {med:11.3f} {low:11.3f} {high:11.3f} {med / (base * 1e3):12.2f}   "
                     f"({how}; per circuit, last round: download {parts[0] * 1e3:.0f} ms, H psi {parts[1] * 1e3:.0f} ms, {len(subsets)} einsums "
                     f"{parts[2] * 1e3:.0f} ms; largest difference to the call {err:.2e})")
        print(lines[-1], flush=True)
        # the kernels' own time: events around them, in calls of their own
        dev.set_option("time_moments", 1)
        kernel = {}
        for name in ("operator_density_matrices", "reduced_density_matrices"):
            ms = []
            for _ in range(args.warm + args.rounds):
                variants[name]()
                ms.append(float(dev.profile()["expect_ms"]))
            kernel[name] = ms[args.warm:]
        dev.set_option("time_moments", 0)
        k_call, k_rdm = float(np.median(kernel["operator_density_matrices"])), float(np.median(kernel["reduced_density_matrices"]))
        state_bytes = 16 << n
        needed = count * 4 * state_bytes
        panel_reads = count * len(subsets) * 2 * state_bytes
        flops = sum(count * float(1 << n) / (1 << (len(s) + 6)) * 16 * 4 * 2 * 16 * 16 * 4 for s in subsets)
        least_bytes, least_flops = needed / HBM_BYTES_PER_SECOND * 1e3, flops / MATRIX_FP64_PER_SECOND * 1e3
        binds = "the matrix pipe" if least_flops >= least_bytes else "the HBM"
        records.append({"shape": shape["name"], "kernel_ms": k_call, "kernel_min_ms": min(kernel["operator_density_matrices"]),
                        "kernel_max_ms": max(kernel["operator_density_matrices"]), "rdm_kernel_ms": k_rdm, "kernel_ratio_to_rdm": k_call / k_rdm,
                        "needed_bytes": needed, "needed_bytes_per_second": needed / (k_call * 1e-3), "panel_read_bytes": panel_reads,
                        "panel_read_bytes_per_second": panel_reads / (k_call * 1e-3), "matrix_flops_per_second": flops / (k_call * 1e-3),
                        "least_ms_bytes": least_bytes, "least_ms_matrix": least_flops, "binds": binds,
                        "share_of_bound": max(least_bytes, least_flops) / k_call})
        lines.append(f"{shape['name']:24s} the call's kernels: {k_call:.3f} ms ({min(kernel['operator_density_matrices']):.3f} .. "
                     f"{max(kernel['operator_density_matrices']):.3f}); the reduced density call's: {k_rdm:.3f} ms; ratio {k_call / k_rdm:.2f}")
        lines.append(f"{'':24s} needed {needed / 1e6:.0f} MB = {needed / (k_call * 1e-3) / 1e12:.3f} TB/s of 8 (least {least_bytes:.3f} ms); panels read "
                     f"{panel_reads / 1e6:.0f} MB = {panel_reads / (k_call * 1e-3) / 1e12:.2f} TB/s (caches); matrix pipe "
                     f"{flops / (k_call * 1e-3) / 1e12:.1f} of 78.6 TFLOP/s fp64 on padded tiles (least {least_flops:.3f} ms); {binds} binds: "
                     f"{100 * max(least_bytes, least_flops) / k_call:.0f} % of that bound")
        print(lines[-2], flush=True)
        print(lines[-1], flush=True)
        del evaluator, dev
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(records))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
