"""Time OperatorCircuitEvaluator.evaluate_covariances on one MI355X and write profiles/r19_covariance.txt.

  subject    evaluate_covariances(circuits, points, parts, with_values=True): the covariance matrix (and the values) of M
             observables per circuit, reduced on the device from the final states (qsv_observables_covariance)
  baseline 1 M evaluate_variances calls, one OperatorCircuitEvaluator per observable on one shared StatevectorDevice (what
             GpuEstimator(shots=N) does for an array pub): the DIAGONAL of the matrix only, M installs and M passes
  baseline 2 the only route to the full matrix before: StatevectorDevice.statevector() per circuit (2^n amplitudes over PCIe
             each), every part applied in NumPy (its diagonal table, built outside the timed window, times the state, plus every
             other string as a sign vector times a gathered copy), then Re(L^H L) - E E^T

Shapes: those of scripts/variancetime.py, the set being the operator's parts -- the strings dealt round-robin into M observables:
the n = 20 Ising operator (210 strings) cut into 8, 16 and 32 parts, the 500-string operator into 16, the n = 24 Ising operator into 8.
All variants of a shape run in one process, interleaved: --warm rounds first, then --rounds timed rounds of one call each; a time
is host wall time around a call that returns its results.  Reported: the medians, and minimum / maximum per variant.  The two
kernels' own time comes from HIP events around them on the handle's stream (option "time_moments", read back as
profile()["expect_ms"]) in calls of their own.  Every figure is what this run measured."""

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
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice  # noqa: E402
from queasars_amd.ir import PauliOperator  # noqa: E402
from variancetime import NumpyOperator, _parity  # noqa: E402

SHAPES = (
    {"name": "n=20 L=4 16 circuits, Ising in 8 parts", "n": 20, "layers": 4, "circuits": 16, "strings": 0, "parts": 8},
    {"name": "n=20 L=4 16 circuits, Ising in 32 parts", "n": 20, "layers": 4, "circuits": 16, "strings": 0, "parts": 32},
    {"name": "n=20 L=8 16 circuits, Ising in 16 parts", "n": 20, "layers": 8, "circuits": 16, "strings": 0, "parts": 16},
    {"name": "n=20 L=4 1 circuit, 500 strings in 16", "n": 20, "layers": 4, "circuits": 1, "strings": 500, "parts": 16},
    {"name": "n=24 L=8 4 circuits, Ising in 8 parts", "n": 24, "layers": 8, "circuits": 4, "strings": 0, "parts": 8},
)


def parts_of(op: PauliOperator, count: int) -> list:
    """The operator's strings dealt round-robin into `count` observables."""
    labels, coeffs = op.labels, op.coeffs
    return [PauliOperator(labels[k::count], coeffs[k::count]) for k in range(count)]


def apply_part(host: NumpyOperator, state: np.ndarray) -> np.ndarray:
    lam = host.table * state if host.table is not None else np.zeros_like(state)
    for x, z, c in host.strings:
        n_y = bin(x & z).count("1")
        lam += (c * (-1j) ** (n_y % 4)) * ((1.0 - 2.0 * _parity(host.idx & z)) * state[host.idx ^ x])
    return lam


def numpy_covariance(hosts, state: np.ndarray):
    panel = np.stack([apply_part(h, state) for h in hosts], axis=1)
    values = np.real(state.conj() @ panel)
    return values, np.real(panel.conj().T @ panel) - np.outer(values, values)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r19_covariance.txt")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("covariancetime.py measures on a GPU: none found")
    import helpers

    c_oracle = helpers.load_c_oracle()
    lines = [f"evaluate_covariances against M evaluate_variances calls (the diagonal only) and against statevector() + NumPy (the full matrix); "
             f"{args.warm} warm-up and {args.rounds} timed rounds per shape, variants interleaved in one process, host wall time per call; "
             "kernel time from HIP events around the two kernels (calls of their own)",
             f"{'shape':42s} {'variant':22s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'vs covariances':>14s}"]
    records = []
    for shape in (SHAPES[i] for i in args.shapes):
        n, count, m = shape["n"], shape["circuits"], shape["parts"]
        _, circuits, params = workloads.population_circuits(n, shape["layers"], count, seed=0)
        op = workloads.random_pauli_operator(n, shape["strings"], seed=1234) if shape["strings"] else workloads.random_ising_operator(n, seed=2020)
        parts = parts_of(op, m)
        hosts = [NumpyOperator(p, c_oracle) for p in parts]
        dev = StatevectorDevice(n)
        evaluator = OperatorCircuitEvaluator(op, statevector_device=dev)
        singles = [OperatorCircuitEvaluator(p, statevector_device=dev) for p in parts]

        def m_variance_calls():
            return [e.evaluate_variances(circuits, params, with_values=True) for e in singles]

        def baseline():
            return [numpy_covariance(hosts, dev.statevector(c, p)) for c, p in zip(circuits, params)]

        variants = {"evaluate_covariances": lambda: evaluator.evaluate_covariances(circuits, params, parts, with_values=True),
                    "M evaluate_variances": m_variance_calls,
                    "statevector+numpy": baseline}
        times = {name: [] for name in variants}
        results = {}
        for rnd in range(args.warm + args.rounds):
            for name, call in variants.items():  # (interleaved: every round runs each variant once)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results[name] = call()
                seconds = time.perf_counter() - t0
                if rnd >= args.warm:
                    times[name].append(seconds)
        values, cov = results["evaluate_covariances"]
        s = np.maximum(1.0, np.asarray([float(np.abs(p.coeffs).sum()) for p in parts]))
        bound = 1e-11 * np.outer(s, s)
        err_cov = np.max([np.abs(cov[k] - b[1]) / bound for k, b in enumerate(results["statevector+numpy"])]) * 1e-11
        err_diag = max(float(np.abs(np.diagonal(cov, axis1=1, axis2=2)[:, k] - np.asarray(r[1])).max() / s[k] ** 2)
                       for k, r in enumerate(results["M evaluate_variances"]))
        err_val = max(float(np.abs(values[:, k] - np.asarray(r[0])).max()) for k, r in enumerate(results["M evaluate_variances"]))
        if err_cov > 1e-11 or err_diag > 1e-11 or err_val > 1e-10:
            raise SystemExit(f"{shape['name']}: the variants disagree (covariance {err_cov:.3e}, diagonal {err_diag:.3e}, value {err_val:.3e})")
        base = float(np.median(times["evaluate_covariances"]))
        for name, t in times.items():
            med = float(np.median(t))
            records.append({"shape": shape["name"], "variant": name, "median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                            "ratio_to_covariances": med / base})
            lines.append(f"{shape['name']:42s} {name:22s} {med * 1e3:10.3f} {min(t) * 1e3:9.3f} {max(t) * 1e3:9.3f} {med / base:14.2f}")
        # the kernels' own time: events around them, in calls of their own
        dev.set_option("time_moments", 1)
        kernel_ms = []
        for _ in range(args.warm + args.rounds):
            evaluator.evaluate_covariances(circuits, params, parts)
            kernel_ms.append(float(dev.profile()["expect_ms"]))
        dev.set_option("time_moments", 0)
        kernel = float(np.median(kernel_ms[args.warm:]))
        groups = sum(h.groups + (1 if h.table is not None else 0) for h in hosts)
        records.append({"shape": shape["name"], "kernel_ms": kernel, "observables": m, "x_mask_groups_over_the_parts": groups,
                        "max_covariance_difference_over_SaSb": float(err_cov), "max_diagonal_difference_over_S2": err_diag,
                        "max_value_difference": err_val})
        lines.append(f"{shape['name']:42s} the two kernels: {kernel:.3f} ms for {count} states, {m} observables, {groups} x-mask groups over the parts;"
                     f" largest |dC| / (S_a S_b) to NumPy {err_cov:.2e}, largest |dC_mm - Var_m| / S_m^2 {err_diag:.2e}, largest |dE| {err_val:.2e}")
        del evaluator, singles, dev
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(records))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
