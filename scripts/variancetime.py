"""Time OperatorCircuitEvaluator.evaluate_variances on one MI355X and write profiles/r18_variance.txt.

  subject    evaluate_variances(circuits, points, with_values=True): the operator's variance (and value) per circuit, reduced
             on the device from the final states (qsv_variance_circuits)
  baseline   the only route the public API had before: StatevectorDevice.statevector() per circuit (2^n amplitudes over PCIe
             each), then H applied in NumPy -- the diagonal table (built once, outside the timed window) times the state, plus
             every other string as a sign vector times a gathered copy of the state
  beside it  evaluate_circuits on the same batch: what the route through the whole state costs over the expectation route

Shapes: n = 20 with 4 and with 8 layers, 16 circuits, the Ising operator; n = 20, 4 layers, a general operator of 500 strings
(ONE circuit: the baseline needs about 20 s of NumPy per circuit there); n = 24, 8 layers, 4 circuits, Ising.  All variants of
a shape run in one process, interleaved: --warm rounds first, then --rounds timed rounds of one call each; a time is host wall
time around a call that returns its results.  Reported: the medians, and minimum / maximum per variant.  The two kernels' own
time comes from HIP events around them on the handle's stream (option "time_moments", read back as profile()["expect_ms"]) in
calls of their own; their rate is (x-mask groups + 1 + [a diagonal table is read]) * state bytes * circuits / that time: the
state read once per group and once for psi_i itself, the table once.  Every figure is what this run measured."""

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
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator  # noqa: E402

SHAPES = (
    {"name": "n=20 L=4 16 circuits, Ising", "n": 20, "layers": 4, "circuits": 16, "strings": 0},
    {"name": "n=20 L=8 16 circuits, Ising", "n": 20, "layers": 8, "circuits": 16, "strings": 0},
    {"name": "n=20 L=4 1 circuit, 500 Pauli strings", "n": 20, "layers": 4, "circuits": 1, "strings": 500},
    {"name": "n=24 L=8 4 circuits, Ising", "n": 24, "layers": 8, "circuits": 4, "strings": 0},
)


BYTES_NOTE = ("bytes per second: (x-mask groups + 1 + [diagonal table]) * 16 * 2^n * circuits over the kernels' time -- the table counted as one more state although "
              "its entries are 8 bytes (under a diagonal operator 0.75 of the figure really moves), and states the last gate pass has just written are read largely "
              "from the Infinity Cache, which is how a figure can exceed what the HBM delivers")


def _parity(v: np.ndarray) -> np.ndarray:
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> s
    return v & 1


class NumpyOperator:
    """What a user of the parent commit keeps per operator: the diagonal table and the other strings."""

    def __init__(self, op, c_oracle):
        real = op.coeffs.real
        diagonal = (op.x_mask == 0) & (real != 0.0)
        self.table = None
        if diagonal.any():
            from queasars_amd.ir import PauliOperator

            part = PauliOperator([label for label, d in zip(op.labels, diagonal) if d], real[diagonal])
            self.table = c_oracle.diagonal_table(part)
        self.strings = [(int(x), int(z), float(c)) for x, z, c in zip(op.x_mask, op.z_mask, real) if x != 0 and c != 0.0]
        self.groups = len({x for x, _, _ in self.strings})
        self.idx = np.arange(1 << op.num_qubits, dtype=np.int64)

    def moments(self, state: np.ndarray) -> tuple[float, float]:
        lam = self.table * state if self.table is not None else np.zeros_like(state)
        for x, z, c in self.strings:
            n_y = bin(x & z).count("1")
            lam += (c * (-1j) ** (n_y % 4)) * ((1.0 - 2.0 * _parity(self.idx & z)) * state[self.idx ^ x])
        value = float(np.vdot(state, lam).real)
        return value, float(np.vdot(lam, lam).real) - value * value


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r18_variance.txt")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("variancetime.py measures on a GPU: none found")
    import helpers

    c_oracle = helpers.load_c_oracle()
    lines = [f"evaluate_variances against statevector() + NumPy and beside evaluate_circuits; {args.warm} warm-up and {args.rounds} timed "
             "rounds per shape, variants interleaved in one process, host wall time per call; kernel time from HIP events around the "
             "two kernels (calls of their own)",
             f"{'shape':40s} {'variant':18s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'vs variances':>12s}"]
    records = []
    for shape in (SHAPES[i] for i in args.shapes):
        n, count = shape["n"], shape["circuits"]
        _, circuits, params = workloads.population_circuits(n, shape["layers"], count, seed=0)
        op = workloads.random_pauli_operator(n, shape["strings"], seed=1234) if shape["strings"] else workloads.random_ising_operator(n, seed=2020)
        host = NumpyOperator(op, c_oracle)
        evaluator = OperatorCircuitEvaluator(op)
        dev = evaluator.statevector_device

        def baseline():
            return [host.moments(dev.statevector(c, p)) for c, p in zip(circuits, params)]

        variants = {"evaluate_variances": lambda: evaluator.evaluate_variances(circuits, params, with_values=True),
                    "evaluate_circuits": lambda: evaluator.evaluate_circuits(circuits, params),
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
        values, variances = results["evaluate_variances"]
        spread = float(np.abs(op.coeffs).sum())
        err_var = max(abs(v - b[1]) for v, b in zip(variances, results["statevector+numpy"]))
        err_val = max(abs(v - e) for v, e in zip(values, results["evaluate_circuits"]))
        if err_var > 1e-11 * max(1.0, spread) ** 2 or err_val > 1e-10:
            raise SystemExit(f"{shape['name']}: the variants disagree (variance {err_var:.3e}, value {err_val:.3e})")
        base = float(np.median(times["evaluate_variances"]))
        for name, t in times.items():
            med = float(np.median(t))
            records.append({"shape": shape["name"], "variant": name, "median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                            "ratio_to_variances": med / base})
            lines.append(f"{shape['name']:40s} {name:18s} {med * 1e3:10.3f} {min(t) * 1e3:9.3f} {max(t) * 1e3:9.3f} {med / base:12.2f}")
        # the kernels' own time: events around them, in calls of their own
        dev.set_option("time_moments", 1)
        kernel_ms = []
        for _ in range(args.warm + args.rounds):
            evaluator.evaluate_variances(circuits, params)
            kernel_ms.append(float(dev.profile()["expect_ms"]))
        dev.set_option("time_moments", 0)
        kernel = float(np.median(kernel_ms[args.warm:]))
        reads = host.groups + 1 + (1 if host.table is not None else 0)
        state_bytes = 16 << n
        moved = reads * state_bytes * count  # (the table counted as one more state, although its entries are 8 bytes)
        records.append({"shape": shape["name"], "kernel_ms": kernel, "x_mask_groups": host.groups, "diagonal_table": host.table is not None,
                        "bytes": moved, "bytes_per_second": moved / (kernel * 1e-3), "max_variance_difference": err_var,
                        "max_value_difference": err_val})
        lines.append(f"{shape['name']:40s} the two kernels: {kernel:.3f} ms for {count} states, {host.groups} x-mask groups"
                     f"{' and the diagonal table' if host.table is not None else ''}: {moved / 1e6:.1f} MB, {moved / (kernel * 1e-3) / 1e12:.3f} TB/s;"
                     f" largest |dVar| to NumPy {err_var:.2e}, largest |dE| to evaluate_circuits {err_val:.2e}")
        del evaluator, dev
    lines.append(BYTES_NOTE)
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(records))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
