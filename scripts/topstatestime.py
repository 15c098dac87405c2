"""Time the exact readout of one circuit's k most probable basis states on one MI355X and write profiles/r13_top_states.txt.

  variants    host        the path there was before ``qsv_top_states``: ``StatevectorDevice.probabilities()`` (the 2^n doubles over
                          PCIe; for a split circuit the state is formed first), ``numpy.argpartition`` for the k largest and a
                          ``numpy.lexsort`` of those k into the order probability descending, index ascending: the yardstick
              device      ``StatevectorDevice.top_states(circuits, values, k)``: selected on the device, 2 k numbers come back

  configurations   n = 20, four layers, a circuit the sampler branch reads from its side tables (split): no 2^n table is formed;
                   n = 24 and n = 28, four layers, ``split`` off: through the state, the probabilities of the last gate pass;
                   each with k = 16 and k = 1024, fp64, the first circuit of the seed-0 population that has the wanted form.

Each configuration is a child process under ``timeout``: --warm rounds first, then --rounds rounds, the two variants interleaved;
a time is host wall time around a call that ends with its result on the host.  Reported: median, minimum, maximum and the spread
(max - min) / median per variant and the ratio of medians.  The two answers are compared (same states; ties aside they must agree).
Every figure is what this run measured; nothing is estimated, and no ratio is claimed in advance."""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CONFIGURATIONS = ((20, True), (24, False), (28, False))  # (qubits, split)
KS = (16, 1024)


def host_top(device, circuit, values, k):
    probs = device.probabilities(circuit, values)
    part = np.argpartition(probs, probs.size - k)[probs.size - k:]
    order = part[np.lexsort((part, -probs[part]))]
    return order.astype(np.uint64), probs[order]


def measure(args) -> dict:
    import torch

    from queasars_amd import workloads
    from queasars_amd.circuit_evaluation import StatevectorDevice

    if not torch.cuda.is_available():
        raise SystemExit("topstatestime.py measures on a GPU: none found")
    device = StatevectorDevice(args.n)
    device.set_option("split", 1 if args.split else 0)
    _, circuits, params = workloads.population_circuits(args.n, args.layers, 16, seed=0)
    pick = next((i for i, c in enumerate(circuits) if device.circuit_form(c)["split_sampled"] == bool(args.split)), None)
    if pick is None:
        raise SystemExit("no circuit of the population has the wanted form")
    circuit, values = circuits[pick], params[pick]
    times = {"host": [], "device": []}
    same_states = True
    worst = 0.0
    for rnd in range(args.warm + args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want_states, want_probs = host_top(device, circuit, values, args.k)
        t1 = time.perf_counter()
        states, probs, _ = device.top_states([circuit], [values], args.k)
        t2 = time.perf_counter()
        if rnd >= args.warm:
            times["host"].append(t1 - t0)
            times["device"].append(t2 - t1)
        same_states = same_states and bool(np.array_equal(states[0], want_states))
        worst = max(worst, float(np.abs(np.sort(probs[0]) - np.sort(want_probs)).max()))
    out = {"n": args.n, "k": args.k, "split": bool(args.split), "circuit": pick, "rounds": args.rounds, "same_states": same_states,
           "worst_probability_difference": worst}
    for variant, t in times.items():
        med = float(np.median(t))
        out[variant] = {"median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3, "spread": (max(t) - min(t)) / med}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[n for n, _ in CONFIGURATIONS])
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds one configuration's child process may take")
    ap.add_argument("--child", action="store_true", help="(one configuration's measurement, as JSON on the last line)")
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--split", type=int, default=1)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r13_top_states.txt")
    args = ap.parse_args()
    if args.rounds < 11:
        raise SystemExit("at least eleven timed rounds")
    if args.child:
        print(json.dumps(measure(args)))
        return

    lines = [f"the k most probable basis states of one circuit ({args.layers} layers, seed-0 population, fp64): host = probabilities() + "
             f"numpy.argpartition + lexsort of the k, device = top_states; {args.warm} warm-up and {args.rounds} timed rounds, "
             "variants interleaved in one process per configuration",
             f"{'n':>3s} {'route':>6s} {'k':>5s} {'variant':>7s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'spread':>7s} {'vs host':>8s}"]
    results = []
    for n, split in CONFIGURATIONS:
        if n not in args.sizes:
            continue
        for k in KS:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, str(Path(__file__).resolve()), "--child", f"--n={n}",
                   f"--k={k}", f"--split={int(split)}", f"--layers={args.layers}", f"--rounds={args.rounds}", f"--warm={args.warm}"]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if res.returncode != 0:
                raise SystemExit(f"n = {n}, k = {k}: the measurement ended with status {res.returncode}\n{res.stdout[-2000:]}")
            r = json.loads(res.stdout.strip().splitlines()[-1])
            results.append(r)
            for variant in ("host", "device"):
                row = r[variant]
                lines.append(f"{n:3d} {'split' if split else 'state':>6s} {k:5d} {variant:>7s} {row['median_ms']:10.3f} {row['min_ms']:9.3f} "
                             f"{row['max_ms']:9.3f} {row['spread']:7.3f} {row['median_ms'] / r['host']['median_ms']:8.3f}")
            lines.append(f"    circuit {r['circuit']}: the two answers name the same states in the same order: {r['same_states']}; "
                         f"largest difference of their sorted probabilities {r['worst_probability_difference']:.3g}")
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(results))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
