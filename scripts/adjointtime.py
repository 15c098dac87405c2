"""Time the adjoint gradients against parameter shift on one MI355X and write
profiles/r14_adjoint_gradients.txt.

  shapes     n = 20, L = 4 and n = 20, L = 8 (EVQE populations, the 210-term Ising operator's family), n = 24, L = 8, and
             config 5's genome at n = 28 (one circuit, four layers, 500 random Pauli strings) -- fewer individuals at the larger
             sizes (--individuals), so that a round stays in seconds
  subject    OperatorCircuitEvaluator.evaluate_gradients with gradient_method "adjoint" and "parameter_shift": the full
             gradient and the last layer's parameters (wrt), fp64 and fp32

Both methods of a shape run in ONE process, interleaved: --warm rounds first, then --rounds rounds of one call each; a time is
host wall time around a call that returns its gradients to the host.  Reported per variant: median, minimum and maximum, the
ratio of the medians (parameter shift / adjoint: above 1 the sweep wins), the evaluations parameter shift ran and the sweep's
counters (qsv_adjoint_stats), and the largest difference between the two methods' gradients.  Every figure is what this run
measured; where the sweep loses the table says so."""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from queasars_amd import workloads  # noqa: E402
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator  # noqa: E402
from queasars_amd.evqe import EVQEPopulation  # noqa: E402

SHAPES = {
    # name: (qubits, layers, default individuals, operator)
    "n20_L4": (20, 4, 16, "ising"),
    "n20_L8": (20, 8, 16, "ising"),
    "n24_L8": (24, 8, 4, "ising"),
    "n28_config5": (28, 4, 1, "pauli500"),
}


def workload(n: int, layers: int, individuals: int):
    pop = EVQEPopulation.random_population(n, layers, individuals, True, 0)
    circuits = [ind.get_parameterized_quantum_circuit() for ind in pop.individuals]
    params = [list(ind.parameter_values) for ind in pop.individuals]
    last = layers - 1
    layer = [list(range(ind.circuit_parameter_offsets[last], ind.circuit_parameter_offsets[last] + ind.layers[last].n_parameters))
             for ind in pop.individuals]
    return circuits, params, {"full": None, "last layer": layer}


def time_shape(name: str, individuals: int, rounds: int, warm: int, emit) -> None:
    n, layers, default_individuals, op_kind = SHAPES[name]
    individuals = individuals or default_individuals
    circuits, params, wrts = workload(n, layers, individuals)
    operator = workloads.random_ising_operator(n, seed=0) if op_kind == "ising" else workloads.random_pauli_operator(n, 500, seed=2028)
    emit(f"## {name}: n = {n}, {layers} layers, {individuals} circuit(s), {sum(c.num_parameters for c in circuits)} parameters, "
         f"{len(operator)} Pauli strings ({op_kind})")
    for dtype in ("fp64", "fp32"):
        methods = {m: OperatorCircuitEvaluator(operator, dtype=dtype, gradient_method=m) for m in ("adjoint", "parameter_shift")}
        routes = sorted({c["route"] for c in methods["adjoint"].circuit_costs(circuits)})
        for which, wrt in wrts.items():
            times = {m: [] for m in methods}
            results, counts = {}, {}
            for r in range(warm + rounds):
                for m, ev in methods.items():
                    t0 = time.perf_counter()
                    results[m] = ev.evaluate_gradients(circuits, params, wrt)
                    if r >= warm:
                        times[m].append(time.perf_counter() - t0)
                    counts[m] = ev.last_gradient_evaluations
            stats = methods["adjoint"].statevector_device.adjoint_stats()
            med = {m: float(np.median(t)) for m, t in times.items()}
            diff = max(float(np.abs(a - b).max(initial=0.0)) for a, b in zip(results["adjoint"], results["parameter_shift"]))
            ratio = med["parameter_shift"] / med["adjoint"]
            for m in methods:
                emit(f"  {dtype} {which:10s} {m:15s} median {med[m] * 1e3:10.3f} ms  min {min(times[m]) * 1e3:10.3f}  max {max(times[m]) * 1e3:10.3f}"
                     f"  evaluations {counts[m]}")
            emit(f"  {dtype} {which:10s} parameter shift / adjoint = {ratio:.3f} ({'the sweep wins' if ratio > 1 else 'the sweep LOSES'});"
                 f" routes {routes}; gates swept {stats['n_gates']}, run launches {stats['n_runs']}, state sweeps {stats['n_state_sweeps']},"
                 f" scratch {stats['scratch_bytes'] / 2**20:.1f} MiB; largest |difference| of the methods {diff:.3e}")
        for ev in methods.values():
            ev.statevector_device.close()


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    parser.add_argument("--individuals", type=int, default=0, help="circuits per shape (0: the shape's default)")
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--warm", type=int, default=1)
    parser.add_argument("--out", default=str(ROOT / "profiles" / "r14_adjoint_gradients.txt"))
    args = parser.parse_args()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)
        out.write_text("\n".join(lines) + "\n")

    emit("# adjoint gradients against parameter shift: scripts/adjointtime.py, one MI355X, host wall time per evaluate_gradients call")
    emit(f"# {args.warm} warm round(s), {args.rounds} timed rounds, the two methods interleaved; medians")
    for name in args.shapes:
        time_shape(name, args.individuals, args.rounds, args.warm, emit)


if __name__ == "__main__":
    main()
