"""Sharded runs on real evaluators: two ranks (gloo for the set-up, both on GPU 0) through queasars_amd.distributed with shares
the cost model deals UNEVENLY, on every kind of evaluator the node's shared table serves, and the sharded solver against the
single-process one.

Populations.  n = 14 (the smallest register wider than the twelve-qubit tile: split forms and gate passes both occur), three-
layer individuals with eight-layer ones at ``DEEP_AT``.  The cost model prices by ROUTE, not by depth: at fourteen qubits a
three-layer circuit splits (1.2 us) and an eight-layer one takes two gate passes over a 2^14 state (0.16 us; 0.08 us on an fp32
handle), so a deep individual is the CHEAP one here and one or two of them among twelve leave the contiguous blocks within
10 % of even or the dealt shares within one of each other; it takes three for shares that differ by two (5 + 7: five shallow
against four shallow and three deep).  Each scenario asserts that of the shares it was really dealt.

Every scenario is held to (a) the same list on every rank, (b) the bits of ONE unsharded ``evaluate_circuits`` of the whole
population on a fresh evaluator in this process -- a value is "a property of the circuit and the handle, never of the batch",
which tests/test_gpu_differential.py holds fp32 handles and the exact CVaR to as well, so neither is excused here --, and (c) the
NumPy / C oracle within the project's bounds (``EXP_TOL``; ``FP32_REL * sum |c_k|`` on an fp32 handle).
"""

from __future__ import annotations

import gc
import os
import pickle
import socket
import sys
from datetime import timedelta
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu

EXP_TOL = 1e-10   # (tests/test_gpu_differential.py)
FP32_REL = 2e-6
WORLD = 2
N = 14
DEEP_AT = (1, 4, 5)     # where a population has eight-layer individuals (those that fit it) ...
DEEP_SEEDS = (1, 2, 3)  # ... and the populations they are the first individuals of
# (individuals, seed) per step through one evaluator: a rank without work (1), fewer circuits than a slot's earlier steps
# filled (2, 1, 5), the dealt population (12) twice in a row -- the same objects: the remembered shares -- and both halves of
# the double-buffered table several times over
STEPS = ((9, 40), (2, 41), (1, 42), (12, 43), (12, 43), (5, 45))
DEALT = 3  # the step whose shares must be uneven and not contiguous
SCENARIOS = {  # name -> the spawn it runs in
    "ising": 0, "general": 0, "matrix": 0,
    "fp32": 1, "initial": 1, "sampler": 1,
}
ALPHA = 0.3


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def mixed_population(count: int, seed: int):
    import helpers

    _, circuits, params = helpers.population_circuits(N, 3, count, seed=seed)
    for at, deep_seed in zip(DEEP_AT, DEEP_SEEDS):
        if at < count:
            _, deep_c, deep_p = helpers.population_circuits(N, 8, 1, seed=deep_seed)
            circuits[at], params[at] = deep_c[0], deep_p[0]
    return circuits, params


def _populations():
    made = {}
    return [made.setdefault(step, mixed_population(*step)) for step in STEPS]


def _operator(name: str):
    import helpers

    return helpers.random_pauli_operator(N, 40, seed=11) if name == "general" else helpers.random_ising_operator(N, seed=7)


def _initial_state():
    from queasars_amd.ir import CircuitIR

    initial = CircuitIR(N)
    for q in range(N):
        initial.u(0.3 + 0.1 * q, 0.2, 0.1 * q, q)
    initial.cu3(0.4, 0.1, 0.9, 0, N - 1)
    return initial


def _evaluator(name: str):
    from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator, OperatorSamplerCircuitEvaluator

    op = _operator(name)
    if name == "sampler":  # (the exact distribution: no shots, deterministic)
        return OperatorSamplerCircuitEvaluator(None, op, alpha=ALPHA, device=0)
    if name == "fp32":
        return OperatorCircuitEvaluator(op, dtype="fp32", device=0)
    if name == "initial":
        return OperatorCircuitEvaluator(op, initial_state_circuit=_initial_state(), device=0)
    return OperatorCircuitEvaluator(op, device=0)


def _device_matrix(params):
    import torch

    host = np.zeros((len(params), max(len(p) for p in params)))
    for row, p in zip(host, params):
        row[: len(p)] = p
    return torch.from_numpy(host).cuda()


def _start(rank: int, port: int):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)  # (both ranks on the one GPU of the box: the table is host memory, every GPU is given it alike)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=timedelta(seconds=60))


def _evaluation_worker(rank: int, port: int, names: list, out_dir: str):
    _start(rank, port)
    import torch
    import torch.distributed as dist

    from queasars_amd import distributed

    try:
        populations = _populations()
        out = {}
        steps_before = 0
        for name in names:
            evaluator = _evaluator(name)
            calls = {"kernels": 0, "refused": 0, "host": 0}
            evaluate = evaluator.evaluate_circuits

            def host(circuits, parameter_values, evaluate=evaluate, calls=calls):
                calls["host"] += 1
                return evaluate(circuits, parameter_values)

            evaluator.evaluate_circuits = host
            to_device = getattr(evaluator, "evaluate_circuits_to_device", None)
            if to_device is not None:
                def kernels(circuits, parameter_values, pointer, to_device=to_device, calls=calls):
                    started = to_device(circuits, parameter_values, pointer)
                    calls["kernels" if started else "refused"] += 1
                    return started

                evaluator.evaluate_circuits_to_device = kernels
            matrices = {}
            values, shares = [], []
            for step, (circuits, params) in zip(STEPS, populations):
                if name == "matrix":  # (ONE matrix per population in this rank's device memory; the second visit reads it again)
                    if step not in matrices:
                        matrices[step] = _device_matrix(params)
                    params = matrices[step]
                values.append(distributed.evaluate_population_sharded(evaluator, circuits, params))
                shares.append(distributed.population_shares(evaluator, circuits, WORLD))  # (the remembered ones: nothing is asked)
            table = distributed._node_table(None, WORLD, rank, torch.device("cuda", 0))
            assert table is not None and table.registered, "the GPU was given the node's shared table"
            assert table.step - steps_before == len(STEPS), "every step went through the table"
            steps_before = table.step
            through_table = dict(calls)
            # one step through the collective instead: the same bits
            circuits, params = populations[DEALT]
            os.environ["QSV_GATHER_NODE"] = "0"
            try:
                collective = distributed.evaluate_population_sharded(evaluator, circuits, matrices.get(STEPS[DEALT], params))
            finally:
                del os.environ["QSV_GATHER_NODE"]
            assert table.step == steps_before and calls["host"] == through_table["host"] + 1
            out[name] = {"values": values, "shares": shares, "calls": through_table, "collective": collective}
        with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
            pickle.dump(out, f)
    finally:
        dist.destroy_process_group()


_SPAWNED: dict = {}


def _spawned(key, worker, args, tmp_path_factory):
    """What the ranks of one spawn left (a list by rank), spawned on first use; a spawn that failed is not tried again."""
    if key not in _SPAWNED:
        out = tmp_path_factory.mktemp(f"sharded_{key}")
        try:
            mp.spawn(worker, args=(_free_port(), *args, str(out)), nprocs=WORLD, join=True)
            ranks = []
            for rank in range(WORLD):
                with open(out / f"rank{rank}.pkl", "rb") as f:
                    ranks.append(pickle.load(f))
            _SPAWNED[key] = ranks
        except BaseException as exc:
            _SPAWNED[key] = exc
            raise
    if isinstance(_SPAWNED[key], BaseException):
        raise RuntimeError(f"the ranks of spawn {key!r} failed earlier") from _SPAWNED[key]
    return _SPAWNED[key]


_ORACLE: dict = {}


def _oracle_values(name: str, c_oracle):
    """The oracle's value of every evaluation of the scenario's steps, computed once per (operator, initial state, quantity)."""
    from oracle import statevector_oracle as so

    kind = name if name in ("general", "initial", "sampler") else "ising"
    if kind not in _ORACLE:
        op = _operator(name)
        table = None if kind == "general" else c_oracle.diagonal_table(op)
        initial = _initial_state() if kind == "initial" else None
        scratch = np.zeros(2 << N)
        by_population = {}
        for step, (circuits, params) in zip(STEPS, _populations()):
            if step in by_population:
                continue
            want = []
            for circuit, p in zip(circuits, params):
                if kind == "sampler":
                    probabilities = np.abs(c_oracle.simulate(circuit, p)) ** 2
                    want.append(so.cvar_expectation(list(zip(range(1 << N), probabilities.tolist(), table.tolist())), ALPHA))
                else:
                    want.append(c_oracle.evaluate(initial.compose(circuit) if initial is not None else circuit, p, op, table, scratch))
            by_population[step] = want
        _ORACLE[kind] = [by_population[step] for step in STEPS]
    return _ORACLE[kind]


def _contiguous(share) -> bool:
    return list(share) == list(range(share[0], share[0] + len(share))) if share else True


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_sharded_evaluation_with_uneven_shares(name, tmp_path_factory, c_oracle):
    """One evaluator through ``STEPS`` on two ranks, then the dealt step once more through the collective (in the ranks: the
    table registered with HIP, one table step per evaluation, the collective's values the table's bits).

    ising    an Ising operator: the kernels store each value into the rank's slot
    general  forty Pauli strings: the values reach the slot by the copy out of the handle's result buffer
    matrix   the Ising evaluator reading ONE matrix in the rank's device memory: a dealt share is gathered from it by
             ``index_select`` on torch's stream before the evaluator's stream reads it
    fp32     a single-precision handle
    initial  circuits composed behind an initial state (their costs are the composed circuits': some shallow ones no longer split)
    sampler  the exact CVaR (alpha = 0.3): no ``evaluate_circuits_to_device`` and no ``circuit_costs`` -- the host writes the
             slot, and the shares are the contiguous blocks
    """
    from queasars_amd.distributed import contiguous_shares

    group = SCENARIOS[name]
    ranks = _spawned(group, _evaluation_worker, ([k for k, g in SCENARIOS.items() if g == group],), tmp_path_factory)
    got = [rank[name] for rank in ranks]
    populations = _populations()
    # the shares: the same on every rank, a partition, and on the dealt step uneven and not contiguous
    assert got[0]["shares"] == got[1]["shares"]
    for (count, _), shares in zip(STEPS, got[0]["shares"]):
        assert sorted(i for share in shares for i in share) == list(range(count))
    dealt = got[0]["shares"][DEALT]
    print(f"\n{name}: shares by step {[[len(s) for s in shares] for shares in got[0]['shares']]}, dealt step {dealt}, "
          f"calls {[g['calls'] for g in got]}")
    if name == "sampler":  # (no circuit_costs: nothing to deal by)
        assert all(shares == contiguous_shares(count, WORLD) for (count, _), shares in zip(STEPS, got[0]["shares"]))
    else:
        assert abs(len(dealt[0]) - len(dealt[1])) >= 2, dealt
        assert not all(_contiguous(share) for share in dealt), dealt
    assert got[0]["shares"][DEALT + 1] == dealt  # (the same objects again: the remembered shares)
    assert [] in got[0]["shares"][2], "a rank without work"
    # who wrote the slots: the kernels wherever the evaluator can leave its values on the device, else the host -- never both
    for rank, g in enumerate(got):
        busy = sum(1 for shares in g["shares"] if shares[rank])
        want = {"kernels": 0, "refused": 0, "host": busy} if name == "sampler" else {"kernels": busy, "refused": 0, "host": 0}
        assert g["calls"] == want, (rank, g["calls"])
    # (a) every rank has the same list, and the collective's bits are the table's
    assert got[0]["values"] == got[1]["values"]
    for g in got:
        assert g["collective"] == g["values"][DEALT]
    # (b) the bits of one unsharded call on a fresh evaluator
    evaluator = _evaluator(name)
    try:
        for step, (circuits, params), values in zip(STEPS, populations, got[0]["values"]):
            assert values == evaluator.evaluate_circuits(circuits, params), (name, step)
    finally:
        evaluator.statevector_device.close()
    # (c) the oracle
    op = _operator(name)
    bound = FP32_REL * float(np.abs(op.coeffs).sum()) if name == "fp32" else EXP_TOL
    worst = max(float(np.abs(np.asarray(values) - np.asarray(want)).max())
                for values, want in zip(got[0]["values"], _oracle_values(name, c_oracle)))
    print(f"{name}: worst |value - oracle| {worst:.3e} (bound {bound:.3e})")
    assert worst < bound, (name, worst)


# ---- the sharded solver against the single-process solver -----------------------------------------------------------------

# (name, device_resident_search, QSV_KEPT_STATES)
SOLVER_RUNS = (("host", False, "0"), ("device", True, "0"), ("kept", False, "1"))
# the initial population's deep individuals, index -> (layers, seed, which): one that splits on five keys (priced 5 us against
# a two-layer individual's 1.2: its rank takes little else) and one that takes gate passes (the kind a search keeps a state for)
SOLVER_DEEP = {1: (8, 8, 0), 5: (8, 1, 0)}


def _solve(shard: bool):
    """The three runs, each on a fresh evaluator: name -> (numbers of the result, (jobs, own share) per sharded search, kept
    states per search)."""
    import helpers
    from queasars_amd import distributed
    from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator
    from queasars_amd.evqe.solver import SPSA, EVQEMinimumEigensolver, EVQEMinimumEigensolverConfiguration

    op = helpers.random_ising_operator(N, seed=5)
    dealt, kept = [], []
    deal, keep = distributed.shard_searches, EVQEMinimumEigensolver._kept_state_circuits

    def recorded_deal(evaluator, jobs, group=None):
        mine = deal(evaluator, jobs, group)
        dealt.append((len(jobs), len(mine)))
        return mine

    def recorded_keep(self, evaluator, individuals, layer_ids):
        circuits = keep(self, evaluator, individuals, layer_ids)
        kept.append(len(circuits))
        return circuits

    out = {}
    distributed.shard_searches, EVQEMinimumEigensolver._kept_state_circuits = recorded_deal, recorded_keep
    before = os.environ.get("QSV_KEPT_STATES")
    try:
        for name, on_device, kept_states in SOLVER_RUNS:
            os.environ["QSV_KEPT_STATES"] = kept_states
            del dealt[:], kept[:]
            evaluator = OperatorCircuitEvaluator(op, device=0)
            cfg = EVQEMinimumEigensolverConfiguration(
                optimizer=SPSA(maxiter=6, learning_rate=0.4, perturbation=0.3), population_size=8, max_generations=3, random_seed=1,
                n_initial_layers=2, randomize_initial_population_parameters=True, speciation_genetic_distance_threshold=2,
                use_tournament_selection=True, tournament_size=2, selection_alpha_penalty=0.1, selection_beta_penalty=0.1,
                parameter_search_probability=0.5, topological_search_probability=0.5, layer_removal_probability=0.05,
                device_resident_search=on_device)
            with helpers.deep_seed_individuals(SOLVER_DEEP):
                result = EVQEMinimumEigensolver(cfg, shard=shard).compute_minimum_eigenvalue(evaluator)
            gc.collect()
            assert evaluator.statevector_device.kept_state_count() == 0, "a search's kept states are released when it ends"
            numbers = {"best": list(result.best_expectation_values), "eigenvalue": result.eigenvalue,
                       "x": list(result.best_individual.parameter_values), "evaluations": list(result.circuit_evaluations)}
            out[name] = (numbers, list(dealt), list(kept))
            evaluator.statevector_device.close()
    finally:
        distributed.shard_searches, EVQEMinimumEigensolver._kept_state_circuits = deal, keep
        if before is None:
            del os.environ["QSV_KEPT_STATES"]
        else:
            os.environ["QSV_KEPT_STATES"] = before
    return out


def _solver_worker(rank: int, port: int, out_dir: str):
    _start(rank, port)
    import torch.distributed as dist

    try:
        out = _solve(shard=True)
        with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
            pickle.dump(out, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", [run[0] for run in SOLVER_RUNS])
def test_sharded_solver_is_the_single_process_solver(name, tmp_path_factory):
    """``EVQEMinimumEigensolver(shard=True)`` on two ranks with real evaluators -- layer searches dealt by cost, kept states made
    per rank and released before the gather, one gather per search, every scoring through the node's table -- against the same
    configuration in one process on the same GPU: best values per generation, eigenvalue, the best individual's parameter values
    and the evaluation counts, bit for bit, with the host driver, with device-resident searches and with kept states forced on
    (both sides keeping states: a kept-state evaluation is a property of the kept circuit, not of which rank made the state)."""
    ranks = _spawned("solver", _solver_worker, (), tmp_path_factory)
    if "single" not in _SPAWNED:
        _SPAWNED["single"] = _solve(shard=False)
    single, _, single_kept = _SPAWNED["single"][name]
    dealt = [rank[name][1] for rank in ranks]
    kept = [rank[name][2] for rank in ranks]
    print(f"\n{name}: (jobs, share of rank 0, of rank 1) per search {[(n, a, b) for (n, a), (_, b) in zip(*dealt)]}; "
          f"kept states per search: ranks {kept}, single process {single_kept}")
    # the searches were dealt unevenly: a share longer than ceil(jobs / ranks)
    assert [n for n, _ in dealt[0]] == [n for n, _ in dealt[1]] and all(a + b == n for (n, a), (_, b) in zip(*dealt))
    assert any(max(a, b) > -(-n // WORLD) for (n, a), (_, b) in zip(*dealt)), dealt
    # kept states: only in the run that asks for them, each rank for its own individuals, together the single process's
    assert [a + b for a, b in zip(*kept)] == single_kept
    assert (sum(single_kept) > 0) == (name == "kept")
    for rank in ranks:
        assert rank[name][0] == single, (name, rank[name][0], single)
