"""Planner and splitter on circuits outside the EVQE genome's shape (tests/circuit_families.py), on the CPU: every plan is
executed by tests/plan_interpreter.py and every split form by tests/test_split.py's NumPy contraction, against the oracle.
The coverage test keeps the families in the regimes they are here for: chains of kMaxChain factors, passes of many rounds,
plans of many passes, rounds of many entries, multiplexed entries.  The GPU half is tests/test_gpu_circuit_families.py."""

import numpy as np
import pytest

import circuit_families as cf
import helpers
import plan_interpreter as pi
import test_split
from queasars_amd.planning import build_plan_words

SIZES = (2, 3, 6, 9, 13, 14)
GENERIC_OPS = (5, 40, 200, 600)
GEOMETRIES = [{}, dict(tile_bits=8, reg_bits=2, low_bits=2), dict(tile_bits=10, reg_bits=3, low_bits=3),
              dict(tile_bits=7, reg_bits=2, low_bits=2)]
AMP_TOL = 1e-12

_CACHE: dict = {}


def family_circuits(n: int):
    """[(name, circuit, parameter list)]: every family at n qubits, ``generic`` at every op count; made once per size."""
    if n not in _CACHE:
        made = [("ladder", cf.ladder(n, 2, False)), ("ladder reversed", cf.ladder(n, 2, True)), ("star", cf.star(n, False)),
                ("fan-in", cf.star(n, True)), ("all_pairs", cf.all_pairs(n, 1)), ("rotation_runs", cf.rotation_runs(n)),
                ("ping_pong", cf.ping_pong(n)), ("two_blocks", cf.two_blocks(n, 2))]
        made += [(f"generic {m}", cf.generic(n, m)) for m in GENERIC_OPS]
        _CACHE[n] = [(name, c, p, helpers.oracle_state(c, p)) for name, (c, p) in made]
    return _CACHE[n]


@pytest.mark.parametrize("n", SIZES)
def test_plans_of_every_family_reproduce_the_circuit(n):
    """plan_interpreter.run within 1e-12 of the oracle and no LDS bank conflict, in the default geometry and in three small-tile
    ones (compact first passes, many passes) where the register is at least a tile."""
    for name, c, p, want in family_circuits(n):
        for cfg in GEOMETRIES:
            if cfg and n < cfg["tile_bits"]:
                continue
            stats = {}
            got = pi.run(build_plan_words(c, **cfg), n, p, stats)
            assert np.abs(got - want).max() < AMP_TOL, (name, cfg)
            assert stats["conflicts"] == 0, (name, cfg)


@pytest.mark.parametrize("n", SIZES)
def test_split_forms_of_every_family_reproduce_the_circuit(n):
    """test_split.check (the virtual circuits through the oracle's gate application, contracted in NumPy: 1e-13 of the
    oracle's state) at three size limits; families that are products or two blocks must split at the widest."""
    split = {}
    for name, c, p, _ in family_circuits(n):
        for max_side in sorted({n // 2 + 1, n // 2 + 2, n - 1}):
            k = test_split.check(c, p, max_side)
            if k is not None:
                split[name] = k
    if n >= 6:
        assert {"rotation_runs", "ping_pong", "two_blocks"} <= set(split), split
        assert split["rotation_runs"] == 0 and split["ping_pong"] == 0 and split["two_blocks"] >= 1, split


@pytest.mark.parametrize("bridges,seed", [(1, 0), (2, 0), (3, 0)])
def test_two_blocks_of_twenty_qubits_cut_at_their_bridges(bridges, seed):
    """two_blocks(20, b) under a limit of 13 qubits a side: b keys (each bridge control is one key, used once or twice)."""
    c, p = cf.two_blocks(20, bridges, seed)
    got = test_split.describe(c, 13)
    assert got is not None and got[0] == bridges, got and got[:2]
    assert got[1] in ((1 << 10) - 1, ((1 << 10) - 1) << 10), bin(got[1])


def test_the_families_leave_the_genomes_regime():
    """Conditions, not measurements: over the circuits of this file some entry is a chain of exactly kMaxChain factors and none
    is longer, some pass has 64 rounds or more, some plan five passes or more, some round sixteen entries or more, some plan
    negated entries; rotation_runs alone reaches every chain length 1 .. kMaxChain."""
    rows = []
    for n in SIZES:
        for name, c, _, _ in family_circuits(n):
            rows.append((n, name, cf.plan_stats(c)))
    print()
    for n, name, s in rows:
        print(f"n = {n:2d} {name:16s} chain {s['longest_chain']} rounds {s['rounds_in_one_pass']:3d} passes {s['passes']} "
              f"entries {s['entries_in_one_round']:2d} factors {s['n_factors']:3d} folds {s['n_fold']:2d} negated {s['negated']}")
    stats = [s for _, _, s in rows]
    assert max(s["longest_chain"] for s in stats) == pi.MAX_CHAIN
    assert max(s["rounds_in_one_pass"] for s in stats) >= 64
    assert max(s["passes"] for s in stats) >= 5
    assert max(s["entries_in_one_round"] for s in stats) >= 16
    assert any(s["negated"] for s in stats)
    runs = [s for n, name, s in rows if name == "rotation_runs" and n >= 9]
    assert runs and all(s["chain_lengths"] == list(range(1, pi.MAX_CHAIN + 1)) for s in runs), runs
    assert max(s["n_factors"] for s in stats) > cf.PREP_MAX_TRIG and max(s["n_factors"] for s in stats if s["passes"] >= 5) > 128


@pytest.mark.parametrize("shape", list(cf.STAGING_SHAPES))
def test_staging_reaches_each_boundary_shape(shape):
    """The generator reaches every shape of prepare_eval's three staging regimes, in the plan of the whole circuit (n = 10) and
    in the plan of one side of a split circuit (n = 14, two keys), and each circuit's plan and split form reproduce the oracle."""
    n_fold, n_trig, n_params = cf.STAGING_SHAPES[shape]
    staged = n_params <= cf.PREP_MAX_PARAMS and n_fold <= cf.PREP_MAX_FOLD
    print(f"\n{shape}: parameters and folds staged: {staged}, sines and cosines staged: {staged and n_trig <= cf.PREP_MAX_TRIG}")
    c, p = cf.staging(10, n_fold, n_trig - n_fold, n_params)
    plan = pi.decode(build_plan_words(c))
    assert (plan["n_fold"], plan["n_factors"] + plan["n_fold"], c.num_parameters, len(p)) == (n_fold, n_trig, n_params, n_params)
    assert np.abs(pi.run(plan["words"], 10, p) - helpers.oracle_state(c, p)).max() < AMP_TOL
    c, p = cf.staging(14, n_fold, n_trig - n_fold, n_params, bridges=2)
    assert cf.side_plan_counts(c) == (n_fold, n_trig - n_fold) and c.num_parameters == n_params == len(p)
    assert test_split.check(c, p, 12) == 2
    assert np.abs(pi.run(build_plan_words(c), 14, p) - helpers.oracle_state(c, p)).max() < AMP_TOL


def test_staging_shapes_are_the_limits_of_prepare_eval():
    """The shapes sit where the kernel's constants put the regimes (kernels.hip kPrepMaxParams, kPrepMaxFold, kPrepMaxTrig)."""
    import re
    from pathlib import Path

    text = (Path(cf.__file__).resolve().parent.parent / "queasars_amd" / "csrc" / "kernels.hip").read_text()
    m = re.search(r"kPrepMaxParams = (\d+), kPrepMaxFold = (\d+), kPrepMaxTrig = (\d+);", text)
    assert m and tuple(int(x) for x in m.groups()) == (cf.PREP_MAX_PARAMS, cf.PREP_MAX_FOLD, cf.PREP_MAX_TRIG)
    s = cf.STAGING_SHAPES
    assert s["256 trig entries"][1] == cf.PREP_MAX_TRIG and s["257 trig entries"][1] == cf.PREP_MAX_TRIG + 1
    assert s["128 folds"][0] == cf.PREP_MAX_FOLD and s["129 folds"][0] == cf.PREP_MAX_FOLD + 1
    assert s["1024 parameters"][2] == cf.PREP_MAX_PARAMS and s["1025 parameters"][2] == cf.PREP_MAX_PARAMS + 1
    for name in ("256 trig entries", "257 trig entries"):  # (the middle regime: parameters and folds staged, trig alone decides)
        assert s[name][0] <= cf.PREP_MAX_FOLD and s[name][2] <= cf.PREP_MAX_PARAMS
    for name in ("128 folds", "129 folds", "1024 parameters", "1025 parameters"):
        assert s[name][1] <= cf.PREP_MAX_TRIG
    assert all(a > b for a, b in zip(s["everything over"], (cf.PREP_MAX_FOLD, cf.PREP_MAX_TRIG, cf.PREP_MAX_PARAMS)))
