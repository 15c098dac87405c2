"""Generators for the large-batch GPU tests (tests only): host-list batches in which one push holds more evaluations than its
lane has slots.  The documented call -- every shifted point of the full gradient of the mixed-depth n = 17 population of
tests/test_gpu_gradients.py, 2170 evaluations, in ONE ``evaluate_circuits`` call -- and the bounds of the pushes the two
host-list feeds cut a batch into."""

from __future__ import annotations

import numpy as np

import helpers
import shift_rules

DOCUMENTED_N = 17
DOCUMENTED_EVALUATIONS = 2170


def mixed_depths(n, seed=0):
    """``test_gpu_gradients._mixed``: layers (2, 2), (4, 2), (6, 1), (9, 1), seeds ``seed + layers``."""
    circuits, params = [], []
    for layers, count in ((2, 2), (4, 2), (6, 1), (9, 1)):
        _, c, p = helpers.population_circuits(n, layers, count, seed=seed + layers)
        circuits += c
        params += p
    return circuits, params


def documented_call():
    """(operator, circuits, points per circuit) of the call DESIGN.md 4.10 records."""
    circuits, params = mixed_depths(DOCUMENTED_N)
    op = helpers.random_ising_operator(DOCUMENTED_N, seed=DOCUMENTED_N)
    points = [shift_rules.shifted_points(c.gradient_terms(), p) for c, p in zip(circuits, params)]
    return op, circuits, points


def flatten(circuits, points):
    """Structures in blocks: (circuit of every evaluation, its point, the index of its circuit)."""
    flat_c, flat_p, owner = [], [], []
    for e, (c, pts) in enumerate(zip(circuits, points)):
        flat_c += [c] * len(pts)
        flat_p += pts
        owner += [e] * len(pts)
    return flat_c, flat_p, owner


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def hex_line(values) -> str:
    return " ".join(f"{int(b):016x}" for b in bits(values))


def from_hex_line(line: str) -> np.ndarray:
    return np.asarray([int(w, 16) for w in line.split()], dtype=np.uint64)


def helper_bounds(n: int, pushes: int) -> list[int]:
    """The pushes of the default helper path (csrc/pyhelp.c, expectation_values): steps of max(8, ceil(n / pushes))."""
    step = max(8, -(-n // max(1, pushes)))
    return list(range(0, n, step)) + [n]


def plan_bounds(n: int, plan) -> list[int]:
    """The pushes of the ctypes path under QSV_PUSH_PLAN (StatevectorDevice.expectation_values): the plan's sizes, the last
    one repeated until the batch is through."""
    bounds, acc = [0], 0
    for size in plan:
        acc = min(n, acc + size)
        bounds.append(acc)
    while bounds[-1] < n:
        bounds.append(min(n, bounds[-1] + plan[-1]))
    return [b for i, b in enumerate(bounds) if i == 0 or b > bounds[i - 1]]


def failure_table(calls, want, owner, routes, bounds, limit=None) -> str:
    """call, push, position in push, circuit, route, got, want of every evaluation whose bits differ (``calls``: name -> values;
    ``limit``: at most so many rows per call)."""
    want_bits = bits(want)
    starts = np.asarray(bounds[:-1])
    lines = []
    for name, got in calls.items():
        bad = np.nonzero(bits(got) != want_bits)[0]
        lines.append(f"{name}: {bad.size} of {want_bits.size} evaluations differ, the first at {bad[:1].tolist()}, the last at {bad[-1:].tolist()}")
        for i in bad[:limit]:
            push = int(np.searchsorted(starts, i, side="right")) - 1
            lines.append(f"  call {name}  push {push}  position {int(i) - bounds[push]:5d}  circuit {owner[i]}  "
                         f"route {routes[owner[i]]!r}  got {float(np.asarray(got)[i])!r}  want {float(np.asarray(want)[i])!r}")
    return "\n".join(lines)


# ---- the regime at the smallest shapes --------------------------------------------------------------------------------------
# An arm is one device: its register, its launch group and the QSV_SIDE_SLOTS it is created under.  With two lanes a push
# has group // 2 state slots and side_slots // 2 side-table slots.

DEFAULT_SIDE_SLOTS = 256  # (csrc/qsv_api.hip, qsv_create)
WAYS = 2                  # lanes of a batch under a diagonal operator with the default streams

ARMS = {
    # one tile a state: the only route the other arms cannot reach
    "n12": {"n": 12, "group": 3, "side_slots": 8, "dtype": "fp64", "mixes": ("one tile",)},
    # the smallest register with both a split route and gate passes: ONE state slot and four side-table slots a lane
    "n14": {"n": 14, "group": 3, "side_slots": 8, "dtype": "fp64", "mixes": ("split", "split+passes", "kept")},
    "n14-fp32": {"n": 14, "group": 3, "side_slots": 8, "dtype": "fp32", "mixes": ("split+passes",)},
    # the default slots, at the documented call's size
    "n17": {"n": 17, "group": 0, "side_slots": None, "dtype": "fp64", "mixes": ("split", "split+passes")},
    # the one-launch route, half sides among its circuits
    "n20": {"n": 20, "group": 0, "side_slots": None, "dtype": "fp64", "mixes": ("strata",)},
}
ORDERS = ("blocks", "round-robin")
SIZES = ("one less", "exactly", "one more", "4.3 times")
CASES = [(arm, mix, order, size) for arm, spec in ARMS.items() for mix in spec["mixes"] for order in ORDERS for size in SIZES]
CLIENT_CASES = [case for case in CASES if case[0] in ("n14", "n17")]


def case_id(case) -> str:
    return "-".join(case).replace(" ", "_")


def count_for(unit: int, size: str) -> int:
    """Evaluations of one kind: relative to ``unit`` = ways * slots of the kind."""
    return {"one less": unit - 1, "exactly": unit, "one more": unit + 1, "4.3 times": int(round(4.3 * unit))}[size]


def units(group: int, side_slots: int) -> dict:
    """ways * slots per kind of evaluation.  Ordinary evaluations and those on kept states share the state slots; at least 8,
    the smallest push the helper path makes (with ONE state slot a lane a unit of 2 would leave batches of one evaluation)."""
    ordinary = max(WAYS * (group // WAYS), 8)
    return {"split": WAYS * (side_slots // WAYS), "ordinary": ordinary, "kept": ordinary}


def candidates(n: int):
    """(label, circuit) pool an arm picks its structures from by route: EVQE individuals of two to nine layers; at n = 20 the
    population of ``test_gpu_gradients._strata_population``."""
    blocks = ((4, 64, 0), (6, 12, 0), (9, 2, 8)) if n == 20 else tuple((L, 6, 100 * n + L) for L in (2, 3, 4, 6, 9))
    out = []
    for layers, count, seed in blocks:
        _, circuits, _ = helpers.population_circuits(n, layers, count, seed=seed)
        out += [(f"L{layers}#{i}", c) for i, c in enumerate(circuits)]
    return out


def points_for(label: str, circuit, count: int, salt: int = 0) -> list[list[float]]:
    """``count`` parameter vectors of a structure, a function of its label alone (the same in every arm, mix and order)."""
    import zlib

    rng = np.random.default_rng(zlib.crc32(repr((label, salt)).encode()))
    return rng.uniform(-np.pi, np.pi, size=(count, circuit.num_parameters)).tolist()


def deal(per_structure: list[int], order: str) -> list[tuple[int, int]]:
    """(structure, index of its point) of every evaluation: structures in blocks, or the same evaluations dealt round-robin."""
    if order == "blocks":
        return [(s, k) for s, m in enumerate(per_structure) for k in range(m)]
    out = []
    for k in range(max(per_structure)):
        out += [(s, k) for s, m in enumerate(per_structure) if k < m]
    return out


def uneven_plan(n: int, slots: int) -> list[int]:
    """QSV_PUSH_PLAN ``1, 2 * slots + 1, rest``."""
    return [1, 2 * slots + 1, max(1, n - 2 * slots - 2)]


def kinds_per_push(bounds, kinds) -> list[dict]:
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        part = kinds[a:b]
        out.append({k: part.count(k) for k in ("split", "ordinary", "kept")})
    return out
