"""The parameter-shift rules of include/qsv.h restated in NumPy (tests only): the shifted points of a gradient and the
combination of their values, with the documented constants, order and association."""

from __future__ import annotations

import math

import numpy as np

S1 = math.pi / 2  # M_PI_2
S3 = 3.0 * S1
CP = (math.sqrt(2.0) + 1.0) / (4.0 * math.sqrt(2.0))
CM = (math.sqrt(2.0) - 1.0) / (4.0 * math.sqrt(2.0))
SHIFTS = (S1, -S1, S3, -S3)  # a parameter's evaluations, in order


def shifted_points(terms, params, wrt=None) -> list[list[float]]:
    """The points a gradient by ``wrt`` (None: every parameter) evaluates, in the documented order; ``terms`` is the circuit's
    shift plan.  Every point is ``params`` with one entry replaced by one fp64 sum."""
    base = np.asarray(params, dtype=np.float64)
    points = []
    for p in range(len(terms)) if wrt is None else wrt:
        assert terms[p] >= 0, f"parameter {p} has no shift rule"
        for shift in SHIFTS[: terms[p]]:
            point = base.copy()
            point[p] = base[p] + np.float64(shift)
            points.append(point.tolist())
    return points


def combine(terms, values, wrt=None) -> np.ndarray:
    """The gradient entries from the values at :func:`shifted_points`, every product and difference rounded on its own."""
    v = np.asarray(values, dtype=np.float64)
    out, cur = [], 0
    for p in range(len(terms)) if wrt is None else wrt:
        t = terms[p]
        if t == 0:
            out.append(np.float64(0.0))
        elif t == 2:
            out.append(np.float64(0.5) * (v[cur] - v[cur + 1]))
        else:
            out.append(np.float64(CP) * (v[cur] - v[cur + 1]) - np.float64(CM) * (v[cur + 2] - v[cur + 3]))
        cur += t
    assert cur == len(v)
    return np.asarray(out, dtype=np.float64)
