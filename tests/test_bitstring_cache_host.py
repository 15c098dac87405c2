"""What the device-resident value cache of the BitstringCircuitEvaluator decides and checks without a device: the bindings of
``qsv_value_cache_*`` / ``qsv_sample_lookup*`` against the header, the claim the GPU tests' exact comparisons rest on (a dyadic
operator's values do not depend on the order of the sum), the ascending-order helper, and the constructor's checks."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from bitstring_cache_cases import dyadic_ising_operator
from queasars_amd import _lib
from queasars_amd.circuit_evaluation import BitstringCircuitEvaluator, BitstringEvaluator, ConfiguredSamplerV2, configured_primitives
from queasars_amd.circuit_evaluation import circuit_evaluation as ce
from queasars_amd.circuit_evaluation.expectation_calculation import basis_state_values
from queasars_amd.ir import PauliOperator

ROOT = Path(__file__).resolve().parent.parent

NAMES = ("qsv_value_cache_create", "qsv_value_cache_destroy", "qsv_value_cache_clear", "qsv_value_cache_stats",
         "qsv_sample_lookup", "qsv_sample_lookup_finish")


def test_the_bindings_match_the_header():
    """Every value-cache prototype of include/qsv.h has a binding with its arguments, kind by kind, and the library exports it."""
    text = (ROOT / "include" / "qsv.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
    declared_names = set(re.findall(r"int\s+(qsv_value_cache_\w+|qsv_sample_lookup\w*)\s*\(", text))
    assert declared_names == set(NAMES)
    lib = _lib.load()
    for name in NAMES:
        match = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert match, f"include/qsv.h does not declare {name}"
        declared = [" ".join(a.split()) for a in match.group(1).split(",")]
        assert name in _lib.SIGNATURES, f"_lib.py does not bind {name}"
        restype, argtypes = _lib.SIGNATURES[name]
        want = [C.c_void_p if "*" in a else kinds[a.rsplit(" ", 1)[0]] for a in declared]
        assert restype is C.c_int and len(argtypes) == len(declared) and argtypes == want, name
        assert hasattr(lib, name)
    assert lib.qsv_value_cache_create(None, 16, 24, None) == _lib.QSV_E_ARG  # (no handle)
    assert lib.qsv_sample_lookup(None, 1, 0, None, None, None, 0, 0, None, None) == _lib.QSV_E_ARG
    assert lib.qsv_sample_lookup_finish(None, 1, 0, None, 0.5, None, None) == _lib.QSV_E_ARG
    fields = [name for name, _ in _lib.QsvValueCacheStats._fields_]
    assert fields == ["entries", "slots", "samples_looked_up", "hits", "new_entries", "rehashes", "clears"]
    struct = re.search(r"typedef struct qsv_value_cache_stats_t \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"int64_t\s+(\w+);", struct) == fields


def test_a_dyadic_operators_values_do_not_depend_on_the_order_of_the_sum():
    n = 16
    op = dyadic_ising_operator(n, seed=11)
    assert op.is_diagonal() and np.all(op.coeffs.imag == 0)
    eighths = op.coeffs.real * 8
    assert np.all(eighths == np.round(eighths)) and np.all(eighths != 0) and np.abs(eighths).max() <= 16
    rng = np.random.default_rng(5)
    states = rng.integers(0, 1 << n, size=2000, dtype=np.uint64)
    labels, coeffs = list(op.labels), list(op.coeffs)
    given = basis_state_values(states, op)
    backwards = basis_state_values(states, PauliOperator(labels[::-1], coeffs[::-1]))
    perm = rng.permutation(len(labels))
    shuffled = basis_state_values(states, PauliOperator([labels[i] for i in perm], [coeffs[i] for i in perm]))
    assert np.array_equal(given, backwards) and np.array_equal(given, shuffled)
    assert len(np.unique(given)) > 100  # (not a degenerate operator)


def test_ascending_order_and_back():
    rng = np.random.default_rng(2)
    missing = rng.permutation(np.arange(5000, dtype=np.uint64) * np.uint64(977))[:1234]
    ordered, order = ce._ascending(missing)
    assert np.array_equal(ordered, np.sort(missing)) and np.array_equal(missing[order], ordered)
    values = ce._unpermuted([float(s) + 0.25 for s in ordered.tolist()], order)
    assert np.array_equal(values, missing.astype(np.float64) + 0.25)
    ordered, order = ce._ascending(np.empty(0, dtype=np.uint64))
    assert ordered.size == 0 and ce._unpermuted([], order).size == 0


def test_constructor_checks_come_before_any_device_call(monkeypatch):
    def no_device(*args, **kwargs):
        raise AssertionError("the check comes before the device")

    monkeypatch.setattr(ce, "StatevectorDevice", no_device)
    scorer = BitstringEvaluator(4, lambda b: float(b.count("1")))
    for flag in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="device_value_cache"):
            BitstringCircuitEvaluator(16, scorer, device_value_cache=flag)
    for alpha in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="alpha"):
            BitstringCircuitEvaluator(16, scorer, alpha=alpha, device_value_cache=True)


def test_evaluator_for_passes_the_flag_through(monkeypatch):
    seen = []

    def record(shots, scorer, **kwargs):
        seen.append(kwargs)
        return "evaluator"

    monkeypatch.setattr(configured_primitives, "BitstringCircuitEvaluator", record)
    configured = ConfiguredSamplerV2(sampler=object(), shots=32)
    scorer = BitstringEvaluator(4, lambda b: 0.0)
    assert configured_primitives.evaluator_for(configured, bitstring_evaluator=scorer) == "evaluator"
    assert configured_primitives.evaluator_for(configured, bitstring_evaluator=scorer, device_value_cache=True) == "evaluator"
    assert [k["device_value_cache"] for k in seen] == [False, True]


def test_a_cache_travels_empty():
    ev = BitstringCircuitEvaluator.__new__(BitstringCircuitEvaluator)
    ev.__dict__.update(_value_cache=object(), _use_value_cache=True, _shots=8)
    state = ev.__getstate__()
    assert state["_value_cache"] is None and state["_use_value_cache"] is True and ev._value_cache is not None
