"""Primitive-shaped front ends: the two call shapes the reference's evaluators use on Qiskit primitives, served by the
GPU backend (SURVEY.md 8(b) "protocol B").

``queasars.circuit_evaluation`` only ever does

    estimator.run(pubs=((circuit, operator, values), ...), precision=p).result()   -> iterable of r with r.data.evs
    sampler.run(pubs=((circuit, values), ...), shots=s).result()                   -> iterable of r with
                                                                                      r.data["meas"].get_counts()

(circuit_evaluation.py:204-215 and :50-59).  The classes below answer exactly that.  Where Qiskit is importable they
subclass ``BaseEstimatorV2`` / ``BaseSamplerV2``; where it is not (this repository's environment) they are plain classes
of the same shape, which is all the reference's evaluators rely on.  Circuits may be :class:`~queasars_amd.ir.CircuitIR` or Qiskit ``QuantumCircuit`` objects, operators
:class:`~queasars_amd.ir.PauliOperator` or ``SparsePauliOp`` (converted by ``queasars_amd.qiskit_adapter`` and cached
per object).
"""

from __future__ import annotations

import weakref
from collections import OrderedDict
from types import SimpleNamespace
from typing import Any, Iterable, Optional, Sequence

import numpy as np

from queasars_amd import qiskit_adapter
from queasars_amd.circuit_evaluation.circuit_evaluation import OperatorCircuitEvaluator, StatevectorDevice
from queasars_amd.ir import CircuitIR, PauliOperator


# On a host that has Qiskit the two front ends ARE Qiskit V2 primitives (subclasses of the abstract bases, so that
# isinstance checks and type annotations of user code hold); without Qiskit they are plain classes of the same shape.
try:  # pragma: no cover - Qiskit is not installable in this repository's environment
    from qiskit.primitives import BaseEstimatorV2 as _EstimatorBase
    from qiskit.primitives import BaseSamplerV2 as _SamplerBase
except Exception:  # ModuleNotFoundError here
    _EstimatorBase = _SamplerBase = object


class _Job:
    def __init__(self, results: list):
        self._results = results

    def result(self) -> list:
        return self._results


class _IdentityCache:
    """Conversion results keyed by object identity WITHOUT pinning the objects: an entry holds its key object weakly
    and disappears with it (so does the converted circuit, and with it the device-side plan); objects that cannot be
    weakly referenced are held in a small bounded table instead.  The reference creates fresh circuits on almost every
    call (``measure_all(inplace=False)``, one circuit per individual and generation), so an unbounded identity cache
    would only ever grow."""

    def __init__(self, convert, limit: int = 512):
        self._convert, self._limit = convert, int(limit)
        self._weak: dict[int, tuple[weakref.ref, Any]] = {}
        self._strong: dict[int, tuple[Any, Any]] = {}

    def __len__(self) -> int:
        return len(self._weak) + len(self._strong)

    def get(self, obj: Any) -> Any:
        key = id(obj)
        hit = self._weak.get(key)
        if hit is not None and hit[0]() is obj:
            return hit[1]
        hit = self._strong.get(key)
        if hit is not None and hit[0] is obj:
            return hit[1]
        value = self._convert(obj)
        try:
            table = self._weak
            table[key] = (weakref.ref(obj, lambda _r, k=key, t=table: t.pop(k, None)), value)
        except TypeError:
            if len(self._strong) >= self._limit:
                for old in list(self._strong)[: self._limit // 2]:
                    self._strong.pop(old, None)
            self._strong[key] = (obj, value)
        return value


class _Converter:
    """Plain-data form of foreign circuit / operator objects (see :class:`_IdentityCache`)."""

    def __init__(self) -> None:
        self._circuits = _IdentityCache(qiskit_adapter.circuit_from_qiskit)
        self._operators = _IdentityCache(qiskit_adapter.operator_from_qiskit)

    def circuit(self, c: Any) -> CircuitIR:
        return c if isinstance(c, CircuitIR) else self._circuits.get(c)

    def operator(self, op: Any) -> PauliOperator:
        return op if isinstance(op, PauliOperator) else self._operators.get(op)


def _operator_key(op: PauliOperator) -> tuple:
    return (op.num_qubits, op.x_mask.tobytes(), op.z_mask.tobytes(), op.coeffs.tobytes())


class GpuEstimator(_EstimatorBase):
    """``run(pubs, precision=...)`` over exact statevector expectation values; ``precision`` other than 0 / None adds
    Gaussian noise of that standard deviation (what an estimator's target precision means to the reference).

    One :class:`StatevectorDevice` per qubit count serves every operator (its tables are rebuilt when the operator
    changes); operators are recognised by content, not identity, and at most ``max_operators`` evaluators are kept.

    ``shots=N`` (``None``, the default: nothing of the above changes) emulates the shot noise of ``N`` shots instead: every
    entry of ``evs`` gets Gaussian noise of ITS OWN standard deviation ``sqrt(max(Var, 0) / N)``, with ``Var`` the observable's
    variance in that entry's state, computed on the device (``OperatorCircuitEvaluator.evaluate_variances``).
    ``data.stds`` holds those standard deviations in the shape of ``evs`` and ``metadata["shots"]`` is ``N``.  In this mode a
    pub's own precision and the call's ``precision`` are ignored.

    ``joint_moments=True`` (with ``shots``; the default ``False`` leaves that route and its numbers as they are): an array pub
    takes the values and the variances of all its distinct observables from ONE ``evaluate_covariances`` call over its distinct
    bindings -- the diagonal of the observables' covariance matrix, DESIGN.md 4.14 -- instead of one evaluator and one pass over
    the states per distinct observable.  The noise stays independent per entry; ``stds`` and ``metadata`` keep their form."""

    def __init__(self, dtype: str = "fp64", device: int = 0, seed: Optional[int] = None, max_operators: int = 8,
                 shots: Optional[int] = None, joint_moments: bool = False):
        if shots is not None and int(shots) <= 0:
            raise ValueError("shots must be a positive number (or None: the precision's noise)")
        if joint_moments and shots is None:
            raise ValueError("joint_moments belongs to the shot noise: set shots")
        self._joint_moments = bool(joint_moments)
        self._shots = None if shots is None else int(shots)
        self._dtype, self._device_index, self._seed = dtype, device, seed
        self._rng = np.random.default_rng(seed)
        self._convert = _Converter()
        self._devices: dict[int, StatevectorDevice] = {}
        self._evaluators: "OrderedDict[tuple, OperatorCircuitEvaluator]" = OrderedDict()
        self._max_operators = max(1, int(max_operators))

    def backend_options(self) -> dict:
        """dtype / device / seed, for ``configured_primitives.evaluator_for``."""
        return {"dtype": self._dtype, "device": self._device_index, "seed": self._seed}

    def _device(self, n_qubits: int) -> StatevectorDevice:
        dev = self._devices.get(n_qubits)
        if dev is None:
            dev = StatevectorDevice(n_qubits, dtype=self._dtype, device=self._device_index)
            self._devices[n_qubits] = dev
        return dev

    def _evaluator(self, operator: PauliOperator) -> OperatorCircuitEvaluator:
        key = _operator_key(operator)
        hit = self._evaluators.get(key)
        if hit is None:
            hit = OperatorCircuitEvaluator(operator, statevector_device=self._device(operator.num_qubits))
            self._evaluators[key] = hit
            while len(self._evaluators) > self._max_operators:
                self._evaluators.popitem(last=False)
        else:
            self._evaluators.move_to_end(key)
        return hit

    def run(self, pubs: Iterable[Sequence[Any]], *, precision: Optional[float] = None) -> _Job:
        """A pub is (circuit, observables[, parameter values[, precision]]): observables one observable or a (nested) list or
        object array of them, parameter values one vector or an array of shape (..., n_params); ``evs`` has their broadcast
        shape (:func:`pub_broadcast`).  A pub's own precision overrides ``precision``; with ``shots`` set both are ignored (see
        the class)."""
        pubs = [tuple(pub) for pub in pubs]
        if self._shots is not None:
            return self._run_with_shots(pubs)
        out: list[Any] = [None] * len(pubs)
        by_operator: dict[tuple, list[int]] = {}
        operators: dict[int, PauliOperator] = {}
        for i, pub in enumerate(pubs):
            values = pub[2] if len(pub) > 2 else None
            if _is_observable_array(pub[1]) or (values is not None and np.ndim(values) > 1):
                out[i] = self._run_array_pub(pub[0], pub[1], values)
                continue
            operators[i] = self._convert.operator(pub[1])
            by_operator.setdefault(_operator_key(operators[i]), []).append(i)
        for indices in by_operator.values():  # one batched call per distinct operator
            evaluator = self._evaluator(operators[indices[0]])
            circuits = [self._convert.circuit(pubs[i][0]) for i in indices]
            values = [list(np.ravel(pubs[i][2])) if len(pubs[i]) > 2 and pubs[i][2] is not None else [] for i in indices]
            for i, value in zip(indices, evaluator.evaluate_circuits(circuits, values)):
                out[i] = value
        results = []
        for pub, v in zip(pubs, out):
            p = pub[3] if len(pub) > 3 and pub[3] is not None else precision
            if p:
                v = v + float(self._rng.normal(0.0, p)) if np.ndim(v) == 0 else v + self._rng.normal(0.0, p, size=np.shape(v))
            results.append(SimpleNamespace(data=SimpleNamespace(evs=np.asarray(v)), metadata={"target_precision": p or 0.0}))
        return _Job(results)

    def _run_array_pub(self, circuit: Any, observables: Any, values: Any) -> np.ndarray:
        """One pub with an array of observables and / or of parameter vectors: ONE observable_values call over its distinct
        bindings and distinct observables, spread to the broadcast shape (:func:`pub_layout`)."""
        circuit = self._convert.circuit(circuit)
        layout = pub_layout(observables, values)
        ops, keys, observable_of = [], {}, []
        for o in layout.observables:
            op = self._convert.operator(o)
            key = _operator_key(op)
            if key not in keys:
                keys[key] = len(ops)
                ops.append(op)
            observable_of.append(keys[key])
        dev = self._device(circuit.num_qubits)
        table = dev.observable_values([circuit] * len(layout.rows), [list(r) for r in layout.rows], ops)
        return table[layout.binding_index, np.asarray(observable_of, dtype=np.intp)[layout.observable_index]]

    def _run_with_shots(self, pubs: list) -> _Job:
        """``run`` with ``shots`` set: the exact values and the variances from the same calls -- single-observable pubs batched
        per distinct operator, an array pub by :meth:`_array_pub_moments` --, then the noise, pub by pub in their order."""
        moments: list[Any] = [None] * len(pubs)  # per pub: (exact values, variances), scalars or arrays of the pub's shape
        by_operator: dict[tuple, list[int]] = {}
        operators: dict[int, PauliOperator] = {}
        for i, pub in enumerate(pubs):
            values = pub[2] if len(pub) > 2 else None
            if _is_observable_array(pub[1]) or (values is not None and np.ndim(values) > 1):
                moments[i] = self._array_pub_moments(pub[0], pub[1], values)
                continue
            operators[i] = self._convert.operator(pub[1])
            by_operator.setdefault(_operator_key(operators[i]), []).append(i)
        for indices in by_operator.values():  # one batched call per distinct operator
            evaluator = self._evaluator(operators[indices[0]])
            circuits = [self._convert.circuit(pubs[i][0]) for i in indices]
            values = [list(np.ravel(pubs[i][2])) if len(pubs[i]) > 2 and pubs[i][2] is not None else [] for i in indices]
            exact, variances = evaluator.evaluate_variances(circuits, values, with_values=True)
            for i, value, variance in zip(indices, exact, variances):
                moments[i] = (value, variance)
        results = []
        for exact, variances in moments:
            stds = np.sqrt(np.maximum(np.asarray(variances, dtype=np.float64), 0.0) / self._shots)
            evs = np.asarray(exact, dtype=np.float64) + self._rng.normal(0.0, stds)
            results.append(SimpleNamespace(data=SimpleNamespace(evs=np.asarray(evs), stds=stds),
                                           metadata={"target_precision": 0.0, "shots": self._shots}))
        return _Job(results)

    def _array_pub_moments(self, circuit: Any, observables: Any, values: Any) -> tuple[np.ndarray, np.ndarray]:
        """(exact values, variances) of one array pub, both of its broadcast shape: one ``evaluate_variances`` call per distinct
        observable over the pub's distinct bindings -- with ``joint_moments`` one ``evaluate_covariances`` call for all of them --,
        spread by :func:`pub_layout`'s indices."""
        circuit = self._convert.circuit(circuit)
        layout = pub_layout(observables, values)
        ops, keys, observable_of = [], {}, []
        for o in layout.observables:
            op = self._convert.operator(o)
            key = _operator_key(op)
            if key not in keys:
                keys[key] = len(ops)
                ops.append(op)
            observable_of.append(keys[key])
        rows = [list(r) for r in layout.rows]
        exact = np.zeros((len(rows), len(ops)))
        variances = np.zeros((len(rows), len(ops)))
        if not rows:
            pass
        elif self._joint_moments:
            evaluator, limit = self._evaluator(ops[0]), StatevectorDevice.MAX_COVARIANCE_OBSERVABLES
            for m in range(0, len(ops), limit):  # (a set holds at most `limit` observables; only the diagonal is wanted)
                part, cov = evaluator.evaluate_covariances([circuit] * len(rows), rows, ops[m:m + limit], with_values=True)
                exact[:, m:m + limit] = part
                variances[:, m:m + limit] = np.diagonal(cov, axis1=1, axis2=2)
        else:
            for m, op in enumerate(ops):
                exact[:, m], variances[:, m] = self._evaluator(op).evaluate_variances([circuit] * len(rows), rows, with_values=True)
        column = np.asarray(observable_of, dtype=np.intp)[layout.observable_index]
        return exact[layout.binding_index, column], variances[layout.binding_index, column]


def pub_layout(observables: Any, values: Any) -> SimpleNamespace:
    """The shape logic of an EstimatorV2 pub (circuit, observables, parameter values), without a device:
      shape             of ``evs`` (:func:`pub_broadcast`)
      observables       the observables in C order of their array (one observable: an array of shape ())
      rows              the distinct parameter vectors, one per row (no values, or vectors of no parameters: one empty row;
                        an empty array of bindings: none)
      binding_index     (shape ``shape``) the row of ``rows`` each entry of ``evs`` is evaluated with
      observable_index  (shape ``shape``) the position in ``observables`` of each entry's observable"""
    obs = _observable_array(observables)
    vals = np.zeros(0) if values is None else np.asarray(values, dtype=np.float64)
    if vals.ndim == 0:
        vals = vals.reshape(1)
    shape = pub_broadcast(obs.shape, vals.shape)
    bindings = vals.shape[:-1]
    rows = vals.reshape(int(np.prod(bindings, dtype=np.int64)), vals.shape[-1])
    if rows.shape[0] and rows.shape[1]:
        rows, inverse = np.unique(rows, axis=0, return_inverse=True)
    elif rows.shape[0]:  # bindings of no parameters: all the same empty vector
        rows, inverse = rows[:1], np.zeros(rows.shape[0], dtype=np.intp)
    else:
        inverse = np.zeros(0, dtype=np.intp)
    b, o = np.broadcast_arrays(np.reshape(inverse, bindings), np.arange(obs.size, dtype=np.intp).reshape(obs.shape))
    return SimpleNamespace(shape=shape, observables=list(obs.flat), rows=rows, binding_index=b, observable_index=o)


def pub_broadcast(observables_shape: Sequence[int], values_shape: Sequence[int]) -> tuple:
    """Shape of ``evs`` for an EstimatorV2 pub (as Qiskit defines it): the NumPy broadcast of the observables' shape and the
    bindings' shape, i.e. the parameter values' shape without its last axis (the parameters of one binding)."""
    bindings = tuple(values_shape)[:-1]
    try:
        return tuple(np.broadcast_shapes(tuple(observables_shape), bindings))
    except ValueError as exc:
        raise ValueError(f"observables of shape {tuple(observables_shape)} and parameter values of shape {tuple(values_shape)} "
                         "do not broadcast") from exc


def _is_observable_array(observables: Any) -> bool:
    return isinstance(observables, (list, tuple, np.ndarray))


def _observable_array(observables: Any) -> np.ndarray:
    """A (nested) list / tuple / object array of observables as an object array of that shape (one observable: shape ())."""
    if isinstance(observables, np.ndarray):
        return observables.astype(object) if observables.dtype != object else observables
    if not isinstance(observables, (list, tuple)):
        leaf = np.empty((), dtype=object)
        leaf[()] = observables
        return leaf
    items = [_observable_array(o) for o in observables]
    if len({item.shape for item in items}) > 1:
        raise ValueError("a nested list of observables must be rectangular")
    out = np.empty((len(items),) + (items[0].shape if items else ()), dtype=object)
    for k, item in enumerate(items):
        out[k, ...] = item
    return out


class _BitArray:
    def __init__(self, states: np.ndarray, n_qubits: int):
        self._states, self._n = states, n_qubits

    def get_counts(self) -> dict[str, int]:
        values, counts = np.unique(self._states, return_counts=True)
        return {format(int(v), f"0{self._n}b"): int(c) for v, c in zip(values, counts)}

    def get_int_counts(self) -> dict[int, int]:
        values, counts = np.unique(self._states, return_counts=True)
        return {int(v): int(c) for v, c in zip(values, counts)}


class GpuSampler(_SamplerBase):
    """``run(pubs, shots=...)``: seeded inverse-CDF sampling of every qubit on the device; results expose
    ``data["meas"].get_counts()`` with Qiskit's bitstring convention (leftmost character = highest qubit)."""

    def __init__(self, n_qubits: int, dtype: str = "fp64", device: int = 0, seed: int = 0):
        self._device = StatevectorDevice(n_qubits, dtype=dtype, device=device)
        self._options = {"dtype": dtype, "device": device, "seed": int(seed)}
        self._convert = _Converter()
        self._seed = int(seed)
        self._calls = 0

    def backend_options(self) -> dict:
        """dtype / device / seed, for ``configured_primitives.evaluator_for``."""
        return dict(self._options)

    def run(self, pubs: Iterable[Sequence[Any]], *, shots: Optional[int] = None) -> _Job:
        shots = 1024 if shots is None else int(shots)
        pubs = [tuple(pub) for pub in pubs]
        circuits = [self._convert.circuit(pub[0]) for pub in pubs]
        values = [list(np.ravel(pub[1])) if len(pub) > 1 and pub[1] is not None else [] for pub in pubs]
        self._calls += 1
        states, _ = self._device.sample_batch(circuits, values, shots, seed=self._seed + self._calls)
        n = self._device.n_qubits
        return _Job([SimpleNamespace(data={"meas": _BitArray(np.asarray(row), n)}, metadata={"shots": shots}) for row in states])


class GpuStateFidelity:
    """``run(circuits_1, circuits_2, values_1, values_2).result().fidelities``: the state fidelities ``|<psi_1|psi_2>|^2`` of
    pairs of parametrised circuits, in the call shape of Qiskit Algorithms' ``BaseStateFidelity`` (duck-typed, as the other
    front ends are; single circuits and single value vectors are accepted as lists of one).  The overlaps are reduced on the
    device (``StatevectorDevice.overlaps``); no statevector leaves it.

    Cost model: the DISTINCT (circuit_2, values_2) pairs are kept on the device in blocks of 64, the DISTINCT (circuit_1,
    values_1) pairs are evaluated against each block, and ``|S|^2`` is picked per requested pair -- so a call computes whole
    blocks, n_1 x n_2 overlaps for n_1 and n_2 distinct states, whatever pairs were asked for.  That is the right trade for a
    few fixed second states against many first ones (a deflation penalty, a target state); for many unrelated pairs most of
    the block is wasted.  Raw numbers: nothing is divided by a norm and nothing clipped to [0, 1]."""

    def __init__(self, dtype: str = "fp64", device: int = 0, statevector_device: Optional[StatevectorDevice] = None):
        self._dtype, self._device_index = dtype, device
        self._convert = _Converter()
        self._devices: dict[int, StatevectorDevice] = {}
        if statevector_device is not None:
            self._devices[statevector_device.n_qubits] = statevector_device

    def _device(self, n_qubits: int) -> StatevectorDevice:
        dev = self._devices.get(n_qubits)
        if dev is None:
            dev = StatevectorDevice(n_qubits, dtype=self._dtype, device=self._device_index)
            self._devices[n_qubits] = dev
        return dev

    @staticmethod
    def _as_lists(circuits: Any, values: Any) -> tuple[list, list]:
        circuits = list(circuits) if isinstance(circuits, (list, tuple)) else [circuits]
        if values is None:
            values = [[] for _ in circuits]
        else:
            values = list(values)
            if len(circuits) == 1 and (len(values) == 0 or np.ndim(values[0]) == 0):
                values = [values]
        if len(values) != len(circuits):
            raise ValueError(f"{len(circuits)} circuits but {len(values)} parameter vectors")
        return circuits, [[float(v) for v in row] for row in values]

    def _distinct(self, circuits: list, values: list) -> tuple[list, list, list]:
        """(distinct circuits, their values, index of each request among them)"""
        found: dict[tuple, int] = {}
        out_c, out_v, index = [], [], []
        for circuit, row in zip(circuits, values):
            ir = self._convert.circuit(circuit)
            if len(row) != ir.num_parameters:
                raise ValueError(f"a circuit has {ir.num_parameters} parameters, {len(row)} values were given")
            key = (id(ir), tuple(row))
            at = found.get(key)
            if at is None:
                at = found[key] = len(out_c)
                out_c.append(ir)
                out_v.append(row)
            index.append(at)
        return out_c, out_v, index

    def run(self, circuits_1: Any, circuits_2: Any, values_1: Any = None, values_2: Any = None) -> _Job:
        circuits_1, values_1 = self._as_lists(circuits_1, values_1)
        circuits_2, values_2 = self._as_lists(circuits_2, values_2)
        if len(circuits_1) != len(circuits_2):
            raise ValueError(f"{len(circuits_1)} first circuits but {len(circuits_2)} second circuits")
        first_c, first_v, first_at = self._distinct(circuits_1, values_1)
        second_c, second_v, second_at = self._distinct(circuits_2, values_2)
        if not first_c:
            return _Job(SimpleNamespace(fidelities=[], raw_fidelities=[], metadata=[]))
        widths = {c.n_qubits for c in first_c + second_c}
        if len(widths) != 1:
            raise ValueError("the circuits of a fidelity act on registers of different sizes")
        device = self._device(widths.pop())
        overlaps = np.zeros((len(first_c), len(second_c)), dtype=np.complex128)
        block = StatevectorDevice.MAX_OVERLAP_STATES
        for k0 in range(0, len(second_c), block):
            kept = device.keep_states(second_c[k0:k0 + block], second_v[k0:k0 + block])
            try:
                overlaps[:, k0:k0 + len(kept)] = device.overlaps(first_c, first_v, kept)
            finally:
                for state in kept:
                    state.release()
        fidelities = [float(abs(overlaps[i, k]) ** 2) for i, k in zip(first_at, second_at)]
        return _Job(SimpleNamespace(fidelities=fidelities, raw_fidelities=list(fidelities), metadata=[{} for _ in fidelities]))


class GpuQFI:
    """``run(circuits, parameter_values).result().qfis``: the quantum Fisher information matrices ``4 G`` of parametrised
    circuits at the given points, G the Fubini-Study metric, in the call shape of Qiskit Algorithms' ``QFI`` (duck-typed, as
    the other front ends are; a single circuit and a single value vector are accepted as lists of one).  ``parameters``: per
    circuit the parameter INDICES (in the circuit's parameter order) to differentiate by, or None for all.  The metric is
    formed on the device from one reverse sweep per circuit (``StatevectorDevice.metric_tensors``); no
    statevector leaves it.  Circuits of different widths go to a device each."""

    def __init__(self, dtype: str = "fp64", device: int = 0, statevector_device: Optional[StatevectorDevice] = None):
        self._dtype, self._device_index = dtype, device
        self._convert = _Converter()
        self._devices: dict[int, StatevectorDevice] = {}
        if statevector_device is not None:
            self._devices[statevector_device.n_qubits] = statevector_device

    _device = GpuStateFidelity._device

    def run(self, circuits: Any, parameter_values: Any = None, parameters: Any = None) -> _Job:
        circuits, values = GpuStateFidelity._as_lists(circuits, parameter_values)
        irs = [self._convert.circuit(c) for c in circuits]
        for ir, row in zip(irs, values):
            if len(row) != ir.num_parameters:
                raise ValueError(f"a circuit has {ir.num_parameters} parameters, {len(row)} values were given")
        if parameters is not None and len(parameters) != len(irs):
            raise ValueError(f"{len(irs)} circuits but {len(parameters)} parameter lists")
        wrt = None if parameters is None else [list(range(ir.num_parameters)) if p is None else [int(i) for i in p]
                                               for ir, p in zip(irs, parameters)]
        qfis: list = [None] * len(irs)
        for width in sorted({ir.n_qubits for ir in irs}):
            rows = [i for i, ir in enumerate(irs) if ir.n_qubits == width]
            metrics = self._device(width).metric_tensors([irs[i] for i in rows], [values[i] for i in rows],
                                                         None if wrt is None else [wrt[i] for i in rows])
            for i, metric in zip(rows, metrics):
                qfis[i] = 4.0 * metric
        return _Job(SimpleNamespace(qfis=qfis, metadata=[{} for _ in qfis]))
