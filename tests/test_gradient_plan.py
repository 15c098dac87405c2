"""Parameter-shift gradients without a device: the shift plan (qsv_gradient_describe), the rules against an independent
dense derivative, and the host logic of the Adam optimiser."""

import json
from pathlib import Path

import numpy as np
import pytest

import dense_gradient
import helpers
import shift_rules
from queasars_amd import _lib
from queasars_amd.evqe import solver
from queasars_amd.ir import CircuitIR, ParamRef, PauliOperator

P = ParamRef
FP64_TOL = 1e-10  # the project's fp64 tolerance; the combination's coefficients sum to at most 1 in absolute value


def describe(circuit: CircuitIR) -> list[int]:
    lib = _lib.load()
    ops = circuit.packed()
    out = np.full(max(1, circuit.num_parameters), 99, dtype=np.int32)
    assert lib.qsv_gradient_describe(len(ops), _lib.as_ptr(ops), circuit.num_parameters, _lib.as_ptr(out)) == _lib.QSV_OK
    return out[: circuit.num_parameters].tolist()


def test_plans_of_hand_built_circuits():
    assert describe(CircuitIR(2).u(0.1, 0.2, 0.3, 0).cu3(0.4, 0.5, 0.6, 0, 1)) == []
    assert describe(CircuitIR(2).u(P(0), P(1), P(2), 1)) == [2, 2, 2]
    assert describe(CircuitIR(2).cu3(P(0), P(1), P(2), 1, 0)) == [4, 2, 2]
    unused = CircuitIR(2).u(P(0), 0.2, 0.3, 0)
    unused.declare_parameters(3)
    assert describe(unused) == [2, 0, 0]
    assert describe(CircuitIR(2).u(P(0), 0.1, P(0), 0).cu3(P(1), 0.2, 0.3, 0, 1)) == [-1, 4]
    assert describe(CircuitIR(2).u(P(0), 0.1, 0.2, 0).cu3(0.3, P(0), 0.3, 0, 1)) == [-1]


def test_plan_argument_errors():
    lib = _lib.load()
    out = np.zeros(4, dtype=np.int32)
    ops = CircuitIR(2).u(P(0), P(1), P(2), 1).packed()
    assert lib.qsv_gradient_describe(len(ops), _lib.as_ptr(ops), 2, _lib.as_ptr(out)) == _lib.QSV_E_ARG  # (a slot reads parameter 2)
    assert lib.qsv_gradient_describe(len(ops), None, 3, _lib.as_ptr(out)) == _lib.QSV_E_ARG
    assert lib.qsv_gradient_describe(len(ops), _lib.as_ptr(ops), 3, None) == _lib.QSV_E_ARG


def test_plans_of_a_population():
    _, circuits, _ = helpers.population_circuits(6, 3, 16, seed=0)
    assert len(circuits) == 16
    for circuit in circuits:
        plan = describe(circuit)
        assert plan == circuit.gradient_terms()
        assert len(plan) == circuit.num_parameters and set(plan) <= {2, 4}  # (a genome: no repeated, no unused parameter)
        four = {int(row["p_theta"]) for row in circuit.packed() if row["kind"] == 2 and row["p_theta"] >= 0}
        assert {p for p, t in enumerate(plan) if t == 4} == four


def _fixture_population():
    from queasars_amd.evqe.serialization import population_from_dict

    data = json.loads((Path(__file__).resolve().parent / "golden" / "population_n6.json").read_text())
    population = population_from_dict(data["population"])
    circuits = [ind.get_parameterized_quantum_circuit() for ind in population.individuals]
    return circuits, [list(ind.parameter_values) for ind in population.individuals]


def _both_control_directions():
    """Four qubits, seven gates mixing u and cu3 with the control above and below the target, 21 parameters."""
    c = CircuitIR(4)
    c.u(P(0), P(1), P(2), 0).u(P(3), P(4), P(5), 2)
    c.cu3(P(6), P(7), P(8), 0, 1).cu3(P(9), P(10), P(11), 3, 2)
    c.u(P(12), P(13), P(14), 1).cu3(P(15), P(16), P(17), 2, 0).cu3(P(18), P(19), P(20), 1, 3)
    rng = np.random.default_rng(11)
    return [c, c], [rng.uniform(-np.pi, np.pi, 21).tolist(), rng.uniform(-7.0, 7.0, 21).tolist()]


@pytest.mark.parametrize("population", ["n6", "cu3"])
@pytest.mark.parametrize("operator", ["ising", "pauli50"])
def test_rules_against_the_differentiated_gate_matrices(population, operator):
    circuits, params = _fixture_population() if population == "n6" else _both_control_directions()
    n = circuits[0].n_qubits
    op = helpers.random_ising_operator(n, seed=3) if operator == "ising" else helpers.random_pauli_operator(n, 50, seed=4)
    assert operator == "ising" or len(op) == 50
    h = dense_gradient.dense_operator(op)
    worst = 0.0
    for circuit, values in zip(circuits, params):
        terms = describe(circuit)
        assert min(terms, default=0) >= 0, "no circuit of these populations may be refused"
        shifted = [helpers.oracle_expectation(circuit, point, op) for point in shift_rules.shifted_points(terms, values)]
        got = shift_rules.combine(terms, shifted)
        want = dense_gradient.gradient(circuit, values, h)
        assert got.shape == want.shape
        worst = max(worst, float(np.abs(got - want).max(initial=0.0)))
    print(f"{population} / {operator}: largest deviation {worst:.3e}")
    assert worst < FP64_TOL


def test_the_dense_derivative_agrees_with_central_differences():
    """The independent derivative is itself checked: fourth-order central differences of the dense expectation value."""
    circuits, params = _both_control_directions()
    op = helpers.random_pauli_operator(4, 50, seed=4)
    h = dense_gradient.dense_operator(op)
    want = dense_gradient.gradient(circuits[0], params[0], h)
    step, got = 1e-3, []
    for p in range(21):
        f = []
        for k in (-2, -1, 1, 2):
            point = list(params[0])
            point[p] += k * step
            f.append(dense_gradient.expectation(circuits[0], point, h))
        got.append((f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * step))
    assert np.abs(np.asarray(got) - want).max() < 1e-8  # (h^4 / 30 * f^(5) ~ 1e-13 * |f^(5)|, rounding 1e-16 * |f| / h ~ 1e-12)


# ---- Adam ----------------------------------------------------------------------------------------


class QuadraticEvaluator:
    """f(x) = sum a_i (x_i - c_i)^2 over a circuit's parameters, differentiated in closed form; counts what a device would."""

    def __init__(self, a, c):
        self.a, self.c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
        self.calls, self.last_gradient_evaluations, self.total = 0, 0, 0

    def evaluate_gradients(self, circuits, parameter_values, wrt=None):
        self.calls += 1
        out, count = [], 0
        for circuit, x, w in zip(circuits, parameter_values, wrt):
            x = np.asarray(x, dtype=np.float64)
            k = len(x)
            out.append((2.0 * self.a[:k] * (x - self.c[:k]))[list(w)])
            count += sum(circuit.gradient_terms()[p] for p in w)
        self.last_gradient_evaluations = count
        self.total += count
        return out


def _adam_reference(cfg, x0, grad, n_steps):
    x = np.asarray(x0, dtype=np.float64).copy()
    m, v = np.zeros_like(x), np.zeros_like(x)
    for t in range(1, n_steps + 1):
        g = grad(x)
        m = cfg.beta_1 * m + (1 - cfg.beta_1) * g
        v = cfg.beta_2 * v + (1 - cfg.beta_2) * (g * g)  # (g squared, then weighted: algorithm 1)
        x = x - cfg.lr * (m / (1 - cfg.beta_1**t)) / (np.sqrt(v / (1 - cfg.beta_2**t)) + cfg.eps)
    return x


def test_adam_iterates_and_evaluation_counts():
    a = np.array([1.0, 0.5, 2.0, 1.5, 0.25, 3.0, 1.0, 0.75, 2.5])
    c = np.array([0.3, -1.2, 0.8, 2.0, -0.4, 0.1, 1.1, -0.9, 0.6])
    free = CircuitIR(2).u(P(0), P(1), P(2), 0).cu3(P(3), P(4), P(5), 0, 1)              # six parameters: 2 2 2 4 2 2
    whole = CircuitIR(2).u(P(0), P(1), P(2), 0).cu3(P(3), P(4), P(5), 0, 1).u(P(6), P(7), P(8), 1)
    cfg = solver.Adam(maxiter=25, lr=0.05)
    assert cfg.n_circuit_evaluations == 50
    plain = cfg.new_run(np.zeros(6), seed=1)
    embedded = cfg.new_run(np.full(3, 0.5), seed=2)
    base = np.arange(9, dtype=np.float64) / 10.0
    embedded.embed = (base, np.array([3, 4, 5]))
    short = solver.Adam(maxiter=7, lr=0.05).new_run(np.ones(6), seed=3)
    evaluator = QuadraticEvaluator(a, c)
    solver._minimize_batched(evaluator, [(free, plain), (whole, embedded), (free, short)])
    assert plain.done and embedded.done and short.done
    assert evaluator.calls == 25  # one call per iteration for all runs
    assert plain.nfev == 25 * 14 and embedded.nfev == 25 * 8 and short.nfev == 7 * 14
    assert evaluator.total == plain.nfev + embedded.nfev + short.nfev
    assert np.array_equal(plain.x, _adam_reference(cfg, np.zeros(6), lambda x: 2.0 * a[:6] * (x - c[:6]), 25))
    assert np.array_equal(embedded.x, _adam_reference(cfg, np.full(3, 0.5), lambda x: 2.0 * a[3:6] * (x - c[3:6]), 25))
    assert np.array_equal(short.x, _adam_reference(short.config, np.ones(6), lambda x: 2.0 * a[:6] * (x - c[:6]), 7))
    assert np.abs(plain.x - c[:6]).max() < np.abs(c[:6]).max()  # (it moved towards the minimum)


def test_adam_stops_by_tolerance():
    evaluator = QuadraticEvaluator([1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    run = solver.Adam(maxiter=1000, lr=0.01, tol=1e-2).new_run([0.0, 0.0, 0.0], seed=0)
    solver._minimize_batched(evaluator, [(CircuitIR(1).u(P(0), P(1), P(2), 0), run)])
    assert run.done and run.iteration == 1 and run.nfev == 6  # (the gradient is 0 there: the first update is below tol)


def test_adam_needs_an_evaluator_with_gradients():
    class ValuesOnly:
        n_qubits = 2

        def evaluate_circuits(self, circuits, parameter_values):
            return [0.0] * len(circuits)

    run = solver.Adam(maxiter=3).new_run([0.1, 0.2, 0.3], seed=0)
    with pytest.raises(ValueError, match="evaluate_gradients"):
        solver._minimize_batched(ValuesOnly(), [(CircuitIR(1).u(P(0), P(1), P(2), 0), run)])
    cfg = solver.EVQEMinimumEigensolverConfiguration(optimizer=solver.Adam(maxiter=3), population_size=2, max_generations=1, random_seed=0)
    with pytest.raises(ValueError, match="evaluate_gradients"):
        solver.EVQEMinimumEigensolver(cfg).compute_minimum_eigenvalue(ValuesOnly())
