"""Interior eigenvalues and eigenstate polishing on top of the EVQE solver: searches on the folded-spectrum cost and on the
variance.

``compute_eigenvalue_near`` minimises ``<psi|(H - target)^2|psi>`` (``FoldedSpectrumCircuitEvaluator``),
whose minimum is the eigenstate with the eigenvalue nearest ``target``: an interior eigenvalue is reached directly, where
deflation (``evqe/deflation.py``) climbs through every lower state first.  ``minimize_variance`` minimises
``<H^2> - <H>^2``, zero exactly on eigenstates: it polishes a state an energy search left near one."""

from __future__ import annotations

from queasars_amd.circuit_evaluation.circuit_evaluation import FoldedSpectrumCircuitEvaluator
from queasars_amd.evqe.solver import NFT


def _run(solver, evaluator, target, solver_kwargs):
    """One run of ``solver`` on the folded evaluator over ``evaluator``'s device, operator and initial state, and what the
    result carries of its best individual: two value-only calls."""
    folded = FoldedSpectrumCircuitEvaluator(evaluator.operator, target, evaluator.initial_state_circuit,
                                            statevector_device=evaluator.statevector_device)
    result = solver.compute_minimum_eigenvalue(folded, **solver_kwargs)
    best = result.best_individual
    circuit = best.get_parameterized_quantum_circuit(shared=getattr(solver, "share_circuits", True))
    point = [list(best.parameter_values)]
    result.folded_value = float(folded.evaluate_circuits([circuit], point)[0])
    result.eigenvalue = float(folded.evaluate_energies([circuit], point)[0])
    if target is None:
        result.eigenvalue_variance = result.folded_value
    else:
        variance = FoldedSpectrumCircuitEvaluator(evaluator.operator, None, evaluator.initial_state_circuit,
                                                  statevector_device=evaluator.statevector_device)
        result.eigenvalue_variance = float(variance.evaluate_circuits([circuit], point)[0])
    return result


def compute_eigenvalue_near(solver, evaluator, target: float, **solver_kwargs):
    """One run of ``solver`` (an ``EVQEMinimumEigensolver``) towards the eigenvalue of ``evaluator``'s operator nearest
    ``target``, as an ``EVQEResult``.

    ``evaluator`` is an ``OperatorCircuitEvaluator`` (exact); the run is ``solver.compute_minimum_eigenvalue`` on a
    ``FoldedSpectrumCircuitEvaluator`` over the same device, operator and initial state.  The result carries ``eigenvalue``
    (``<H>`` at the best individual, in place of the cost the solver minimised), ``folded_value`` (that cost,
    ``<(H - target)^2>``) and ``eigenvalue_variance`` (the centred variance there; ``folded_value`` is it plus
    ``(eigenvalue - target)^2``).  With a fixed target the cost is an expectation value, so every optimiser of the solver
    applies: SPSA and NFT through the cost's values, Adam and NaturalGradient through ``evaluate_gradients`` /
    ``metric_tensors`` (host drivers; a device-resident search on the folded cost is not built)."""
    if target is None:
        raise ValueError("target must be a number (minimize_variance searches on the variance)")
    return _run(solver, evaluator, float(target), solver_kwargs)


def minimize_variance(solver, evaluator, **solver_kwargs):
    """One run of ``solver`` on the variance ``<H^2> - <H>^2`` of ``evaluator``'s operator (a
    ``FoldedSpectrumCircuitEvaluator`` with ``target=None``), as an ``EVQEResult`` that carries ``eigenvalue`` (``<H>`` at the
    best individual) and ``folded_value`` = ``eigenvalue_variance`` (the centred variance there).

    The variance is not an expectation value: in every angle it has a second harmonic, so NFT's fit of one sinusoid does not
    describe it and an NFT optimiser is refused with a ``ValueError``.  SPSA, Adam and NaturalGradient apply."""
    optimizer = getattr(getattr(solver, "configuration", None), "optimizer", None)
    if isinstance(optimizer, NFT):
        raise ValueError("the variance is not an expectation value (it has a second harmonic in each angle): NFT's sinusoidal "
                         "fit does not apply to it -- use SPSA, Adam or NaturalGradient")
    return _run(solver, evaluator, None, solver_kwargs)
