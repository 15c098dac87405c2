"""Variational deflation on top of the EVQE solver: the k lowest eigenvalues of an operator, one run after the other.

Run 0 is the solver's own ``compute_minimum_eigenvalue``.  After each run the best individual's state is kept on the
evaluator's device, and the next run minimises the deflated cost ``E + sum_k beta_k |<phi_k|psi>|^2`` against every state
kept so far (``DeflatedOperatorCircuitEvaluator``), which pushes it away from them: for a diagonal cost
operator the runs give the best, second-best, ... solutions and every member of a degenerate optimum."""

from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np

from queasars_amd.circuit_evaluation.circuit_evaluation import DeflatedOperatorCircuitEvaluator


def _betas_for(betas, n_kept: int) -> Optional[list]:
    """The weights of a run against ``n_kept`` states: None (the evaluator's default), one number for all, or the first
    ``n_kept`` of a sequence that holds one per deflated state."""
    if betas is None:
        return None
    if np.ndim(betas) == 0:
        return [float(betas)] * n_kept
    betas = [float(b) for b in betas]
    if len(betas) < n_kept:
        raise ValueError(f"betas holds {len(betas)} weights, a run against {n_kept} kept states needs as many")
    return betas[:n_kept]


def compute_eigenvalues(solver, evaluator, k: int, betas: Union[None, float, Sequence[float]] = None, keep: bool = False,
                        **solver_kwargs) -> list:
    """``k`` runs of ``solver`` (an ``EVQEMinimumEigensolver``), one ``EVQEResult`` each, in the order found.

    ``evaluator`` is an ``OperatorCircuitEvaluator`` (exact): run 0 is ``solver.compute_minimum_eigenvalue(evaluator,
    **solver_kwargs)``; run j > 0 uses a ``DeflatedOperatorCircuitEvaluator`` over the same device, operator and initial state
    against the j states kept so far, with ``betas`` -- None: 2 * sum|c_k| of the operator for every state (at least its
    spectral width, so the deflated minimum is the next eigenvalue whatever the gap); a number: that weight for every state; a
    sequence: weight i for the state run i found.  Each result additionally carries ``deflated_value`` (the cost its run
    minimised, at the best individual), ``eigenvalue`` (the energy alone) and ``overlaps_with_previous`` (complex, one entry
    per earlier run).  The kept states are released at the end unless ``keep`` is set; then result j carries its state as
    ``kept_state``.  Works with every optimiser of the solver: SPSA and NFT through the cost's values, Adam and
    NaturalGradient through ``evaluate_gradients`` / ``metric_tensors`` (host drivers; a device-resident search on the
    deflated cost is not built)."""
    if k < 1:
        raise ValueError("k must be at least 1")
    if k - 1 > DeflatedOperatorCircuitEvaluator.MAX_KEPT_STATES:
        raise ValueError(f"at most {DeflatedOperatorCircuitEvaluator.MAX_KEPT_STATES + 1} eigenvalues: a deflated cost takes that many kept states")
    share = getattr(solver, "share_circuits", True)
    kept, results = [], []
    try:
        for run in range(k):
            if run == 0:
                current = evaluator
            else:
                current = DeflatedOperatorCircuitEvaluator(
                    evaluator.operator, list(kept), _betas_for(betas, len(kept)), evaluator.initial_state_circuit,
                    statevector_device=evaluator.statevector_device)
            result = solver.compute_minimum_eigenvalue(current, **solver_kwargs)
            best = result.best_individual
            circuit = best.get_parameterized_quantum_circuit(shared=share)
            point = [list(best.parameter_values)]
            if run == 0:
                result.deflated_value = float(result.eigenvalue)
                result.overlaps_with_previous = np.zeros(0, dtype=np.complex128)
            else:
                energies, overlaps = current.evaluate_deflation_terms([circuit], point)
                result.deflated_value = float(current.evaluate_circuits([circuit], point)[0])
                result.eigenvalue = float(energies[0])
                result.overlaps_with_previous = np.array(overlaps[0], dtype=np.complex128)
            state = evaluator.keep_states([circuit], point)[0]
            kept.append(state)
            if keep:
                result.kept_state = state
            results.append(result)
    finally:
        if not keep:
            for state in kept:
                state.release()
    return results
