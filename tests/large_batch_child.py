"""Child process of tests/test_gpu_large_batches.py: the documented call (tests/batch_shapes.py) three times on a fresh
evaluator with default options in a fresh process -- nothing else runs on the GPU before it.  Prints the bits of each call
as one line of hex words and exits."""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import batch_shapes  # noqa: E402
from queasars_amd.circuit_evaluation import OperatorCircuitEvaluator  # noqa: E402


def main() -> int:
    op, circuits, points = batch_shapes.documented_call()
    flat_c, flat_p, _ = batch_shapes.flatten(circuits, points)
    evaluator = OperatorCircuitEvaluator(op)
    for call in range(3):
        print(f"call {call}: " + batch_shapes.hex_line(evaluator.evaluate_circuits(flat_c, flat_p)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
