"""Golden vectors for PaddedCollatorForActionPrediction (util/data_utils.py:88-196) from the REAL reference class -- build container only.

    PYTHONDONTWRITEBYTECODE=1 python oracle/capture_golden_collator.py

Inputs: oracle/recipe.py collator_batches() (padding, truncation, optional tactile fields). Writes tests/golden/collator.npz, which
tests/test_host_logic.py::test_padded_collator_matches_reference_semantics compares the product's collator against.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import recipe, ref_import  # noqa: E402


def main():
    ref_import.setup()
    from util.data_utils import PaddedCollatorForActionPrediction
    res = {}
    for tactile, batch in recipe.collator_batches().items():
        res.update(recipe.collator_to_arrays(PaddedCollatorForActionPrediction(model_max_length=12, pad_token_id=512)(batch), f"tactile={tactile}"))
    out = os.path.join(ROOT, "tests", "golden", "collator.npz")
    np.savez_compressed(out, **res)
    print(f"wrote {out}: {len(res)} arrays")


if __name__ == "__main__":
    main()
