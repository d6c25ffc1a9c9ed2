"""Record the reference implementation's results for the equivalence suite.

Runs every case of tests/_equivalence_cases.py on a checkout of the
reference implementation (the upstream rl-replicas package this project
is API-compatible with) and stores what it computed — post-update
parameters, metrics, primitive outputs — as plain arrays in
tests/golden/reference_equivalence.npz.  tests/test_reference_equivalence.py
compares our stack against that file, so the suite needs no reference
checkout.  Re-run only when a case's inputs change:

    python tools/record_reference_golden.py --reference-src <checkout>/src

CPU only; takes a few seconds.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir)
sys.path.insert(0, os.path.abspath(REPO))

from tests import _equivalence_cases as cases  # noqa: E402
from tests._reference_loader import load_reference  # noqa: E402


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument(
        "--reference-src",
        required=True,
        help="directory holding the reference's rl_replicas package (its src/)",
    )
    parser.add_argument("--out", default=cases.GOLDEN_PATH)
    args = parser.parse_args()

    results = cases.run_all(load_reference(os.path.abspath(args.reference_src)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **results)
    print(f"recorded {len(results)} arrays from {len(cases.CASES)} cases -> {args.out}")


if __name__ == "__main__":
    main()
