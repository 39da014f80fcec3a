"""Writes tests/golden/grid_subsampling_reference.json: for each case of tests/test_grid_subsampling.py::test_matches_the_reference_cpp
and each choice of features / classes, the row count and the SHA-256 of the sorted rows (points, features, classes as float32) that
the reference's own grid_subsampling.cpp returns — through oracle/_ref/libgrid_subsampling_ref.so, which `make -C oracle ref
REF=<upstream checkout>` compiles from the upstream sources where they lie.

    python tests/golden/gen_grid_subsampling_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import grid_ref                           # noqa: E402
from tests import test_grid_subsampling as T          # noqa: E402


def main():
    assert grid_ref.available(), "oracle/_ref/libgrid_subsampling_ref.so is not built"
    out = {}
    for n, dl, seed in T.REF_CASES:
        pts, feats, labels = T.reference_cloud(n, seed)
        for use_f, use_c in T.REF_VARIANTS:
            P, F, C = grid_ref.compute(pts, feats if use_f else None, labels if use_c else None, dl)
            out[T.golden_key(n, dl, seed, use_f, use_c)] = T.rows_digest(P, F, C)
    with open(os.path.join(HERE, "grid_subsampling_reference.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
