"""Writes tests/golden/completion_items_reference.npz for tests/test_completion_items_gpu.py: what the upstream project's own
`partial_postproces` (utils/pcd_utils.py:24-51) returns for 2 * partial, as train_inpainter.py:180 calls it, on a CPU with
numpy and torch seeded.  Data only: the input and the function's two outputs.

    python tests/golden/gen_completion_golden.py /path/to/upstream/checkout [out.npz]

B 4, n_in 64, gt 256, distinct random rows: a cloud with a zero tail (40 valid rows); a cloud with zero rows interleaved, one
valid row with a single zero coordinate and one (-0.0, 0, 0) row; a full cloud; a cloud with one valid row."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, N_IN, GT = 4, 64, 256


def inputs():
    rng = np.random.default_rng(20240607)
    p = rng.uniform(-0.5, 0.5, (B, N_IN, 3)).astype(np.float32)
    p[0, 40:] = 0.0
    p[1, 1::3] = 0.0                       # interleaved padding
    p[1, 5] = [-0.0, 0.0, 0.0]             # a zero row by IEEE comparison
    p[1, 6, 1] = 0.0                       # a valid row with one zero coordinate
    p[1, 60:] = 0.0
    p[3] = 0.0
    p[3, 17] = [0.25, -0.125, 0.375]
    for b in range(B):
        rows = p[b][~(p[b] == 0).all(1)]
        assert len({r.tobytes() for r in rows}) == len(rows), "rows must be distinct"
    return p


def main(ref, out):
    spec = importlib.util.spec_from_file_location("ref_pcd_utils", os.path.join(ref, "utils", "pcd_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = inputs()
    np.random.seed(1234)
    torch.manual_seed(1234)
    part, noise = mod.partial_postproces(2 * torch.from_numpy(p), GT)
    assert tuple(part.shape) == (B, N_IN, 3) and tuple(noise.shape) == (B, GT, 4)
    np.savez_compressed(out, partial=p, part=part.numpy().astype(np.float32), noise=noise.numpy().astype(np.float32))
    print(out, os.path.getsize(out), "bytes; valid rows", [int((~(p[b] == 0).all(1)).sum()) for b in range(B)])


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]),
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "completion_items_reference.npz"))
