"""Writes tests/golden/unused_blocks_reference.npz for tests/test_unused_blocks_cpu.py: the upstream project's own
unet2d.unet_model.UNet(2, 3, 16) and layers.v2v_groups.V2VModel(2, 3, groups=2), built after torch.manual_seed(0) — the names
and SHA-256 digests of their state-dict tensors — and their eval-mode outputs on the test's input (torch.manual_seed(1)).

    python tests/golden/gen_unused_blocks_golden.py <upstream checkout>"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main(ref_dir):
    # the upstream unet2d / layers, not this package's: this checkout stays off sys.path (its regular packages would win over
    # the upstream namespace packages); the test module is loaded by its path (it imports nothing from either at import time)
    sys.path[:] = [ref_dir] + [p for p in sys.path if os.path.abspath(p or ".") not in (ROOT, HERE)]
    spec = importlib.util.spec_from_file_location("unused_blocks_test", os.path.join(ROOT, "tests", "test_unused_blocks_cpu.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    out = {}
    for kind in ("unet", "v2v"):
        model = T.build(kind)
        assert ref_dir in sys.modules[model.__class__.__module__].__file__, sys.modules[model.__class__.__module__].__file__
        sd = model.state_dict()
        out[kind + "/sd_names"] = np.array(list(sd))
        out[kind + "/sd_sha256"] = np.array([T.tensor_digest(v) for v in sd.values()])
        out[kind + "/out"] = T.forward(model, kind).numpy()
    np.savez(os.path.join(HERE, "unused_blocks_reference.npz"), **out)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
