"""Writes tests/golden/scan_items_reference.npz for tests/test_scan_items_cpu.py and tests/test_scan_items_gpu.py: what the
upstream project's own `ScanObjectNN.__getitem__` (datasets/scanobjectnn.py:102-122) returns with train=True, for subsample
64 and for subsample None, on the synthetic file of tests/test_datasets_cpu.py (6 clouds x 256 points), with numpy seeded
before every item — together with the draws the item consumed, replayed from the same seed in the order the upstream code
makes them: randn(1, P, 3) (jitter), uniform() (the angle is 2 pi times it), choice(P, 64, replace=False).  Data only.

    python tests/golden/gen_scan_items_golden.py /path/to/upstream/checkout [out.npz]

h5py is not needed: as in tests/test_datasets_cpu.py a stand-in module serves the file's arrays from its .npz twin."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SUBSAMPLE = 64


def seed_of(i):
    return 1000 + 17 * i


def main(ref, out):
    sys.path.insert(0, ROOT)
    from tests.test_datasets_cpu import make_files
    h5 = types.ModuleType("h5py")

    class File(dict):
        def __init__(self, name, mode="r"):
            z = np.load(os.path.splitext(str(name))[0] + ".npz")
            super().__init__({k: z[k] for k in z.files})

    h5.File = File
    sys.modules["h5py"] = h5
    spec = importlib.util.spec_from_file_location("ref_scanobjectnn", os.path.join(ref, "datasets", "scanobjectnn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {}
    with tempfile.TemporaryDirectory() as d:
        make_files(d)
        for name, sub in (("sub", SUBSAMPLE), ("full", None)):
            ds = mod.ScanObjectNN(os.path.join(d, "scan.h5"), train=True, subsample=sub)
            M, P = ds.data.shape[0], ds.data.shape[1]
            pcs, mas, labs = [], [], []
            for i in range(M):
                np.random.seed(seed_of(i))
                pc, lab, ma = ds[i]
                pcs.append(pc.numpy()), mas.append(ma.numpy()), labs.append(int(lab))
            res["pc_" + name], res["ma_" + name], res["label_" + name] = np.stack(pcs), np.stack(mas), np.asarray(labs, np.int64)
        res["data"], res["mask"], res["label"] = ds.data.astype(np.float32), ds.mask.astype(np.uint8), np.asarray(ds.label, np.int64)
        assert np.array_equal(res["data"], ds.data) and set(np.unique(ds.mask)) <= {0.0, 1.0}
    randn, uniform, choice = [], [], []
    for i in range(M):
        np.random.seed(seed_of(i))
        randn.append(np.random.randn(1, P, 3)[0])
        uniform.append(np.random.uniform())
        choice.append(np.random.choice(P, size=SUBSAMPLE, replace=False))
    res["randn"], res["uniform"], res["choice"] = np.stack(randn), np.asarray(uniform), np.stack(choice).astype(np.int64)
    assert res["pc_sub"].shape == (M, SUBSAMPLE, 3) and res["pc_full"].shape == (M, P, 3) and res["pc_sub"].dtype == np.float32
    np.savez_compressed(out, **res)
    print(out, os.path.getsize(out), "bytes;", {k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]),
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "scan_items_reference.npz"))
