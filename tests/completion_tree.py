"""Helpers of the completion tests: PCD writers and a tiny ShapeNetCompletion-like tree (two taxonomies, three models, two
renderings per model; ASCII and binary files; partial clouds both shorter and longer than the input size)."""
import json
import os

import numpy as np

TAXONOMIES = {"02691156": ["a1", "a2"], "03001627": ["c1"]}


def write_pcd(path, xyz, encoding="ascii", dtype=np.float32, extra=False):
    """PCD v0.7 of xyz [n, 3]; `extra`: an intensity field before x and an rgb field (U 4) after z."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0]
    size = np.dtype(dtype).itemsize
    fields, sizes, types = ["x", "y", "z"], [size] * 3, ["F"] * 3
    if extra:
        fields, sizes, types = ["intensity"] + fields + ["rgb"], [4] + sizes + [4], ["F"] + types + ["U"]
    head = ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7", "FIELDS " + " ".join(fields),
            "SIZE " + " ".join(str(s) for s in sizes), "TYPE " + " ".join(types), "COUNT " + " ".join("1" for _ in fields),
            "WIDTH %d" % n, "HEIGHT 1", "VIEWPOINT 0 0 0 1 0 0 0", "POINTS %d" % n, "DATA " + encoding]
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with open(str(path), "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if encoding == "ascii":
            fmt = "%.9g" if size == 4 else "%.17g"
            for i in range(n):
                cols = [fmt % v for v in xyz[i].astype(dtype)]
                if extra:
                    cols = ["%.9g" % (0.5 + i)] + cols + [str(4000000000 - i)]
                f.write((" ".join(cols) + "\n").encode("ascii"))
        else:
            spec = [(name, {"F": "<f%d", "U": "<u%d"}[t] % s) for name, s, t in zip(fields, sizes, types)]
            rec = np.zeros(n, dtype=np.dtype(spec))
            for k, name in enumerate("xyz"):
                rec[name] = xyz[:, k].astype(dtype)
            if extra:
                rec["intensity"] = 0.5 + np.arange(n)
                rec["rgb"] = 4000000000 - np.arange(n)
            f.write(rec.tobytes())


def make_tree(root, input_size, gt_size, seed=0):
    """Writes the tree under `root`; returns the `data` keys of the reference config for it (configs/inpainting.yaml)."""
    rng = np.random.default_rng(seed)
    root = str(root)
    cats = [{"taxonomy_id": t, "taxonomy_name": "name_" + t, "train": list(m), "val": list(m), "test": list(m)}
            for t, m in TAXONOMIES.items()]
    with open(os.path.join(root, "ShapeNet.json"), "w") as f:
        json.dump(cats, f)
    k = 0
    for subset in ("train", "val", "test"):
        for t, models in TAXONOMIES.items():
            for m in models:
                n_gt = gt_size if subset == "test" else gt_size + 76          # TEST leaves gtcloud unsampled
                gt = rng.normal(size=(n_gt, 3))
                gt = (gt / np.linalg.norm(gt, axis=1, keepdims=True) * rng.uniform(0.2, 0.45)).astype(np.float32)
                write_pcd(os.path.join(root, subset, "complete", t, m + ".pcd"), gt, "binary" if k % 2 else "ascii")
                for r in range(2):
                    n_part = (input_size // 2 + 3, input_size + 40)[(k + r) % 2]
                    part = gt[rng.permutation(n_gt)[:n_part]]
                    write_pcd(os.path.join(root, subset, "partial", t, m, "%02d.pcd" % r), part, "ascii" if (k + r) % 2 else "binary",
                              extra=bool(r))
                k += 1
    return {"category_path": os.path.join(root, "ShapeNet.json"),
            "partial_path": os.path.join(root, "%s", "partial", "%s", "%s", "%02d.pcd"),
            "gt_path": os.path.join(root, "%s", "complete", "%s", "%s.pcd"),
            "n_renders": 2, "input_size": input_size, "gt_size": gt_size}
