"""Helpers of the What3D reconstruction tests: PLY writers and a tiny What3D-like tree (two categories, PNG renderings written
by PIL, PLY clouds in both encodings)."""
import os

import numpy as np

CATEGORIES = {"02691156": "airplane", "03001627": "chair"}


def write_ply(path, xyz, encoding="ascii", dtype=np.float32, colour=False, faces=False, fmt=None, list_prop=False):
    """A PLY file of xyz [n, 3].  `colour`: a uchar property between x and y, and one after z; `faces`: a trailing `face` element
    with list properties; `fmt`: the format line's word (default: ascii, or binary_little_endian for encoding "binary");
    `list_prop`: a list property inside `vertex` (not readable)."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0]
    word = {np.dtype(np.float32): "float", np.dtype(np.float64): "double"}[np.dtype(dtype)]
    props = [("x", word), ("y", word), ("z", word)]
    if colour:
        props = [("x", word), ("red", "uchar"), ("y", word), ("z", word), ("alpha", "uchar")]
    head = ["ply", "format %s 1.0" % (fmt or ("ascii" if encoding == "ascii" else "binary_little_endian")), "comment made by a test",
            "element vertex %d" % n] + ["property %s %s" % (t, name) for name, t in props]
    if list_prop:
        head.append("property list uchar int neighbours")
    if faces:
        head += ["element face 2", "property list uchar int vertex_indices"]
    head.append("end_header")
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with open(str(path), "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if encoding == "ascii":
            real = "%.9g" if word == "float" else "%.17g"
            for i in range(n):
                cols = {"x": real % xyz[i, 0], "y": real % xyz[i, 1], "z": real % xyz[i, 2], "red": str(i % 256), "alpha": str(255 - i % 256)}
                f.write((" ".join(cols[name] for name, _ in props) + "\n").encode("ascii"))
            if faces:
                f.write(b"3 0 1 2\n3 0 2 1\n")
        else:
            spec = [(name, {"float": "<f4", "double": "<f8", "uchar": "u1"}[t]) for name, t in props]
            rec = np.zeros(n, dtype=np.dtype(spec))
            for k, name in enumerate("xyz"):
                rec[name] = xyz[:, k].astype(dtype)
            if colour:
                rec["red"], rec["alpha"] = np.arange(n) % 256, 255 - np.arange(n) % 256
            f.write(rec.tobytes())
            if faces:
                f.write(np.array([3], "u1").tobytes() + np.array([0, 1, 2], "<i4").tobytes())
                f.write(np.array([3], "u1").tobytes() + np.array([0, 2, 1], "<i4").tobytes())


def make_tree(root, objects=4, views=1, size=(32, 32), cloud=64, seed=0, splits=("train", "val", "test")):
    """Writes the tree under `root`: per category `objects` object ids (every split lists them all), per object `views`
    renderings v<k>.png of `size` = (H, W) with their clouds v<k>.ply (`cloud` points, or cloud[k] when it is a list, cycling
    over the pairs; encodings alternate).  Returns {"pairs": [(category, object, stem)] in the loader's order, "images": {pair:
    u8[H, W, 3]}, "clouds": {pair: f32[n, 3]}}."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    root = str(root)
    with open(os.path.join(root, "classes.txt"), "w") as f:
        for cat, name in CATEGORIES.items():
            f.write("%s %s\n" % (name, cat))
    out = {"pairs": [], "images": {}, "clouds": {}}
    k = 0
    for cat in sorted(CATEGORIES):
        ids = ["obj%d" % i for i in range(objects)]
        os.makedirs(os.path.join(root, "lists", cat), exist_ok=True)
        for split in splits:
            with open(os.path.join(root, "lists", cat, split + ".txt"), "w") as f:
                f.write("\n".join(ids) + "\n")
        for obj in ids:
            os.makedirs(os.path.join(root, "renderings", cat, obj), exist_ok=True)
            for v in range(views):
                stem = "v%d" % v
                img = rng.integers(0, 256, size=(size[0], size[1], 3), dtype=np.uint8)
                Image.fromarray(img, "RGB").save(os.path.join(root, "renderings", cat, obj, stem + ".png"))
                n = cloud[k % len(cloud)] if isinstance(cloud, (list, tuple)) else cloud
                xyz = rng.uniform(0.1, 0.9, size=(n, 3)).astype(np.float32)
                write_ply(os.path.join(root, "points", cat, obj, stem + ".ply"), xyz, "binary" if k % 2 else "ascii", colour=k % 3 == 0)
                pair = (cat, obj, stem)
                out["pairs"].append(pair)
                out["images"][pair], out["clouds"][pair] = img, xyz
                k += 1
    return out
