"""Cost of one training batch of the What3D reconstruction protocol (cloud_transformers_amd.data.image_point) beside the host
loader's per-item procedure (datasets/image_point.py:128-150 through data.image_point.ImageToPoint: per item a PLY read, the
resample, a PNG decode, Pillow's resize, ToTensor and Normalize; then the default collate and the two host-to-device copies of
train_image_reconstruction.py:166-167), in one process without loader workers.

    python tools/image_data_bench.py [--iters 2000] [--repeats 3] [--objects 16] [--cloud 10000]

B 4, 224 x 224 renderings -> 128 x 128, 8192 points, a temporary tree of `--objects` synthetic pairs (random pixels, random
points): `image_items` eager (the draws, the argsort and the one launch) and replayed from a HIP graph; `ct_image_items` alone,
20 launches per graph replay; the host procedure.  Every figure is the median of `--repeats` timed windows, with the lowest and
highest beside it.  The graph replays assemble the same 4 pairs every time, so their source bytes are cache-warm; a cold-cache
batch is not measured, nor are the reference's four loader workers overlapping the host procedure with the step."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gpu_ms(fn, iters, repeats, warmup=10):
    """[median, lowest, highest] of `repeats` windows of `iters` calls, each ended by a device synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return [round(float(np.median(out)), 5), round(min(out), 5), round(max(out), 5)]


def write_tree(root, objects, cloud, size, rng):
    """classes.txt, lists/c0/train.txt, renderings/c0/<obj>/v0.png and points/c0/<obj>/v0.ply (binary, float x y z)."""
    from PIL import Image
    with open(os.path.join(root, "classes.txt"), "w") as f:
        f.write("thing c0\n")
    ids = ["obj%03d" % i for i in range(objects)]
    os.makedirs(os.path.join(root, "lists", "c0"))
    with open(os.path.join(root, "lists", "c0", "train.txt"), "w") as f:
        f.write("\n".join(ids) + "\n")
    for obj in ids:
        for sub in ("renderings", "points"):
            os.makedirs(os.path.join(root, sub, "c0", obj))
        Image.fromarray(rng.integers(0, 256, size=(size, size, 3), dtype=np.uint8), "RGB").save(os.path.join(root, "renderings", "c0", obj, "v0.png"))
        n = int(cloud + rng.integers(-cloud // 10, cloud // 10 + 1))
        head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % n
        with open(os.path.join(root, "points", "c0", obj, "v0.ply"), "wb") as f:
            f.write(head.encode("ascii") + rng.random((n, 3), dtype=np.float32).astype("<f4").tobytes())


def host_procedure(ds, idx, dev):
    """What the upstream loop does for one batch: the items, the collate, then the image and the cloud on the device."""
    img, pcd = torch.utils.data.default_collate([ds[int(i)] for i in idx])
    return img.to(dev), pcd[:, :, None].to(dev, non_blocking=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--objects", type=int, default=16)
    ap.add_argument("--cloud", type=int, default=10000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_data_bench needs a GPU: nothing is measured without one")
    from cloud_transformers_amd.data.image_point import (DeviceImageToPoint, ImageToPoint, image_draws, image_items,
                                                         image_items_from_draws)
    dev = torch.device("cuda", 0)
    B, n, size, im_size = 4, 8192, 224, 128
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, args.objects, args.cloud, size, rng)
        host = ImageToPoint(root, split="train", im_size=im_size, points=n)
        ds = DeviceImageToPoint(host, dev)
        idx = rng.integers(0, len(host), size=B)
        item = torch.from_numpy(idx).to(dev)
        gen = None                                                          # (the device's default generator: known to graph capture)
        res = {"B": B, "points": n, "image": "%dx%d -> %dx%d" % (size, size, ds.OH, ds.OW), "pairs": len(ds), "p_cap": ds.p_cap,
               "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "format": "[median, lowest, highest] ms"}
        res["image_items_eager_ms"] = gpu_ms(lambda: image_items(ds, item, n, gen), args.iters, args.repeats)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            image_items(ds, item, n, gen)
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            outs = image_items(ds, item, n, gen)
        res["image_items_graph_replay_ms"] = gpu_ms(graph.replay, args.iters, args.repeats)
        assert bool(torch.isfinite(outs[0]).all()) and bool(torch.isfinite(outs[1]).all())
        perm, u_dup = image_draws(B, ds.p_cap, n, dev, gen)
        reps = 20
        kgraph = torch.cuda.CUDAGraph()
        image_items_from_draws(ds, item, perm, u_dup, n)
        torch.cuda.synchronize()
        with torch.cuda.graph(kgraph):
            for _ in range(reps):
                image_items_from_draws(ds, item, perm, u_dup, n)
        k = gpu_ms(kgraph.replay, max(args.iters // 4, 10), args.repeats)
        moved = B * (size * size * 3 + 3 * ds.OH * ds.OW * 4 + ds.p_cap * 8 + n * 4 + 2 * n * 12)      # image in / out, perm, u_dup, points in / out
        res["kernel_alone_ms"] = [round(v / reps, 6) for v in k]
        res["kernel_bytes_in_and_out"] = moved
        res["kernel_GB_per_s"] = round(moved / (k[0] / reps * 1e-3) / 1e9, 1)
        res["host_procedure_with_copies_ms"] = gpu_ms(lambda: host_procedure(host, idx, dev), max(args.iters // 100, 5), args.repeats, warmup=2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
