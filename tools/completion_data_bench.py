"""Cost of the ShapeNet completion protocol's per-batch preparation (cloud_transformers_amd.data.completion) beside the
upstream procedure restated on the host (utils/pcd_utils.py:24-51 and train_inpainter.py:178-183: per cloud, drop the zero
rows, draw the sphere noise, label and concatenate, resample; then stack and copy the three tensors to the device).

    python tools/completion_data_bench.py [--iters 200]

Per shape (B 2 and B 32 at n_in 2048, gt 16384): `completion_items` eager (the draws, the argsort and the one launch, from
device-resident loader output) and replayed from a HIP graph; `ct_completion_items` alone, 20 launches per graph replay, with
the bytes it has to move per second of that time; the host procedure including its three host-to-device copies.

Then the items themselves (key "resident"), on a synthetic ShapeNetCompletion-like tree of binary .pcd files written to a
temporary directory (--models models of 8 renderings of 1200 .. 3600 points, gt clouds of 16384) and kept on the device as a
`DeviceShapeNetCompletion`; per shape, all in this one run: `completion_gather` eager and replayed from a HIP graph;
`ct_completion_gather` alone, 20 launches per graph replay; a whole `DeviceCompletionBatches` batch (the gather, the items'
draws and `ct_completion_items`); and the host path for the same batch size: the `Dataset` items (two file reads and the numpy
transforms each), `collate_fn` and the two host-to-device copies with the `2 *`, in this process without workers, the files
in the page cache."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gpu_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def host_procedure(partial, gtcloud, dev):
    """What the upstream training loop does with one loader batch (host tensors in, the model's three inputs on the device out)."""
    gt = (2 * gtcloud.permute(0, 2, 1)[:, :, None]).to(dev, non_blocking=True)
    scaled, gt_size, n_in = 2 * partial, gtcloud.shape[1], partial.shape[1]
    parts, labelled = [], []
    for b in range(scaled.shape[0]):
        cur = scaled[b]
        kept = cur[~(cur == 0.0).all(dim=1)]
        m = gt_size - kept.shape[0]
        theta = 2 * np.pi * torch.rand(1, m)
        phi = torch.acos(1 - 2 * torch.rand(1, m))
        sph = torch.stack([torch.sin(phi) * torch.cos(theta), torch.sin(phi) * torch.sin(theta), torch.cos(phi)], dim=1)[0].permute(1, 0)
        labelled.append(torch.cat([torch.cat([sph, torch.zeros(m, 1)], dim=1), torch.cat([kept, torch.ones(kept.shape[0], 1)], dim=1)], dim=0))
        idx = np.random.permutation(kept.shape[0])
        if idx.shape[0] < n_in:
            idx = np.concatenate([idx, np.random.randint(kept.shape[0], size=n_in - kept.shape[0])])
        parts.append(kept[idx[:n_in]])
    enc = torch.stack(parts, dim=0).permute(0, 2, 1)[:, :, None].to(dev)
    noise = torch.stack(labelled, dim=0).permute(0, 2, 1).to(dev)
    return noise, enc, gt


def write_binary_pcd(path, xyz):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    n = xyz.shape[0]
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH %d\n"
            "HEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (n, n))
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(np.ascontiguousarray(xyz, dtype="<f4").tobytes())


def synthetic_tree(root, models, renders, gt_size, seed=0):
    """A train subset of `models` models in two taxonomies; returns the `data` keys of the reference config for it."""
    rng = np.random.default_rng(seed)
    ids = ["m%04d" % k for k in range(models)]
    cats = [{"taxonomy_id": "02691156", "taxonomy_name": "a", "train": ids[::2], "val": [], "test": []},
            {"taxonomy_id": "03001627", "taxonomy_name": "b", "train": ids[1::2], "val": [], "test": []}]
    with open(os.path.join(root, "ShapeNet.json"), "w") as f:
        json.dump(cats, f)
    for c in cats:
        for m in c["train"]:
            gt = (rng.random((gt_size, 3), dtype=np.float32) - 0.5)
            write_binary_pcd(os.path.join(root, "train", "complete", c["taxonomy_id"], m + ".pcd"), gt)
            for r in range(renders):
                write_binary_pcd(os.path.join(root, "train", "partial", c["taxonomy_id"], m, "%02d.pcd" % r),
                                 gt[rng.permutation(gt_size)[:int(rng.integers(1200, 3601))]])
    return {"category_path": os.path.join(root, "ShapeNet.json"), "partial_path": os.path.join(root, "%s", "partial", "%s", "%s", "%02d.pcd"),
            "gt_path": os.path.join(root, "%s", "complete", "%s", "%s.pcd"), "n_renders": renders, "input_size": 2048, "gt_size": gt_size}


def resident_rows(args, dev, n_in, gt):
    from cloud_transformers_amd.data import completion as C
    out = {}
    with tempfile.TemporaryDirectory() as root:
        host_ds = C.shapenet_loader(synthetic_tree(root, args.models, 8, gt)).get_dataset(C.DatasetSubset.TRAIN)
        t0 = time.perf_counter()
        ds = C.DeviceShapeNetCompletion(host_ds, dev)
        torch.cuda.synchronize()
        out["split"] = {"models": ds.M, "renderings": ds.R, "p_cap": ds.p_cap, "g_cap": ds.g_cap, "resident_bytes": ds.nbytes,
                        "decode_and_upload_s": round(time.perf_counter() - t0, 3)}
        for B in (2, 32):
            gen = torch.Generator(device=dev).manual_seed(B)
            item = torch.randint(0, ds.M, (B,), device=dev, generator=gen)
            row = {}
            row["completion_gather_eager_ms"] = round(gpu_ms(lambda: C.completion_gather(ds, item, True, gen), args.iters), 4)
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                C.completion_gather(ds, item, True)
            torch.cuda.current_stream().wait_stream(side)
            with torch.cuda.graph(graph):
                outs = C.completion_gather(ds, item, True)
            row["completion_gather_graph_replay_ms"] = round(gpu_ms(graph.replay, args.iters), 4)
            assert bool(torch.isfinite(outs[1]).all())
            draws = C.completion_gather_draws(ds, B, True, gen)
            reps = 20
            kgraph = torch.cuda.CUDAGraph()
            C.completion_gather_from_draws(ds, item, *draws)
            torch.cuda.synchronize()
            with torch.cuda.graph(kgraph):
                for _ in range(reps):
                    C.completion_gather_from_draws(ds, item, *draws)
            k_ms = gpu_ms(kgraph.replay, max(args.iters // 4, 10)) / reps
            moved = B * ((ds.p_cap + ds.g_cap) * 8 + 2 * (n_in + gt) * 12)         # both permutations once, every output row read and written
            row["kernel_alone_ms"] = round(k_ms, 5)
            row["kernel_bytes_in_and_out"] = moved
            row["kernel_GB_per_s"] = round(moved / (k_ms * 1e-3) / 1e9, 1)
            row["workgroups_per_row"] = min(-(-max(ds.p_cap, n_in) // 1024), 32) + min(-(-max(ds.g_cap, gt) // 1024), 32)
            batches = C.DeviceCompletionBatches(ds, B, train=True, seed=1)
            state = {"it": iter(batches), "epoch": 0}

            def device_batch():
                try:
                    return next(state["it"])
                except StopIteration:
                    state["epoch"] += 1
                    batches.set_epoch(state["epoch"])
                    state["it"] = iter(batches)
                    return next(state["it"])

            row["device_batch_ms"] = round(gpu_ms(device_batch, args.iters), 4)
            order = np.random.default_rng(B).integers(0, len(host_ds), size=(64, B))
            step = {"k": 0}

            def host_batch():
                idx = order[step["k"] % len(order)]
                step["k"] += 1
                _, _, data = C.collate_fn([host_ds[int(i)] for i in idx])
                return 2 * data["gtcloud"].to(dev, non_blocking=True), data["partial_cloud"].to(dev, non_blocking=True)

            row["host_items_collate_copies_ms"] = round(gpu_ms(host_batch, max(args.iters // 10, 5), warmup=2), 3)
            out["B%d" % B] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--models", type=int, default=64, help="models of the synthetic resident split")
    args = ap.parse_args()
    from cloud_transformers_amd.data.completion import completion_draws, completion_items, completion_items_from_draws
    dev = torch.device("cuda", 0)
    n_in, gt = 2048, 16384
    res = {"n_in": n_in, "gt": gt, "device": torch.cuda.get_device_name(0)}
    for B in (2, 32):
        g = torch.Generator().manual_seed(B)
        partial = torch.rand(B, n_in, 3, generator=g) - 0.5
        for b in range(B):
            partial[b, n_in - (b * 997) % 1500:] = 0.0             # zero tails of mixed length, as the loader pads short renderings
        gtcloud = torch.rand(B, gt, 3, generator=g) - 0.5
        p_dev = partial.to(dev)
        row = {}
        row["completion_items_eager_ms"] = round(gpu_ms(lambda: completion_items(p_dev, gt), args.iters), 4)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            completion_items(p_dev, gt)
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            outs = completion_items(p_dev, gt)
        row["completion_items_graph_replay_ms"] = round(gpu_ms(graph.replay, args.iters), 4)
        assert int(outs[2].min()) > 0
        draws = completion_draws(B, n_in, gt, dev)
        reps = 20
        kgraph = torch.cuda.CUDAGraph()
        completion_items_from_draws(p_dev, *draws)
        torch.cuda.synchronize()
        with torch.cuda.graph(kgraph):
            for _ in range(reps):
                completion_items_from_draws(p_dev, *draws)
        k_ms = gpu_ms(kgraph.replay, max(args.iters // 4, 10)) / reps
        moved = B * (n_in * (12 + 8 + 4) + 3 * gt * 4 + n_in * 12 + 4 * gt * 4 + 4)
        row["kernel_alone_ms"] = round(k_ms, 5)
        row["kernel_bytes_in_and_out"] = moved
        row["kernel_GB_per_s"] = round(moved / (k_ms * 1e-3) / 1e9, 1)
        row["workgroups_per_cloud"] = min(max((512 + B - 1) // B, 1), (gt + 1023) // 1024)
        host_iters = max(args.iters // 10, 5)
        row["host_procedure_with_copies_ms"] = round(gpu_ms(lambda: host_procedure(partial, gtcloud, dev), host_iters, warmup=2), 3)
        res["B%d" % B] = row
    res["resident"] = resident_rows(args, dev, n_in, gt)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
