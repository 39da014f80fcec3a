"""Cost of the ShapeNet completion protocol's per-batch preparation (cloud_transformers_amd.data.completion) beside the
upstream procedure restated on the host (utils/pcd_utils.py:24-51 and train_inpainter.py:178-183: per cloud, drop the zero
rows, draw the sphere noise, label and concatenate, resample; then stack and copy the three tensors to the device).

    python tools/completion_data_bench.py [--iters 200]

Per shape (B 2 and B 32 at n_in 2048, gt 16384): `completion_items` eager (the draws, the argsort and the one launch, from
device-resident loader output) and replayed from a HIP graph; `ct_completion_items` alone, 20 launches per graph replay, with
the bytes it has to move per second of that time; the host procedure including its three host-to-device copies."""
import argparse
import json
import os
import sys
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
