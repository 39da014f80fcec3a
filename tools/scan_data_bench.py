"""Cost of one training batch of the ScanObjectNN classification protocol (cloud_transformers_amd.data.scanobjectnn) beside
the upstream per-item procedure restated on the host (datasets/scanobjectnn.py:102-122 through data.datasets.ScanObjectNN:
per item a randn(P, 3) jitter, the clip, the rotation, the copies; then the default collate, the `permute` and the three
host-to-device copies of train_classification.py:195-197), in one process without loader workers.

    python tools/scan_data_bench.py [--iters 5000] [--repeats 3]

B 8, N = P = 2048, a resident split of 11416 clouds (the main split's size, synthetic points): `scan_items` eager (the
draws, cos / sin and the one launch) and replayed from a HIP graph; `ct_scan_items` alone, 20 launches per graph replay; the
host procedure.  Every figure is the median of `--repeats` timed windows, with the lowest and highest beside it.  The
graph replays gather the same 8 clouds every time, so their source rows are cache-warm; a cold-cache batch is not measured."""
import argparse
import json
import os
import sys
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


def host_procedure(ds, idx, dev):
    """What the upstream loop does for one batch: the items, the collate, then the model's input and the targets on the device."""
    pcd, labels, mask = torch.utils.data.default_collate([ds[int(i)] for i in idx])
    pcd = pcd.permute(0, 2, 1)[:, :, None].to(dev)
    return pcd, labels.long().to(dev, non_blocking=True), mask.float().to(dev, non_blocking=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=11416)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_data_bench needs a GPU: nothing is measured without one")
    from cloud_transformers_amd.data import datasets as D
    from cloud_transformers_amd.data.scanobjectnn import DeviceScanObjectNN, scan_draws, scan_items, scan_items_from_draws
    dev = torch.device("cuda", 0)
    B, P, M = 8, 2048, args.clouds
    rng = np.random.default_rng(0)
    host = object.__new__(D.ScanObjectNN)                                   # the loader's arrays without a file
    host.data = (rng.random((M, P, 3), dtype=np.float32) - 0.5)
    host.mask = (rng.random((M, P)) > 0.3).astype(np.float64)
    host.label = rng.integers(0, 15, size=(M,)).astype(np.int64)
    host.train, host.subsample = True, None
    ds = DeviceScanObjectNN(host, dev)
    item = torch.from_numpy(rng.integers(0, M, size=B)).to(dev)
    gen = None                                                              # (the device's default generator: known to graph capture)
    res = {"B": B, "N": P, "P": P, "clouds": M, "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats,
           "format": "[median, lowest, highest] ms"}
    res["scan_items_eager_ms"] = gpu_ms(lambda: scan_items(ds, item, P, True, gen), args.iters, args.repeats)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scan_items(ds, item, P, True, gen)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        outs = scan_items(ds, item, P, True, gen)
    res["scan_items_graph_replay_ms"] = gpu_ms(graph.replay, args.iters, args.repeats)
    assert bool(torch.isfinite(outs[0]).all())
    perm, rot, jit = scan_draws(B, P, P, True, dev, gen)
    reps = 20
    kgraph = torch.cuda.CUDAGraph()
    scan_items_from_draws(ds, item, perm, rot, jit, P)
    torch.cuda.synchronize()
    with torch.cuda.graph(kgraph):
        for _ in range(reps):
            scan_items_from_draws(ds, item, perm, rot, jit, P)
    k = gpu_ms(kgraph.replay, max(args.iters // 4, 10), args.repeats)
    moved = B * (P * (12 + 1) + P * 12 + 8 + 8 + 3 * P * 4 + P * 4 + 8)    # points, mask bytes, jitter, (cos, sin), item; outputs
    res["kernel_alone_ms"] = [round(v / reps, 6) for v in k]
    res["kernel_bytes_in_and_out"] = moved
    res["kernel_GB_per_s"] = round(moved / (k[0] / reps * 1e-3) / 1e9, 1)
    idx = rng.integers(0, M, size=B)
    res["host_procedure_with_copies_ms"] = gpu_ms(lambda: host_procedure(host, idx, dev), max(args.iters // 20, 5), args.repeats, warmup=3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
