"""Cost of one training batch of the S3DIS 1x1 m block protocol (cloud_transformers_amd.data.s3dis_blocks) beside the host
loader's (data.datasets.Indoor3DSemSeg with aug=True: per item the shuffle and eight numpy transforms, among them a float64
RGB -> HSV -> RGB round trip; then the default collate, the `permute` and the host-to-device copies of
train_segmentation.py:180-181), and what either does to the segmenter's training step.

    python tools/block_data_bench.py [--iters 2000] [--repeats 3] [--blocks 4096] [--steps 30] [--workers 8]

B 8, N = P = 4096, a resident split of `--blocks` synthetic blocks.
- `block_items` eager (the draws, the stage choices and the one launch) and replayed from a HIP graph; `ct_block_items`
  alone, 20 launches per graph replay, with the auto-contrast taken by every row and by none;
- the host loader's eight items with the collate and the copies, in this process;
- `ct_seg_confusion` (eager, and 20 launches per graph replay) against torch's argmax + bincount on the same predictions;
- the S3DIS-shaped segmenter's step (tools/segmenter_step_bench.py: forward + loss + backward as one HIP graph, SGD step and
  the train confusion outside it) fed by `BlockBatches`, by the host loader in this process and by a DataLoader with
  `--workers` worker processes.
Every kernel figure is the median of `--repeats` timed windows, with the lowest and highest beside it.  The graph replays
gather the same 8 blocks every time, so their source rows are cache-warm; a cold-cache batch is not measured."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


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


def graph_of(fn, reps=1, warm=1):
    """A HIP graph of `reps` calls of fn (after `warm` calls outside it, on a side stream)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            out = fn()
    return graph, out


def host_batch(ds, idx, dev):
    """What the upstream loop does for one batch: the items, the collate, then the model's input and the targets on the device."""
    pcd, labels = torch.utils.data.default_collate([ds[int(i)] for i in idx])
    return pcd.permute(0, 2, 1)[:, :, None].to(dev), labels.to(dev, non_blocking=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--no-step", action="store_true", help="skip the segmenter's step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("block_data_bench needs a GPU: nothing is measured without one")
    from cloud_transformers_amd.data import datasets as D
    from cloud_transformers_amd.data.s3dis_blocks import (BlockBatches, DeviceS3DISBlocks, SegmentationMeter, block_draws, block_items,
                                                          block_items_from_draws)
    dev = torch.device("cuda", 0)
    B, P, M, C = 8, 4096, args.blocks, 13
    rng = np.random.default_rng(0)
    host = object.__new__(D.Indoor3DSemSeg)                                 # the loader's arrays without files
    host.points = rng.random((M, P, 9), dtype=np.float32)
    host.points[:, :, :3] = host.points[:, :, :3] * 2 - 0.5
    host.labels = rng.integers(0, C, size=(M, P)).astype(np.uint8)
    host.num_points, host.aug, host.train, host.data_precent, host.test_area = P, True, True, 1.0, "Area_5"
    ds = DeviceS3DISBlocks(host, dev)
    item = torch.from_numpy(rng.integers(0, M, size=B)).to(dev)
    gen = None                                                              # (the device's default generator: known to graph capture)
    res = {"B": B, "N": P, "P": P, "blocks": M, "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats,
           "format": "[median, lowest, highest] ms"}

    # -- the batch assembly --------------------------------------------------------------------------------------------
    res["block_items_eager_ms"] = gpu_ms(lambda: block_items(ds, item, P, True, True, gen), args.iters, args.repeats)
    graph, outs = graph_of(lambda: block_items(ds, item, P, True, True, gen))
    res["block_items_graph_replay_ms"] = gpu_ms(graph.replay, args.iters, args.repeats)
    assert bool(torch.isfinite(outs[0]).all())
    perm, aug, jit, cjit = block_draws(B, P, True, True, dev, gen)
    reps = 20
    moved = B * (P * (24 + 1) + P * 8 + 64 + 2 * P * 12 + 6 * P * 4 + P * 8 + 8)     # rows, label bytes, perm, aug, jitters; outputs
    for name, w in (("contrast_all", 0.5), ("contrast_none", -1.0)):
        a = aug.clone()
        a[:, 5] = w
        kgraph, _ = graph_of(lambda: block_items_from_draws(ds, item, perm, a, jit, cjit, P), reps)
        k = gpu_ms(kgraph.replay, max(args.iters // 4, 10), args.repeats)
        res["kernel_alone_%s_ms" % name] = [round(v / reps, 6) for v in k]
        res["kernel_%s_GB_per_s" % name] = round(moved / (k[0] / reps * 1e-3) / 1e9, 1)
    res["kernel_bytes_in_and_out"] = moved
    idx = rng.integers(0, M, size=B)
    res["host_loader_with_copies_ms"] = gpu_ms(lambda: host_batch(host, idx, dev), max(args.iters // 100, 5), args.repeats, warmup=2)

    # -- the confusion matrix -----------------------------------------------------------------------------------------
    pred = torch.randn(B, C, 1, P, device=dev)
    labels = torch.randint(C, (B, P), device=dev)
    meter = SegmentationMeter(C)
    conf_t = torch.zeros(C * C, dtype=torch.int64, device=dev)

    def torch_confusion():
        conf_t.add_(torch.bincount((labels * C + pred[:, :, 0].argmax(dim=1)).reshape(-1), minlength=C * C))

    meter.update(pred, labels)
    torch_confusion()
    assert torch.equal(meter.conf.reshape(-1), conf_t)
    g1, _ = graph_of(lambda: meter.update(pred, labels), reps)
    res["ct_seg_confusion_ms"] = [round(v / reps, 6) for v in gpu_ms(g1.replay, max(args.iters // 4, 10), args.repeats)]
    res["torch_argmax_bincount_eager_ms"] = gpu_ms(torch_confusion, args.iters, args.repeats)
    res["ct_seg_confusion_eager_ms"] = gpu_ms(lambda: meter.update(pred, labels), args.iters, args.repeats)
    # (bincount reads the data's maximum back to size its output, so the torch form synchronises and cannot be captured)

    # -- the segmenter's step ------------------------------------------------------------------------------------------
    if not args.no_step:
        from segmenter_step_bench import Segmenter
        from cloud_transformers_amd.layers.pointwise import convert_pointwise
        torch.manual_seed(0)
        net = convert_pointwise(Segmenter().cuda()).train()
        opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
        ce = torch.nn.CrossEntropyLoss()
        cloud, target = torch.zeros(B, 6, 1, P, device=dev), torch.zeros(B, P, dtype=torch.int64, device=dev)
        static = {}

        def fwd_bwd():
            opt.zero_grad(set_to_none=True)
            pred = net(cloud[:, :, 0])
            static["pred"] = pred.detach()                                  # (no grad_fn kept across steps: see harness._loss)
            loss = ce(pred, target)
            loss.backward()
            return loss

        cloud.copy_(block_items(ds, item, P, True, True, gen)[0][:, :, None])
        target.copy_(labels)
        graph_step, _ = graph_of(fwd_bwd, warm=3)
        train_meter = SegmentationMeter(C)

        def step(batch):
            cloud.copy_(batch[0], non_blocking=True)
            target.copy_(batch[1], non_blocking=True)
            graph_step.replay()
            opt.step()
            train_meter.update(static["pred"], target)

        def timed(batches):
            it = iter(batches)
            for _ in range(3):
                step(next(it))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(next(it))
            torch.cuda.synchronize()
            return round((time.perf_counter() - t0) * 1e3 / args.steps, 3)

        def fixed():
            batch = block_items(ds, item, P, True, True, gen)
            batch = (batch[0][:, :, None], batch[1])
            while True:
                yield batch

        def host_in_process():
            while True:
                yield host_batch(host, rng.integers(0, M, size=B), dev)

        def host_workers():
            from cloud_transformers_amd.harness import worker_init_fn
            loader = torch.utils.data.DataLoader(host, batch_size=B, shuffle=True, num_workers=args.workers, drop_last=True,
                                                 worker_init_fn=worker_init_fn)
            for pcd, lab in loader:
                yield pcd.permute(0, 2, 1)[:, :, None].to(dev), lab.to(dev, non_blocking=True)

        res["steps"] = args.steps
        res["step_on_a_resident_batch_ms"] = timed(fixed())
        res["step_fed_by_block_batches_ms"] = timed(BlockBatches(ds, B, train=True, aug=True, seed=0, drop_last=True))
        res["step_fed_by_host_loader_in_process_ms"] = timed(host_in_process())
        if args.workers > 0:
            res["step_fed_by_host_loader_%d_workers_ms" % args.workers] = timed(host_workers())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
