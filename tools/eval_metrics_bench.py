"""The metric side of `train_completion --eval`, per sample against batched, and ct_chamfer_fwd_counts against ct_chamfer_fwd.

  (a) the per-sample sequence of the batch-of-one loop, for 8 samples at n = m = 16384: ChamferDistance()(dense, gt),
      Metrics._get_f_score and Metrics._get_chamfer_distance — three dense Chamfer calls, fscore_batch, three .item();
  (b) Metrics.get_batch(with_dense=True) on the same 8 clouds as one batch, a TableMeter update, one copy at the end.

The two sides alternate in one process over HIP-event windows (tools/loss_bench.py's timing); (a) ends in host reads, so
its window also holds the host time between them.  Then ct_chamfer_fwd_counts with full counts against ct_chamfer_fwd at
B2 n = m = 16384 and B8 2048, alternating, with the spread of the windows.  Prints plain lines; --out FILE also writes them."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cloud_transformers_amd.chamfer import chamfer_with_counts, chamfer_with_indices  # noqa: E402
from cloud_transformers_amd.metrics import ChamferDistance, Metrics, TableMeter  # noqa: E402


def window(f, iters):
    """ms per call of f over one HIP-event window of `iters` calls."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(sides, iters, windows):
    """{name: [ms per call of each window]} with the sides taken in turn, after two warm-up calls of each."""
    for f in sides.values():
        f(), f()
    times = {name: [] for name in sides}
    for _ in range(windows):
        for name, f in sides.items():
            times[name].append(window(f, iters))
    return times


def summary(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    S, n = 8, 16384
    gt = torch.rand(S, n, 3, device=dev, generator=g) - 0.5
    dense = gt[:, torch.randperm(n, device=dev, generator=g)] + 0.004 * torch.randn(S, n, 3, device=dev, generator=g)
    dense[:, :64] = 0.0                                                    # padding rows for ignore_zeros to drop
    dense = dense.contiguous()
    chamfer = ChamferDistance()
    rows = torch.arange(S, device=dev) % 3

    def per_sample():
        out = []
        for k in range(S):
            d, t = dense[k:k + 1], gt[k:k + 1]
            out.append((chamfer(d, t).item() * 1000, Metrics._get_f_score(d, t), Metrics._get_chamfer_distance(d, t)))
        return out

    def batched():
        meter = TableMeter(3, 3, dev)
        meter.update(rows, Metrics.get_batch(dense, gt, with_dense=True))
        return meter.result()

    ref = per_sample()
    got = Metrics.get_batch(dense, gt, with_dense=True).cpu()
    worst = max(max(abs(float(got[k, 0]) - ref[k][1]), abs(float(got[k, 1]) - ref[k][2]) / ref[k][2], abs(float(got[k, 2]) - ref[k][0]) / ref[k][0])
                for k in range(S))
    say("metrics of %d samples at n = m = %d: batched against per sample, worst difference %.3g (F-Score absolute, Chamfer relative)" % (S, n, worst))
    t = alternate({"per_sample": per_sample, "batched": batched}, 3, args.windows)
    a, b = summary(t["per_sample"]), summary(t["batched"])
    say("  (a) per sample, 3 dense Chamfer + fscore_batch + 3 .item() each: median %.3f ms  (min %.3f, max %.3f) for the %d samples" % (a + (S,)))
    say("  (b) Metrics.get_batch B%d + TableMeter, one copy:                median %.3f ms  (min %.3f, max %.3f)" % ((S,) + b))
    say("  (a) / (b) = %.2f" % (a[0] / b[0]))

    for B, m in ((2, 16384), (8, 2048)):
        x = torch.rand(B, m, 3, device=dev, generator=g)
        y = torch.rand(B, m, 3, device=dev, generator=g)
        full = torch.full((B,), m, dtype=torch.int32, device=dev)
        same = all(torch.equal(p, q) for p, q in zip(chamfer_with_counts(x, y, full, full), chamfer_with_indices(x, y)))
        t = alternate({"dense": lambda: chamfer_with_indices(x, y), "dense_again": lambda: chamfer_with_indices(x, y),
                       "counts": lambda: chamfer_with_counts(x, y, full, full)}, 20, args.windows)
        d, d2, c = summary(t["dense"]), summary(t["dense_again"]), summary(t["counts"])
        say("chamfer forward B%d n = m = %d, outputs equal: %s" % (B, m, same))
        say("  ct_chamfer_fwd                      median %.1f us  (min %.1f, max %.1f)" % tuple(1e3 * v for v in d))
        say("  ct_chamfer_fwd, second series       median %.1f us  (min %.1f, max %.1f)" % tuple(1e3 * v for v in d2))
        say("  ct_chamfer_fwd_counts, full counts  median %.1f us  (min %.1f, max %.1f)   counts / dense = %.4f"
            % (tuple(1e3 * v for v in c) + (c[0] / d[0],)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
