"""Eval-mode head norms in the Slice write-out (ct_slice_fwd_norm / ct_mhct_core_fwd_norm), at kernel and at model level:

    python tools/slice_norm_bench.py [--part kernel|model|default|all] [--rounds 3] [--iters 20]

(a) kernel: the heads of the S3DIS segmenter's three block kinds at B8 N4096 (H16; 2D 128^2 C4 / 64^2 C16 / 16^2 C16 and 3D 32^3 C4
    / 16^3 C16 / 8^3 C32) — Slice (or the plane-resident core) with the head's eval BatchNorm1d + ReLU in its store against the
    same kernel followed by ct_bn_eval_group_fwd, each replayed from a HIP graph and timed with device events after a warm-up.
    The bytes the fusion removes are one write and one read of the head's [B, H*C, N] tensor.
(b) model: the eval + no-grad forward of the segmenter's structure at B8 N4096 (tools/bn_eval_bench.py's model: 12
    MultiHeadUnion blocks, model_dim 512; random weights, synthetic clouds), eager and replayed from a HIP graph, in fresh child
    processes that alternate CLOUDCT_SLICE_NORM=1 / 0.
(c) default: the same forward with the switch left alone, three fresh processes — only public API, so the same file runs on a
    revision without the switch: this commit's default path against its parent's."""
import argparse
import json
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)

from bn_eval_bench import COPY_RATE, build_model, graphed, timed  # noqa: E402

HEADS = [(2, 128, 4), (2, 64, 16), (2, 16, 16), (3, 32, 4), (3, 16, 16), (3, 8, 32)]      # (dim, W, C) at H16


def kernel_part(iters):
    import torch
    from cloud_transformers_amd import ops
    B, H, N = 8, 16, 4096
    print("(a) a head's Slice + eval BatchNorm1d + ReLU at B8 H16 N4096, graphed, us per call")
    saved = ops.SLICE_NORM
    for dim, W, C in HEADS:
        torch.manual_seed(C * W)
        HC = H * C
        bn = torch.nn.BatchNorm1d(HC).cuda().eval()
        with torch.no_grad():
            bn.running_mean.uniform_(-1, 1)
            bn.running_var.uniform_(0.5, 2)
            bn.weight.uniform_(-1.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
            keys = torch.tanh(torch.randn(B, H * dim, N, device="cuda"))
            core = ops.mhct_core_supported(B, H, C, N, [W] * dim)
            if core:
                feat = torch.randn(B, HC, N, device="cuda")
                w = torch.randn(HC, C, *([3] * dim), device="cuda") / (C * 3 ** dim) ** 0.5
                bias = torch.randn(HC, device="cuda") * 0.1
                two = lambda: ops.bn_eval(ops.mhct_core(keys, feat, None, w, bias, W, H, dim)[0], bn)
                one = lambda: ops.mhct_core_norm(keys, feat, None, w, bias, W, H, dim, ops.NormTarget(bn))[0]
            else:
                grid = torch.randn(B, HC, *([W] * dim), device="cuda")
                two = lambda: ops.bn_eval(ops.slice_keys(keys, grid, None, W, H, dim), bn)
                one = lambda: ops.slice_keys_norm(keys, grid, None, W, H, dim, ops.NormTarget(bn))
            ops.SLICE_NORM = True
            try:
                assert torch.equal(one(), two())
                t_two, t_one = timed(graphed(two), iters), timed(graphed(one), iters)
            finally:
                ops.SLICE_NORM = saved
        nbytes = 2 * B * HC * N * 4
        print(f"{W}^{dim} C{C:<2d} ({'core ' if core else 'slice'}): fused {t_one * 1e3:7.1f} us | + ct_bn_eval_group_fwd {t_two * 1e3:7.1f} us "
              f"({t_two / t_one:4.2f}x; {nbytes / 1e6:5.1f} MB less traffic = {nbytes / COPY_RATE * 1e6:4.1f} us at the copy rate)")


def model_child(iters):
    import torch
    net, args = build_model("segmenter")
    with torch.no_grad():
        eager = timed(lambda: net(*args), iters)
        graph = timed(graphed(lambda: net(*args)), iters)
    print(json.dumps({"slice_norm": os.environ.get("CLOUDCT_SLICE_NORM", "unset"), "eager_ms": round(eager, 3),
                      "graph_ms": round(graph, 3)}), flush=True)


def _child(env, iters):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(iters)], env=env, check=True,
                         capture_output=True, text=True, timeout=600).stdout
    return json.loads([line for line in out.splitlines() if line.startswith("{")][-1])


def _summary(label, rows):
    for key in ("eager_ms", "graph_ms"):
        v = sorted(r[key] for r in rows)
        print(f"{label} {key[:-3]:5s}: min {v[0]:8.3f}  median {v[len(v) // 2]:8.3f}  max {v[-1]:8.3f}")


def model_part(rounds, iters):
    print("(b) segmenter B8 N4096, eval + no-grad forward, ms (fresh process per row, CLOUDCT_SLICE_NORM alternating)")
    rows = {"1": [], "0": []}
    for _ in range(rounds):
        for flag in ("1", "0"):
            row = _child(dict(os.environ, CLOUDCT_SLICE_NORM=flag), iters)
            rows[flag].append(row)
            print(f"CLOUDCT_SLICE_NORM={flag}: eager {row['eager_ms']:8.3f}  graph {row['graph_ms']:8.3f}", flush=True)
    for flag in ("1", "0"):
        _summary("CLOUDCT_SLICE_NORM=%s" % flag, rows[flag])
    # what the switch removes by arithmetic: one write and one read of every union block's [B, sum H*C, N] concatenation
    from bn_eval_bench import ZOO
    nbytes = sum(2 * 8 * sum(16 * f for f in feats) * 4096 * 4 for _ in range(4) for feats, _ in ZOO)
    print(f"bytes removed by arithmetic: {nbytes / 1e6:.0f} MB per forward = {nbytes / COPY_RATE * 1e3:.3f} ms at the copy rate")


def default_part(rounds, iters):
    print("(c) segmenter B8 N4096, eval + no-grad forward, ms, the switch left alone (fresh process per row)")
    env = {k: v for k, v in os.environ.items() if k != "CLOUDCT_SLICE_NORM"}
    rows = []
    for _ in range(rounds):
        rows.append(_child(env, iters))
        print(f"default path: eager {rows[-1]['eager_ms']:8.3f}  graph {rows[-1]['graph_ms']:8.3f}", flush=True)
    _summary("default path", rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernel", "model", "default", "all"], default="all")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return model_child(a.iters)
    if a.part in ("kernel", "all"):
        kernel_part(a.iters)
    if a.part in ("model", "all"):
        model_part(a.rounds, a.iters)
    if a.part in ("default", "all"):
        default_part(a.rounds, a.iters)


if __name__ == "__main__":
    main()
