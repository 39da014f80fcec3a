"""Eval-mode BatchNorm on the fused kernels (ct_bn_eval_*), at kernel and at model level:

    python tools/bn_eval_bench.py [--part kernel|model|after|pw_norm|all] [--rounds 3] [--iters 20]

(a) kernel: eval BatchNorm1d + ReLU (+ the skip connection) as one ct_bn_eval_group_fwd launch (a table of one norm) against torch's modules, at
    tools/bn_bench.py's shapes and at a key norm's (B6 C48 N8192, cut over several workgroups); each replayed from a HIP
    graph and timed with device events after a warm-up.  The fused pass moves read x + write y (+ read residual): its
    bytes per second are printed as a share of the chip's measured float4 copy rate (6.29 TB/s).
(b) model: the eval + no-grad forward of the S3DIS segmenter's structure at B8 N4096 and of segmenter_pad's at B6 N8192
    (12 MultiHeadUnion blocks, model_dim 512; random weights, synthetic clouds), eager and replayed from a HIP graph, in
    fresh child processes that alternate CLOUDCT_BN_EVAL=1 / 0.  Only public API is used, so the same file runs on a
    revision without the eval kernels, where both settings are the module path and the rows give that revision's
    run-to-run spread.
(c) after: a union block's `after` at B8 N4096, 512 output channels — projection, eval BatchNorm1d, ReLU and the skip
    connection as ONE ct_pw_gemm_rs_norm launch against the GEMM followed by ct_bn_eval_group_fwd (ops.PW_NORM flipped in
    process: the same two kernels either way), graphed; the bytes the fusion removes are one write and one read of the
    [B, 512, N] tensor.
(d) pw_norm: the forwards of (b) in fresh child processes that alternate CLOUDCT_PW_NORM=1 / 0."""
import argparse
import json
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))

COPY_RATE = 6.29e12      # bytes/s, float4 copy on one MI355X
ZOO = [([4, 4], [128, 32]), ([16, 16], [64, 16]), ([16, 32], [16, 8])]


def timed(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters      # ms


def graphed(fn):
    """fn captured in a HIP graph after a side-stream warm-up; returns the replay callable."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def kernel_part(iters):
    import torch
    from cloud_transformers_amd import ops
    print("(a) eval BatchNorm1d + ReLU [+ skip], graphed, us per call; bytes = read x + write y [+ read skip]")
    for B, C, N in [(8, 512, 4096), (16, 512, 4096), (32, 512, 2048), (4, 512, 16384), (6, 48, 8192)]:
        bn = torch.nn.BatchNorm1d(C).cuda().eval()
        with torch.no_grad():
            bn.running_mean.uniform_(-1, 1)
            bn.running_var.uniform_(0.5, 2)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
        relu = torch.nn.ReLU()
        x = torch.randn(B, C, N, device="cuda")
        res = torch.randn(B, C, N, device="cuda")
        for skip in (False, True):
            r = res if skip else None
            with torch.no_grad():
                assert ops.bn_eval_eligible(bn, x, residual=r)
                fused = timed(graphed(lambda: ops.bn_eval(x, bn, True, r)), iters)
                lib = timed(graphed((lambda: r + relu(bn(x))) if skip else (lambda: relu(bn(x)))), iters)
            nbytes = (3 if skip else 2) * x.numel() * 4
            rate = nbytes / (fused * 1e-3)
            print(f"B{B} C{C} N{N}{' + skip' if skip else '       '}: fused {fused * 1e3:7.1f} us = {rate / 1e12:5.2f} TB/s "
                  f"({100 * rate / COPY_RATE:5.1f} % of the float4 copy rate) | torch modules {lib * 1e3:7.1f} us "
                  f"({lib / fused:4.2f}x)")
        if C == 48:      # the key / values norms carry no maxima: their channels are cut over several workgroups
            y = torch.empty_like(x)
            with torch.no_grad():
                cut = timed(graphed(lambda: ops._bn_eval_group(
                    [ops._bn_eval_item(bn, x.data_ptr(), 0, y.data_ptr(), 0, False)], B, N)), iters)
            rate = 2 * x.numel() * 4 / (cut * 1e-3)
            print(f"B{B} C{C} N{N} no maxima (channels cut): fused {cut * 1e3:7.1f} us = {rate / 1e12:5.2f} TB/s "
                  f"({100 * rate / COPY_RATE:5.1f} % of the float4 copy rate)")


def after_part(iters):
    import torch
    from torch import nn
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers.multihead_ct import run_after
    from cloud_transformers_amd.layers.pointwise import PointwiseConv1d
    print("(c) union `after` (projection + eval BatchNorm1d + ReLU + skip), B8 N4096, 512 output channels, graphed, us per call")
    B, Co, N = 8, 512, 4096
    for Ci in (128, 512, 768):                           # the concatenation widths of the segmenter's three block kinds
        torch.manual_seed(Ci)
        after = nn.Sequential(PointwiseConv1d(Ci, Co, kernel_size=1, bias=False), nn.BatchNorm1d(Co), nn.ReLU(inplace=True)).cuda().eval()
        with torch.no_grad():
            after[1].running_mean.uniform_(-0.2, 0.2)
            after[1].running_var.uniform_(0.5, 1.5)
            x = ops.bn_eval(torch.randn(B, Ci, N, device="cuda"), nn.BatchNorm1d(Ci).cuda().eval())      # carries its maxima, as a join's output
            res = torch.randn(B, Co, N, device="cuda")
            row = {}
            for flag in (True, False):
                ops.PW_NORM = flag
                try:
                    assert ops.pw_norm_eligible(after[0], [after[1]], x, residual=res) == flag
                    row[flag] = timed(graphed(lambda: run_after(after, x, res)), iters)
                    out = run_after(after, x, res)
                finally:
                    ops.PW_NORM = True
                row[flag, "out"] = out
            assert torch.equal(row[True, "out"], row[False, "out"])
        saved = 2 * B * Co * N * 4
        print(f"Ci{Ci:4d}: fused {row[True] * 1e3:7.1f} us | GEMM + ct_bn_eval_group_fwd {row[False] * 1e3:7.1f} us "
              f"({row[False] / row[True]:4.2f}x; {saved / 1e6:.0f} MB less traffic = {saved / COPY_RATE * 1e6:.1f} us at the copy rate)")


def build_model(name):
    import torch
    from torch import nn
    from cloud_transformers_amd.layers.multihead_ct import MultiHeadUnion
    from cloud_transformers_amd.layers.pointwise import convert_pointwise

    class Segmenter(nn.Module):
        """model_zoo/s3dis/segmenter.py's structure; pad: segmenter_pad.py's (stem on [xyz, 4 features], padding mask)."""

        def __init__(self, pad, n_classes=13, d=512):
            super().__init__()
            self.pad = pad
            self.first_process = nn.Sequential(nn.Conv1d(7 if pad else 6, d, kernel_size=1, bias=True), nn.BatchNorm1d(d),
                                               nn.ReLU(inplace=True))
            self.attentions_encoder = nn.ModuleList([MultiHeadUnion(model_dim=d, features_dims=f, heads=[16, 16], tensor_sizes=s,
                                                                    model_dim_out=d, tensor_dims=[2, 3])
                                                     for _ in range(4) for f, s in ZOO])
            self.final = nn.Sequential(nn.Conv1d(d, d, kernel_size=1, bias=False), nn.BatchNorm1d(d), nn.ReLU(inplace=True),
                                       nn.Conv1d(d, n_classes, kernel_size=1))

        def forward(self, xyz, pts_pad, features):       # xyz [B,3,N], features [B,3|4,N]
            x = self.first_process(torch.cat([xyz, features], dim=1))
            for blk in self.attentions_encoder:
                x, _ = blk(x, (xyz, pts_pad) if self.pad else xyz)
            return self.final(x)

    torch.manual_seed(0)
    pad = name == "segmenter_pad"
    B, N = (6, 8192) if pad else (8, 4096)
    net = convert_pointwise(Segmenter(pad).cuda()).eval()
    with torch.no_grad():                                # statistics and learned keys off their initial values
        for m in net.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                if float(m.weight.abs().max()) == 0.0:
                    m.weight.fill_(0.1)
    xyz = torch.rand(B, 3, N, device="cuda") * 2 - 1
    feats = torch.randn(B, 4 if pad else 3, N, device="cuda")
    mask = None
    if pad:
        mask = torch.ones(B, N, device="cuda", dtype=torch.int32)
        mask[:, N - 500:] = 0
    return net, (xyz, mask, feats)


def model_child(name, iters):
    import torch
    net, args = build_model(name)
    with torch.no_grad():
        eager = timed(lambda: net(*args), iters)
        graph = timed(graphed(lambda: net(*args)), iters)
    print(json.dumps({"model": name, "bn_eval": os.environ.get("CLOUDCT_BN_EVAL", "1"), "pw_norm": os.environ.get("CLOUDCT_PW_NORM", "1"),
                      "eager_ms": round(eager, 3), "graph_ms": round(graph, 3)}), flush=True)


def model_part(rounds, iters, switch="CLOUDCT_BN_EVAL"):
    print("(%s) eval + no-grad forward, ms (fresh process per row, %s alternating)" % ("b" if switch == "CLOUDCT_BN_EVAL" else "d", switch))
    for name in ("segmenter", "segmenter_pad"):
        rows = {"1": [], "0": []}
        for _ in range(rounds):
            for flag in ("1", "0"):
                env = dict(os.environ, **{switch: flag})
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(iters)], env=env,
                                     check=True, capture_output=True, text=True, timeout=600).stdout
                row = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
                rows[flag].append(row)
                print(f"{name:13s} {switch}={flag}: eager {row['eager_ms']:8.3f}  graph {row['graph_ms']:8.3f}", flush=True)
        for flag in ("1", "0"):
            for key in ("eager_ms", "graph_ms"):
                v = sorted(r[key] for r in rows[flag])
                print(f"{name:13s} {switch}={flag} {key[:-3]:5s}: min {v[0]:8.3f}  median {v[len(v) // 2]:8.3f}  max {v[-1]:8.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernel", "model", "after", "pw_norm", "all"], default="all")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return model_child(a.child, a.iters)
    if a.part in ("kernel", "all"):
        kernel_part(a.iters)
    if a.part in ("model", "all"):
        model_part(a.rounds, a.iters)
    if a.part in ("after", "all"):
        after_part(a.iters)
    if a.part in ("pw_norm", "all"):
        model_part(a.rounds, a.iters, switch="CLOUDCT_PW_NORM")


if __name__ == "__main__":
    main()
