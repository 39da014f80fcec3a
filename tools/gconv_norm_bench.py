"""Eval-mode norms of the grouped-conv Res blocks in the convolution's write-out (ct_gconv_fwd_norm), at block and at kernel level:

    python tools/gconv_norm_bench.py [--part blocks|plain|all] [--rounds 3] [--iters 300] [--parent-lib PATH]

(a) blocks: the eval + no-grad forward of the Res blocks the classifier / inpainter tails are made of (groups 16), at B8 and B2:
    Res3DBlock(512, 1024) on 8^3, Res3DBlock(1024, 1024) on 4^3 and 2^3, Res2DBlock(256, 512) on 16^2, (512, 1024) on 8^2 and
    (1024, 1024) on 4^2 — with ops.GCONV_NORM on (two convolution launches and the skip GEMM) and off (the modules' path: three
    torch BatchNorm launches, an add and two ReLUs more), each replayed from a HIP graph and timed with device events after a
    warm-up, the two settings alternating over the rounds.
(b) plain: ct_gconv_fwd on the convolutions of those blocks, this build against a build of the parent commit (--parent-lib, a
    libcloudct.so of that revision), in fresh child processes that alternate the two libraries; each child loads its library
    with ctypes alone, so the same file runs against a library without the new symbols.  The plain kernels are meant to be the
    same code: this build's median has to lie within the parent's own spread over its runs."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)

from bn_eval_bench import graphed, timed  # noqa: E402

GROUPS = 16
BLOCKS = [(3, 512, 1024, 8), (3, 1024, 1024, 4), (3, 1024, 1024, 2),
          (2, 256, 512, 16), (2, 512, 1024, 8), (2, 1024, 1024, 4)]        # (dim, in_planes, out_planes, W): the tails' stages
BATCHES = (8, 2)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _block(dim, cin, cout, seed):
    import torch
    from cloud_transformers_amd.layers.grouped_conv import Res2DBlock, Res3DBlock
    torch.manual_seed(seed)
    blk = (Res3DBlock if dim == 3 else Res2DBlock)(cin, cout, groups=GROUPS)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 2)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    return blk.cuda().eval()


def blocks_part(rounds, iters):
    import torch
    from cloud_transformers_amd import ops
    print("(a) Res block, eval + no-grad forward, graphed, us per forward: ops.GCONV_NORM on | off, median of %d alternating rounds "
          "of %d replays (min .. max)" % (rounds, iters))
    saved = ops.GCONV_NORM
    worst = 0.0
    try:
        for dim, cin, cout, W in BLOCKS:
            for B in BATCHES:
                blk = _block(dim, cin, cout, cin + W)
                x = torch.randn(B, cin, *([W] * dim), device="cuda")
                with torch.no_grad():
                    ops.GCONV_NORM = True
                    got, on = blk(x), graphed(lambda: blk(x))
                    ops.GCONV_NORM = False
                    want, off = blk(x), graphed(lambda: blk(x))
                err = float((got - want).abs().max()) / max(1.0, float(want.abs().max()))
                assert err <= 1e-4, err
                t_on, t_off = [], []
                for _ in range(rounds):
                    t_on.append(timed(on, iters) * 1e3)
                    t_off.append(timed(off, iters) * 1e3)
                ratio = _median(t_on) / _median(t_off)
                worst = max(worst, ratio)
                print(f"Res{dim}DBlock({cin:4d}, {cout:4d}) {W:2d}^{dim} B{B}: on {_median(t_on):7.1f} ({min(t_on):7.1f} .. {max(t_on):7.1f}) | "
                      f"off {_median(t_off):7.1f} ({min(t_off):7.1f} .. {max(t_off):7.1f})  on/off {ratio:4.2f}", flush=True)
    finally:
        ops.GCONV_NORM = saved
    print("largest on/off ratio: %.2f (%s)" % (worst, "the fused block is nowhere slower" if worst <= 1.0 else "SLOWER somewhere"))


def _conv_shapes():
    """the distinct (B, groups, Cin, Cout, W) of the two 3^d convolutions of every block"""
    seen = []
    for dim, cin, cout, W in BLOCKS:
        for B in BATCHES:
            for ci in (cin, cout):
                s = (B, GROUPS, ci // GROUPS, cout // GROUPS, (W,) * dim)
                if s not in seen:
                    seen.append(s)
    return seen


def plain_child(lib_path, iters):
    import torch
    from cloud_transformers_amd.ops import _stream
    lib = ctypes.CDLL(lib_path)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.ct_gconv_fwd.restype = i
    lib.ct_gconv_fwd.argtypes = [vp, vp, vp, vp, i, i, i, i, i, ctypes.POINTER(i), vp]
    out = {}
    for B, G, Cin, Cout, W in _conv_shapes():
        torch.manual_seed(Cin * W[0])
        x = torch.randn(B, G * Cin, *W, device="cuda")
        w = torch.randn(G * Cout, Cin, *([3] * len(W)), device="cuda")
        y = torch.empty(B, G * Cout, *W, device="cuda")
        Wa = (i * len(W))(*W)

        def run():
            rc = lib.ct_gconv_fwd(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), B, G, Cin, Cout, len(W), Wa, _stream())
            assert rc == 0, rc

        out["B%d %d->%d %s" % (B, Cin, Cout, "x".join(map(str, W)))] = round(timed(graphed(run), iters) * 1e3, 2)
    print(json.dumps(out), flush=True)


def plain_part(rounds, iters, parent_lib):
    from cloud_transformers_amd import _lib
    this_lib = _lib.build()
    if not parent_lib or not os.path.exists(parent_lib):
        raise SystemExit("--parent-lib: a libcloudct.so built from the parent commit is needed for part (b)")
    print("(b) ct_gconv_fwd (no bias), graphed, us per call, channels per group at groups 16: this build | the parent's, %d fresh "
          "processes each, alternating, %d replays" % (rounds, iters))
    rows = {"this": [], "parent": []}
    for _ in range(rounds):
        for name, path in (("this", this_lib), ("parent", parent_lib)):
            env = {k: v for k, v in os.environ.items() if k != "CLOUDCT_LIB"}
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--iters", str(iters)], env=env, check=True,
                                 capture_output=True, text=True, timeout=900).stdout
            rows[name].append(json.loads([line for line in res.splitlines() if line.startswith("{")][-1]))
    outside = 0
    for key in rows["this"][0]:
        t = [r[key] for r in rows["this"]]
        p = [r[key] for r in rows["parent"]]
        ok = min(p) <= _median(t) <= max(p)
        outside += not ok
        print(f"{key:24s}: this {_median(t):7.2f} ({min(t):7.2f} .. {max(t):7.2f}) | parent {_median(p):7.2f} ({min(p):7.2f} .. {max(p):7.2f})"
              f"  {'within the parent spread' if ok else ('below' if _median(t) < min(p) else 'ABOVE') + ' the parent spread'}")
    print("%d of %d shapes outside the parent's spread" % (outside, len(rows["this"][0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["blocks", "plain", "all"], default="all")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--parent-lib", default=os.environ.get("CLOUDCT_PARENT_LIB"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return plain_child(a.child, a.iters)
    if a.part in ("blocks", "all"):
        blocks_part(a.rounds, a.iters)
    if a.part in ("plain", "all"):
        plain_part(a.rounds, a.iters, a.parent_lib)


if __name__ == "__main__":
    main()
