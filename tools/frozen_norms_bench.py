"""Frozen-statistics fine-tuning on the fused kernels (ct_bn_eval_group_fwd / ct_bn_eval_group_bwd), at kernel and at step level:

    python tools/frozen_norms_bench.py [--part kernel|step|all] [--parent PATH] [--models segmenter,segmenter_pad] [--rounds 3] [--iters 20]
    python tools/frozen_norms_bench.py --path module|frozen|train [--model segmenter|segmenter_pad] [--root PATH]

(a) kernel: ct_bn_eval_group_bwd alone (a table of one norm, with ReLU) at C512 B8 N4096 and at a key norm's C48 B6 N8192, replayed
    from a HIP graph and timed with device events after a warm-up — once asking for everything (gx, the two sums, the maxima: one
    workgroup per channel) and once as a pure stream (gx only: channels cut over workgroups).  Its algorithmic bytes are read x,
    read gy, write gx; their rate is printed as a share of the chip's measured float4 copy rate (6.29 TB/s).
(b) step: forward + cross-entropy + backward of the S3DIS segmenter's structure at B8 N4096 (and segmenter_pad's at B6 N8192: 12
    MultiHeadUnion blocks, model_dim 512; random weights, synthetic clouds), replayed from a HIP graph, one fresh child process per
    figure, the paths alternating:
      module  model.train(), then m.eval() on every norm — torch's own API only, so this path also runs on a revision without
              freeze_norms (`--parent PATH`: a checkout of the parent commit with its library built; the baseline of the purpose bar);
      frozen  freeze_norms(model), model.train();
      train   model.train(): ordinary training, statistics and all.
    The purpose bar: the median of `frozen` here below the median of `module` on the parent by more than the parent's own spread
    (max - min of its rounds)."""
import argparse
import json
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)

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


def graphed(fn, before=None):
    """fn captured in a HIP graph after a side-stream warm-up (`before()` ahead of every pass); returns the replay callable."""
    import torch
    before = before or (lambda: None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            before()
            fn()
    torch.cuda.current_stream().wait_stream(side)
    before()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def kernel_part(iters):
    import torch
    from cloud_transformers_amd import _lib, ops
    lib = _lib.load()
    print("(a) ct_bn_eval_group_bwd alone (relu on), graphed, us per call; bytes = read x + read gy + write gx")
    for B, C, N in [(8, 512, 4096), (6, 48, 8192)]:
        x, gy = torch.randn(B, C, N, device="cuda"), torch.randn(B, C, N, device="cuda")
        gx = torch.empty_like(x)
        w, b = torch.rand(C, device="cuda") + 0.5, torch.rand(C, device="cuda") - 0.5
        rm, rv = torch.rand(C, device="cuda") * 2 - 1, torch.rand(C, device="cuda") + 0.5
        gw, gb, am = (torch.empty(C, device="cuda") for _ in range(3))
        base = dict(x=x.data_ptr(), xbs=0, C=C, w=w, b=b, rm=rm, rv=rv, eps=1e-5, relu=1, gy=gy.data_ptr(), gybs=0, gx=gx.data_ptr(), gxbs=0)
        for name, item in (("gx + sums + maxima (a workgroup per channel)", dict(base, gw=gw, gb=gb, amax=am.data_ptr())),
                           ("gx only (a pure stream, channels cut)", base)):
            arr = ops._bn_eval_bwd_table([item])

            def call():
                _lib.check(lib.ct_bn_eval_group_bwd(ops._at(arr, 0), 1, B, N, ops._stream()), "ct_bn_eval_group_bwd")

            ms = timed(graphed(call), iters)
            rate = 3 * x.numel() * 4 / (ms * 1e-3)
            print(f"B{B} C{C} N{N} {name}: {ms * 1e3:7.1f} us = {rate / 1e12:5.2f} TB/s "
                  f"({100 * rate / COPY_RATE:5.1f} % of the float4 copy rate)", flush=True)


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
    net = convert_pointwise(Segmenter(pad).cuda())
    with torch.no_grad():                                # statistics and learned keys off their initial values
        for m in net.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                if float(m.weight.abs().max()) == 0.0:
                    m.weight.fill_(0.1)
    xyz = torch.rand(B, 3, N, device="cuda") * 2 - 1
    feats = torch.randn(B, 4 if pad else 3, N, device="cuda")
    labels = torch.randint(0, 13, (B, N), device="cuda")
    mask = None
    if pad:
        mask = torch.ones(B, N, device="cuda", dtype=torch.int32)
        mask[:, N - 500:] = 0
    return net, (xyz, mask, feats), labels


def step_child(name, path, iters):
    import torch
    from torch import nn
    net, args, labels = build_model(name)
    net.train()
    if path == "module":                                 # torch's own API only: runs on any revision
        for m in net.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.eval()
    elif path == "frozen":
        from cloud_transformers_amd import freeze_norms
        freeze_norms(net)
        net.train()
    ce = nn.CrossEntropyLoss()
    stats = [m.running_mean.clone() for m in net.modules() if isinstance(m, nn.BatchNorm1d)]

    def step():
        ce(net(*args), labels).backward()

    ms = timed(graphed(step, before=lambda: net.zero_grad(set_to_none=True)), iters)
    held = all(torch.equal(a, m.running_mean) for a, m in zip(stats, (m for m in net.modules() if isinstance(m, nn.BatchNorm1d))))
    assert held == (path != "train"), "running statistics %s on path %s" % ("held" if held else "moved", path)
    print(json.dumps({"model": name, "path": path, "graph_ms": round(ms, 3)}), flush=True)


def run_child(root, name, path, iters):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--path", path, "--model", name, "--iters", str(iters)],
                         capture_output=True, text=True, timeout=900, cwd=root)
    if out.returncode != 0:                              # a child that failed ends the run: nothing more is started on the GPU
        raise SystemExit("%s on path %s in %s: exit %d\n%s" % (name, path, root, out.returncode, out.stderr[-3000:]))
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])["graph_ms"]


def summary(values):
    v = sorted(values)
    return v[len(v) // 2], v[0], v[-1]


def step_part(rounds, iters, parent, models=("segmenter", "segmenter_pad")):
    print("(b) training step (forward + cross-entropy + backward), graphed, ms; a fresh process per figure, paths alternating")
    for name in models:
        rows = [("this commit, frozen", ROOT, "frozen"), ("this commit, module", ROOT, "module"), ("this commit, train", ROOT, "train")]
        if parent:
            rows.insert(0, ("parent, module", parent, "module"))
        got = {label: [] for label, _, _ in rows}
        for _ in range(rounds):
            for label, root, path in rows:
                got[label].append(run_child(root, name, path, iters))
                print(f"{name:13s} {label:20s}: {got[label][-1]:8.3f}", flush=True)
        for label, _, _ in rows:
            med, lo, hi = summary(got[label])
            print(f"{name:13s} {label:20s}: median {med:8.3f}  min {lo:8.3f}  max {hi:8.3f}  spread {hi - lo:6.3f}")
        base = "parent, module" if parent else "this commit, module"
        (b_med, b_lo, b_hi), (f_med, _, _) = summary(got[base]), summary(got["this commit, frozen"])
        verdict = "MET" if b_med - f_med > b_hi - b_lo else "NOT met"
        print(f"{name:13s} purpose bar vs '{base}': {b_med:.3f} - {f_med:.3f} = {b_med - f_med:+.3f} ms against a spread of "
              f"{b_hi - b_lo:.3f}: {verdict}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernel", "step", "all"], default="all")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: the baseline of the purpose bar")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--path", choices=["module", "frozen", "train"], default=None, help="one step figure in this process")
    ap.add_argument("--model", choices=["segmenter", "segmenter_pad"], default="segmenter")
    ap.add_argument("--models", default="segmenter,segmenter_pad", help="the step part's models, comma-separated")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package --path imports (default: this file's)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.path:
        return step_child(a.model, a.path, a.iters)
    if a.part in ("step", "all"):        # first: the children are started before this process opens the GPU itself
        step_part(a.rounds, a.iters, os.path.abspath(a.parent) if a.parent else None, tuple(a.models.split(",")))
    if a.part in ("kernel", "all"):
        kernel_part(a.iters)


if __name__ == "__main__":
    main()
