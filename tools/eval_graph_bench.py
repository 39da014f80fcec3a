"""Graph replay against eager launches where the harness runs a model: the reconstruction task's training step and one
validation step (eval-mode forward plus the validation loss terms) of each of the five tasks.

    python tools/eval_graph_bench.py [--rows a,b,...] [--windows 7] [--iters 3] [--window-ms 500]
    python tools/eval_graph_bench.py --row NAME            # one row in this process

The models are the zoo's structures at the protocols' shapes on synthetic inputs (random weights, running statistics off
their initial values): segmenter B8 N4096, classifier B8 N2048, segmenter_pad B6 N8192, inpainter B2 with 2048 / 16384 points,
reconstructor (ResNet-50 encoder, twelve AdaIN blocks) B4 N8192 at 128^2.  The steps are the harness's own: a `harness.Trainer`
without its data side (`bare_trainer`) runs `_eager_step` / `_graph_step` for (a) and `_val_step`, eagerly or through
`_val_runner(True)` (graphs.GraphedForward), for (b); the two EMD tasks at `val_emd_iters` 3000 (the protocol) and 50.
A row name with `_tail` appended (not in the default list) runs that EMD row with `train.val_emd_tail` on.

Timing: device events around a window of steps — as many as fill `--window-ms` at the eager step's warmed-up time, at least
`--iters`, the same count for both paths; eager and graphed windows alternate in one process after a warm-up of both (the
captures included); `--windows` windows each (at least seven); median [lowest, highest] in ms per step.  The bar of
a row: the graphed median below the eager median by more than twice the eager windows' max - min.  One child process per row,
started one after the other; a child that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
ZOO = [([4, 4], [128, 32]), ([16, 16], [64, 16]), ([16, 32], [16, 8])]
ROWS = ["train_reconstruction", "val_segmentation_blocks", "val_classification", "val_kpconv", "val_completion_3000",
        "val_completion_50", "val_reconstruction_3000", "val_reconstruction_50"]


def _encoder_blocks(dim):
    from torch import nn
    from cloud_transformers_amd.layers.multihead_ct import MultiHeadUnion
    return nn.ModuleList([MultiHeadUnion(model_dim=dim, features_dims=f, heads=[16, 16], tensor_sizes=s, model_dim_out=dim,
                                         tensor_dims=[2, 3]) for _ in range(4) for f, s in ZOO])


def _decoder_blocks(dim, latent):
    from torch import nn
    from cloud_transformers_amd.layers.multihead_ct import MultiHeadUnionAdaIn
    return nn.ModuleList([MultiHeadUnionAdaIn(model_dim=dim, features_dims=f, heads=[16, 16], tensor_sizes=s, model_dim_out=dim,
                                              n_latent=latent, tensor_dims=[2, 3]) for _ in range(4) for f, s in ZOO])


def build(name):
    """(model on the GPU, the validation / training step's input tensors) of one zoo structure."""
    import torch
    from torch import nn
    from cloud_transformers_amd.layers.grouped_conv import Pool3DBlock, Res2DBlock, Res3DBlock
    from cloud_transformers_amd.layers.multihead_ct import MultiHeadPool, forward_style
    from cloud_transformers_amd.layers.pointwise import convert_pointwise
    from cloud_transformers_amd.layers.resnet import resnet50
    from cloud_transformers_amd.layers.utils import AdaIn1dUpd
    d = 512

    class Segmenter(nn.Module):                      # model_zoo/s3dis/segmenter.py; pad: segmenter_pad.py
        def __init__(self, pad):
            super().__init__()
            self.pad = pad
            self.first_process = nn.Sequential(nn.Conv1d(7 if pad else 6, d, 1, bias=True), nn.BatchNorm1d(d), nn.ReLU(inplace=True))
            self.attentions_encoder = _encoder_blocks(d)
            self.final = nn.Sequential(nn.Conv1d(d, d, 1, bias=False), nn.BatchNorm1d(d), nn.ReLU(inplace=True), nn.Conv1d(d, 13, 1))

        def forward(self, *a):
            if self.pad:
                points, pts_pad, features = a
                xyz = points.permute(0, 2, 1)
                x = self.first_process(torch.cat([xyz, features], dim=1))
                for blk in self.attentions_encoder:
                    x, _ = blk(x, (xyz, pts_pad))
                return self.final(x)
            cloud = a[0].squeeze(2)
            x = self.first_process(cloud)
            for blk in self.attentions_encoder:
                x, _ = blk(x, cloud[:, :3])
            return self.final(x).unsqueeze(2)

    class Trunk(nn.Module):                          # the classifier's encoder, pools and Res blocks -> [B, 2048] and the features
        def __init__(self):
            super().__init__()
            self.first_process = nn.Sequential(nn.Conv1d(3, d, 1, bias=False), nn.BatchNorm1d(d), nn.ReLU(inplace=True))
            self.attentions_encoder = _encoder_blocks(d)
            self.pool3d = MultiHeadPool(model_dim=d, in_feature_dim=32, heads=16, tensor_size=8, tensor_dim=3)
            self.after_pool3d = nn.Sequential(Res3DBlock(512, 1024, groups=16), Pool3DBlock(2), Res3DBlock(1024, 1024, groups=16),
                                              Pool3DBlock(2), Res3DBlock(1024, 1024, groups=16), nn.AdaptiveAvgPool3d((1, 1, 1)))
            self.pool2d = MultiHeadPool(model_dim=d, in_feature_dim=16, heads=16, tensor_size=16, tensor_dim=2)
            self.after_pool2d = nn.Sequential(Res2DBlock(256, 512, groups=16), nn.MaxPool2d(2), Res2DBlock(512, 1024, groups=16),
                                              nn.MaxPool2d(2), Res2DBlock(1024, 1024, groups=16), nn.AdaptiveAvgPool2d((1, 1)))

        def forward(self, cloud):
            xyz = cloud.squeeze(2)
            x = self.first_process(xyz)
            for blk in self.attentions_encoder:
                x, _ = blk(x, xyz)
            to_3d, _ = self.pool3d(x, xyz)
            to_2d, _ = self.pool2d(x, xyz)
            return torch.cat([self.after_pool2d(to_2d).reshape(-1, 1024), self.after_pool3d(to_3d).reshape(-1, 1024)], dim=-1), x

    class Classifier(nn.Module):                     # model_zoo/scanobject/classifier.py
        def __init__(self):
            super().__init__()
            self.trunk = Trunk()
            self.class_vector = nn.Sequential(nn.Linear(2048, 1024), nn.BatchNorm1d(1024), nn.ReLU(inplace=True))
            self.class_head = nn.Sequential(nn.Dropout(0.5), nn.Linear(1024, 15))
            self.mask_head = nn.Sequential(nn.Dropout(0.5), nn.Conv1d(d + 1024, 256, 1, bias=False), nn.BatchNorm1d(256), nn.ReLU(),
                                           nn.Conv1d(256, 1, 1))

        def forward(self, cloud):
            pooled, x = self.trunk(cloud)
            vect = self.class_vector(pooled)
            mask = self.mask_head(torch.cat([x, vect[:, :, None].expand(-1, -1, x.size(-1))], dim=1))
            return self.class_head(vect), mask.unsqueeze(2)

    class Inpainter(nn.Module):                      # model_zoo/completion/inpainter.py
        def __init__(self, latent=512):
            super().__init__()
            self.trunk = Trunk()
            self.class_head = nn.Sequential(nn.Linear(2048, 1024), nn.BatchNorm1d(1024), nn.ReLU(inplace=True))
            self.mapping = nn.Sequential(nn.Linear(1024, latent), nn.ReLU(inplace=True))
            self.start = nn.Sequential(nn.Conv1d(4, d, 1, bias=False), AdaIn1dUpd(d, num_latent=latent), nn.ReLU(True))
            self.attentions_decoder = _decoder_blocks(d, latent)
            self.final = nn.Sequential(nn.Conv1d(d + 4, d, 1, bias=False), AdaIn1dUpd(d, num_latent=latent), nn.ReLU(inplace=True),
                                       nn.Conv1d(d, 3, 1))

        def forward(self, noise, partial):
            z = self.mapping(self.class_head(self.trunk(partial)[0]))
            x = forward_style(self.start, noise, z)
            for blk in self.attentions_decoder:
                x, _ = blk(x, z, noise[:, :3])
            return forward_style(self.final, torch.cat([x, noise], dim=1), z).unsqueeze(2)

    class Reconstructor(nn.Module):                  # model_zoo/image_reconstruction/reconstructor.py
        def __init__(self, latent=512):
            super().__init__()
            self.res50_model = nn.Sequential(nn.Sequential(*list(resnet50(pretrained=False).children())[:-2]), nn.AdaptiveAvgPool2d((1, 1)))
            self.mapping = nn.Sequential(nn.Linear(2048, latent), nn.ReLU(inplace=True))
            self.start = nn.Sequential(nn.Conv1d(3, d, 1, bias=False), AdaIn1dUpd(d, num_latent=latent), nn.ReLU(True))
            self.attentions_decoder = _decoder_blocks(d, latent)
            self.final = nn.Sequential(nn.Conv1d(d, d, 1, bias=False), AdaIn1dUpd(d, num_latent=latent), nn.ReLU(inplace=True),
                                       nn.Conv1d(d, 3, 1), nn.Sigmoid())

        def forward(self, noise, image):
            z = self.mapping(self.res50_model(image).reshape(-1, 2048))
            x = forward_style(self.start, noise, z)
            for blk in self.attentions_decoder:
                x, _ = blk(x, z, noise)
            return forward_style(self.final, x, z).unsqueeze(2), []

    torch.manual_seed(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=g)          # noqa: E731
    if name == "segmenter":
        net, B, N = Segmenter(False), 8, 4096
        args = (rand(B, 6, 1, N) * 2 - 1, torch.randint(0, 13, (B, N), device="cuda", generator=g))
    elif name == "segmenter_pad":
        net, B, N = Segmenter(True), 6, 8192
        mask = torch.ones(B, N, device="cuda", dtype=torch.int32)
        mask[:, N - 500:] = 0
        args = (rand(B, N, 3) * 2 - 1, mask, rand(B, 4, N), torch.randint(0, 13, (B, N), device="cuda", generator=g))
    elif name == "classifier":
        net, B, N = Classifier(), 8, 2048
        args = (rand(B, 3, 1, N) * 2 - 1, torch.randint(0, 15, (B,), device="cuda", generator=g), (rand(B, N) > 0.5).float())
    elif name == "inpainter":
        net, B = Inpainter(), 2
        sphere = torch.nn.functional.normalize(rand(B, 3, 16384) - 0.5, dim=1)
        args = (torch.cat([sphere, (rand(B, 1, 16384) > 0.5).float()], dim=1), rand(B, 2048, 3) - 0.5, rand(B, 16384, 3) - 0.5)
    else:
        net, B = Reconstructor(), 4
        args = (torch.randn(B, 3, 128, 128, device="cuda", generator=g), rand(B, 3, 8192))
    net = convert_pointwise(net.cuda())
    with torch.no_grad():                            # statistics and zero-initialised weights off their initial values
        for m in net.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                if float(m.weight.abs().max()) == 0.0:
                    m.weight.fill_(0.1)
    return net, args


def bare_trainer(task, model, train_cfg):
    """A harness.Trainer without its data side: the task's protocol and what the steps and `_val_runner` read of the trainer."""
    import torch
    from cloud_transformers_amd import harness as H, protocols
    tr = object.__new__(H.Trainer)
    tr.cfg, tr.model, tr.device = {"data": {"seed": 0}, "train": dict(train_cfg)}, model, torch.device("cuda", torch.cuda.current_device())
    tr.dist, tr.rank, tr.n_classes, tr._stream, tr.clip, tr._graphs, tr._val_graph = None, 0, 13, None, None, {}, None
    tr.protocol = protocols.PROTOCOLS[task](tr)
    tr.protocol.noise_gen = torch.Generator(device=tr.device).manual_seed(3)
    tr.optimizer = torch.optim.Adam(model.parameters(), lr=1e-5)
    return tr


def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def row(name, windows, iters, window_ms):
    import torch
    tail = name.endswith("_tail")                    # `train.val_emd_tail` on (§4.20): val_completion_3000_tail, val_reconstruction_3000_tail
    name = name[:-len("_tail")] if tail else name
    emd = {"val_emd_eps": 0.004, "val_emd_iters": int(name.rsplit("_", 1)[1]), "val_emd_tail": tail} if name[-1].isdigit() else {}
    if name == "train_reconstruction":
        net, args = build("reconstructor")
        tr = bare_trainer("reconstruction", net, {"emd_eps": 0.005, "emd_iters": 50})
        net.train()
        eager, graphed = (lambda: tr._eager_step(args)), (lambda: tr._graph_step(args))
    else:
        task, model = {"val_segmentation_blocks": ("segmentation_blocks", "segmenter"),
                       "val_classification": ("classification_scanobjectnn", "classifier"),
                       "val_kpconv": ("segmentation_kpconv", "segmenter_pad"),
                       "val_completion": ("completion", "inpainter"),
                       "val_reconstruction": ("reconstruction", "reconstructor")}[name.rstrip("0123456789").rstrip("_")]
        net, args = build(model)
        tr = bare_trainer(task, net, dict(emd, seg_weight=0.5))
        net.eval()
        replay = tr._val_runner(True)
        inputs = (lambda: args + (tr.protocol._draw_noise(args[1]),)) if task == "reconstruction" else (lambda: args)

        def eager():
            with torch.no_grad():
                tr._val_step(*inputs())

        def graphed():
            replay(*inputs())

    for _ in range(2):                               # warm-up of both, the capture included
        eager()
        graphed()
    torch.cuda.synchronize()
    if name == "train_reconstruction":
        assert all(rec is not False for rec in tr._graphs.values()), "the training step fell back to eager steps"
    else:
        assert not tr._val_graph.eager, "the validation step fell back to eager forwards"
    iters = min(200, max(iters, int(window_ms / max(window(eager, 3), 1e-3)) + 1))
    got = {"eager": [], "graphed": []}
    for _ in range(windows):
        got["eager"].append(window(eager, iters))
        got["graphed"].append(window(graphed, iters))
    print(json.dumps({"row": name + ("_tail" if tail else ""), "steps": iters, **{k: [round(x, 3) for x in v] for k, v in got.items()}}), flush=True)


def summary(values):
    v = sorted(values)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", default=None, help="one row in this process")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=500.0)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.row:
        return row(a.row, max(a.windows, 7), a.iters, a.window_ms)
    print("ms per step, device events, %d windows of >= %.0f ms (steps per window in the row), eager and graphed alternating: "
          "median [lowest, highest]" % (max(a.windows, 7), a.window_ms))
    for name in a.rows.split(","):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", name, "--windows", str(a.windows), "--iters", str(a.iters),
                              "--window-ms", str(a.window_ms)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        if out.returncode != 0:                      # a child that failed ends the run: nothing more is started on the GPU
            raise SystemExit("%s: exit %d\n%s" % (name, out.returncode, out.stderr[-3000:]))
        for line in out.stdout.splitlines():
            if "capture failed" in line:
                print(line)
        res = json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])
        (e_med, e_lo, e_hi), (g_med, g_lo, g_hi) = summary(res["eager"]), summary(res["graphed"])
        verdict = "MET" if e_med - g_med > 2 * (e_hi - e_lo) else "NOT met"
        print(f"{name:26s} x{res['steps']:<4d} eager {e_med:9.3f} [{e_lo:9.3f}, {e_hi:9.3f}]   graphed {g_med:9.3f} [{g_lo:9.3f}, {g_hi:9.3f}]   "
              f"gain {e_med - g_med:+9.3f} against 2 x {e_hi - e_lo:.3f}: {verdict}", flush=True)


if __name__ == "__main__":
    main()
