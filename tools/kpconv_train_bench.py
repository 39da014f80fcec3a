"""Cost of the S3DIS KPConv training loop's parts on the device, on a synthetic Area-like cloud (tools/kpconv_data_bench.py's
room, grid-subsampled at 0.04):

    python tools/kpconv_train_bench.py [--points 1000000] [--iters 20] [--step-iters 10] [--no-step]

Rows:
- the raw cloud's grid subsampling through the host library and on the device, whole and in parts (`subsample_*`:
  tools/kpconv_data_bench.py `subsample_rows`);
- the batch assembly of 6 items at N = 8192 from the same ball query results: the torch sequence SphereSampler.sample used
  before ct_kp_items (restated here; with augmentation, the rotation, scale and jitter added in torch) against one
  ct_kp_items launch, without and with augmentation (the slot keys' argsort is in both);
- SphereSampler.sample(6), beside the 2.0 ms recorded before ct_kp_items (profiles/r7_kpconv_data_bench.txt);
- one epoch plan of 2000 picks: SphereSampler.plan (one ct_kp_plan call) and the torch loop it replaced (_plan_torch), alternating
  in this run from the same sampler state and seed, three repeats each (the mean and the [min, max] spread), on the one cloud
  and on five Area-like clouds in the proportions of the S3DIS training Areas (together ~2.5 x the one cloud);
- one training step (masked cross-entropy, clip_grad_norm 10, Adam) of model_zoo/s3dis/segmenter_pad.py's structure
  (defined here: 12 MultiHeadUnion blocks, model_dim 512) at B6 N8192 through harness.Trainer, eager and graphed, on one
  fixed batch and with the data side (items of an epoch plan, augmented) in the loop."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)

SEGMENTER_PAD = '''
import torch
from torch import nn
from layers.multihead_ct import MultiHeadUnion


class Model(nn.Module):
    """model_zoo/s3dis/segmenter_pad.py: stem on [xyz, 4 features], 4 x 3 MultiHeadUnion blocks, classifier head."""

    def __init__(self, n_classes=13):
        super().__init__()
        d = 512
        cfgs = [([4, 4], [128, 32]), ([16, 16], [64, 16]), ([16, 32], [16, 8])] * 4
        self.first_process = nn.Sequential(nn.Conv1d(7, d, kernel_size=1, bias=True), nn.BatchNorm1d(d), nn.ReLU(inplace=True))
        self.attentions_encoder = nn.ModuleList([MultiHeadUnion(model_dim=d, features_dims=f, heads=[16, 16], tensor_sizes=s,
                                                                model_dim_out=d, tensor_dims=[2, 3]) for f, s in cfgs])
        self.final = nn.Sequential(nn.Conv1d(d, d, kernel_size=1, bias=False), nn.BatchNorm1d(d), nn.ReLU(inplace=True),
                                   nn.Conv1d(d, n_classes, kernel_size=1))

    def forward(self, points, pts_pad, features):
        input_pts = points.permute(0, 2, 1)
        x = self.first_process(torch.cat([input_pts, features], dim=1))
        for blk in self.attentions_encoder:
            x, _ = blk(x, (input_pts, pts_pad))
        return self.final(x)
'''


def torch_assembly(smp, idx, count, picks, cloud, gen, aug=None):
    """The parent revision's batch assembly after the ball queries (+ the augmentation in torch when `aug` = (R, s, j))."""
    from cloud_transformers_amd.data.s3dis_kpconv import scene_seg_features
    B, N = idx.shape
    dev = idx.device
    nvalid = torch.clamp(count, max=N)
    live = torch.arange(N, device=dev)[None, :] < nvalid[:, None]
    keys = torch.where(live, torch.rand(B, N, generator=gen, device=dev), torch.full((B, N), 2.0, device=dev))
    perm = torch.argsort(keys, dim=1)
    pad = torch.floor(torch.rand(B, N, generator=gen, device=dev) * nvalid[:, None]).long().clamp_(0, N - 1)
    src = torch.where(live, perm, perm.gather(1, pad))
    input_inds = idx.gather(1, src).clamp_(min=0)
    mask = live.to(torch.int32)
    g = input_inds + smp.offsets[cloud][:, None]
    original = smp._all_points[g]
    points = original - picks[:, None, :]
    height = original[:, :, 2:]
    colors = (smp._all_colors[g] - smp._mean) / smp._std
    drop = (torch.rand(B, generator=gen, device=dev) > smp.color_drop).float()
    colors = colors * drop[:, None, None]
    labels = smp._all_labels[g]
    if aug is not None:
        R, s, j = aug
        points = torch.matmul(points, R.transpose(1, 2)) * s[:, None, :] + j
    return points, mask, scene_seg_features(smp.input_features_dim, points, colors, height), labels, input_inds


def kernel_assembly(smp, idx, count, picks, cloud, gen, aug=None):
    """The same draws and the argsort, then one ct_kp_items launch."""
    from cloud_transformers_amd.data.s3dis_kpconv import COLOR_MEAN, COLOR_STD, kp_items
    B, N = idx.shape
    dev = idx.device
    live = torch.arange(N, device=dev)[None, :] < torch.clamp(count, max=N)[:, None]
    keys = torch.where(live, torch.rand(B, N, generator=gen, device=dev), torch.full((B, N), 2.0, device=dev))
    perm = torch.argsort(keys, dim=1)
    u_pad = torch.rand(B, N, generator=gen, device=dev)
    drop = (torch.rand(B, generator=gen, device=dev) > smp.color_drop).float()
    R, s, j = aug if aug is not None else (None, None, None)
    return kp_items(idx, count, perm, u_pad, smp.offsets[cloud], picks, drop, smp._all_points, smp._all_colors, smp._all_labels,
                    COLOR_MEAN, COLOR_STD, smp.input_features_dim, R, s, j)


def plan_pair(smp, n, repeats=3):
    """(device plan ms, torch loop ms, equal): `plan(n)` and `_plan_torch(n)` alternating, each from the same potentials and the
    same generator state; per side the mean and the [min, max] over the repeats, after one warm-up each."""
    import time
    state = (smp._all_potentials.clone(), smp.min_potentials.clone(), smp.gen.get_state())
    times, outs = {"device": [], "torch": []}, {}
    for rep in range(repeats + 1):
        for name, fn in (("device", smp.plan), ("torch", smp._plan_torch)):
            smp._all_potentials.copy_(state[0])
            smp.min_potentials.copy_(state[1])
            smp.gen.set_state(state[2])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(n)
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e3)
            outs[name] = (out[0], out[1], smp._all_potentials.clone())
    equal = all(torch.equal(a, b) for a, b in zip(outs["device"], outs["torch"]))
    row = lambda t: [round(sum(t) / len(t), 1), round(min(t), 1), round(max(t), 1)]        # noqa: E731
    return row(times["device"]), row(times["torch"]), equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000, help="target size of the subsampled cloud")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step rows")
    args = ap.parse_args()
    from kpconv_data_bench import area_like, gpu_ms, subsample_rows
    from cloud_transformers_amd.data.s3dis_kpconv import Area, Augment, SphereSampler
    from cloud_transformers_amd.data.subsampling import grid_subsampling

    side = float(np.sqrt(args.points / 625.0 / 2.6))
    size = (1.6 * side, side, 3.5)
    raw = area_like(int(args.points * 2.5), 0, size)
    rng = np.random.default_rng(1)
    cols = rng.integers(0, 256, (raw.shape[0], 3)).astype(np.float32)
    labs = rng.integers(0, 13, raw.shape[0]).astype(np.int32)
    sp, sc, sl = grid_subsampling(raw, features=cols, labels=labs[:, None], sampleDl=0.04)
    area = Area("Area_bench", raw, cols, labs, sp, sc / np.float32(255), sl[:, 0])
    res = {"sub_points": int(sp.shape[0]), "B": 6, "N": 8192}
    res.update(subsample_rows(raw, cols, labs, 0.04, max(2, args.iters // 4)))      # the raw cloud through both subsampling paths
    gen = torch.Generator(device="cuda").manual_seed(0)
    smp = SphereSampler([area], 8192, in_radius=2.0, input_features_dim=4, generator=gen)

    cloud, picks = smp.plan(6)
    idx, _, count = smp.indices[0].query_radius(picks, 2.0, 8192)
    res["ball_counts"] = count.tolist()
    aug = Augment().draw(6, 8192, gen, "cuda")
    for name, a in (("", None), ("_aug", aug)):
        t = torch_assembly(smp, idx, count, picks, cloud, torch.Generator(device="cuda").manual_seed(3), a)
        k = kernel_assembly(smp, idx, count, picks, cloud, torch.Generator(device="cuda").manual_seed(3), a)
        res["assembly%s_equal" % name] = all(torch.equal(x, y) for x, y in zip(t[1:], k[1:])) and (
            torch.equal(t[0], k[0]) if a is None else bool(torch.allclose(t[0], k[0], atol=1e-5)))
        res["assembly%s_torch_ms" % name] = round(gpu_ms(lambda: torch_assembly(smp, idx, count, picks, cloud, gen, a), args.iters), 3)
        res["assembly%s_ct_kp_items_ms" % name] = round(gpu_ms(lambda: kernel_assembly(smp, idx, count, picks, cloud, gen, a),
                                                               args.iters), 3)
    res["sample6_N8192_ms"] = round(gpu_ms(lambda: smp.sample(6), args.iters), 3)
    res["sample6_N8192_aug_ms"] = round(gpu_ms(lambda: smp.sample(6, Augment()), args.iters), 3)
    res["sample6_N8192_recorded_before_ms"] = 2.0
    dev_ms, torch_ms, same = plan_pair(smp, 2000)
    res["plan2000_ms"], res["plan2000_spread_ms"] = dev_ms[0], dev_ms[1:]
    res["plan2000_torch_ms"], res["plan2000_torch_spread_ms"] = torch_ms[0], torch_ms[1:]
    res["plan2000_equal"] = same
    five = []
    for k, share in enumerate((0.57, 0.61, 0.24, 0.55, 0.53)):
        side5 = float(np.sqrt(args.points * share / 625.0 / 2.6))
        raw5 = area_like(int(args.points * share * 2.5), 10 + k, (1.6 * side5, side5, 3.5))
        rng5 = np.random.default_rng(20 + k)
        c5 = rng5.integers(0, 256, (raw5.shape[0], 3)).astype(np.float32)
        l5 = rng5.integers(0, 13, raw5.shape[0]).astype(np.int32)
        p5, sc5, sl5 = grid_subsampling(raw5, features=c5, labels=l5[:, None], sampleDl=0.04)
        five.append(Area("Area_bench_%d" % k, raw5, c5, l5, p5, sc5 / np.float32(255), sl5[:, 0]))
    smp5 = SphereSampler(five, 8192, in_radius=2.0, input_features_dim=4, generator=torch.Generator(device="cuda").manual_seed(0))
    res["five_clouds_sub_points"] = [int(a.sub_points.shape[0]) for a in five]
    dev_ms, torch_ms, same = plan_pair(smp5, 2000)
    res["plan2000_five_clouds_ms"], res["plan2000_five_clouds_spread_ms"] = dev_ms[0], dev_ms[1:]
    res["plan2000_five_clouds_torch_ms"], res["plan2000_five_clouds_torch_spread_ms"] = torch_ms[0], torch_ms[1:]
    res["plan2000_five_clouds_equal"] = same
    del smp5, five

    if not args.no_step:
        from cloud_transformers_amd import harness
        with tempfile.TemporaryDirectory() as tmp:
            model_file = os.path.join(tmp, "segmenter_pad.py")
            with open(model_file, "w") as f:
                f.write(SEGMENTER_PAD)
            cfg = {"experiment": {"root": tmp, "writer_root": tmp},
                   "data": {"kind": "s3dis_kpconv", "batch_size": 6, "num_points": 8192, "num_steps": 2000},
                   "model": {"generator": model_file},
                   "train": {"num_epochs": 1, "optimizer": {"type": "Adam", "lr": 1e-3},
                             "scheduler": {"type": "StepLR", "gamma": 0.7, "step_size": 25000}}}
            torch.manual_seed(0)
            tr = harness.Trainer(cfg, "segmentation_kpconv", 13, make_dirs=False, dataset=([area], [area]))
            tr._graphs = {}
            plan = tr.kp.train.plan(2000)
            sel = torch.arange(6, device="cuda")
            fixed = tr.kp.train.items(plan[0][sel], plan[1][sel], tr.kp.augment, generator=tr.kp.train_gen)[:4]

            def with_data(step):
                def run():
                    b = tr.kp.train.items(plan[0][sel], plan[1][sel], tr.kp.augment, generator=tr.kp.train_gen)[:4]
                    step(b)
                return run

            res["step_params"] = sum(p.numel() for p in tr.model.parameters())
            res["step_eager_ms"] = round(gpu_ms(lambda: tr._eager_step(fixed), args.step_iters, warmup=2), 2)
            res["step_eager_with_data_ms"] = round(gpu_ms(with_data(tr._eager_step), args.step_iters, warmup=1), 2)
            res["step_graph_ms"] = round(gpu_ms(lambda: tr._graph_step(fixed), args.step_iters, warmup=2), 2)
            res["step_graph_with_data_ms"] = round(gpu_ms(with_data(tr._graph_step), args.step_iters, warmup=1), 2)
            res["step_graph_captured"] = bool(tr._graphs) and all(v is not False for v in tr._graphs.values())
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
