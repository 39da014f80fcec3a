"""The segmentation_kpconv task of harness.Trainer and its entry point (cloud_transformers_amd.train_kpconv) end to end on
a tiny Stanford3dDataset_v1.2 tree written here: six one-room Areas whose labels follow the geometry (floor, ceiling,
walls, clutter), read by the real loader, a small model file with segmenter_pad's forward(points, pts_pad, features)."""
import json

import numpy as np
import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

MODEL = '''
import torch
from torch import nn
from layers.multihead_ct import MultiHeadUnion


class Model(nn.Module):
    """model_zoo/s3dis/segmenter_pad.py's structure, narrower and with one block per head configuration."""

    def __init__(self, n_classes=13, dim=64, n_features=4):
        super().__init__()
        zoo = [([4, 4], [128, 32]), ([16, 16], [64, 16]), ([16, 32], [16, 8])]
        self.first_process = nn.Sequential(nn.Conv1d(3 + n_features, dim, kernel_size=1, bias=True), nn.BatchNorm1d(dim),
                                           nn.ReLU(inplace=True))
        self.attentions_encoder = nn.ModuleList([MultiHeadUnion(model_dim=dim, features_dims=f, heads=[16, 16], tensor_sizes=s,
                                                                model_dim_out=dim, tensor_dims=[2, 3]) for f, s in zoo])
        self.final = nn.Sequential(nn.Conv1d(dim, dim, kernel_size=1, bias=False), nn.BatchNorm1d(dim), nn.ReLU(inplace=True),
                                   nn.Conv1d(dim, n_classes, kernel_size=1))

    def forward(self, points, pts_pad, features):
        input_pts = points.permute(0, 2, 1)
        x = self.first_process(torch.cat([input_pts, features], dim=1))
        for blk in self.attentions_encoder:
            x, _ = blk(x, (input_pts, pts_pad))
        return self.final(x)
'''

CONFIG = """
experiment:
    root: '{root}/exp'
    writer_root: '{root}/runs'
data:
    path: '{root}/Stanford3dDataset_v1.2'
    batch_size: 4
    num_workers: 0
    num_points: 2048
    test_area: 'Area_5'
    aug: True
    num_steps: 24
model:
    generator: '{root}/segmenter_pad_small.py'
train:
    num_epochs: 3
    save_each: 25000
    save_each_epoch: 1
    val_step: 1
    val_votes: 2
    final_votes: 3
    hip_graph: {graph}
    log_each: 1
    optimizer:
        type: 'Adam'
        lr: !!float 2e-3
    scheduler:
       type: 'StepLR'
       gamma: !!float 0.7
       step_size: 25000
"""


def _write_room(folder, seed, size):
    """One room: floor (label 1), ceiling (0), four walls (2) and clutter blobs (12), colours by class plus noise."""
    rng = np.random.default_rng(seed)
    X, Y, Z = size
    ann = folder / "room_1" / "Annotations"
    ann.mkdir(parents=True)
    u = lambda m, lo, hi: rng.uniform(lo, hi, m)       # noqa: E731
    k = 2500
    parts = {"floor_1": (np.stack([u(k, 0, X), u(k, 0, Y), u(k, 0, 0.02)], 1), (200, 60, 60)),
             "ceiling_1": (np.stack([u(k, 0, X), u(k, 0, Y), Z - u(k, 0, 0.02)], 1), (60, 200, 60)),
             "wall_1": (np.concatenate([np.stack([u(k, 0, 0.02), u(k, 0, Y), u(k, 0, Z)], 1),
                                        np.stack([X - u(k, 0, 0.02), u(k, 0, Y), u(k, 0, Z)], 1),
                                        np.stack([u(k, 0, X), u(k, 0, 0.02), u(k, 0, Z)], 1),
                                        np.stack([u(k, 0, X), Y - u(k, 0, 0.02), u(k, 0, Z)], 1)]), (60, 60, 200)),
             "clutter_1": (rng.uniform([1, 1, 0.3], [X - 1, Y - 1, 1.2], (6, 3))[rng.integers(0, 6, 1500)]
                           + rng.normal(0, 0.2, (1500, 3)), (180, 180, 40))}
    for name, (pts, col) in parts.items():
        c = np.clip(np.asarray(col)[None, :] + rng.normal(0, 20, (pts.shape[0], 3)), 0, 255).astype(np.int64)
        np.savetxt(ann / (name + ".txt"), np.concatenate([pts, c], 1), fmt=["%.4f"] * 3 + ["%d"] * 3)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("kpconv")
    for a in range(1, 7):
        _write_room(root / "Stanford3dDataset_v1.2" / ("Area_%d" % a), 40 + a, (6.0 + a % 3, 5.0, 3.0))
    (root / "segmenter_pad_small.py").write_text(MODEL)
    return root


def _config(root, graph, name="cfg.yaml", extra=""):
    path = root / name
    path.write_text(CONFIG.format(root=root, graph="true" if graph else "false") + extra)
    return path


def _check_records(records, epochs=3, votes=2, final=3):
    want = [(e, v) for e in range(1, epochs + 1) for v in range(votes)] + [("Last", v) for v in range(final)]
    assert [(r["epoch"], r["vote"]) for r in records] == want
    for r in records:
        assert np.isfinite(r["loss"])
        for k in ("part", "running_sub", "sub", "full"):
            ious = np.asarray(r[k + "_ious"])
            assert ious.shape == (13,) and (ious >= 0).all() and (ious <= 1).all(), (k, ious)
            assert abs(r[k + "_miou"] - ious.mean()) < 1e-6


@pytest.mark.parametrize("graph", [False, True])
def test_train_validate_checkpoint_and_eval(tree, graph):
    from cloud_transformers_amd import harness
    from cloud_transformers_amd.train_kpconv import load_kpconv_areas, main
    torch.manual_seed(0)
    cfg = harness.load_config(_config(tree, graph))
    cfg["data"]["kind"] = "s3dis_kpconv"
    tr = harness.Trainer(cfg, "segmentation", 13, exp_name="kp_%s" % graph, dataset=load_kpconv_areas(cfg))
    assert tr.task == "segmentation_kpconv" and tr.clip == 10.0              # selected by data.kind; the clip defaults to 10
    hist = tr.fit()
    if graph:
        assert tr._graphs and all(rec is not False for rec in tr._graphs.values())        # replayed, not the eager fallback
    assert len(hist) == 3 * (24 // 4) and all(np.isfinite(hist))
    assert np.mean(hist[-4:]) < np.mean(hist[:4]), hist
    _check_records(tr.val_records)
    lines = [json.loads(x) for x in (tr.exp_dir / "kpconv_val.jsonl").read_text().splitlines()]
    assert lines == tr.val_records
    for e in (1, 2, 3):
        assert (tr.exp_dir / ("generator_epoch_%d.t7" % e)).exists() and (tr.exp_dir / ("g_opt_epoch_%d.t7" % e)).exists()
    assert not list(tr.exp_dir.glob("*_iter_*.t7"))

    # vote sums and counts restart at each validation, the running logits carry on
    ev = tr.kp.evaluator
    T = ev.total                                                             # (column T: the write target of masked slots)
    running = ev.running[:, :T].clone()
    assert float(running.abs().sum()) > 0 and float(ev.counts[0, :T].max()) > 1.5
    tr.validate(1, "extra")
    unvisited = ev.counts[0, :T] < 1e-3
    assert bool(unvisited.any()) and not bool(unvisited.all())
    assert float(ev.logits_sum[:, :T][:, unvisited].abs().sum()) == 0
    assert torch.equal(ev.running[:, :T][:, unvisited], running[:, unvisited])
    assert float(running[:, unvisited].abs().sum()) > 0

    if not graph:
        # eval_segmentation_kpconv.py: restore the last checkpoint, one 20-vote validation (3 here); a repeat gives the same
        extra = "restore:\n    generator: '%s'\n" % (tr.exp_dir / "generator_epoch_3.t7")
        path = _config(tree, False, name="eval.yaml", extra=extra)
        a = main(["eval_a", "-c", str(path), "--eval"])
        b = main(["eval_b", "-c", str(path), "--eval"])
        assert [(r["epoch"], r["vote"]) for r in a] == [("Last", v) for v in range(3)]
        assert a == b


def test_one_epoch_under_a_world_one_process_group(tree):
    """One rank of RCCL: DistributedDataParallel + SyncBatchNorm, and the vote state all-reduced before the metrics."""
    from cloud_transformers_amd import harness
    from cloud_transformers_amd.train_kpconv import load_kpconv_areas
    from tests.test_ddp_gpu import _free_port
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        torch.manual_seed(0)
        cfg = harness.load_config(_config(tree, False, name="ddp.yaml"))
        cfg["train"]["num_epochs"] = 1
        tr = harness.Trainer(cfg, "segmentation_kpconv", 13, device=torch.device("cuda", 0), dist=dist, exp_name="kp_ddp",
                             dataset=load_kpconv_areas(cfg))
        assert isinstance(tr.model, torch.nn.parallel.DistributedDataParallel)
        hist = tr.fit()
        assert len(hist) == 6 and all(np.isfinite(hist))
        _check_records(tr.val_records, epochs=1)
        red = tr.kp.evaluator.synced(dist)
        assert red is not tr.kp.evaluator
        assert torch.equal(red.counts, tr.kp.evaluator.counts) and torch.equal(red.logits_sum, tr.kp.evaluator.logits_sum)
    finally:
        dist.destroy_process_group()
