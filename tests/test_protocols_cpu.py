"""protocols.py and the task-free loop of harness.Trainer on the CPU: the table, the configs, make_dataset's look-up, the one
validation loop on a stub protocol, the scan and blocks validation folds on hand-made batches, and launch.run_entry."""
import copy
import json
import math
import os

import pytest
import torch
from torch import nn

from cloud_transformers_amd import harness as H, launch, protocols as P

CPU = torch.device("cpu")
TASKS = ("segmentation", "classification", "completion", "segmentation_kpconv", "classification_scanobjectnn", "segmentation_blocks",
         "reconstruction")
KINDS = {"s3dis_kpconv": "segmentation_kpconv", "scanobjectnn_device": "classification_scanobjectnn", "s3dis_device": "segmentation_blocks",
         "what3d_device": "reconstruction", "shapenet_completion": "completion", "shapenet_completion_device": "completion"}


class Batches(list):
    def set_epoch(self, epoch):
        self.epoch = epoch


def _bare(model, protocol, cfg=None, exp_dir=None, n_classes=3):
    """A Trainer with what `_validate` reads, around `protocol` (a class)."""
    tr = object.__new__(H.Trainer)
    tr.cfg = cfg if cfg is not None else {"data": {}, "train": {}}
    tr.model, tr.device, tr.dist, tr.rank, tr.n_classes, tr.task = model, CPU, None, 0, n_classes, protocol.name
    tr.writer, tr.exp_dir, tr.iters, tr.val_loader, tr.val_records, tr._val_graph = H.NullWriter(), exp_dir, 5, None, [], None
    tr.optimizer = torch.optim.SGD(model.parameters(), lr=0.1)
    tr.protocol = protocol(tr)
    return tr


# ---------------------------------------------------------------------------------------------------------------------
# the table and the configs
def test_the_table_covers_the_tasks_and_the_device_kinds():
    assert set(P.PROTOCOLS) == set(TASKS) | set(KINDS)
    assert all(P.PROTOCOLS[t].name == t for t in TASKS)
    assert all(P.PROTOCOLS[k].name == t and P.pick("segmentation" if P.PROTOCOLS[k].kind_selects else t, k).name == t for k, t in KINDS.items())
    assert P.pick("classification", "scanobjectnn") is P.Classification and P.pick("segmentation", "") is P.Segmentation
    with pytest.raises(AssertionError, match="data.kind shapenet_completion_device is the completion task"):
        P.pick("segmentation", "shapenet_completion_device")


@pytest.mark.parametrize("task", TASKS)
def test_config_leaves_its_input_untouched_and_keeps_present_keys(task):
    cfg = {"data": {"batch_size": 3, "seed": 11, "kind": "mine", "test_area": "Area_2"}, "train": {"val_step": 7, "emd_eps": 0.5}, "model": {"x": [1]}}
    before = copy.deepcopy(cfg)
    out = P.PROTOCOLS[task].config(cfg)
    assert cfg == before and out is not cfg and out["model"]["x"] is not cfg["model"]["x"]
    for sect in ("data", "train"):
        assert all(out[sect][k] == v for k, v in before[sect].items())
    cls = P.PROTOCOLS[task]
    assert all(k in out["data"] for k in cls.DATA) and all(k in out["train"] for k in cls.TRAIN)
    assert out["data"].get("batch_size_val") == (3 if cls.batch_size_val else None)


def test_the_entry_points_configs_are_the_protocols():
    from cloud_transformers_amd.train_classification import classification_config
    from cloud_transformers_amd.train_completion import completion_config
    from cloud_transformers_amd.train_kpconv import kpconv_config
    from cloud_transformers_amd.train_reconstruction import reconstruction_config
    from cloud_transformers_amd.train_segmentation import segmentation_config
    cfg = {"data": {"batch_size": 2}, "train": {}}
    assert classification_config(cfg) == P.Scan.config(cfg) and classification_config(cfg)["data"]["jitter_clip"] == 0.05
    assert segmentation_config(cfg) == P.Blocks.config(cfg) and segmentation_config(cfg)["train"]["save_each_epoch"] == 100
    assert reconstruction_config(cfg) == P.Reconstruction.config(cfg) and reconstruction_config(cfg)["data"]["seed"] == 42
    assert kpconv_config(cfg) == P.KPConv.config(cfg) and "batch_size_val" not in kpconv_config(cfg)["data"]
    assert P.Completion.config(cfg) == cfg                     # the trainer has never applied the completion defaults
    assert completion_config(cfg)["data"] == {"batch_size": 2, "kind": "shapenet_completion", "n_renders": 1, "input_size": 2048,
                                              "gt_size": 16384, "seed": 0, "batch_size_val": 2}


def test_a_kind_in_the_config_selects_the_blocks_protocol(tmp_path):
    from tests.test_block_items_cpu import _host_dataset
    from tests.test_harness_cpu import MODEL
    from cloud_transformers_amd.data.s3dis_blocks import BlockBatches
    (tmp_path / "toy_model.py").write_text(MODEL)
    cfg = {"experiment": {"root": str(tmp_path), "writer_root": str(tmp_path)}, "model": {"generator": str(tmp_path / "toy_model.py")},
           "data": {"kind": "s3dis_device", "batch_size": 4, "num_points": 8},
           "train": {"num_epochs": 1, "optimizer": {"type": "SGD", "lr": 0.1}}}
    tr = H.Trainer(cfg, "segmentation", 13, device=CPU, make_dirs=False, dataset=_host_dataset(9, 8, 8, seed=3))
    assert type(tr.protocol) is P.Blocks and tr.task == "segmentation_blocks" and tr.cfg["data"]["hue_max"] == 0.5 and "hue_max" not in cfg["data"]
    assert isinstance(tr.loader, BlockBatches) and tr.loader.train and tr.sampler is None and tr.protocol.loader_epochs
    val = tr.protocol.loader(tr, tr.loader.ds, train=False)
    assert not val.train and val.ds is tr.loader.ds and val.sampler.seed == tr.loader.sampler.seed + 7919
    assert tr.protocol.train_meter is not None and tr.protocol.train_records == [] and tr.val_records == []


def test_make_dataset_messages():
    cfg = {"data": {"kind": "nonsense", "num_points": 8}}
    with pytest.raises(ValueError) as ex:
        H.make_dataset(cfg, "segmentation", 3)
    assert str(ex.value) == ("data.kind must be synthetic, scanobjectnn, scanobjectnn_device, s3dis, s3dis_device, s3dis_kpconv, "
                             "shapenet_completion, shapenet_completion_device or what3d_device (got 'nonsense')")
    for kind, task, text in (("what3d_device", "segmentation", "data.kind what3d_device is the reconstruction task"),
                             ("s3dis_device", "segmentation", "data.kind s3dis_device is the segmentation_blocks task"),
                             ("scanobjectnn_device", "classification", "data.kind scanobjectnn_device is the classification_scanobjectnn task"),
                             ("shapenet_completion", "segmentation", "ShapeNet completion items are (partial cloud, complete cloud): the completion task"),
                             ("s3dis_kpconv", "segmentation", "S3DIS KPConv items are (points, mask, features, labels): the segmentation_kpconv task"),
                             ("scanobjectnn", "segmentation", "ScanObjectNN items are (points, label, mask): the classification task"),
                             ("s3dis", "classification", "S3DIS blocks are (points, labels): the segmentation task")):
        with pytest.raises(AssertionError) as ex:
            H.make_dataset({"data": {"kind": kind}}, task, 3)
        assert str(ex.value) == text
    assert isinstance(H.make_dataset({"data": {"num_points": 8}}, "segmentation", 3, length=2), H.SyntheticClouds)


# ---------------------------------------------------------------------------------------------------------------------
# the one validation loop
class Stub(P.Protocol):
    """Two summed terms, a min-rule on the first; the loader is the data itself."""
    name, val_terms, val_file, best_key = "stub", ("first", "second"), "stub_val.jsonl", "first"

    def loader(self, trainer, data, train):
        return data

    def val_step(self, trainer, *t):
        y = trainer.model(t[0])
        return y.mean(), (y * y).mean()

    def val_batch(self, trainer, step, batch, meter):
        assert meter is None and not trainer.model.training and not torch.is_grad_enabled()
        return step(*batch)


def test_the_validation_loop_on_a_stub_protocol(tmp_path):
    model = nn.Linear(2, 1, bias=False)
    with torch.no_grad():
        model.weight.copy_(torch.tensor([[1.0, 2.0]]))
    model.train()
    data = Batches([(torch.tensor([[1.0, 1.0], [3.0, 0.0]]),), (torch.tensor([[0.0, 0.5]]),)])           # y = (3, 3) and (1)
    tr = _bare(model, Stub, exp_dir=tmp_path)
    (rec,) = tr.validate(epoch=2, dataset=data)
    assert rec == {"epoch": 2, "iters": 5, "batches": 2, "first": 2.0, "second": 5.0, "best": True}
    assert list(rec) == ["epoch", "iters", "batches", "first", "second", "best"]
    assert model.training and data.epoch == 2 and tr.val_loader is data
    assert tr.writer.scalars == {"val/val_first": (2.0, 2), "val/val_second": (5.0, 2)}
    best = sorted(f for f in os.listdir(tmp_path) if f.endswith(".t7"))
    assert best == ["g_opt_best_0.t7", "generator_best_0.t7"]
    stamp = os.stat(tmp_path / "generator_best_0.t7").st_mtime_ns
    with torch.no_grad():
        model.weight.mul_(2.0)                                  # a worse second pass
    model.eval()
    (again,) = tr.validate(epoch="eval")
    assert again == {"epoch": "eval", "iters": 5, "batches": 2, "first": 4.0, "second": 20.0, "best": False}
    assert not model.training and data.epoch == 0 and tr.writer.scalars["val/val_first"] == (4.0, 5)      # not an int: at `iters`
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".t7")) == best and os.stat(tmp_path / "generator_best_0.t7").st_mtime_ns == stamp
    assert tr.val_records == [rec, again] and tr.protocol.best_val == 2.0
    lines = (tmp_path / "stub_val.jsonl").read_text().splitlines()
    assert lines == [json.dumps(rec), json.dumps(again)]
    assert lines[0] == '{"epoch": 2, "iters": 5, "batches": 2, "first": 2.0, "second": 5.0, "best": true}'


# ---------------------------------------------------------------------------------------------------------------------
# the folds of two real protocols, hand-made batches
class ScanOnLists(P.Scan):
    loader = Stub.loader


class BlocksOnLists(P.Blocks):
    loader = Stub.loader


class Fixed(nn.Module):
    """Returns what it was given, whatever the input (a parameter keeps optimizers and checkpoints happy)."""

    def __init__(self, *out):
        super().__init__()
        self.p, self.out = nn.Parameter(torch.zeros(1)), out

    def forward(self, cloud):
        return self.out if len(self.out) > 1 else self.out[0]


def test_scan_validation_fold_against_hand_numbers(tmp_path):
    a, m, w, C, B, N = 2.0, 1.0, 0.25, 3, 4, 5
    logits = torch.zeros(B, C)
    logits[:, 0] = a                                            # every cloud is predicted class 0
    mask_logits = torch.full((B, 1, 1, N), m)                   # every point is predicted object
    label = torch.tensor([0, 0, 1, 2])
    mask = torch.zeros(B, N)
    mask[:, :2] = 1.0
    tr = _bare(Fixed(logits, mask_logits), ScanOnLists, cfg={"data": {}, "train": {"seg_weight": w}}, exp_dir=tmp_path, n_classes=C)
    lse = math.log(math.exp(a) + C - 1)
    cls = (2 * (lse - a) + 2 * lse) / 4
    seg = (2 * math.log(1 + math.exp(-m)) + 3 * math.log(1 + math.exp(m))) / 5
    out = tr._val_step(torch.zeros(B, 3, 1, N), label, mask)
    assert len(out) == 5 and out[3] is logits and out[4] is mask_logits
    assert [float(v) for v in out[:3]] == pytest.approx([(1 - w) * cls + w * seg, cls, seg], rel=1e-6)
    batch = (torch.zeros(B, 3, 1, N), label, mask)
    (rec,) = tr.validate(epoch=0, dataset=Batches([batch, batch]))
    assert list(rec) == ["epoch", "iters", "batches", "loss", "loss_cls", "loss_seg", "cls_acc", "seg_acc", "m_acc", "class_acc", "best", "macc_best"]
    assert rec["batches"] == 2 and rec["loss"] == pytest.approx((1 - w) * cls + w * seg, rel=1e-6)
    assert (rec["loss_cls"], rec["loss_seg"]) == pytest.approx((cls, seg), rel=1e-6)
    assert rec["cls_acc"] == 0.5 and rec["seg_acc"] == 0.4 and rec["m_acc"] == pytest.approx(1 / 3) and rec["class_acc"] == [1.0, 0.0, 0.0]
    assert rec["best"] is True and rec["macc_best"] is True
    assert set(tr.writer.scalars) == {"val/" + k for k in ("loss", "loss_cls", "loss_seg", "cls_acc", "seg_acc", "m_acc")}
    (again,) = tr.validate(epoch=1)                              # equal is not strictly greater
    assert again["best"] is False and again["macc_best"] is False and tr.protocol.best_acc == 0.5
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".t7"))
    assert files == ["g_opt_best_0.t7", "g_opt_macc_best_0.t7", "generator_best_0.t7", "generator_macc_best_0.t7"]
    nan = _bare(Fixed(logits, mask_logits), ScanOnLists, cfg={"data": {}, "train": {"seg_weight": w}}, n_classes=C)
    (rec,) = nan.validate(epoch=0, dataset=Batches([(batch[0], torch.tensor([0, 0, 1, 1]), mask)]))
    assert rec["m_acc"] != rec["m_acc"] and rec["best"] is True and rec["macc_best"] is False        # a NaN m_acc is never best


def test_blocks_validation_fold_against_hand_numbers(tmp_path, monkeypatch):
    from cloud_transformers_amd.data import s3dis_blocks

    class Meter:                                                # (the real one fills its matrix with a library kernel)
        def __init__(self, n_classes):
            self.n, self.seen = n_classes, []

        def update(self, pred, labels):
            self.seen.append((pred, labels))

        def result(self):
            return {"overall_acc": 0.75, "mean_iou": float(len(self.seen))}

    monkeypatch.setattr(s3dis_blocks, "SegmentationMeter", Meter)
    a, C, B, N = 1.5, 4, 2, 3
    pred = torch.zeros(B, C, 1, N)
    pred[:, 1] = a
    labels = torch.tensor([[1, 1, 0], [2, 1, 3]])
    tr = _bare(Fixed(pred, []), BlocksOnLists, exp_dir=tmp_path, n_classes=C)
    lse = math.log(math.exp(a) + C - 1)
    want = (3 * (lse - a) + 3 * lse) / 6
    got_pred, loss = tr._val_step(torch.zeros(B, 6, 1, N), labels)
    assert got_pred is pred and float(loss) == pytest.approx(want, rel=1e-6)
    batch = (torch.zeros(B, 6, 1, N), labels)
    (rec,) = tr.validate(epoch=3, dataset=Batches([batch, batch, batch]))
    assert list(rec) == ["epoch", "iters", "batches", "loss", "overall_acc", "mean_iou"]
    assert rec["batches"] == 3 and rec["loss"] == pytest.approx(want, rel=1e-6) and rec["mean_iou"] == 3.0
    assert tr.writer.scalars == {"val/loss": (rec["loss"], 3), "val/overall_acc": (0.75, 3), "val/mean_iou": (3.0, 3)}
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".t7")]                                 # no best rule
    assert (tmp_path / "segmentation_val.jsonl").read_text() == json.dumps(rec) + "\n"


# ---------------------------------------------------------------------------------------------------------------------
# the entry points' shared launcher
@pytest.mark.parametrize("hip_graph", [False, True])
def test_run_entry_strips_gpus_and_spawns(tmp_path, monkeypatch, hip_graph):
    cfg = tmp_path / "c.yaml"
    cfg.write_text("train:\n    hip_graph: %s\n" % ("true" if hip_graph else "false"))
    calls = []
    monkeypatch.setattr(launch, "spawn_ranks", lambda script, argv, nproc, capture=False: calls.append((script, argv, nproc, capture)) or 0)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    body = lambda dist: ("ran", dist)                          # noqa: E731
    for argv in (["exp", "-c", str(cfg), "--gpus", "2"], ["--gpus", "2", "exp", "-c", str(cfg)], ["exp", "--gpus=2", "-c", str(cfg)]):
        del calls[:]
        assert launch.run_entry("some/entry.py", argv, 2, str(cfg), body) == []
        rest = [a for i, a in enumerate(argv) if a != "--gpus" and (i == 0 or argv[i - 1] != "--gpus") and not a.startswith("--gpus=")]
        assert calls == [(os.path.abspath("some/entry.py"), rest, 2, hip_graph)] and sorted(rest) == sorted(["exp", "-c", str(cfg)])
    del calls[:]
    assert launch.run_entry("some/entry.py", ["exp", "-c", str(cfg)], 1, str(cfg), body) == ("ran", None) and calls == []
    assert launch.run_entry("some/entry.py", ["exp", "--gpus", "2"], 2, str(cfg), body, spawn=False) == ("ran", None) and calls == []
    monkeypatch.setattr(launch, "spawn_ranks", lambda *a, **k: 3)
    with pytest.raises(SystemExit) as ex:
        launch.run_entry("some/entry.py", ["exp"], 2, str(cfg), body)
    assert ex.value.code == 3


@pytest.mark.parametrize("entry,spawns_for_eval", [("train_classification", False), ("train_segmentation", False), ("train_reconstruction", False),
                                                   ("train_completion", False), ("train_kpconv", True)])
def test_only_kpconv_spawns_ranks_for_eval(tmp_path, monkeypatch, entry, spawns_for_eval):
    import importlib
    mod = importlib.import_module("cloud_transformers_amd." + entry)
    seen = []

    def run_entry(script, argv, gpus, config, body, spawn=True):
        seen.append((os.path.basename(script), list(argv), gpus, config, spawn))
        return "done"

    monkeypatch.setattr(launch, "run_entry", run_entry)
    assert mod.main(["exp", "-c", "c.yaml", "--gpus", "2", "--eval"]) == "done"
    assert mod.main(["exp", "-c", "c.yaml", "--gpus", "2"]) == "done"
    assert seen == [(entry + ".py", ["exp", "-c", "c.yaml", "--gpus", "2", "--eval"], 2, "c.yaml", spawns_for_eval),
                    (entry + ".py", ["exp", "-c", "c.yaml", "--gpus", "2"], 2, "c.yaml", True)]
