"""The tasks of `harness.Trainer`, one class each; `PROTOCOLS` maps a task name — and a `data.kind` that belongs to one task —
to its class.  A Trainer holds one instance (`trainer.protocol`), which owns what only its task has: noise generator, train
meter, best values, the last Chamfer term.  The base class gives the neutral answer to every hook:

* `config(cfg)`: a copy of the config with the task's defaults under the keys it lacks (the `*_config` of the entry points).
* `dataset(cfg, train)`: the task's arm of `harness.make_dataset`.
* `loader(trainer, data, train)`: this rank's batches over `data`; may set `trainer.sampler`; `loader_epochs` says whether
  `fit` calls the train loader's `set_epoch`.
* `loss(trainer, batch)` -> the loss; what the step leaves besides it goes, detached, to `self.out`.  A captured graph keeps
  that `out` in its record; after an eager step or a replay `after_step(out, batch)` consumes it.  `logged`: extra per-step
  scalars for the writer (`train/<name>`), or None.  `graph_inputs(trainer, batch)`: the static inputs of a graphed step.
* `val_step(trainer, *t)`: one validation batch, device tensors in and out.  The validation pass is described by `val_terms`
  (the per-batch scalars that are summed, in the record's order), `val_meter` (an accumulator with update / reduce / result, or
  None), `val_batch` (runs the step, feeds the accumulator, returns the terms), `best` (the flags of a record; each true flag
  saves `generator_<flag>_0.t7` / `g_opt_<flag>_0.t7`), `val_scalars` (writer tags) and `val_file` (the jsonl beside the experiment).
  `validate` is the entry `Trainer.validate` forwards to.
* `after_epoch(trainer, epoch)`: the end of an epoch of `fit` (0-based `epoch`).

The imports of data/*, emd, chamfer and metrics are lazy: importing this module needs no GPU and no optional library."""
import copy

import torch
from torch import nn

from . import parallel


def with_defaults(cfg, data, train, batch_size_val=True):
    """A copy of `cfg` with `data` / `train` under the keys its sections lack; `data.batch_size_val` defaults to `data.batch_size`."""
    cfg = copy.deepcopy(cfg)
    for key, defaults in (("data", data), ("train", train)):
        sect = cfg.setdefault(key, {})
        for k, v in defaults.items():
            sect.setdefault(k, v)
    if batch_size_val:
        cfg["data"].setdefault("batch_size_val", cfg["data"].get("batch_size", 1))
    return cfg


def device_batches(trainer, data, train, device_set, batches, drop_last=False, cache=False, **kw):
    """`batches` over `data` (a host set is uploaded into a `device_set` first) with the config's sizes, this rank's shard."""
    d = trainer.cfg["data"]
    if not isinstance(data, device_set):
        data = device_set(data, trainer.device, **({"cache_dir": d.get("cache_dir")} if cache else {}))
    return batches(data, d["batch_size"] if train else d.get("batch_size_val", d["batch_size"]), train=train,
                   seed=int(d.get("seed", 0)) + (0 if train else 7919), rank=trainer.rank, world=parallel.world_size(trainer.dist),
                   drop_last=bool(d.get("drop_last", drop_last)) and train, **kw)


class EmdTail:
    """The validation accumulator of the two EMD tasks: float64 [sum of the first iteration without a bidder, clouds whose auction
    did not finish, clouds] (`_val_emd`).  It is all-reduced whether or not `train.val_emd_tail` is set; with the key the record
    also says how the auctions ended — the mean over the clouds of the first iteration without a bidder (`val_emd_iters` where
    there was none) and the clouds whose auction did not finish."""

    def __init__(self, trainer):
        self.on = bool(trainer.cfg["train"].get("val_emd_tail", False))
        self.sum = torch.zeros(3, dtype=torch.float64, device=trainer.device)

    def update(self, stats):
        if stats:
            self.sum += stats[0]

    def reduce(self, dist):
        dist.all_reduce(self.sum)

    def result(self):
        t = self.sum.tolist() if self.on else (0, 0, 0)
        return {"emd_first_empty_mean": t[0] / t[2], "emd_unfinished": int(t[1])} if t[2] > 0 else {}


def _val_emd(trainer, rec_bn3, gt_bn3, eps, iters):
    """The validation EMD of a batch -> (dist [B, n], stats).  `train.val_emd_tail` (default false): the auction through
    emd_with_info where its shape is supported — the same dist, a cloud's long tail in one launch — and stats = float64
    [sum of info[:, 0], clouds whose auction did not finish, clouds] on the device; otherwise today's call and stats None."""
    from .emd import emd_distance, emd_tail_supported, emd_with_info
    if bool(trainer.cfg["train"].get("val_emd_tail", False)) and emd_tail_supported(rec_bn3.size(0), rec_bn3.size(1)):
        dist, _, info = emd_with_info(rec_bn3, gt_bn3, eps, iters)
        clouds = torch.full((), float(info.size(0)), dtype=torch.float64, device=info.device)
        return dist, torch.stack([info[:, 0].sum().double(), (info[:, 1] > 0).sum().double(), clouds])
    return emd_distance(rec_bn3, gt_bn3, eps, iters)[0], None


class Protocol:
    """The neutral protocol: a plain DataLoader (with a DistributedSampler the trainer owns), no validation, nothing at the end
    of an epoch, `generator_iter_{n}.t7` every `train.save_each` iterations."""
    name, kinds, host_kinds, kind_selects, mismatch = None, (), (), True, None
    DATA, TRAIN, batch_size_val = {}, {}, False
    loader_epochs, save_by_iter = False, True
    val_terms, val_file, best_key = (), None, None

    def __init__(self, trainer):
        self.ce, self.bce = nn.CrossEntropyLoss(), nn.BCEWithLogitsLoss()
        self.out = self.logged = self.best_val = None

    @classmethod
    def config(cls, cfg):
        return with_defaults(cfg, cls.DATA, cls.TRAIN, cls.batch_size_val)

    def loader(self, trainer, data, train):
        from .harness import worker_init_fn
        d = trainer.cfg["data"]
        trainer.sampler = torch.utils.data.distributed.DistributedSampler(data) if parallel._active(trainer.dist) else None
        return torch.utils.data.DataLoader(data, batch_size=d["batch_size"], shuffle=trainer.sampler is None,
                                           num_workers=int(d.get("num_workers", 0)), sampler=trainer.sampler,
                                           drop_last=bool(d.get("drop_last", True)), worker_init_fn=worker_init_fn)

    def graph_inputs(self, trainer, batch):
        return batch

    def after_step(self, out, batch):
        pass

    def val_step(self, trainer, *t):
        raise ValueError("task %r has no validation step" % (self.name,))

    def val_meter(self, trainer):
        return None

    def best(self, rec):
        """`best_key`: a new minimum of that key is `best`."""
        if self.best_key is None:
            return {}
        better = self.best_val is None or rec[self.best_key] < self.best_val
        if better:
            self.best_val = rec[self.best_key]
        return {"best": bool(better)}

    def val_scalars(self, rec):
        return {"val/val_" + k: rec[k] for k in self.val_terms}

    def validate(self, trainer, num_votes=None, epoch=None, hip_graph=None, dataset=None):
        return trainer._validate(epoch, hip_graph, dataset)

    def after_epoch(self, trainer, epoch):
        pass


class Segmentation(Protocol):
    """loss = CE(pred[:, :, 0], labels) (train_segmentation.py:178) on host batches (points [B, N, channels], labels [B, N])."""
    name, host_kinds, mismatch = "segmentation", ("s3dis",), "S3DIS blocks are (points, labels): the segmentation task"

    @staticmethod
    def dataset(cfg, train):
        from .data import datasets as D
        data = cfg["data"]
        return D.Indoor3DSemSeg(data["path"], data["num_points"], train=train, aug=bool(data.get("aug", train)),
                                test_area=data.get("test_area", "Area_5"), data_precent=float(data.get("data_precent", 1.0)))

    def loss(self, trainer, batch):
        pts, labels = batch
        pcd = pts.permute(0, 2, 1)[:, :, None].to(trainer.device)                 # (B, channels, 1, N)
        out = trainer.model(pcd)
        pred = out[0] if isinstance(out, (tuple, list)) else out                  # the reference returns (pred, lattice stats)
        return self.ce(pred[:, :, 0], labels.to(trainer.device))


class Classification(Protocol):
    """loss = CE(logits, label) + seg_weight * BCE-with-logits(mask) (train_classification.py) on host batches (points, label, mask)."""
    name, host_kinds, mismatch = "classification", ("scanobjectnn",), "ScanObjectNN items are (points, label, mask): the classification task"

    @staticmethod
    def dataset(cfg, train):
        from .data import datasets as D
        data = cfg["data"]
        return D.ScanObjectNN(data["path"], train=train, subsample=data.get("num_points"), center=data.get("center", True),
                              normalize=data.get("normalize", True))

    def loss(self, trainer, batch):
        pts, label, mask = batch
        logits, mask_pred = trainer.model(pts.permute(0, 2, 1)[:, :, None].to(trainer.device))
        w = float(trainer.cfg["train"].get("seg_weight", 0.5))
        return (self.ce(logits, label.to(trainer.device).long())
                + w * self.bce(mask_pred.reshape(mask.shape[0], -1), mask.to(trainer.device).float()))     # (ScanObjectNN's mask is int64)


class Completion(Protocol):
    """loss = mean sqrt(EMD(rec, gt, 0.005, 50)) + chamfer_weight * loss_chamfer(rec, gt) (train_inpainter.py:186-192; `n_classes`
    is the size of the partial cloud).  With `data.kind: shapenet_completion` (`data.category_path`, `data.partial_path`,
    `data.gt_path`, `data.n_renders`, `data.input_size`, `data.gt_size` as configs/inpainting.yaml has them) the ShapeNetCompletion
    .pcd files are read (data/completion.py) and every batch is prepared on the device (CompletionBatches); `fit` validates once
    per epoch (train_completion.py, train_inpainter.py).  With `data.kind: shapenet_completion_device` (the same keys, optional
    `data.cache_dir`) every file of a subset is read once, the clouds stay on the device and every batch is gathered, sampled and
    mirrored there in one launch (DeviceCompletionBatches; `dataset` may be a completion Dataset or a DeviceShapeNetCompletion).
    The kinds do not select the task, and the trainer applies no defaults: the losses read their keys with the defaults of
    train_completion.completion_config.

    Validation (train_inpainter.py:253-311): eval mode, no grad, the VAL subset in batches of `data.batch_size_val`; per batch
    sqrt(EMD(rec, gt, val_emd_eps, val_emd_iters)).mean(1).mean() and loss_chamfer, averaged over the batches and the ranks; the
    record goes to <exp>/completion_val.jsonl and a new minimum of the loss saves `generator_best_0.t7` / `g_opt_best_0.t7`."""
    name, kinds, kind_selects = "completion", ("shapenet_completion", "shapenet_completion_device"), False
    mismatch = "ShapeNet completion items are (partial cloud, complete cloud): the completion task"
    val_terms, val_file, best_key = ("loss", "loss_emd", "loss_chamfer"), "completion_val.jsonl", "loss"

    def __init__(self, trainer):
        super().__init__(trainer)
        kind = str(trainer.cfg["data"].get("kind", "")).lower()
        self.shapenet, self.shapenet_device = kind in self.kinds, kind == "shapenet_completion_device"
        self.loader_epochs = self.shapenet_device

    @staticmethod
    def dataset(cfg, train):
        from .data.completion import DatasetSubset, shapenet_loader
        return shapenet_loader(cfg["data"]).get_dataset(DatasetSubset.TRAIN if train else DatasetSubset.VAL)

    def loader(self, trainer, data, train):
        if not self.shapenet:
            return super().loader(trainer, data, train)
        from .data.completion import CompletionBatches, DeviceCompletionBatches, DeviceShapeNetCompletion
        if self.shapenet_device:                         # (DeviceCompletionBatches holds torch's DistributedSampler itself)
            return device_batches(trainer, data, train, DeviceShapeNetCompletion, DeviceCompletionBatches, drop_last=True, cache=True)
        from .harness import worker_init_fn
        d = trainer.cfg["data"]
        smp = torch.utils.data.distributed.DistributedSampler(data, shuffle=train) if parallel._active(trainer.dist) else None
        if train:
            trainer.sampler = smp
        return CompletionBatches(data, d["batch_size"] if train else d.get("batch_size_val", d["batch_size"]), trainer.device,
                                 seed=int(d.get("seed", 0)) + (0 if train else 7919), rank=trainer.rank, shuffle=train,
                                 drop_last=bool(d.get("drop_last", True)) and train, num_workers=int(d.get("num_workers", 0)),
                                 sampler=smp, worker_init_fn=worker_init_fn)

    def loss(self, trainer, batch):
        from .chamfer import loss_chamfer
        from .emd import emd_distance
        noise, part, gt = batch
        out = trainer.model(noise.to(trainer.device), part.permute(0, 2, 1)[:, :, None].to(trainer.device))
        rec = out[0] if isinstance(out, (tuple, list)) else out                   # (B, 3, 1, N)
        gt4 = gt.permute(0, 2, 1)[:, :, None].to(trainer.device)
        tr = trainer.cfg["train"]
        dist, _ = emd_distance(rec[:, :, 0].permute(0, 2, 1), gt4[:, :, 0].permute(0, 2, 1),
                               float(tr.get("emd_eps", 0.005)), int(tr.get("emd_iters", 50)))
        return torch.sqrt(dist).mean(1).mean() + float(tr.get("chamfer_weight", 1.0)) * loss_chamfer(rec, gt4)

    def val_step(self, trainer, *t):
        """(noise, partial, gt) -> (loss_emd, loss_chamfer), the stats of `_val_emd` third under `train.val_emd_tail`."""
        from .chamfer import loss_chamfer
        tr = trainer.cfg["train"]
        noise, part, gt = t
        out = trainer.model(noise, part.permute(0, 2, 1)[:, :, None])
        rec = out[0] if isinstance(out, (tuple, list)) else out
        gt4 = gt.permute(0, 2, 1)[:, :, None]
        dist, stats = _val_emd(trainer, rec[:, :, 0].permute(0, 2, 1), gt4[:, :, 0].permute(0, 2, 1),
                               float(tr.get("val_emd_eps", 0.004)), int(tr.get("val_emd_iters", 3000)))
        return (torch.sqrt(dist).mean(1).mean(), loss_chamfer(rec, gt4)) + (() if stats is None else (stats,))

    val_meter = EmdTail

    def val_batch(self, trainer, step, batch, tail):
        l_emd, l_cd, *stats = step(*batch)
        tail.update(stats)
        return l_emd + float(trainer.cfg["train"].get("chamfer_weight", 1.0)) * l_cd, l_emd, l_cd

    def after_epoch(self, trainer, epoch):
        if self.shapenet:
            trainer._flush()
            trainer.validate(epoch=epoch)                # train_inpainter.py:253-311: once per epoch


class KPConv(Protocol):
    """Selected by `data.kind: s3dis_kpconv` too (`data.path` = the Stanford3dDataset_v1.2 folder): sphere items sampled on the
    device, loss = sum(CE * mask) / sum(mask) of model(points, mask, features), gradients clipped to `train.clip_grad_norm` (10),
    vote validation every `train.val_step` epochs and after the last, `generator_epoch_{e}.t7` / `g_opt_epoch_{e}.t7` every
    `train.save_each_epoch` epochs, none by iteration; `dataset` may be the (train, validation) Areas (train_kpconv.py,
    train_segmentation_kpconv.py).  The protocol's data object is `trainer.kp`.

    Validation: `num_votes` vote passes (train_kpconv.KPConvData.validate) on the unwrapped model; the records go to the writer
    (`val/<k>_v<vote>` at the iteration count) and, on rank 0, to <exp>/kpconv_val.jsonl."""
    name, kinds = "segmentation_kpconv", ("s3dis_kpconv",)
    mismatch = "S3DIS KPConv items are (points, mask, features, labels): the segmentation_kpconv task"
    DATA = {"kind": "s3dis_kpconv", "num_steps": 2000, "input_features_dim": 4, "num_classes": 13, "sampleDl": 0.04,
            "in_radius": 2.0, "color_drop": 0.2, "val_color_drop": 0.2, "test_area": "Area_5", "seed": 0}
    TRAIN = {"clip_grad_norm": 10.0, "val_step": 1, "save_each_epoch": 1, "val_votes": 2, "final_votes": 20}
    save_by_iter = False

    @staticmethod
    def dataset(cfg, train):
        from .train_kpconv import load_kpconv_areas
        return load_kpconv_areas(cfg, train=train)

    def loader(self, trainer, data, train):
        from .train_kpconv import KPConvData
        # one iteration over the loader is one epoch of device batches (a plan of sphere picks, sharded over the ranks)
        trainer.kp, trainer.clip = KPConvData(trainer.cfg, trainer.device, trainer.dist, areas=data), float(trainer.cfg["train"]["clip_grad_norm"])
        return trainer.kp

    def loss(self, trainer, batch):
        from .train_kpconv import masked_cross_entropy
        points, mask, features, labels = batch
        return masked_cross_entropy(trainer.model(points, mask, features), labels, mask)

    def val_step(self, trainer, *t):
        """(points, mask, features, labels) -> (pred, loss)."""
        from .train_kpconv import masked_cross_entropy
        points, mask, features, labels = t
        pred = parallel._plain_module(trainer.model)(points, mask, features)
        return pred, masked_cross_entropy(pred, labels, mask)

    def validate(self, trainer, num_votes=None, epoch=None, hip_graph=None, dataset=None):
        import json
        from pathlib import Path
        records = trainer.kp.validate(parallel._plain_module(trainer.model), num_votes, epoch, step=trainer._val_runner(hip_graph))
        if trainer.rank == 0:
            for rec in records:
                for k in ("loss", "part_miou", "running_sub_miou", "sub_miou", "full_miou"):
                    trainer.writer.add_scalar("val/%s_v%d" % (k, rec["vote"]), rec[k], global_step=trainer.iters)
            if trainer.exp_dir is not None:
                with open(str(Path(trainer.exp_dir) / "kpconv_val.jsonl"), "a") as f:
                    for rec in records:
                        f.write(json.dumps(rec) + "\n")
        trainer.val_records += records
        return records

    def after_epoch(self, trainer, epoch):
        # train_segmentation_kpconv.py:240-266: 2-vote validation every val_step epochs, checkpoints per epoch
        tr, e = trainer.cfg["train"], epoch + 1
        trainer._flush()
        if trainer.rank == 0:
            trainer.writer.add_scalar("learning_rate", trainer.optimizer.param_groups[0]["lr"], global_step=e)
        if e % int(tr["val_step"]) == 0:
            trainer.validate(int(tr["val_votes"]), e)
        if e % int(tr["save_each_epoch"]) == 0:
            trainer.save(epoch=e)
        if e == tr["num_epochs"]:                        # after the last epoch (a fit cut short by `max_iters` never gets here)
            trainer.validate(int(tr["final_votes"]), "Last")


class Scan(Protocol):
    """Selected by `data.kind: scanobjectnn_device` too (`data.path`, `data.path_val`, `data.batch_size_val`, optional
    `data.subsample`; `dataset` may be a data.datasets.ScanObjectNN or a data.scanobjectnn.DeviceScanObjectNN): the ScanObjectNN
    split stays on the device and every batch is gathered there (data/scanobjectnn.py ScanBatches; `n_classes` sizes the
    per-class accuracies); loss = (1 - seg_weight) * CE(out[0], label) + seg_weight * BCE-with-logits(out[1][:, 0, 0], mask) of
    train_classification.py:201-204 (the model's output is indexed, so the reference's three-output classifier and two-output
    models both fit); validation every `train.val_step` epochs, `generator_epoch_{e}.t7` every `train.save_each_epoch` epochs
    (train_classification.py).  Defaults: train_classification.py:146,176,281-286; datasets/scanobjectnn.py:30.

    Validation (train_classification.py:286-374): eval mode, no grad, `data.path_val` in batches of `data.batch_size_val`; the
    three losses averaged over the batches and the ranks, the accuracies from ClassificationMeter's counts all-reduced over the
    ranks.  As in the reference the shards are padded to equal length, so with several ranks a few clouds count twice.  The
    record (losses, cls_acc, seg_acc, m_acc, class_acc) goes to <exp>/classification_val.jsonl.  `best` / `macc_best`
    (`generator_best_0.t7` / `generator_macc_best_0.t7` and their `g_opt` twins): a strictly higher cls_acc / m_acc than any
    validation before (the first one always is, unless m_acc is NaN: a class absent from the split)."""
    name, kinds = "classification_scanobjectnn", ("scanobjectnn_device",)
    DATA = {"kind": "scanobjectnn_device", "n_classes": 15, "jitter_sigma": 0.01, "jitter_clip": 0.05, "seed": 0, "center": True,
            "normalize": True}
    TRAIN, batch_size_val = {"seg_weight": 0.5, "val_step": 1, "save_each_epoch": 10}, True
    loader_epochs = True
    val_terms, val_file = ("loss", "loss_cls", "loss_seg"), "classification_val.jsonl"

    def __init__(self, trainer):
        super().__init__(trainer)
        self.best_acc = self.best_macc = float("-inf")

    @staticmethod
    def dataset(cfg, train):
        from .data import datasets as D
        data = cfg["data"]
        # (augmentation and subsampling happen on the device: the host object only reads, centres and normalises)
        return D.ScanObjectNN(data["path"] if train else data["path_val"], train=False, subsample=None,
                              center=data.get("center", True), normalize=data.get("normalize", True))

    def loader(self, trainer, data, train):
        from .data.scanobjectnn import DeviceScanObjectNN, ScanBatches
        d = trainer.cfg["data"]
        return device_batches(trainer, data, train, DeviceScanObjectNN, ScanBatches, subsample=d.get("subsample"),
                              sigma=float(d["jitter_sigma"]), clip=float(d["jitter_clip"]))

    def _scan_losses(self, trainer, batch):
        """(loss, loss_cls, loss_seg, model output) of train_classification.py:199-204."""
        pcd, label, mask = batch
        out = trainer.model(pcd)
        w = float(trainer.cfg["train"]["seg_weight"])
        cls_loss, seg_loss = self.ce(out[0], label), self.bce(out[1][:, 0, 0], mask)
        return (1 - w) * cls_loss + w * seg_loss, cls_loss, seg_loss, out

    def loss(self, trainer, batch):
        return self._scan_losses(trainer, batch)[0]

    def val_step(self, trainer, *t):
        """(points, label, mask) -> (loss, loss_cls, loss_seg, logits, mask logits)."""
        loss, cls_loss, seg_loss, out = self._scan_losses(trainer, t)
        return loss, cls_loss, seg_loss, out[0], out[1]

    def val_meter(self, trainer):
        from .data.scanobjectnn import ClassificationMeter
        return ClassificationMeter(trainer.n_classes)

    def val_batch(self, trainer, step, batch, meter):
        loss, cls_loss, seg_loss, logits, mask_logits = step(*batch)
        meter.update(logits, mask_logits, batch[1], batch[2])
        return loss, cls_loss, seg_loss

    def best(self, rec):
        flags = {"best": bool(rec["cls_acc"] > self.best_acc), "macc_best": bool(rec["m_acc"] > self.best_macc)}
        if flags["best"]:
            self.best_acc = rec["cls_acc"]
        if flags["macc_best"]:
            self.best_macc = rec["m_acc"]
        return flags

    def val_scalars(self, rec):
        return {"val/" + k: rec[k] for k in ("loss", "loss_cls", "loss_seg", "cls_acc", "seg_acc", "m_acc")}

    def after_epoch(self, trainer, epoch):
        # train_classification.py:281-286: checkpoints and validation by the 0-based epoch
        tr = trainer.cfg["train"]
        trainer._flush()
        if epoch > 0 and epoch % int(tr["save_each_epoch"]) == 0:
            trainer.save(epoch=epoch)
        if epoch % int(tr["val_step"]) == 0:
            trainer.validate(epoch=epoch)


class Blocks(Protocol):
    """Selected by `data.kind: s3dis_device` too (`data.path`, `data.num_points`, `data.test_area`, `data.data_percent`,
    `data.aug`, `data.batch_size_val` as configs/s3dis.yaml has them; `dataset` may be a data.datasets.Indoor3DSemSeg or a
    data.s3dis_blocks.DeviceS3DISBlocks): the 1x1 m blocks stay on the device and every batch is assembled and augmented there in
    one launch (data/s3dis_blocks.py BlockBatches); loss = CE(pred[:, :, 0], labels); a train confusion matrix updated every
    step on the device and reported per epoch (`train_records`, `train/<k>` at the epoch); validation every `train.val_step`
    epochs, `generator_iter_{n}.t7` every `train.save_each` iterations and `generator_epoch_{e}.t7` every
    `train.save_each_epoch` epochs (train_segmentation.py).  Defaults: datasets/s3dis_v2.py:185-196,246-366,546-554 (the
    transforms' constants); train_segmentation.py:71-73,175 (`aug` off unless the config asks, 13 classes).

    Validation (train_segmentation.py:244-288): eval mode, no grad, the blocks of `data.test_area` in batches of
    `data.batch_size_val` (shuffled points, no augmentation); the loss averaged over the batches and the ranks, the confusion
    matrix filled on the device (SegmentationMeter) and all-reduced over the ranks, `return_metrics_dict`'s numbers from it.  As
    in the reference the shards are padded to equal length, so with several ranks a few blocks count twice.  The record (loss,
    overall_acc, mean_class_acc, iou_<name>, mean_iou) goes to <exp>/segmentation_val.jsonl; there is no best rule."""
    name, kinds = "segmentation_blocks", ("s3dis_device",)
    DATA = {"kind": "s3dis_device", "n_classes": 13, "seed": 0, "jitter_sigma": 0.01, "jitter_clip": 0.05, "color_jitter_std": 0.05,
            "color_shift_ratio": 0.1, "hue_max": 0.5, "saturation_max": 0.2, "test_area": "Area_5", "data_percent": 1.0, "aug": False}
    TRAIN, batch_size_val = {"val_step": 1, "save_each_epoch": 100}, True
    loader_epochs = True
    val_terms, val_file = ("loss",), "segmentation_val.jsonl"

    def __init__(self, trainer):
        super().__init__(trainer)
        from .data.s3dis_blocks import SegmentationMeter
        self.train_meter, self.train_records = SegmentationMeter(trainer.n_classes), []

    @staticmethod
    def dataset(cfg, train):
        from .data import datasets as D
        data = cfg["data"]
        # (shuffle and augmentation happen on the device: the host object only reads the shards and splits them by Area)
        return D.Indoor3DSemSeg(data["path"], data["num_points"], train=train, aug=False, test_area=data.get("test_area", "Area_5"),
                                data_precent=float(data.get("data_percent", 1.0)))

    def loader(self, trainer, data, train):
        from .data.s3dis_blocks import BlockBatches, DeviceS3DISBlocks
        d = trainer.cfg["data"]
        return device_batches(trainer, data, train, DeviceS3DISBlocks, BlockBatches, num_points=d["num_points"],
                              aug=bool(d["aug"]) and train, data_percent=float(d["data_percent"]), sigma=float(d["jitter_sigma"]),
                              clip=float(d["jitter_clip"]), cstd=float(d["color_jitter_std"]), ratio=float(d["color_shift_ratio"]),
                              hue_max=float(d["hue_max"]), sat_max=float(d["saturation_max"]))

    def _block_pred(self, trainer, pcd):
        out = trainer.model(pcd)
        return out[0] if isinstance(out, (tuple, list)) else out                      # the reference returns (pred, lattice stats)

    def loss(self, trainer, batch):
        pcd, labels = batch
        pred = self._block_pred(trainer, pcd)
        # kept for the train confusion (the step's, or a graph's static one) — detached: a tensor with a grad_fn held across
        # steps keeps the autograd graph and its AccumulateGrad nodes alive, pinned to the stream of the first step, and a
        # later capture on another stream then breaks
        self.out = pred.detach()
        return self.ce(pred[:, :, 0], labels)

    def after_step(self, out, batch):
        self.train_meter.update(out, batch[1])

    def val_step(self, trainer, *t):
        """(points, labels) -> (pred, loss)."""
        pred = self._block_pred(trainer, t[0])
        return pred, self.ce(pred[:, :, 0], t[1])

    def val_meter(self, trainer):
        from .data.s3dis_blocks import SegmentationMeter
        return SegmentationMeter(trainer.n_classes)

    def val_batch(self, trainer, step, batch, meter):
        pred, loss = step(*batch)
        meter.update(pred, batch[1])
        return (loss,)

    def val_scalars(self, rec):
        return {"val/" + k: v for k, v in rec.items() if k not in ("epoch", "iters", "batches")}

    def _report_train_confusion(self, trainer, epoch):
        """The epoch's train metrics (train_segmentation.py:236-237) from the confusion matrix the steps filled; it starts anew."""
        if self.train_meter.conf is None:
            return
        if parallel._active(trainer.dist):
            self.train_meter.reduce(trainer.dist)
        rec = dict(self.train_meter.result(), epoch=epoch, iters=trainer.iters)
        self.train_meter.reset()
        if trainer.rank == 0:
            for k, v in rec.items():
                if k not in ("epoch", "iters"):
                    trainer.writer.add_scalar("train/" + k, v, global_step=epoch)
        self.train_records.append(rec)

    def after_epoch(self, trainer, epoch):
        # train_segmentation.py:236-244: the train metrics, then checkpoints and validation by the 0-based epoch
        tr = trainer.cfg["train"]
        trainer._flush()
        self._report_train_confusion(trainer, epoch)
        if epoch > 0 and epoch % int(tr["save_each_epoch"]) == 0:
            trainer.save(epoch=epoch)
        if epoch % int(tr["val_step"]) == 0:
            trainer.validate(epoch=epoch)


class Reconstruction(Protocol):
    """Selected by `data.kind: what3d_device` too (`data.path`, `data.im_size`, `data.gt_size`, `data.batch_size_val` as
    configs/reconstruction.yaml has them, optional `data.cache_dir`; `dataset` may be a data.image_point.ImageToPoint or a
    data.image_point.DeviceImageToPoint; `n_classes` is not used): the decoded renderings and the clouds of a What3D split stay
    on the device, every batch is resized, normalised and resampled in one launch (data/image_point.py ImageBatches);
    noise = sphere_noise(B, gt_size), rec = model(noise, img)[0], loss = mean sqrt(EMD(rec, gt, train.emd_eps, train.emd_iters));
    loss_chamfer_adj is computed without gradient and logged (`last_chamfer`, `train/loss_chamfer`); the scheduler steps per
    iteration, `generator_iter_{n}.t7` every `train.save_each` iterations; a validation every epoch, `generator_epoch_{e}.t7`
    every `train.save_each_epoch` epochs (train_reconstruction.py, train_image_reconstruction.py; F1 on the test split:
    eval_reconstruction_f1.py).  Defaults: train_image_reconstruction.py:95-96,173-174,237-239; eval_reconstruction_f1.py:51,98-104.

    The noise: `noise_gen` is seeded by `data.seed * 1000003 + 15485863 + rank` and `_draw_noise` is the one place that draws
    from it, once per step.  Under `hip_graph` the noise is an INPUT of the graph: one eager draw per step, before the replay, in
    step order, so a graphed and an eager run of one seed see the same noise at step k; neither the warm-up nor the capture draws,
    and the logged Chamfer term is a static output of the graph (`fit` keeps a clone).

    Validation (train_image_reconstruction.py:225-268): eval mode, no grad, the 'val' split in batches of `data.batch_size_val`;
    per batch sqrt(EMD(rec, gt, val_emd_eps, val_emd_iters)).mean(1).mean() and loss_chamfer_adj, averaged over the batches and
    the ranks; the record goes to <exp>/reconstruction_val.jsonl and a new minimum of the EMD saves `generator_best_0.t7` /
    `g_opt_best_0.t7`."""
    name, kinds = "reconstruction", ("what3d_device",)
    DATA = {"kind": "what3d_device", "im_size": 128, "gt_size": 8192, "seed": 42, "eval_points": 10000, "eval_noise": 8192}
    TRAIN = {"emd_eps": 0.005, "emd_iters": 50, "val_emd_eps": 0.004, "val_emd_iters": 3000, "f1_threshold": 0.01, "save_each_epoch": 1}
    batch_size_val, loader_epochs = True, True
    val_terms, val_file, best_key = ("loss_emd", "loss_chamfer"), "reconstruction_val.jsonl", "loss_emd"

    def __init__(self, trainer):
        super().__init__(trainer)
        self.last_chamfer = None
        self.noise_gen = torch.Generator(device=trainer.device).manual_seed(int(trainer.cfg["data"]["seed"]) * 1000003 + 15485863 + trainer.rank)

    @staticmethod
    def dataset(cfg, train):
        from .data.image_point import ImageToPoint
        data = cfg["data"]
        split = "test" if train == "test" else ("train" if train else "val")
        return ImageToPoint(data["path"], split=split, im_size=data["im_size"],
                            points=data["eval_points"] if split == "test" else data["gt_size"])

    def loader(self, trainer, data, train):
        from .data.image_point import DeviceImageToPoint, ImageBatches
        return device_batches(trainer, data, train, DeviceImageToPoint, ImageBatches, cache=True)

    def _draw_noise(self, pcd_gt, n_noise=None):
        """The step's sphere noise [B, 3, gt_size]: ONE draw from `noise_gen` (the only place the harness draws from it)."""
        from .metrics import sphere_noise
        return sphere_noise(pcd_gt.shape[0], pcd_gt.shape[-1] if n_noise is None else n_noise, pcd_gt.device, generator=self.noise_gen)

    def _reconstruct(self, trainer, img, pcd_gt, eps, iters, n_noise=None, noise=None, val=False):
        """(sqrt-EMD loss, rec [B, 3, 1, N], gt [B, 3, 1, n]) of train_image_reconstruction.py:166-175 for a device batch.
        `noise`: the sphere noise to use (a graph's static buffer, filled from an eager draw); by default it is drawn here.
        `val`: the validation call — the EMD through `_val_emd`, whose stats come fourth."""
        from .emd import emd_distance
        gt = pcd_gt[:, :, None]
        if noise is None:
            noise = self._draw_noise(pcd_gt, n_noise)
        out = trainer.model(noise, img)
        rec = out[0] if isinstance(out, (tuple, list)) else out
        if val:
            dist, stats = _val_emd(trainer, rec[:, :, 0].permute(0, 2, 1), gt[:, :, 0].permute(0, 2, 1), eps, iters)
            return torch.sqrt(dist).mean(1).mean(), rec, gt, stats
        dist, _ = emd_distance(rec[:, :, 0].permute(0, 2, 1), gt[:, :, 0].permute(0, 2, 1), eps, iters)
        return torch.sqrt(dist).mean(1).mean(), rec, gt

    def loss(self, trainer, batch):
        from .chamfer import loss_chamfer_adj
        tr = trainer.cfg["train"]
        loss, rec, gt = self._reconstruct(trainer, batch[0], batch[1], float(tr["emd_eps"]), int(tr["emd_iters"]),
                                          noise=batch[2] if len(batch) > 2 else None)      # (a graph's batch carries its noise)
        with torch.no_grad():
            self.out = loss_chamfer_adj(rec.detach(), gt)
        return loss

    def graph_inputs(self, trainer, batch):
        # the step's noise: the same generator, the same call and the same one draw per step as the eager step's, drawn outside
        # the graph and handed to it as a third static input (a capture that fell back to eager steps gets it as batch[2])
        return batch[0], batch[1], self._draw_noise(batch[1])

    def after_step(self, out, batch):
        self.last_chamfer, self.logged = out, {"loss_chamfer": out}

    def val_step(self, trainer, *t):
        """(img, cloud, noise) -> (loss_emd, loss_chamfer), the stats of `_val_emd` third under `train.val_emd_tail`."""
        from .chamfer import loss_chamfer_adj
        tr = trainer.cfg["train"]
        l_emd, rec, gt, stats = self._reconstruct(trainer, t[0], t[1], float(tr["val_emd_eps"]), int(tr["val_emd_iters"]), noise=t[2], val=True)
        return (l_emd, loss_chamfer_adj(rec, gt)) + (() if stats is None else (stats,))

    val_meter = EmdTail

    def val_batch(self, trainer, step, batch, tail):
        l_emd, l_cd, *stats = step(batch[0], batch[1], self._draw_noise(batch[1]))    # (the noise: one eager draw per batch, as ever)
        tail.update(stats)
        return l_emd, l_cd

    def after_epoch(self, trainer, epoch):
        # train_image_reconstruction.py:225-268: a validation every epoch, checkpoints by the 0-based epoch
        trainer._flush()
        trainer.validate(epoch=epoch)
        if epoch % int(trainer.cfg["train"]["save_each_epoch"]) == 0:
            trainer.save(epoch=epoch)


_CLASSES = (Segmentation, Classification, Completion, KPConv, Scan, Blocks, Reconstruction)
PROTOCOLS = {key: cls for cls in _CLASSES for key in (cls.name,) + cls.kinds}
DATASETS = {kind: cls for cls in _CLASSES for kind in cls.kinds + cls.host_kinds}       # the arms of harness.make_dataset


def pick(task, kind=""):
    """The protocol class of a Trainer: the one `data.kind` belongs to, else the task's."""
    cls = PROTOCOLS.get(kind) or PROTOCOLS[task]
    assert cls.kind_selects or cls.name == task, "data.kind %s is the %s task" % (kind, cls.name)
    return cls
