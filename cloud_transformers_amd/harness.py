"""YAML-driven training harness around the hot path: the reference's experiment plumbing
(utils/train_util.py:19-134) and the skeleton of its training scripts (train_segmentation.py:64-230,
train_classification.py) with synthetic loaders, so that a reference config + model file runs end to end on this
package's layers and checkpoints stay interchangeable.

* config: the reference's YAML schema — `experiment.{root,writer_root}`, `data.{batch_size,num_points,...}`,
  `model.generator` (a python file defining `Model`; the remaining `model.*` keys are its kwargs),
  `train.{optimizer,scheduler,num_epochs,save_each,...}`, optional `restore.{generator,optimizer,new_lr}`; `train.deterministic:
  true` (this package's own key) runs `fit` in deterministic mode (determinism.py): equal seeds, equal gradients. `train.matmul_precision:
  high` (likewise) runs `fit` with the pointwise GEMMs in the TF32-class mode of precision.py. `train.conv_precision: high`
  (likewise, independent of it) does the same for the grouped 3^d convolutions.
  `train.freeze_norms: true` (optionally `train.freeze_norm_affine: true`; this package's own keys) fine-tunes on frozen
  norm statistics (norms.py `freeze_norms`, applied after the data-parallel wrap): the running statistics never move, no
  statistics are exchanged between ranks, validation and checkpoints are unchanged.
* checkpoints: `<exp>/<name>_<epoch_name>_<n>.t7` holding a plain `state_dict()` (train_util.py:74-80); parameter names of
  this package's modules equal the reference's, so released weights load with `strict=True`; `restore_exp_fix` drops the
  `module.` prefix DistributedDataParallel adds (train_util.py:98-117).
* data: `SyntheticClouds` produces batches of the shapes and dtypes the reference loaders yield (no files needed); with
  `data.kind` in the config (or `Trainer(dataset=...)`) the loop runs on `data/datasets.py`'s readers instead — `scanobjectnn`
  (datasets/scanobjectnn.py: `data.path` = the .h5 / .npz file) and `s3dis` (datasets/s3dis_v2.py: `data.path` = the
  indoor3d_sem_seg_hdf5_data directory), items equal to the reference loaders' under the same seeds.  `s3dis_kpconv`
  (`data.path` = the Stanford3dDataset_v1.2 folder) selects the `segmentation_kpconv` task: sphere items sampled on the
  device, masked cross-entropy with gradient clipping, vote validation and per-epoch checkpoints (train_kpconv.py,
  train_segmentation_kpconv.py).  `shapenet_completion` (the `completion` task; `data.category_path`, `data.partial_path`,
  `data.gt_path`, `data.n_renders`, `data.input_size`, `data.gt_size` as configs/inpainting.yaml has them) reads the
  ShapeNetCompletion .pcd files (data/completion.py) and prepares every batch on the device; one validation per epoch
  (train_completion.py, train_inpainter.py).  `shapenet_completion_device` (the same keys, optional `data.cache_dir`) reads every
  file of a subset once, keeps the clouds on the device and gathers, samples and mirrors every batch there in one launch
  (data/completion.py DeviceCompletionBatches).  `scanobjectnn_device` (the `classification_scanobjectnn` task; `data.path`,
  `data.path_val`, `data.batch_size_val`, optional `data.subsample`) keeps the ScanObjectNN split on the device and gathers
  every batch there (data/scanobjectnn.py), validates every `train.val_step` epochs with the reference's accuracies and keeps
  the `best` / `macc_best` checkpoints (train_classification.py).  `s3dis_device` (the `segmentation_blocks` task; `data.path`,
  `data.num_points`, `data.test_area`, `data.data_percent`, `data.aug`, `data.batch_size_val` as configs/s3dis.yaml has them)
  keeps the 1x1 m blocks on the device, assembles and augments every batch in one launch (data/s3dis_blocks.py), fills the
  train and validation confusion matrices on the device and appends every validation to <exp>/segmentation_val.jsonl
  (train_segmentation.py).  `what3d_device` (the `reconstruction` task; `data.path`, `data.im_size`, `data.gt_size`,
  `data.batch_size_val` as configs/reconstruction.yaml has them, optional `data.cache_dir`) keeps the decoded renderings and
  the clouds of a What3D split on the device, resizes, normalises and resamples every batch in one launch
  (data/image_point.py), trains on the EMD, validates every epoch (<exp>/reconstruction_val.jsonl, the `best` checkpoints) and
  scores F1 on the test split (train_reconstruction.py; train_image_reconstruction.py, eval_reconstruction_f1.py).
"""
import copy
import datetime
import shutil
import time
from collections import OrderedDict
from pathlib import Path

import torch
from torch import nn

from . import parallel


def worker_init_fn(worker_id):
    import random
    import numpy as np
    seed = int(np.random.get_state()[1][0]) + worker_id
    np.random.seed(seed % (2 ** 32))
    random.seed(seed)


def get_model(model_file, params_dict, exp_dir=None):
    """Instantiate `Model(**params_dict)` from a model python file; keep a copy beside the experiment.  A model file that
    imports `torchvision.models` for its `resnet50` (model_zoo/image_reconstruction/reconstructor.py) builds without
    torchvision too: while the file executes, and only when `import torchvision` fails, layers/resnet.py's stand-in pair sits in
    sys.modules; it is removed afterwards."""
    from .layers.resnet import stand_in_for_torchvision
    env = {"__name__": "model_file"}
    with stand_in_for_torchvision():
        with open(str(model_file), "r") as f:
            exec(compile(f.read(), str(model_file), "exec"), env)
        model = env["Model"](**params_dict)
    if exp_dir is not None:
        assert Path(exp_dir).exists()
        shutil.copy2(str(model_file), str(exp_dir))
    return model


def check_model_paths(*paths):
    out = []
    for p in paths:
        f = Path(p)
        assert f.exists() and f.suffix == ".py", p
        out.append((p, f.name[:-3]))
    return out


class NullWriter:
    """Stands in for tensorboardX.SummaryWriter when it is not installed: keeps the last value of every tag."""

    def __init__(self, logdir=None):
        self.logdir, self.scalars = logdir, {}

    def add_scalar(self, tag, value, global_step=None):
        self.scalars[tag] = (float(value), global_step)

    def close(self):
        pass


def _summary_writer(path):
    try:
        from tensorboardX import SummaryWriter
    except ImportError:
        try:
            from torch.utils.tensorboard import SummaryWriter
        except ImportError:
            return NullWriter(str(path))
    return SummaryWriter(str(path))


def create_experiment(*desc, params_dict):
    exp_path, writer_path = Path(params_dict["exp_root"]), Path(params_dict["writer_root"])
    assert writer_path.exists(), writer_path
    full_desc = "_".join([*desc, datetime.datetime.now().strftime("%d_%m_%y_%H_%M_%S")])
    writer = _summary_writer(writer_path.joinpath(full_desc))
    exp_dir = exp_path.joinpath(full_desc)
    exp_dir.mkdir(parents=True)
    if "config_path" in params_dict:
        cfg = Path(params_dict["config_path"])
        assert cfg.exists()
        shutil.copy2(str(cfg), str(exp_dir))
    return writer, exp_dir, full_desc


def save_exp(objects, names, exp_path, epoch, epoch_name="epoch"):
    assert len(objects) == len(names)
    for obj, name in zip(objects, names):
        with open("{}/{}_{}_{}.t7".format(str(exp_path), name, epoch_name, epoch), "wb") as f:
            torch.save(obj.state_dict(), f)


def restore_exp(objects, names, device, verbose=True, strict=True):
    assert len(objects) == len(names)
    for obj, name in zip(objects, names):
        assert Path(name).exists(), name
        if verbose:
            print("restoring from {}".format(name))
        with open(name, "rb") as f:
            state = torch.load(f, map_location=device)
        if isinstance(obj, nn.Module):
            obj.load_state_dict(state, strict=strict)
        else:
            obj.load_state_dict(state)


def restore_exp_fix(objects, names, device=None, verbose=True):
    """Load checkpoints written from a DistributedDataParallel wrapper into plain modules (strict)."""
    device = device if device is not None else torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    assert len(objects) == len(names)
    for obj, name in zip(objects, names):
        assert Path(name).exists(), name
        if verbose:
            print("restoring from {}".format(name))
        with open(name, "rb") as f:
            state = torch.load(f, map_location=device)
        obj.load_state_dict(OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in state.items()), strict=True)


def make_optimizer(params, opt_cfg):
    cfg = dict(opt_cfg)                        # (the reference deletes `type` from the caller's dict; a copy keeps cfg reusable)
    return getattr(torch.optim, cfg.pop("type"))(params, **cfg)


def make_scheduler(optimizer, scheduler_cfg):
    cfg = dict(scheduler_cfg)
    return getattr(torch.optim.lr_scheduler, cfg.pop("type"))(optimizer, **cfg)


class SyntheticClouds(torch.utils.data.Dataset):
    """Batches shaped like the reference loaders': `segmentation` -> (points f32 [N, 3], labels i64 [N]) as
    datasets/s3dis_v2.py yields; `classification` -> (points f32 [N, 3], label i64 [], mask f32 [N]) as
    datasets/scanobjectnn.py yields; `completion` -> (noise f32 [4, N]: points on the unit sphere + the "is a real point"
    label, partial cloud f32 [n_classes, 3] (n_classes = its size), ground truth f32 [N, 3]) — what train_inpainter.py:178-185
    hands to the generator and the losses after `partial_postproces`.  Deterministic per index."""

    def __init__(self, task, num_points, n_classes, length=64, seed=0, channels=3):
        assert task in ("segmentation", "classification", "completion") and channels >= 3
        self.task, self.n, self.k, self.length, self.seed, self.ch = task, num_points, n_classes, length, seed, channels

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        if self.task == "completion":
            gt = torch.nn.functional.normalize(torch.randn(self.n, 3, generator=g), dim=1) * (0.5 + 0.4 * torch.rand((), generator=g))
            part = gt[torch.randperm(self.n, generator=g)[: self.k]] + 0.01 * torch.randn(self.k, 3, generator=g)
            sphere = torch.nn.functional.normalize(torch.randn(3, self.n, generator=g), dim=0)
            noise = torch.cat([sphere, (torch.rand(1, self.n, generator=g) > 0.5).float()], dim=0)
            return noise, part, gt
        pts = torch.rand(self.n, self.ch, generator=g) * 2 - 1          # xyz (+ colour / normalised position channels)
        if self.task == "segmentation":
            # labels follow the geometry (octants), so a few steps of training move the loss
            lab = ((pts[:, 0] > 0).long() + 2 * (pts[:, 1] > 0).long() + 4 * (pts[:, 2] > 0).long()) % self.k
            return pts, lab
        lab = torch.randint(self.k, (), generator=g)
        pts = pts * (0.5 + 0.5 * (lab.float() + 1) / self.k)
        return pts, lab, (pts[:, 2] > 0).float()


def make_dataset(cfg, task, n_classes, length=64, channels=3, train=True):
    """The dataset `data.kind` of the config names: "synthetic" (default), "scanobjectnn" or "s3dis" (data/datasets.py);
    "s3dis_kpconv" gives the (train, validation) Areas of train_kpconv.load_kpconv_areas (`train=False`: no train Areas);
    "shapenet_completion" and "shapenet_completion_device" the TRAIN (`train=False`: VAL) subset of data/completion.py's
    ShapeNetDataLoader (the second leaves its items to the device);
    "scanobjectnn_device" the ScanObjectNN of `data.path` (`train=False`: `data.path_val`) with its items left to the device;
    "s3dis_device" the Indoor3DSemSeg of `data.path` (`train=False`: the blocks of `data.test_area`), its items left to the device;
    "what3d_device" the ImageToPoint of `data.path`, split 'train' (`train=False`: 'val'; `train="test"`: 'test' with
    `data.eval_points` points), its items left to the device."""
    data = cfg["data"]
    kind = str(data.get("kind", "synthetic")).lower()
    if kind == "what3d_device":
        assert task == "reconstruction", "data.kind what3d_device is the reconstruction task"
        from .data.image_point import ImageToPoint
        split = "test" if train == "test" else ("train" if train else "val")
        return ImageToPoint(data["path"], split=split, im_size=data["im_size"],
                            points=data["eval_points"] if split == "test" else data["gt_size"])
    if kind == "s3dis_device":
        assert task == "segmentation_blocks", "data.kind s3dis_device is the segmentation_blocks task"
        from .data import datasets as D
        # (shuffle and augmentation happen on the device: the host object only reads the shards and splits them by Area)
        return D.Indoor3DSemSeg(data["path"], data["num_points"], train=train, aug=False, test_area=data.get("test_area", "Area_5"),
                                data_precent=float(data.get("data_percent", 1.0)))
    if kind == "scanobjectnn_device":
        assert task == "classification_scanobjectnn", "data.kind scanobjectnn_device is the classification_scanobjectnn task"
        from .data import datasets as D
        # (augmentation and subsampling happen on the device: the host object only reads, centres and normalises)
        return D.ScanObjectNN(data["path"] if train else data["path_val"], train=False, subsample=None,
                              center=data.get("center", True), normalize=data.get("normalize", True))
    if kind in ("shapenet_completion", "shapenet_completion_device"):
        assert task == "completion", "ShapeNet completion items are (partial cloud, complete cloud): the completion task"
        from .data.completion import DatasetSubset, shapenet_loader
        return shapenet_loader(data).get_dataset(DatasetSubset.TRAIN if train else DatasetSubset.VAL)
    if kind == "s3dis_kpconv":
        assert task == "segmentation_kpconv", "S3DIS KPConv items are (points, mask, features, labels): the segmentation_kpconv task"
        from .train_kpconv import load_kpconv_areas
        return load_kpconv_areas(cfg, train=train)
    if kind == "synthetic":
        return SyntheticClouds(task, data["num_points"], n_classes, length=length, channels=channels)
    from .data import datasets as D
    if kind == "scanobjectnn":
        assert task == "classification", "ScanObjectNN items are (points, label, mask): the classification task"
        return D.ScanObjectNN(data["path"], train=train, subsample=data.get("num_points"), center=data.get("center", True),
                              normalize=data.get("normalize", True))
    if kind == "s3dis":
        assert task == "segmentation", "S3DIS blocks are (points, labels): the segmentation task"
        return D.Indoor3DSemSeg(data["path"], data["num_points"], train=train, aug=bool(data.get("aug", train)),
                                test_area=data.get("test_area", "Area_5"), data_precent=float(data.get("data_precent", 1.0)))
    raise ValueError("data.kind must be synthetic, scanobjectnn, scanobjectnn_device, s3dis, s3dis_device, s3dis_kpconv, shapenet_completion, "
                     "shapenet_completion_device or what3d_device (got %r)" % kind)


class Trainer:
    """The reference scripts' loop: model file + YAML config -> DDP(+SyncBN) model, optimizer, scheduler, steps with
    loss reduction to rank 0, `.t7` checkpoints every `train.save_each` iterations.

    `task`: "segmentation" (loss = CE(pred[:, :, 0], labels), train_segmentation.py:178), "classification"
    (loss = CE(logits, label) + seg_weight * BCE-with-logits(mask), train_classification.py) or "completion"
    (loss = mean sqrt(EMD(rec, gt, 0.005, 50)) + chamfer_weight * loss_chamfer(rec, gt), train_inpainter.py:186-192;
    `n_classes` is then the size of the partial cloud) or "segmentation_kpconv" (selected by `data.kind: s3dis_kpconv` too:
    loss = sum(CE * mask) / sum(mask) of model(points, mask, features), gradients clipped to `train.clip_grad_norm` (10),
    validation every `train.val_step` epochs and after the last, `generator_epoch_{e}.t7` / `g_opt_epoch_{e}.t7` every
    `train.save_each_epoch` epochs; `dataset` may be the (train, validation) Areas — train_kpconv.py).  With `data.kind:
    shapenet_completion` the completion task's batches are prepared on the device (data/completion.py CompletionBatches)
    and `fit` validates once per epoch (`validate`); with `data.kind: shapenet_completion_device` the subset stays on the device
    and the items are gathered there too (DeviceCompletionBatches; `dataset` may be a completion Dataset or a
    DeviceShapeNetCompletion).  "classification_scanobjectnn" (selected by `data.kind:
    scanobjectnn_device` too; `dataset` may be a data.datasets.ScanObjectNN or a data.scanobjectnn.DeviceScanObjectNN):
    loss = (1 - seg_weight) * CE(out[0], label) + seg_weight * BCE-with-logits(out[1][:, 0, 0], mask) of train_classification.py:
    201-204 (the model's output is indexed, so the reference's three-output classifier and two-output models both fit),
    batches gathered on the device (data/scanobjectnn.py ScanBatches; `n_classes` sizes the per-class accuracies), validation
    every `train.val_step` epochs, `generator_epoch_{e}.t7` every `train.save_each_epoch` epochs (train_classification.py).
    "segmentation_blocks" (selected by `data.kind: s3dis_device` too; `dataset` may be a data.datasets.Indoor3DSemSeg or a
    data.s3dis_blocks.DeviceS3DISBlocks): loss = CE(pred[:, :, 0], labels) on batches assembled on the device (data/s3dis_blocks.py
    BlockBatches), a train confusion matrix updated every step on the device and reported per epoch (`train_records`),
    validation every `train.val_step` epochs (<exp>/segmentation_val.jsonl), `generator_iter_{n}.t7` every `train.save_each`
    iterations and `generator_epoch_{e}.t7` every `train.save_each_epoch` epochs (train_segmentation.py).
    "reconstruction" (selected by `data.kind: what3d_device` too; `dataset` may be a data.image_point.ImageToPoint or a
    data.image_point.DeviceImageToPoint; `n_classes` is not used): noise = sphere_noise(B, gt_size), rec = model(noise, img)[0],
    loss = mean sqrt(EMD(rec, gt, train.emd_eps, train.emd_iters)) on batches assembled on the device (data/image_point.py
    ImageBatches); loss_chamfer_adj is computed without gradient and logged (`last_chamfer`); the scheduler steps per iteration,
    `generator_iter_{n}.t7` every `train.save_each` iterations; a validation every epoch (<exp>/reconstruction_val.jsonl,
    `generator_epoch_{e}.t7` every `train.save_each_epoch` epochs, `generator_best_0.t7` on a new minimum of the EMD —
    train_reconstruction.py, train_image_reconstruction.py)."""

    def __init__(self, cfg, task, n_classes, device=None, dist=None, exp_name="exp", dataset_length=64, make_dirs=True,
                 channels=3, dataset=None):
        self.cfg = cfg = copy.deepcopy(cfg)
        if task == "segmentation_kpconv" or str(cfg["data"].get("kind", "")).lower() == "s3dis_kpconv":
            from .train_kpconv import kpconv_config
            task, self.cfg = "segmentation_kpconv", kpconv_config(cfg)
            cfg = self.cfg
        if task == "classification_scanobjectnn" or str(cfg["data"].get("kind", "")).lower() == "scanobjectnn_device":
            from .train_classification import classification_config
            task, self.cfg = "classification_scanobjectnn", classification_config(cfg)
            cfg = self.cfg
        if task == "segmentation_blocks" or str(cfg["data"].get("kind", "")).lower() == "s3dis_device":
            from .train_segmentation import segmentation_config
            task, self.cfg = "segmentation_blocks", segmentation_config(cfg)
            cfg = self.cfg
        if task == "reconstruction" or str(cfg["data"].get("kind", "")).lower() == "what3d_device":
            from .train_reconstruction import reconstruction_config
            task, self.cfg = "reconstruction", reconstruction_config(cfg)
            cfg = self.cfg
        self.task, self.dist, self.n_classes = task, dist, n_classes
        self.rank = dist.get_rank() if parallel._active(dist) else 0
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        model_cfg = dict(cfg["model"])
        model_file, _ = check_model_paths(model_cfg.pop("generator"))[0]
        self.writer, self.exp_dir = NullWriter(), None
        if self.rank == 0 and make_dirs:
            Path(cfg["experiment"]["writer_root"]).mkdir(parents=True, exist_ok=True)
            params = {"exp_root": cfg["experiment"]["root"], "writer_root": cfg["experiment"]["writer_root"]}
            if "config_path" in cfg:
                params["config_path"] = cfg["config_path"]
            self.writer, self.exp_dir, _ = create_experiment(exp_name, params_dict=params)
        model = get_model(model_file, model_cfg, exp_dir=self.exp_dir).to(self.device)
        if self.device.type == "cuda":
            from .layers.pointwise import convert_pointwise
            convert_pointwise(model)      # the model file's plain nn.Conv1d(k=1) stems / heads onto the blocks' GEMM kernels
        if "restore" in cfg and "generator" in cfg["restore"]:
            restore_exp_fix([model], [cfg["restore"]["generator"]], device=self.device, verbose=self.rank == 0)
        self._stream = None
        tr = cfg["train"]
        freeze, freeze_affine = bool(tr.get("freeze_norms", False)), bool(tr.get("freeze_norm_affine", False))
        if freeze_affine and not freeze:
            raise ValueError("train.freeze_norm_affine needs train.freeze_norms: true")
        if freeze and freeze_affine and parallel._active(dist):
            # DistributedDataParallel fixes the set of parameters it reduces when it is built: the norms' weight and bias stop
            # taking gradients before the wrap (the conversion to SyncBatchNorm keeps the Parameter objects and their flags)
            for m in model.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.affine:
                    m.weight.requires_grad_(False)
                    m.bias.requires_grad_(False)
        if parallel._active(dist):
            if self.device.type == "cuda":
                # DDP's gradient hooks (and its bucketed all-reduce) run on the stream the wrapper was BUILT on: the training
                # steps, and the capture of fit(hip_graph=True), use that same side stream (torch notes/cuda.rst, "Usage
                # with DistributedDataParallel")
                self._stream = torch.cuda.Stream(device=self.device)
                self._stream.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(self._stream):
                    model = parallel.data_parallel(model, self.device.index)
            else:
                model = parallel.data_parallel(model, None)
        if freeze:
            # after the conversion to SyncBatchNorm (which builds new modules and would drop the marks) and the wrap: every norm
            # in eval mode on its stored statistics, also through fit's model.train() — no statistics, no exchange of them
            from .norms import freeze_norms
            freeze_norms(model, affine=freeze_affine)
        self.model = model
        if "scale_lr" in tr:      # the learnable residual scales of the AdaIN blocks get their own rate
            named = list(model.named_parameters())
            params = [{"params": [p for n, p in named if not n.endswith("scale")]},
                      {"params": [p for n, p in named if n.endswith("scale")], "lr": tr["scale_lr"]}]
        else:
            params = model.parameters()
        self.optimizer = make_optimizer(params, tr["optimizer"])
        if "restore" in cfg and "optimizer" in cfg["restore"]:
            restore_exp([self.optimizer], [cfg["restore"]["optimizer"]], self.device, verbose=self.rank == 0)
            if "new_lr" in cfg["restore"]:
                for g in self.optimizer.param_groups:
                    g["lr"] = cfg["restore"]["new_lr"]
        self.scheduler = make_scheduler(self.optimizer, tr["scheduler"]) if "scheduler" in tr else None
        # `dataset`: any torch Dataset whose items have the task's layout; else what `data.kind` of the config names
        data = dataset if dataset is not None else make_dataset(cfg, task, n_classes, length=dataset_length, channels=channels)
        self.kp, self.clip, self.val_records = None, None, []
        kind = str(cfg["data"].get("kind", "")).lower()
        self.shapenet_device = kind == "shapenet_completion_device"
        self.shapenet, self.val_loader, self.best_val = kind == "shapenet_completion" or self.shapenet_device, None, None
        self.scan, self.best_acc, self.best_macc = task == "classification_scanobjectnn", float("-inf"), float("-inf")
        self.blocks, self.train_meter, self.train_records, self._pred = task == "segmentation_blocks", None, [], None
        self._graph_preds, self._graph_chamfers, self._val_graph = {}, {}, None
        self.recon, self.last_chamfer, self._noise_gen = task == "reconstruction", None, None
        if self.recon:
            self.sampler = None                          # (ImageBatches holds torch's DistributedSampler itself)
            self.loader = self._image_batches(data, train=True)
            self._noise_gen = torch.Generator(device=self.device).manual_seed(int(cfg["data"]["seed"]) * 1000003 + 15485863 + self.rank)
        elif self.blocks:
            from .data.s3dis_blocks import SegmentationMeter
            self.sampler = None                          # (BlockBatches holds torch's DistributedSampler itself)
            self.loader = self._block_batches(data, train=True)
            self.train_meter = SegmentationMeter(n_classes)
        elif self.scan:
            self.sampler = None                          # (ScanBatches holds torch's DistributedSampler itself)
            self.loader = self._scan_batches(data, train=True)
        elif self.shapenet_device:
            assert task == "completion", "data.kind shapenet_completion_device is the completion task"
            self.sampler = None                          # (DeviceCompletionBatches holds torch's DistributedSampler itself)
            self.loader = self._completion_batches(data, train=True)
        elif self.shapenet:
            from .data.completion import CompletionBatches
            assert task == "completion", "data.kind shapenet_completion is the completion task"
            self.sampler = torch.utils.data.distributed.DistributedSampler(data) if parallel._active(dist) else None
            self.loader = CompletionBatches(data, cfg["data"]["batch_size"], self.device, seed=int(cfg["data"].get("seed", 0)),
                                            rank=self.rank, shuffle=True, drop_last=bool(cfg["data"].get("drop_last", True)),
                                            num_workers=int(cfg["data"].get("num_workers", 0)), sampler=self.sampler,
                                            worker_init_fn=worker_init_fn)
        elif task == "segmentation_kpconv":
            from .train_kpconv import KPConvData
            # one iteration over the loader is one epoch of device batches (a plan of sphere picks, sharded over the ranks)
            self.kp = self.loader = KPConvData(cfg, self.device, dist, areas=data)
            self.sampler, self.clip = None, float(tr["clip_grad_norm"])
        else:
            self.sampler = torch.utils.data.distributed.DistributedSampler(data) if parallel._active(dist) else None
            self.loader = torch.utils.data.DataLoader(data, batch_size=cfg["data"]["batch_size"], shuffle=self.sampler is None,
                                                      num_workers=int(cfg["data"].get("num_workers", 0)), sampler=self.sampler,
                                                      drop_last=bool(cfg["data"].get("drop_last", True)),
                                                      worker_init_fn=worker_init_fn)
        self.ce, self.bce = nn.CrossEntropyLoss(), nn.BCEWithLogitsLoss()
        self.iters = 0

    def _completion_batches(self, data, train):
        """DeviceCompletionBatches over `data` (a host completion Dataset is read and uploaded first), this rank's shard."""
        from .data.completion import DeviceCompletionBatches, DeviceShapeNetCompletion
        d = self.cfg["data"]
        ds = data if isinstance(data, DeviceShapeNetCompletion) else DeviceShapeNetCompletion(data, self.device, cache_dir=d.get("cache_dir"))
        active = parallel._active(self.dist)
        return DeviceCompletionBatches(ds, d["batch_size"] if train else d.get("batch_size_val", d["batch_size"]), train=train,
                                       seed=int(d.get("seed", 0)) + (0 if train else 7919), rank=self.rank,
                                       world=self.dist.get_world_size() if active else 1, drop_last=bool(d.get("drop_last", True)) and train)

    def _scan_batches(self, data, train):
        """ScanBatches over `data` (a host ScanObjectNN is uploaded first) with the config's sizes, this rank's shard."""
        from .data.scanobjectnn import DeviceScanObjectNN, ScanBatches
        d = self.cfg["data"]
        ds = data if isinstance(data, DeviceScanObjectNN) else DeviceScanObjectNN(data, self.device)
        active = parallel._active(self.dist)
        return ScanBatches(ds, d["batch_size"] if train else d["batch_size_val"], train=train, seed=int(d["seed"]) + (0 if train else 7919), rank=self.rank,
                           world=self.dist.get_world_size() if active else 1, drop_last=bool(d.get("drop_last", False)) and train,
                           subsample=d.get("subsample"), sigma=float(d["jitter_sigma"]), clip=float(d["jitter_clip"]))

    def _scan_losses(self, batch):
        """(loss, loss_cls, loss_seg, model output) of train_classification.py:199-204."""
        pcd, label, mask = batch
        out = self.model(pcd)
        w = float(self.cfg["train"]["seg_weight"])
        cls_loss, seg_loss = self.ce(out[0], label), self.bce(out[1][:, 0, 0], mask)
        return (1 - w) * cls_loss + w * seg_loss, cls_loss, seg_loss, out

    def _block_batches(self, data, train):
        """BlockBatches over `data` (a host Indoor3DSemSeg is uploaded first) with the config's sizes, this rank's shard."""
        from .data.s3dis_blocks import BlockBatches, DeviceS3DISBlocks
        d = self.cfg["data"]
        ds = data if isinstance(data, DeviceS3DISBlocks) else DeviceS3DISBlocks(data, self.device)
        active = parallel._active(self.dist)
        return BlockBatches(ds, d["batch_size"] if train else d["batch_size_val"], num_points=d["num_points"], train=train,
                            aug=bool(d["aug"]) and train, seed=int(d["seed"]) + (0 if train else 7919), rank=self.rank,
                            world=self.dist.get_world_size() if active else 1, drop_last=bool(d.get("drop_last", False)) and train,
                            data_percent=float(d["data_percent"]), sigma=float(d["jitter_sigma"]), clip=float(d["jitter_clip"]),
                            cstd=float(d["color_jitter_std"]), ratio=float(d["color_shift_ratio"]), hue_max=float(d["hue_max"]),
                            sat_max=float(d["saturation_max"]))

    def _image_batches(self, data, train, points=None):
        """ImageBatches over `data` (a host ImageToPoint is decoded and uploaded first) with the config's sizes, this rank's shard."""
        from .data.image_point import DeviceImageToPoint, ImageBatches
        d = self.cfg["data"]
        ds = data if isinstance(data, DeviceImageToPoint) else DeviceImageToPoint(data, self.device, cache_dir=d.get("cache_dir"))
        active = parallel._active(self.dist)
        return ImageBatches(ds, d["batch_size"] if train else d["batch_size_val"], train=train, seed=int(d["seed"]) + (0 if train else 7919),
                            rank=self.rank, world=self.dist.get_world_size() if active else 1,
                            drop_last=bool(d.get("drop_last", False)) and train, points=points)

    def _draw_noise(self, pcd_gt, n_noise=None):
        """The step's sphere noise [B, 3, gt_size]: ONE draw from `_noise_gen` (the only place the harness draws from it)."""
        from .metrics import sphere_noise
        return sphere_noise(pcd_gt.shape[0], pcd_gt.shape[-1] if n_noise is None else n_noise, pcd_gt.device, generator=self._noise_gen)

    def _val_emd(self, rec_bn3, gt_bn3, eps, iters):
        """The validation EMD of a batch -> (dist [B, n], stats).  `train.val_emd_tail` (default false): the auction through
        emd_with_info where its shape is supported — the same dist, a cloud's long tail in one launch — and stats = float64
        [sum of info[:, 0], clouds whose auction did not finish, clouds] on the device; otherwise today's call and stats None."""
        from .emd import emd_distance, emd_tail_supported, emd_with_info
        if bool(self.cfg["train"].get("val_emd_tail", False)) and emd_tail_supported(rec_bn3.size(0), rec_bn3.size(1)):
            dist, _, info = emd_with_info(rec_bn3, gt_bn3, eps, iters)
            clouds = torch.full((), float(info.size(0)), dtype=torch.float64, device=info.device)
            return dist, torch.stack([info[:, 0].sum().double(), (info[:, 1] > 0).sum().double(), clouds])
        return emd_distance(rec_bn3, gt_bn3, eps, iters)[0], None

    def _reconstruct(self, img, pcd_gt, eps, iters, n_noise=None, noise=None, val=False):
        """(sqrt-EMD loss, rec [B, 3, 1, N], gt [B, 3, 1, n]) of train_image_reconstruction.py:166-175 for a device batch.
        `noise`: the sphere noise to use (a graph's static buffer, filled from an eager draw); by default it is drawn here.
        `val`: the validation call — the EMD through `_val_emd`, whose stats come fourth."""
        from .emd import emd_distance
        gt = pcd_gt[:, :, None]
        if noise is None:
            noise = self._draw_noise(pcd_gt, n_noise)
        out = self.model(noise, img)
        rec = out[0] if isinstance(out, (tuple, list)) else out
        if val:
            dist, stats = self._val_emd(rec[:, :, 0].permute(0, 2, 1), gt[:, :, 0].permute(0, 2, 1), eps, iters)
            return torch.sqrt(dist).mean(1).mean(), rec, gt, stats
        dist, _ = emd_distance(rec[:, :, 0].permute(0, 2, 1), gt[:, :, 0].permute(0, 2, 1), eps, iters)
        return torch.sqrt(dist).mean(1).mean(), rec, gt

    def _block_pred(self, pcd):
        out = self.model(pcd)
        return out[0] if isinstance(out, (tuple, list)) else out                      # the reference returns (pred, lattice stats)

    def _loss(self, batch):
        if self.task == "reconstruction":
            from .chamfer import loss_chamfer_adj
            tr = self.cfg["train"]
            loss, rec, gt = self._reconstruct(batch[0], batch[1], float(tr["emd_eps"]), int(tr["emd_iters"]),
                                              noise=batch[2] if len(batch) > 2 else None)      # (a graph's batch carries its noise)
            with torch.no_grad():
                self.last_chamfer = loss_chamfer_adj(rec.detach(), gt)
            return loss
        if self.task == "segmentation_blocks":
            pcd, labels = batch
            pred = self._block_pred(pcd)
            # kept for the train confusion (the step's, or a graph's static one) — detached: a tensor with a grad_fn held across
            # steps keeps the autograd graph and its AccumulateGrad nodes alive, pinned to the stream of the first step, and a
            # later capture on another stream then breaks
            self._pred = pred.detach()
            return self.ce(pred[:, :, 0], labels)
        if self.task == "classification_scanobjectnn":
            return self._scan_losses(batch)[0]
        if self.task == "segmentation_kpconv":
            from .train_kpconv import masked_cross_entropy
            points, mask, features, labels = batch
            return masked_cross_entropy(self.model(points, mask, features), labels, mask)
        if self.task == "segmentation":
            pts, labels = batch
            pcd = pts.permute(0, 2, 1)[:, :, None].to(self.device)                    # (B, channels, 1, N)
            out = self.model(pcd)
            pred = out[0] if isinstance(out, (tuple, list)) else out                  # the reference returns (pred, lattice stats)
            return self.ce(pred[:, :, 0], labels.to(self.device))
        if self.task == "completion":
            from .chamfer import loss_chamfer
            from .emd import emd_distance
            noise, part, gt = batch
            out = self.model(noise.to(self.device), part.permute(0, 2, 1)[:, :, None].to(self.device))
            rec = out[0] if isinstance(out, (tuple, list)) else out                   # (B, 3, 1, N)
            gt4 = gt.permute(0, 2, 1)[:, :, None].to(self.device)
            tr = self.cfg["train"]
            dist, _ = emd_distance(rec[:, :, 0].permute(0, 2, 1), gt4[:, :, 0].permute(0, 2, 1),
                                   float(tr.get("emd_eps", 0.005)), int(tr.get("emd_iters", 50)))
            return torch.sqrt(dist).mean(1).mean() + float(tr.get("chamfer_weight", 1.0)) * loss_chamfer(rec, gt4)
        pts, label, mask = batch
        logits, mask_pred = self.model(pts.permute(0, 2, 1)[:, :, None].to(self.device))
        w = float(self.cfg["train"].get("seg_weight", 0.5))
        return (self.ce(logits, label.to(self.device).long())
                + w * self.bce(mask_pred.reshape(mask.shape[0], -1), mask.to(self.device).float()))     # (ScanObjectNN's mask is int64)

    def save(self, epoch=None):
        """`generator_iter_{iters}.t7` / `g_opt_iter_{iters}.t7`; with `epoch`, `generator_epoch_{epoch}.t7` / `g_opt_epoch_{epoch}.t7`."""
        if self.rank == 0 and self.exp_dir is not None:
            parallel.save_exp_parallel([self.model, self.optimizer], ["generator", "g_opt"], exp_path=self.exp_dir,
                                       epoch=self.iters if epoch is None else epoch, epoch_name="iter" if epoch is None else "epoch")

    # -- validation: the per-batch work as one function of device tensors, run eagerly or by graph replay ------------------
    def _val_step(self, *t):
        """One validation batch of this task: the eval-mode forward plus the task's validation loss terms, device tensors in,
        device tensors out (the caller holds eval mode and no_grad; the meters stay with the caller).
        reconstruction (img, cloud, noise) -> (loss_emd, loss_chamfer); completion (noise, partial, gt) -> (loss_emd,
        loss_chamfer) — both with the stats of `_val_emd` third under `train.val_emd_tail`; segmentation_blocks (points, labels) -> (pred, loss); classification_scanobjectnn (points, label, mask)
        -> (loss, loss_cls, loss_seg, logits, mask logits); segmentation_kpconv (points, mask, features, labels) -> (pred, loss)."""
        tr = self.cfg["train"]
        if self.task == "reconstruction":
            from .chamfer import loss_chamfer_adj
            l_emd, rec, gt, stats = self._reconstruct(t[0], t[1], float(tr["val_emd_eps"]), int(tr["val_emd_iters"]), noise=t[2], val=True)
            return (l_emd, loss_chamfer_adj(rec, gt)) + (() if stats is None else (stats,))
        if self.task == "completion":
            from .chamfer import loss_chamfer
            from .emd import emd_distance
            noise, part, gt = t
            out = self.model(noise, part.permute(0, 2, 1)[:, :, None])
            rec = out[0] if isinstance(out, (tuple, list)) else out
            gt4 = gt.permute(0, 2, 1)[:, :, None]
            dist, stats = self._val_emd(rec[:, :, 0].permute(0, 2, 1), gt4[:, :, 0].permute(0, 2, 1),
                                        float(tr.get("val_emd_eps", 0.004)), int(tr.get("val_emd_iters", 3000)))
            return (torch.sqrt(dist).mean(1).mean(), loss_chamfer(rec, gt4)) + (() if stats is None else (stats,))
        if self.task == "segmentation_blocks":
            pred = self._block_pred(t[0])
            return pred, self.ce(pred[:, :, 0], t[1])
        if self.task == "classification_scanobjectnn":
            loss, cls_loss, seg_loss, out = self._scan_losses(t)
            return loss, cls_loss, seg_loss, out[0], out[1]
        if self.task == "segmentation_kpconv":
            from .train_kpconv import masked_cross_entropy
            points, mask, features, labels = t
            pred = parallel._plain_module(self.model)(points, mask, features)
            return pred, masked_cross_entropy(pred, labels, mask)
        raise ValueError("task %r has no validation step" % (self.task,))

    def _val_runner(self, hip_graph=None):
        """What a validation pass calls per batch: `_val_step` itself (the launches of today), or — with `hip_graph`, by default
        `train.hip_graph_val` of the config — a graphs.GraphedForward over it (`_val_graph`, built on first use and kept between
        validations: a graph per batch shape, parameter addresses and modes; a refused capture is printed once on rank 0 and
        the step runs eagerly from then on — no rank agreement: an eval forward holds no collective).  The outputs of a replay
        are static: the callers consume them before the next batch."""
        use = bool(self.cfg["train"].get("hip_graph_val", False) if hip_graph is None else hip_graph)
        if not use or self.device.type != "cuda":
            return self._val_step
        if self._val_graph is None:
            from .graphs import GraphedForward
            # (the plain module names the parameters: a data-parallel wrapper keeps its own training flag through model.eval()
            #  of the module inside, which is what the KPConv vote passes switch)
            self._val_graph = GraphedForward(parallel._plain_module(self.model), fn=self._val_step, fallback=True, verbose=self.rank == 0)
        return self._val_graph

    def _tail_record(self, rec, tail):
        """`train.val_emd_tail`: the validation record also says how the auctions ended — the mean over the clouds of the first
        iteration without a bidder (`val_emd_iters` where there was none) and the clouds whose auction did not finish."""
        if bool(self.cfg["train"].get("val_emd_tail", False)):
            t = tail.tolist()
            if t[2] > 0:
                rec["emd_first_empty_mean"] = t[0] / t[2]
                rec["emd_unfinished"] = int(t[1])

    def _validate_completion(self, epoch, dataset=None, hip_graph=None):
        """train_inpainter.py:253-311: eval mode, no grad, the VAL subset in batches of `data.batch_size_val`; per batch
        sqrt(EMD(rec, gt, val_emd_eps, val_emd_iters)).mean(1).mean() and loss_chamfer, averaged over the batches and the
        ranks (sums and the count stay on the device until the one read at the end)."""
        import json
        from .data.completion import CompletionBatches
        cfg, tr = self.cfg, self.cfg["train"]
        if self.shapenet_device and (self.val_loader is None or dataset is not None):
            self.val_loader = self._completion_batches(dataset if dataset is not None else make_dataset(cfg, "completion", None, train=False),
                                                       train=False)
        elif self.val_loader is None or dataset is not None:
            data = dataset if dataset is not None else make_dataset(cfg, "completion", None, train=False)
            smp = torch.utils.data.distributed.DistributedSampler(data, shuffle=False) if parallel._active(self.dist) else None
            self.val_loader = CompletionBatches(data, cfg["data"].get("batch_size_val", cfg["data"]["batch_size"]), self.device,
                                                seed=int(cfg["data"].get("seed", 0)) + 7919, rank=self.rank, sampler=smp,
                                                num_workers=int(cfg["data"].get("num_workers", 0)), worker_init_fn=worker_init_fn)
        w = float(tr.get("chamfer_weight", 1.0))
        model = self.model
        was_training = model.training
        model.eval()
        self.val_loader.set_epoch(epoch if isinstance(epoch, int) else 0)
        step = self._val_runner(hip_graph)
        sums = torch.zeros(4, dtype=torch.float64, device=self.device)            # loss, loss_emd, loss_chamfer, batches
        tail = torch.zeros(3, dtype=torch.float64, device=self.device)            # `train.val_emd_tail`: see _val_emd
        with torch.no_grad():
            for noise, part, gt in self.val_loader:
                l_emd, l_cd, *stats = step(noise, part, gt)
                sums += torch.stack([l_emd + w * l_cd, l_emd, l_cd, torch.ones_like(l_cd)]).double()
                if stats:
                    tail += stats[0]
        model.train(was_training)
        if parallel._active(self.dist):
            self.dist.all_reduce(sums)
            self.dist.all_reduce(tail)
        s = sums.tolist()
        n = max(s[3], 1.0)
        rec = {"epoch": epoch, "iters": self.iters, "batches": int(s[3]), "loss": s[0] / n, "loss_emd": s[1] / n,
               "loss_chamfer": s[2] / n}
        self._tail_record(rec, tail)
        best = self.best_val is None or rec["loss"] < self.best_val
        rec["best"] = bool(best)
        if best:
            self.best_val = rec["loss"]
        if self.rank == 0:
            step = epoch if isinstance(epoch, int) else self.iters
            for k in ("loss", "loss_emd", "loss_chamfer"):
                self.writer.add_scalar("val/val_" + k, rec[k], global_step=step)
            if self.exp_dir is not None:
                with open(str(Path(self.exp_dir) / "completion_val.jsonl"), "a") as f:
                    f.write(json.dumps(rec) + "\n")
                if best:
                    parallel.save_exp_parallel([self.model, self.optimizer], ["generator", "g_opt"], exp_path=self.exp_dir,
                                               epoch=0, epoch_name="best")
        self.val_records.append(rec)
        return [rec]

    def _validate_reconstruction(self, epoch, dataset=None, hip_graph=None):
        """train_image_reconstruction.py:225-268: eval mode, no grad, the 'val' split in batches of `data.batch_size_val`; per
        batch sqrt(EMD(rec, gt, val_emd_eps, val_emd_iters)).mean(1).mean() and loss_chamfer_adj, averaged over the batches and
        the ranks (sums and the count stay on the device until the one read at the end); `best`: a new minimum of the EMD."""
        import json
        if self.val_loader is None or dataset is not None:
            data = dataset if dataset is not None else make_dataset(self.cfg, self.task, self.n_classes, train=False)
            self.val_loader = self._image_batches(data, train=False)
        model = self.model
        was_training = model.training
        model.eval()
        self.val_loader.set_epoch(epoch if isinstance(epoch, int) else 0)
        step = self._val_runner(hip_graph)
        sums = torch.zeros(3, dtype=torch.float64, device=self.device)            # loss_emd, loss_chamfer, batches
        tail = torch.zeros(3, dtype=torch.float64, device=self.device)            # `train.val_emd_tail`: see _val_emd
        with torch.no_grad():
            for img, pcd in self.val_loader:
                l_emd, l_cd, *stats = step(img, pcd, self._draw_noise(pcd))    # (the noise: one eager draw per batch, as ever)
                sums += torch.stack([l_emd, l_cd, torch.ones_like(l_cd)]).double()
                if stats:
                    tail += stats[0]
        model.train(was_training)
        if parallel._active(self.dist):
            self.dist.all_reduce(sums)
            self.dist.all_reduce(tail)
        s = sums.tolist()
        n = max(s[2], 1.0)
        rec = {"epoch": epoch, "iters": self.iters, "batches": int(s[2]), "loss_emd": s[0] / n, "loss_chamfer": s[1] / n}
        self._tail_record(rec, tail)
        best = self.best_val is None or rec["loss_emd"] < self.best_val
        rec["best"] = bool(best)
        if best:
            self.best_val = rec["loss_emd"]
        if self.rank == 0:
            step = epoch if isinstance(epoch, int) else self.iters
            for k in ("loss_emd", "loss_chamfer"):
                self.writer.add_scalar("val/val_" + k, rec[k], global_step=step)
            if self.exp_dir is not None:
                with open(str(Path(self.exp_dir) / "reconstruction_val.jsonl"), "a") as f:
                    f.write(json.dumps(rec) + "\n")
                if best:
                    parallel.save_exp_parallel([self.model, self.optimizer], ["generator", "g_opt"], exp_path=self.exp_dir,
                                               epoch=0, epoch_name="best")
        self.val_records.append(rec)
        return [rec]

    def _validate_scan(self, epoch, dataset=None, hip_graph=None):
        """train_classification.py:286-374: eval mode, no grad, `data.path_val` in batches of `data.batch_size_val`; the three
        losses averaged over the batches and the ranks, the accuracies from ClassificationMeter's counts all-reduced over the
        ranks (counts and sums stay on the device until the two reads at the end).  As in the reference the shards are padded
        to equal length, so with several ranks a few clouds count twice.  `best` / `macc_best`: a strictly higher cls_acc /
        m_acc than any validation before (the first one always is, unless m_acc is NaN: a class absent from the split)."""
        import json
        from .data.scanobjectnn import ClassificationMeter
        if self.val_loader is None or dataset is not None:
            data = dataset if dataset is not None else make_dataset(self.cfg, self.task, self.n_classes, train=False)
            self.val_loader = self._scan_batches(data, train=False)
        model = self.model
        was_training = model.training
        model.eval()
        self.val_loader.set_epoch(epoch if isinstance(epoch, int) else 0)
        meter = ClassificationMeter(self.n_classes)
        step = self._val_runner(hip_graph)
        sums = torch.zeros(4, dtype=torch.float64, device=self.device)            # loss, loss_cls, loss_seg, batches
        with torch.no_grad():
            for batch in self.val_loader:
                loss, cls_loss, seg_loss, logits, mask_logits = step(*batch)
                sums += torch.stack([loss, cls_loss, seg_loss, torch.ones_like(loss)]).double()
                meter.update(logits, mask_logits, batch[1], batch[2])
        model.train(was_training)
        if parallel._active(self.dist):
            self.dist.all_reduce(sums)
            meter.reduce(self.dist)
        s = sums.tolist()
        n = max(s[3], 1.0)
        rec = {"epoch": epoch, "iters": self.iters, "batches": int(s[3]), "loss": s[0] / n, "loss_cls": s[1] / n, "loss_seg": s[2] / n}
        rec.update(meter.result())
        rec["best"], rec["macc_best"] = bool(rec["cls_acc"] > self.best_acc), bool(rec["m_acc"] > self.best_macc)
        if rec["best"]:
            self.best_acc = rec["cls_acc"]
        if rec["macc_best"]:
            self.best_macc = rec["m_acc"]
        if self.rank == 0:
            step = epoch if isinstance(epoch, int) else self.iters
            for k in ("loss", "loss_cls", "loss_seg", "cls_acc", "seg_acc", "m_acc"):
                self.writer.add_scalar("val/" + k, rec[k], global_step=step)
            if self.exp_dir is not None:
                with open(str(Path(self.exp_dir) / "classification_val.jsonl"), "a") as f:
                    f.write(json.dumps(rec) + "\n")
                for flag in ("best", "macc_best"):
                    if rec[flag]:
                        parallel.save_exp_parallel([self.model, self.optimizer], ["generator", "g_opt"], exp_path=self.exp_dir,
                                                   epoch=0, epoch_name=flag)
        self.val_records.append(rec)
        return [rec]

    def _validate_blocks(self, epoch, dataset=None, hip_graph=None):
        """train_segmentation.py:244-288: eval mode, no grad, the blocks of `data.test_area` in batches of `data.batch_size_val`
        (shuffled points, no augmentation); the loss averaged over the batches and the ranks, the confusion matrix filled on the
        device (SegmentationMeter) and all-reduced over the ranks, `return_metrics_dict`'s numbers from it (sums and counts stay
        on the device until the two reads at the end).  As in the reference the shards are padded to equal length, so with
        several ranks a few blocks count twice."""
        import json
        from .data.s3dis_blocks import SegmentationMeter
        if self.val_loader is None or dataset is not None:
            data = dataset if dataset is not None else make_dataset(self.cfg, self.task, self.n_classes, train=False)
            self.val_loader = self._block_batches(data, train=False)
        model = self.model
        was_training = model.training
        model.eval()
        self.val_loader.set_epoch(epoch if isinstance(epoch, int) else 0)
        meter = SegmentationMeter(self.n_classes)
        step = self._val_runner(hip_graph)
        sums = torch.zeros(2, dtype=torch.float64, device=self.device)            # loss, batches
        with torch.no_grad():
            for pcd, labels in self.val_loader:
                pred, loss = step(pcd, labels)
                sums += torch.stack([loss, torch.ones_like(loss)]).double()
                meter.update(pred, labels)
        model.train(was_training)
        if parallel._active(self.dist):
            self.dist.all_reduce(sums)
            meter.reduce(self.dist)
        s = sums.tolist()
        rec = {"epoch": epoch, "iters": self.iters, "batches": int(s[1]), "loss": s[0] / max(s[1], 1.0)}
        rec.update(meter.result())
        if self.rank == 0:
            step = epoch if isinstance(epoch, int) else self.iters
            for k, v in rec.items():
                if k not in ("epoch", "iters", "batches"):
                    self.writer.add_scalar("val/" + k, v, global_step=step)
            if self.exp_dir is not None:
                with open(str(Path(self.exp_dir) / "segmentation_val.jsonl"), "a") as f:
                    f.write(json.dumps(rec) + "\n")
        self.val_records.append(rec)
        return [rec]

    def _report_train_confusion(self, epoch):
        """The epoch's train metrics (train_segmentation.py:236-237) from the confusion matrix the steps filled; it starts anew."""
        if self.train_meter.conf is None:
            return
        if parallel._active(self.dist):
            self.train_meter.reduce(self.dist)
        rec = dict(self.train_meter.result(), epoch=epoch, iters=self.iters)
        self.train_meter.reset()
        if self.rank == 0:
            for k, v in rec.items():
                if k not in ("epoch", "iters"):
                    self.writer.add_scalar("train/" + k, v, global_step=epoch)
        self.train_records.append(rec)

    def validate(self, num_votes=None, epoch=None, hip_graph=None):
        """segmentation_kpconv: one validation of `num_votes` vote passes (train_kpconv.KPConvData.validate) on the unwrapped
        model; the records go to the writer and, on rank 0, to <exp>/kpconv_val.jsonl.  Returns them.
        completion (`num_votes` is not used): one pass over the VAL subset (`_validate_completion`), its record appended to
        <exp>/completion_val.jsonl and, on a new minimum of the loss, `generator_best_0.t7` / `g_opt_best_0.t7` saved.
        classification_scanobjectnn (`num_votes` is not used): one pass over `data.path_val` (`_validate_scan`), its record
        (losses, cls_acc, seg_acc, m_acc, class_acc) appended to <exp>/classification_val.jsonl; `generator_best_0.t7` /
        `g_opt_best_0.t7` saved on a new best cls_acc, `generator_macc_best_0.t7` / `g_opt_macc_best_0.t7` on a new best m_acc.
        segmentation_blocks (`num_votes` is not used): one pass over the blocks of `data.test_area` (`_validate_blocks`), its record
        (loss, overall_acc, mean_class_acc, iou_<name>, mean_iou) appended to <exp>/segmentation_val.jsonl.
        reconstruction (`num_votes` is not used): one pass over the 'val' split (`_validate_reconstruction`), its record (loss_emd,
        loss_chamfer) appended to <exp>/reconstruction_val.jsonl; `generator_best_0.t7` / `g_opt_best_0.t7` on a new minimum.

        `hip_graph` (default: `train.hip_graph_val` of the config, else False; independent of `train.hip_graph`): the per-batch
        work — eval-mode forward plus the validation loss terms, `_val_step` — runs by replay of one HIP graph per batch shape
        (`_val_runner`, graphs.GraphedForward); the meters and tables stay eager on the graph's static outputs.  The graphs read
        the parameters where they live and are kept between validations: training steps in between need no new capture."""
        import json
        if self.task == "reconstruction":
            return self._validate_reconstruction(epoch, hip_graph=hip_graph)
        if self.task == "segmentation_blocks":
            return self._validate_blocks(epoch, hip_graph=hip_graph)
        if self.task == "completion":
            return self._validate_completion(epoch, hip_graph=hip_graph)
        if self.task == "classification_scanobjectnn":
            return self._validate_scan(epoch, hip_graph=hip_graph)
        records = self.kp.validate(parallel._plain_module(self.model), num_votes, epoch, step=self._val_runner(hip_graph))
        if self.rank == 0:
            for rec in records:
                step = self.iters
                for k in ("loss", "part_miou", "running_sub_miou", "sub_miou", "full_miou"):
                    self.writer.add_scalar("val/%s_v%d" % (k, rec["vote"]), rec[k], global_step=step)
            if self.exp_dir is not None:
                with open(str(Path(self.exp_dir) / "kpconv_val.jsonl"), "a") as f:
                    for rec in records:
                        f.write(json.dumps(rec) + "\n")
        self.val_records += records
        return records

    def _clip(self):
        if self.clip is not None:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.clip)

    # -- one training step -------------------------------------------------------------------------------------------
    def _eager_step(self, batch):
        loss = self._loss(batch)
        if self.blocks:
            self.train_meter.update(self._pred, batch[1])
        loss.backward()
        self._clip()
        self.optimizer.step()
        self.optimizer.zero_grad()
        return loss.detach()

    # DistributedDataParallel needs this many eager iterations before a capture (its reducer rebuilds the buckets after the
    # first one and settles its bookkeeping; torch notes/cuda.rst "Usage with DistributedDataParallel")
    DDP_WARMUP = 11

    def _capture(self, batch):
        """forward + loss + backward of one batch shape as ONE HIP graph on static input buffers (every libcloudct launch
        goes to torch's current stream, so the whole step captures — under DistributedDataParallel with its bucketed
        gradient all-reduce and the norms' statistics exchanges: RCCL collectives are captured like kernels); the optimizer
        step stays outside.  The blocks' eager launch rate is host-bound (~250 launches per block through Python / ctypes:
        the segmenter step 30.8 ms eager vs 24.8 ms graphed, profiles/r3_tools_output.txt).  Returns the record of the
        capture: (graph, static inputs, static loss, the gradient tensors the graph writes).  Reconstruction: the static inputs
        are (image, cloud, noise) — the noise is an input of the graph, and neither the warm-up nor the capture draws from
        `_noise_gen`; `last_chamfer` of the capture is a static output."""
        static = [t.to(self.device).clone() for t in batch]
        buffers = [b.clone() for b in self.model.buffers()]          # the warm-up passes must not count as training steps
        params = [p for p in self.model.parameters() if p.requires_grad]
        side = self._stream if self._stream is not None else torch.cuda.Stream()      # (DDP: the stream it was built on)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(self.DDP_WARMUP if parallel._active(self.dist) else 2):
                self.optimizer.zero_grad(set_to_none=True)
                self._loss(static).backward()
        torch.cuda.current_stream().wait_stream(side)
        with torch.no_grad():
            for b, saved in zip(self.model.buffers(), buffers):
                b.copy_(saved)
        self.optimizer.zero_grad(set_to_none=True)                   # the graph creates its own gradient tensors
        if parallel._active(self.dist):
            parallel.barrier(self.dist)
            parallel.quiesce()                                       # the process group's watchdog drops the warm-up's work items
        graph = torch.cuda.CUDAGraph()
        # (captured on the stream the warm-up ran on — under DDP the wrapper's, else `side`: the per-stream workspaces and
        #  tickets of the raster ops were created by the warm-up, outside the capture and outside the graph's private pool)
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            static_loss = self._loss(static)
            static_loss.backward()
        return graph, static, static_loss, [p.grad for p in params]

    def _graph_step(self, batch):
        """One step by graph replay.  A graph is captured per batch SHAPE (a ragged last batch, `data.drop_last: false`,
        gets its own); every graph owns the gradient tensors it writes, so the parameters' `.grad` are pointed at the
        replayed graph's before the optimizer steps — stepping with another graph's (stale) gradients, or dropping the
        captured tensors with zero_grad(), would silently stop the training."""
        key = tuple(tuple(t.shape) for t in batch)
        rec = self._graphs.get(key)
        if self.recon and rec is not False:
            # the step's noise: the same generator, the same call and the same one draw per step as the eager step's, drawn
            # here, outside the graph, and handed to it as a third static input (an eager fall-back step draws its own)
            batch = (batch[0], batch[1], self._draw_noise(batch[1]))
        if rec is None:
            rec, failure = None, None
            try:
                rec = self._capture(batch)
                if self.blocks:
                    self._graph_preds[key] = self._pred       # the graph's static prediction: read after every replay
                if self.recon:
                    self._graph_chamfers[key] = self.last_chamfer      # likewise the logged Chamfer term
            except RuntimeError as ex:
                # only what a refused CAPTURE raises (HIP's stream-capture errors, e.g. the process group's watchdog touching an
                # event of the capturing stream); a genuine error inside the model or the loss is not swallowed as "capture failed"
                if not _is_capture_error(ex):
                    raise
                failure = ex
                torch.cuda.synchronize(self.device)
            # every rank takes the SAME path: one replaying a graph beside others stepping eagerly would deadlock in the reducer
            if parallel._active(self.dist):
                ok = torch.tensor([0 if failure is not None else 1], device=self.device, dtype=torch.int32)
                self.dist.all_reduce(ok, op=self.dist.ReduceOp.MIN)
                if int(ok.item()) == 0 and failure is None:
                    failure, rec = RuntimeError("HIP-graph capture failed on another rank"), None
                if failure is not None:
                    # a capture that failed inside backward leaves DistributedDataParallel's reducer mid-iteration ("Expected to have
                    # finished reduction ..." on the next forward): there is no clean eager state to fall back to under DDP
                    raise RuntimeError("harness: HIP-graph capture failed under DistributedDataParallel (%s); rerun with "
                                       "train.hip_graph: false" % (failure,)) from failure
            if failure is not None:
                if self.rank == 0:
                    print("harness: HIP-graph capture failed (%s); continuing with eager steps" % (failure,), flush=True)
                rec = False
            self._graphs[key] = rec
        if rec is False:
            return self._eager_step(batch)            # (reconstruction: a noise drawn above rides along as batch[2])
        graph, static, static_loss, grads = rec
        for dst, src in zip(static, batch):
            dst.copy_(src, non_blocking=True)
        graph.replay()
        if self.blocks:
            self.train_meter.update(self._graph_preds[key], static[1])
        if self.recon:
            self.last_chamfer = self._graph_chamfers[key]             # static: _fit appends a clone
        for p, g in zip((p for p in self.model.parameters() if p.requires_grad), grads):
            p.grad = g
        self._clip()
        self.optimizer.step()
        return static_loss.detach().clone()

    def fit(self, max_iters=None, hip_graph=None, log_each=None):
        """Runs `train.num_epochs` epochs (or `max_iters` steps); returns the rank-0 loss history.

        `hip_graph` (default: `train.hip_graph` of the config, else False): replay forward + loss + backward as one HIP graph
        (under DistributedDataParallel too: the gradient all-reduce and the norms' statistics exchanges are captured with
        the kernels, after DDP's warm-up iterations; the process group must have been created with
        TORCH_NCCL_ASYNC_ERROR_HANDLING=0 in the environment — launch.rank_env(capture=True) / spawn_ranks(capture=True) set it,
        torchrun users set it themselves; the price is that a hung collective then hangs the job instead of aborting it.  A capture that
        fails falls back to eager steps on one device and RAISES under DistributedDataParallel — the ranks agree on it first).  Losses stay on the
        device and are read back every `log_each` steps (default `train.log_each`, else 10) in ONE transfer — no host
        synchronisation per step (the reference reads the loss every step: train_segmentation.py:180-186).  The reconstruction
        task's sphere noise is an INPUT of its graph: one eager draw per step from `_noise_gen`, before the replay, in step order,
        so a graphed and an eager run of one seed see the same noise at step k; the logged Chamfer term is a static output.

        `train.deterministic: true` runs the whole fit in deterministic mode (determinism.py: run-to-run equal gradients from
        the library's kernels, all five tasks); the seeds are set as without it and nothing else changes.

        `train.matmul_precision: high` (or `medium` / `highest`) runs the whole fit, the validation inside it included, with
        the pointwise-convolution GEMMs in that mode (precision.py: one f16 MFMA term per operand, TF32-class); the previous
        mode comes back when fit returns.  With `hip_graph` the captured kernels are those of this mode.
        `train.conv_precision` does the same for the grouped 3^d convolutions (precision.py `conv_precision`), independently;
        a value that is not a mode's name raises ValueError here, before any device work."""
        import contextlib
        conv_mode = self.cfg["train"].get("conv_precision")
        if conv_mode is not None and conv_mode not in ("highest", "high", "medium"):
            raise ValueError("train.conv_precision expects 'highest', 'high' or 'medium', got %r" % (conv_mode,))
        with contextlib.ExitStack() as scopes:
            if self.cfg["train"].get("deterministic", False):
                from . import determinism
                scopes.enter_context(determinism.deterministic(True))
            if self.cfg["train"].get("matmul_precision") is not None:
                from . import precision
                scopes.enter_context(precision.matmul_precision(self.cfg["train"]["matmul_precision"]))
            if self.cfg["train"].get("conv_precision") is not None:
                from . import precision
                scopes.enter_context(precision.conv_precision(self.cfg["train"]["conv_precision"]))
            return self._fit(max_iters, hip_graph, log_each)

    def _fit(self, max_iters, hip_graph, log_each):
        tr = self.cfg["train"]
        use_graph = bool(tr.get("hip_graph", False) if hip_graph is None else hip_graph)
        log_each = int(tr.get("log_each", 10) if log_each is None else log_each)
        self._graphs, self._graph_preds, self._graph_chamfers = {}, {}, {}
        history, pending, pending_chamfer = [], [], []

        def flush():
            if self.device.type == "cuda":
                from . import ops
                ops.mhct_core_check()        # (the one place the loop waits for the device anyway: a cluster timeout raises here)
            if pending and self.rank == 0:
                stamps, vals = zip(*pending)
                for it, v in zip(stamps, torch.stack(vals).tolist()):      # one device-to-host copy for the interval
                    history.append(v)
                    self.writer.add_scalar("train/loss", v, global_step=it)
            pending.clear()
            if pending_chamfer and self.rank == 0:
                stamps, vals = zip(*pending_chamfer)
                for it, v in zip(stamps, torch.stack(vals).tolist()):
                    self.writer.add_scalar("train/loss_chamfer", v, global_step=it)
            pending_chamfer.clear()

        for epoch in range(tr["num_epochs"]):
            if self.sampler is not None:
                self.sampler.set_epoch(epoch)
            if self.scan or self.blocks or self.recon or self.shapenet_device:
                self.loader.set_epoch(epoch)
            self.model.train()
            end = time.time()
            for batch in self.loader:
                if self._stream is not None:            # under DDP every step runs on the wrapper's stream (see __init__)
                    self._stream.wait_stream(torch.cuda.current_stream(self.device))
                    with torch.cuda.stream(self._stream):
                        loss = self._graph_step(batch) if use_graph else self._eager_step(batch)
                    torch.cuda.current_stream(self.device).wait_stream(self._stream)
                else:
                    loss = self._graph_step(batch) if use_graph else self._eager_step(batch)
                if self.scheduler is not None:
                    self.scheduler.step()
                reduced = parallel.reduce_loss_dict(self.dist, {"loss": loss})
                pending.append((self.iters, reduced["loss"].detach().reshape(())))
                if self.recon and self.last_chamfer is not None:
                    chamfer = parallel.reduce_loss_dict(self.dist, {"loss_chamfer": self.last_chamfer})["loss_chamfer"]
                    chamfer = chamfer.detach().reshape(())
                    # (under hip_graph `last_chamfer` is a static output that the next replay overwrites: a clone is kept)
                    pending_chamfer.append((self.iters, chamfer.clone() if use_graph else chamfer))
                self.iters += 1
                if self.iters % log_each == 0:
                    flush()
                    if self.rank == 0:
                        self.writer.add_scalar("train/batch_time", (time.time() - end) / log_each, global_step=self.iters)
                    end = time.time()
                if self.kp is None and self.iters % tr.get("save_each", 1 << 62) == 0:
                    self.save()
                if max_iters is not None and self.iters >= max_iters:
                    flush()
                    return history
            if self.kp is not None:
                # train_segmentation_kpconv.py:240-266: 2-vote validation every val_step epochs, checkpoints per epoch
                flush()
                e = epoch + 1
                if self.rank == 0:
                    self.writer.add_scalar("learning_rate", self.optimizer.param_groups[0]["lr"], global_step=e)
                if e % int(tr["val_step"]) == 0:
                    self.validate(int(tr["val_votes"]), e)
                if e % int(tr["save_each_epoch"]) == 0:
                    self.save(epoch=e)
            if self.shapenet:
                flush()
                self.validate(epoch=epoch)                # train_inpainter.py:253-311: once per epoch
            if self.blocks:
                # train_segmentation.py:236-244: the train metrics, then checkpoints and validation by the 0-based epoch
                flush()
                self._report_train_confusion(epoch)
                if epoch > 0 and epoch % int(tr["save_each_epoch"]) == 0:
                    self.save(epoch=epoch)
                if epoch % int(tr["val_step"]) == 0:
                    self.validate(epoch=epoch)
            if self.recon:
                # train_image_reconstruction.py:225-268: a validation every epoch, checkpoints by the 0-based epoch
                flush()
                self.validate(epoch=epoch)
                if epoch % int(tr["save_each_epoch"]) == 0:
                    self.save(epoch=epoch)
            if self.scan:
                # train_classification.py:281-286: checkpoints and validation by the 0-based epoch
                flush()
                if epoch > 0 and epoch % int(tr["save_each_epoch"]) == 0:
                    self.save(epoch=epoch)
                if epoch % int(tr["val_step"]) == 0:
                    self.validate(epoch=epoch)
        flush()
        if self.kp is not None:
            self.validate(int(tr["final_votes"]), "Last")
        return history


def _is_capture_error(ex):
    """Is this RuntimeError HIP refusing or invalidating a stream capture (as opposed to an error of the captured code)?"""
    from .graphs import is_capture_error
    return is_capture_error(ex)


def load_config(path):
    import yaml
    with open(path, "r") as f:
        cfg = yaml.load(f, Loader=yaml.FullLoader)
    cfg["config_path"] = str(path)
    return cfg
