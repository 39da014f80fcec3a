"""YAML-driven training harness around the hot path: the reference's experiment plumbing
(utils/train_util.py:19-134) and the skeleton of its training scripts (train_segmentation.py:64-230,
train_classification.py) with synthetic loaders, so that a reference config + model file runs end to end on this
package's layers and checkpoints stay interchangeable.  This module is the generic loop; what a task adds to it — its
defaults, dataset, batches, loss, validation and end of epoch — is its class in protocols.py.

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
  indoor3d_sem_seg_hdf5_data directory), items equal to the reference loaders' under the same seeds.  The kinds `s3dis_kpconv`,
  `scanobjectnn_device`, `s3dis_device` and `what3d_device` select their task, `shapenet_completion` and
  `shapenet_completion_device` belong to the `completion` task (protocols.py `PROTOCOLS`, each class's docstring).
"""
import copy
import datetime
import shutil
import time
from collections import OrderedDict
from pathlib import Path

import torch
from torch import nn

from . import parallel, protocols


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
    `data.eval_points` points), its items left to the device.  Every kind but "synthetic" is the `dataset` of one protocol."""
    kind = str(cfg["data"].get("kind", "synthetic")).lower()
    if kind == "synthetic":
        return SyntheticClouds(task, cfg["data"]["num_points"], n_classes, length=length, channels=channels)
    protocol = protocols.DATASETS.get(kind)
    if protocol is None:
        raise ValueError("data.kind must be synthetic, scanobjectnn, scanobjectnn_device, s3dis, s3dis_device, s3dis_kpconv, shapenet_completion, "
                         "shapenet_completion_device or what3d_device (got %r)" % kind)
    assert task == protocol.name, protocol.mismatch or "data.kind %s is the %s task" % (kind, protocol.name)
    return protocol.dataset(cfg, train)


class Trainer:
    """The reference scripts' loop: model file + YAML config -> DDP(+SyncBN) model, optimizer, scheduler, steps with
    loss reduction to rank 0, `.t7` checkpoints every `train.save_each` iterations.

    `task`: "segmentation", "classification", "completion", "segmentation_kpconv", "classification_scanobjectnn",
    "segmentation_blocks" or "reconstruction"; a `data.kind` that selects a task overrides it.  The trainer holds one instance of
    the task's class of protocols.py (`protocol`): loss, batches, validation rules, end of epoch and the state only that task has
    are there.  Here are the model, the optimizer and scheduler, the loaders (`loader`, `val_loader`, `sampler`), the step (eager
    or by graph replay, `_graphs`), the validation pass (`_validate`, `_val_graph`, `val_records`), `iters`, the writer and the
    experiment directory."""

    def __init__(self, cfg, task, n_classes, device=None, dist=None, exp_name="exp", dataset_length=64, make_dirs=True,
                 channels=3, dataset=None):
        protocol = protocols.pick(task, str(cfg["data"].get("kind", "")).lower())
        self.cfg = cfg = protocol.config(cfg)
        self.task, self.dist, self.n_classes = protocol.name, dist, n_classes
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
        data = dataset if dataset is not None else make_dataset(cfg, self.task, n_classes, length=dataset_length, channels=channels)
        self.kp, self.clip, self.sampler, self.val_loader, self.val_records = None, None, None, None, []
        self._graphs, self._val_graph, self.iters = {}, None, 0
        self.protocol = protocol(self)
        self.loader = self.protocol.loader(self, data, train=True)

    def _loss(self, batch):
        return self.protocol.loss(self, batch)

    def save(self, epoch=None):
        """`generator_iter_{iters}.t7` / `g_opt_iter_{iters}.t7`; with `epoch`, `generator_epoch_{epoch}.t7` / `g_opt_epoch_{epoch}.t7`."""
        if self.rank == 0 and self.exp_dir is not None:
            parallel.save_exp_parallel([self.model, self.optimizer], ["generator", "g_opt"], exp_path=self.exp_dir,
                                       epoch=self.iters if epoch is None else epoch, epoch_name="iter" if epoch is None else "epoch")

    # -- validation: the per-batch work as one function of device tensors, run eagerly or by graph replay ------------------
    def _val_step(self, *t):
        """One validation batch of the task (the protocol's `val_step`): the eval-mode forward plus the task's validation loss
        terms, device tensors in, device tensors out (the caller holds eval mode and no_grad; the meters stay with the caller)."""
        return self.protocol.val_step(self, *t)

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

    def _validate(self, epoch=None, hip_graph=None, dataset=None):
        """One validation pass as the protocol describes it: eval mode, no grad, the validation set (`dataset`, else
        `make_dataset(train=False)`; the loader is kept) in this rank's batches; the protocol's terms are summed per batch on the
        device in float64 with the batch count, all-reduced and read once; its meter, reduced after them, adds its keys; the
        record gets the protocol's best flags, goes to the writer (at `epoch` when it is an int, else at `iters`), to
        <exp>/<val_file> and to `val_records`; every true flag saves `generator_<flag>_0.t7` / `g_opt_<flag>_0.t7`."""
        import json
        p = self.protocol
        if self.val_loader is None or dataset is not None:
            data = dataset if dataset is not None else make_dataset(self.cfg, self.task, self.n_classes, train=False)
            self.val_loader = p.loader(self, data, train=False)
        model = self.model
        was_training = model.training
        model.eval()
        self.val_loader.set_epoch(epoch if isinstance(epoch, int) else 0)
        step = self._val_runner(hip_graph)
        sums = torch.zeros(len(p.val_terms) + 1, dtype=torch.float64, device=self.device)            # the terms, batches
        meter = p.val_meter(self)
        with torch.no_grad():
            for batch in self.val_loader:
                terms = p.val_batch(self, step, batch, meter)
                sums += torch.stack([*terms, torch.ones_like(terms[0])]).double()
        model.train(was_training)
        if parallel._active(self.dist):
            self.dist.all_reduce(sums)
            if meter is not None:
                meter.reduce(self.dist)
        s = sums.tolist()
        n = max(s[-1], 1.0)
        rec = {"epoch": epoch, "iters": self.iters, "batches": int(s[-1])}
        rec.update((k, v / n) for k, v in zip(p.val_terms, s))
        if meter is not None:
            rec.update(meter.result())
        flags = p.best(rec)
        rec.update(flags)
        if self.rank == 0:
            at = epoch if isinstance(epoch, int) else self.iters
            for tag, v in p.val_scalars(rec).items():
                self.writer.add_scalar(tag, v, global_step=at)
            if self.exp_dir is not None:
                with open(str(Path(self.exp_dir) / p.val_file), "a") as f:
                    f.write(json.dumps(rec) + "\n")
                for flag, on in flags.items():
                    if on:
                        parallel.save_exp_parallel([self.model, self.optimizer], ["generator", "g_opt"], exp_path=self.exp_dir,
                                                   epoch=0, epoch_name=flag)
        self.val_records.append(rec)
        return [rec]

    def validate(self, num_votes=None, epoch=None, hip_graph=None, dataset=None):
        """One validation of the task (the protocol's `validate`: `_validate`, or the KPConv vote passes, which alone use
        `num_votes`); returns its records.  `dataset`: validate on this set instead of the config's (the loader is rebuilt).

        `hip_graph` (default: `train.hip_graph_val` of the config, else False; independent of `train.hip_graph`): the per-batch
        work — eval-mode forward plus the validation loss terms, `_val_step` — runs by replay of one HIP graph per batch shape
        (`_val_runner`, graphs.GraphedForward); the meters and tables stay eager on the graph's static outputs.  The graphs read
        the parameters where they live and are kept between validations: training steps in between need no new capture."""
        return self.protocol.validate(self, num_votes, epoch, hip_graph, dataset)

    def _clip(self):
        if self.clip is not None:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.clip)

    # -- one training step -------------------------------------------------------------------------------------------
    def _eager_step(self, batch):
        loss = self._loss(batch)
        self.protocol.after_step(self.protocol.out, batch)
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
        capture: (graph, static inputs, static loss, the gradient tensors the graph writes, the protocol's `out` of the captured
        step: static too).  The static inputs are the protocol's `graph_inputs`; the warm-up and the capture take them as given."""
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
        return graph, static, static_loss, [p.grad for p in params], self.protocol.out

    def _graph_step(self, batch):
        """One step by graph replay.  A graph is captured per batch SHAPE (a ragged last batch, `data.drop_last: false`,
        gets its own); every graph owns the gradient tensors it writes, so the parameters' `.grad` are pointed at the
        replayed graph's before the optimizer steps — stepping with another graph's (stale) gradients, or dropping the
        captured tensors with zero_grad(), would silently stop the training."""
        key = tuple(tuple(t.shape) for t in batch)
        rec = self._graphs.get(key)
        if rec is not False:
            batch = self.protocol.graph_inputs(self, batch)      # (drawn out here, outside the graph; an eager fall-back step makes its own)
        if rec is None:
            rec, failure = None, None
            try:
                rec = self._capture(batch)
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
            return self._eager_step(batch)            # (graph inputs made above ride along in the batch)
        graph, static, static_loss, grads, out = rec
        for dst, src in zip(static, batch):
            dst.copy_(src, non_blocking=True)
        graph.replay()
        self.protocol.after_step(out, static)         # (`out` is static: the next replay overwrites it)
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
        synchronisation per step (the reference reads the loss every step: train_segmentation.py:180-186); so are the protocol's
        `logged` scalars (the reconstruction's Chamfer term; its noise under `hip_graph`: protocols.Reconstruction).

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

    def _flush(self):
        """The pending losses (and logged scalars) of this rank to the history and the writer: one transfer each."""
        if self.device.type == "cuda":
            from . import ops
            ops.mhct_core_check()        # (the one place the loop waits for the device anyway: a cluster timeout raises here)
        for pending in (self._pending, self._pending_logged):
            if pending and self.rank == 0:
                tags, stamps, vals = zip(*pending)
                for tag, it, v in zip(tags, stamps, torch.stack(vals).tolist()):      # one device-to-host copy for the interval
                    if tag == "train/loss":
                        self._history.append(v)
                    self.writer.add_scalar(tag, v, global_step=it)
            pending.clear()

    def _fit(self, max_iters, hip_graph, log_each):
        tr, p = self.cfg["train"], self.protocol
        use_graph = bool(tr.get("hip_graph", False) if hip_graph is None else hip_graph)
        log_each = int(tr.get("log_each", 10) if log_each is None else log_each)
        self._graphs = {}
        self._history, self._pending, self._pending_logged = [], [], []
        history = self._history
        for epoch in range(tr["num_epochs"]):
            if self.sampler is not None:
                self.sampler.set_epoch(epoch)
            if p.loader_epochs:
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
                self._pending.append(("train/loss", self.iters, reduced["loss"].detach().reshape(())))
                if p.logged is not None:
                    for k, v in parallel.reduce_loss_dict(self.dist, p.logged).items():
                        v = v.detach().reshape(())
                        # (under hip_graph a logged scalar is a static output that the next replay overwrites: a clone is kept)
                        self._pending_logged.append(("train/" + k, self.iters, v.clone() if use_graph else v))
                self.iters += 1
                if self.iters % log_each == 0:
                    self._flush()
                    if self.rank == 0:
                        self.writer.add_scalar("train/batch_time", (time.time() - end) / log_each, global_step=self.iters)
                    end = time.time()
                if p.save_by_iter and self.iters % tr.get("save_each", 1 << 62) == 0:
                    self.save()
                if max_iters is not None and self.iters >= max_iters:
                    self._flush()
                    return history
            p.after_epoch(self, epoch)
        self._flush()
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
