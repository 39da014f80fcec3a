"""Training and evaluation of the ScanObjectNN classification protocol (train_classification.py) on the device: the
`classification_scanobjectnn` task of `harness.Trainer` on `data.kind: scanobjectnn_device`.

    python -m cloud_transformers_amd.train_classification EXP -c configs/scanobjectnn.yaml [--gpus N] [--eval]

The config is the reference's YAML as it is (`data.path`, `data.path_val`, `data.batch_size`, `data.batch_size_val`,
`data.center`, `data.normalize`, optional `data.subsample`; `train.seg_weight`, `train.val_step`, `train.save_each_epoch`);
`data.kind` is filled in.  The values the reference hard-codes are defaults here: `data.n_classes` 15, `data.jitter_sigma`
0.01, `data.jitter_clip` 0.05, `train.seg_weight` 0.5, `data.seed` 0; `data.subsample` absent means all points.  The files
are HDF5 (or their .npz twins: data/datasets.py).

- training: the split lives on the device and every batch is one gather launch (data/scanobjectnn.py ScanBatches), loss
  (1 - seg_weight) * CE + seg_weight * BCE, the scheduler stepped per iteration, a validation every `train.val_step` epochs
  (`Trainer.validate`: <exp>/classification_val.jsonl, `generator_best_0.t7` on a new best cls_acc,
  `generator_macc_best_0.t7` on a new best m_acc), `generator_epoch_{e}.t7` every `train.save_each_epoch` epochs.
- `--eval`: restore `restore.generator`, then one validation over `data.path_val` (`train.hip_graph_val: true`: its per-batch
  work by HIP-graph replay, as in the validations of a training run); its record is printed and returned.
- `--gpus N > 1`: N ranks through `launch.spawn_ranks`, one process group over RCCL (training only)."""
import argparse
import copy
import json
import os
import sys

import torch

CLASSIFICATION_DATA = {"kind": "scanobjectnn_device", "n_classes": 15, "jitter_sigma": 0.01, "jitter_clip": 0.05, "seed": 0,
                       "center": True, "normalize": True}
CLASSIFICATION_TRAIN = {"seg_weight": 0.5, "val_step": 1, "save_each_epoch": 10}


def classification_config(cfg):
    """A copy of `cfg` with the protocol's defaults (train_classification.py:146,176,281-286; datasets/scanobjectnn.py:30)
    under the keys it lacks; `data.batch_size_val` defaults to `data.batch_size`."""
    cfg = copy.deepcopy(cfg)
    for key, defaults in (("data", CLASSIFICATION_DATA), ("train", CLASSIFICATION_TRAIN)):
        sect = cfg.setdefault(key, {})
        for k, v in defaults.items():
            sect.setdefault(k, v)
    cfg["data"].setdefault("batch_size_val", cfg["data"].get("batch_size", 1))
    return cfg


def _parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("exp_name")
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--eval", action="store_true", help="restore restore.generator, then one validation over data.path_val")
    return ap.parse_args(argv)


def main(argv=None):
    """Train one experiment (returns the validation records of this rank) or, with --eval, validate it once (returns the record)."""
    from . import harness, launch
    argv = list(sys.argv[1:] if argv is None else argv)
    args = _parse(argv)
    if args.gpus > 1 and not args.eval and not launch.under_launcher():
        rest = [a for i, a in enumerate(argv) if a != "--gpus" and (i == 0 or argv[i - 1] != "--gpus") and not a.startswith("--gpus=")]
        cfg = harness.load_config(args.config)
        rc = launch.spawn_ranks(os.path.abspath(__file__), rest, args.gpus, capture=bool(cfg.get("train", {}).get("hip_graph", False)))
        if rc != 0:
            raise SystemExit(rc)
        return []
    dist = None
    if launch.under_launcher():
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]),
                                device_id=torch.device("cuda", local))
    try:
        cfg = classification_config(harness.load_config(args.config))
        task, n_classes = "classification_scanobjectnn", int(cfg["data"]["n_classes"])
        if args.eval:
            if "generator" not in cfg.get("restore", {}):
                raise SystemExit("--eval needs restore.generator in the config")
            from .data.scanobjectnn import DeviceScanObjectNN
            device = torch.device("cuda", torch.cuda.current_device())
            val = DeviceScanObjectNN(harness.make_dataset(cfg, task, n_classes, train=False), device)      # (the training file is not read)
            tr = harness.Trainer(cfg, task, n_classes, device=device, dist=dist, exp_name=args.exp_name, dataset=val)
            rec = tr._validate_scan("eval", dataset=val)[0]
            if tr.rank == 0:
                print(json.dumps(rec))
            return rec
        tr = harness.Trainer(cfg, task, n_classes, dist=dist, exp_name=args.exp_name)
        tr.fit()
        return tr.val_records
    finally:
        if dist is not None:
            dist.destroy_process_group()


if __name__ == "__main__":
    if __package__ in (None, ""):            # started as a file by launch.spawn_ranks
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from cloud_transformers_amd.train_classification import main as _main
        _main()
    else:
        main()
