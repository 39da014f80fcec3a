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
import json
import os
import sys

import torch


def classification_config(cfg):
    """A copy of `cfg` with the protocol's defaults (protocols.Scan `DATA` / `TRAIN`) under the keys it lacks;
    `data.batch_size_val` defaults to `data.batch_size`."""
    from .protocols import Scan
    return Scan.config(cfg)


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

    def run(dist):
        cfg = classification_config(harness.load_config(args.config))
        task, n_classes = "classification_scanobjectnn", int(cfg["data"]["n_classes"])
        if args.eval:
            if "generator" not in cfg.get("restore", {}):
                raise SystemExit("--eval needs restore.generator in the config")
            from .data.scanobjectnn import DeviceScanObjectNN
            device = torch.device("cuda", torch.cuda.current_device())
            val = DeviceScanObjectNN(harness.make_dataset(cfg, task, n_classes, train=False), device)      # (the training file is not read)
            tr = harness.Trainer(cfg, task, n_classes, device=device, dist=dist, exp_name=args.exp_name, dataset=val)
            rec = tr.validate(epoch="eval", dataset=val)[0]
            if tr.rank == 0:
                print(json.dumps(rec))
            return rec
        tr = harness.Trainer(cfg, task, n_classes, dist=dist, exp_name=args.exp_name)
        tr.fit()
        return tr.val_records

    return launch.run_entry(__file__, argv, args.gpus, args.config, run, spawn=not args.eval)


if __name__ == "__main__":
    if __package__ in (None, ""):            # started as a file by launch.spawn_ranks
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from cloud_transformers_amd.train_classification import main as _main
        _main()
    else:
        main()
