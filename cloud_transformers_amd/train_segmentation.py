"""Training and evaluation of the S3DIS 1x1 m block protocol (train_segmentation.py, configs/s3dis.yaml) on the device: the
`segmentation_blocks` task of `harness.Trainer` on `data.kind: s3dis_device`.

    python -m cloud_transformers_amd.train_segmentation EXP -c configs/s3dis.yaml [--gpus N] [--eval]

The config is the reference's YAML as it is (`data.path`, `data.batch_size`, `data.batch_size_val`, `data.num_points`,
`data.test_area`, `data.data_percent`, `data.aug`; `train.save_each`, `train.save_each_epoch`, `train.val_step`); `data.kind`
is filled in.  The values the reference hard-codes are defaults here: `data.n_classes` 13, `data.seed` 0, `data.jitter_sigma`
0.01, `data.jitter_clip` 0.05, `data.color_jitter_std` 0.05, `data.color_shift_ratio` 0.1, `data.hue_max` 0.5,
`data.saturation_max` 0.2.  The files are HDF5 (or their .npz twins: data/datasets.py).

- training: the blocks live on the device and every batch — shuffle and the eight augmentations included — is one launch
  (data/s3dis_blocks.py BlockBatches), loss CE(pred[:, :, 0], labels), the scheduler stepped per iteration, the train
  confusion matrix filled on the device every step and reported per epoch, a validation every `train.val_step` epochs
  (`Trainer.validate`: <exp>/segmentation_val.jsonl), `generator_iter_{n}.t7` every `train.save_each` iterations,
  `generator_epoch_{e}.t7` every `train.save_each_epoch` epochs.
- `--eval`: restore `restore.generator`, then one validation over the blocks of `data.test_area` (`train.hip_graph_val: true`:
  its per-batch work by HIP-graph replay, as in the validations of a training run); its record is printed and
  returned.
- `--gpus N > 1`: N ranks through `launch.spawn_ranks`, one process group over RCCL (training only)."""
import argparse
import json
import os
import sys

import torch


def segmentation_config(cfg):
    """A copy of `cfg` with the protocol's defaults (protocols.Blocks `DATA` / `TRAIN`) under the keys it lacks;
    `data.batch_size_val` defaults to `data.batch_size`."""
    from .protocols import Blocks
    return Blocks.config(cfg)


def _parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("exp_name")
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--eval", action="store_true", help="restore restore.generator, then one validation over data.test_area")
    return ap.parse_args(argv)


def main(argv=None):
    """Train one experiment (returns the validation records of this rank) or, with --eval, validate it once (returns the record)."""
    from . import harness, launch
    argv = list(sys.argv[1:] if argv is None else argv)
    args = _parse(argv)

    def run(dist):
        cfg = segmentation_config(harness.load_config(args.config))
        task, n_classes = "segmentation_blocks", int(cfg["data"]["n_classes"])
        if args.eval:
            if "generator" not in cfg.get("restore", {}):
                raise SystemExit("--eval needs restore.generator in the config")
            from .data.s3dis_blocks import DeviceS3DISBlocks
            device = torch.device("cuda", torch.cuda.current_device())
            val = DeviceS3DISBlocks(harness.make_dataset(cfg, task, n_classes, train=False), device)      # (only the test Area is uploaded)
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
        from cloud_transformers_amd.train_segmentation import main as _main
        _main()
    else:
        main()
