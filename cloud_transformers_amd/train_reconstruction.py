"""Training and evaluation of the What3D single-view reconstruction protocol (train_image_reconstruction.py,
eval_reconstruction_f1.py) on the device: the `reconstruction` task of `harness.Trainer` on `data.kind: what3d_device`.

    python -m cloud_transformers_amd.train_reconstruction EXP -c configs/reconstruction.yaml [--gpus N] [--eval]

The config is the reference's YAML as it is (`data.path`, `data.batch_size`, `data.batch_size_val`, `data.im_size`,
`data.gt_size`; `train.save_each`, `train.save_each_epoch`); `data.kind` is filled in.  The values the reference hard-codes are
defaults here: `train.emd_eps` 0.005 and `train.emd_iters` 50 for the training loss, `train.val_emd_eps` 0.004 and
`train.val_emd_iters` 3000 for validation, `data.seed` 42, and for `--eval` `data.eval_points` 10000, `data.eval_noise` 8192
and `train.f1_threshold` 0.01.  `data.cache_dir` (optional) keeps the decoded renderings and clouds between runs.
`train.hip_graph: true` replays the training step and `train.hip_graph_val: true` the validation step and the `--eval`
forwards as HIP graphs; the sphere noise is drawn eagerly before every replay and copied into the graph's input.

- training: the split lives on the device and every batch is one launch (data/image_point.py ImageBatches); noise on the unit
  sphere, loss = mean sqrt(EMD(rec, gt)), loss_chamfer_adj logged; the scheduler stepped per iteration;
  `generator_iter_{n}.t7` every `train.save_each` iterations; a validation every epoch (`Trainer.validate`:
  <exp>/reconstruction_val.jsonl, `generator_best_0.t7` on a new minimum), `generator_epoch_{e}.t7` every
  `train.save_each_epoch` epochs.
- `--eval` (eval_reconstruction_f1.py:94-126): restore `restore.generator`, then the test split with `data.eval_points`
  ground-truth points in batches of `data.batch_size`: two reconstructions from two draws of `data.eval_noise` sphere points,
  `metrics.get_f1_scores_merge` at `train.f1_threshold`; the mean F1, precision and recall per category and overall are
  printed and written to <exp>/reconstruction_test.json (the reference's per-batch pickles are not written).
- `--gpus N > 1`: N ranks through `launch.spawn_ranks`, one process group over RCCL (training only)."""
import argparse
import json
import os
import sys

import torch


def reconstruction_config(cfg):
    """A copy of `cfg` with the protocol's defaults (protocols.Reconstruction `DATA` / `TRAIN`) under the keys it lacks;
    `data.batch_size_val` defaults to `data.batch_size`."""
    from .protocols import Reconstruction
    return Reconstruction.config(cfg)


def evaluate(model, batches, cfg, exp_dir=None, generator=None, verbose=True):
    """eval_reconstruction_f1.py:94-126 over `batches` (an ImageBatches of the test split) -> {"names": ["f1", "precision",
    "recall"], "categories": {name: {"count", "avg"}}, "overall": {"count", "avg"}}; printed and, with `exp_dir`, written to
    <exp_dir>/reconstruction_test.json."""
    from .graphs import eval_forward
    from .metrics import get_f1_scores_merge, sphere_noise
    ds = batches.ds
    n_noise, th = int(cfg["data"]["eval_noise"]), float(cfg["train"]["f1_threshold"])
    scores = {}
    was_training = model.training
    model.eval()
    # `train.hip_graph_val`: the forward by graph replay; both noise draws of a batch are eager inputs of the same graph, so the
    # first reconstruction must outlive the second replay (clone_outputs)
    forward = eval_forward(model, cfg, clone_outputs=True, verbose=verbose)
    with torch.no_grad():
        for img, pcd_gt in batches:
            recs = []
            for _ in range(2):
                noise = sphere_noise(img.shape[0], n_noise, img.device, generator=generator)
                out = forward(noise, img)
                recs.append((out[0] if isinstance(out, (tuple, list)) else out)[:, :, 0])
            f1, pr, rc = get_f1_scores_merge(pcd=recs[0], pcd_2=recs[1], pcd_gt=pcd_gt, th=th, generator=generator)
            for c, row in zip(batches.last_classes.tolist(), zip(f1, pr, rc)):
                scores.setdefault(ds.class_names[c], []).append(row)
    model.train(was_training)

    def mean(rows):
        return [float(sum(r[k] for r in rows) / len(rows)) for k in range(3)]

    every = [r for rows in scores.values() for r in rows]
    res = {"names": ["f1", "precision", "recall"],
           "categories": {name: {"count": len(rows), "avg": mean(rows)} for name, rows in sorted(scores.items())},
           "overall": {"count": len(every), "avg": mean(every) if every else [float("nan")] * 3}}
    if verbose:
        print("\t".join(["Category", "#Sample"] + res["names"]))
        for name, row in res["categories"].items():
            print("\t".join([name, str(row["count"])] + ["%.4f" % v for v in row["avg"]]))
        print("\t".join(["Overall", str(res["overall"]["count"])] + ["%.4f" % v for v in res["overall"]["avg"]]))
    if exp_dir is not None:
        with open(os.path.join(str(exp_dir), "reconstruction_test.json"), "w") as f:
            json.dump(res, f, indent=1)
    return res


def _parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("exp_name")
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--eval", action="store_true", help="restore restore.generator, then the per-category F1 table of the test split")
    return ap.parse_args(argv)


def main(argv=None):
    """Train one experiment (returns the validation records of this rank) or, with --eval, evaluate it (returns the table)."""
    from . import harness, launch, parallel
    argv = list(sys.argv[1:] if argv is None else argv)
    args = _parse(argv)

    def run(dist):
        cfg = reconstruction_config(harness.load_config(args.config))
        task = "reconstruction"
        if args.eval:
            if "generator" not in cfg.get("restore", {}):
                raise SystemExit("--eval needs restore.generator in the config")
            from .data.image_point import DeviceImageToPoint, ImageBatches
            device = torch.device("cuda", torch.cuda.current_device())
            test = DeviceImageToPoint(harness.make_dataset(cfg, task, None, train="test"), device,      # (the train split is not read)
                                      cache_dir=cfg["data"].get("cache_dir"))
            tr = harness.Trainer(cfg, task, None, device=device, dist=dist, exp_name=args.exp_name, dataset=test)
            batches = ImageBatches(test, int(cfg["data"]["batch_size"]), train=False, seed=int(cfg["data"]["seed"]))      # eval_reconstruction_f1.py:55
            gen = torch.Generator(device=device).manual_seed(int(cfg["data"]["seed"]) * 1000003 + 104729)
            return evaluate(parallel._plain_module(tr.model), batches, cfg, exp_dir=tr.exp_dir, generator=gen)
        tr = harness.Trainer(cfg, task, None, dist=dist, exp_name=args.exp_name)
        tr.fit()
        return tr.val_records

    return launch.run_entry(__file__, argv, args.gpus, args.config, run, spawn=not args.eval)


if __name__ == "__main__":
    if __package__ in (None, ""):            # started as a file by launch.spawn_ranks
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from cloud_transformers_amd.train_reconstruction import main as _main
        _main()
    else:
        main()
