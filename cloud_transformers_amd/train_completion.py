"""Training and evaluation of the ShapeNet completion protocol (train_inpainter.py, eval_inpainting.py) on the device: the
`completion` task of `harness.Trainer` on `data.kind: shapenet_completion` or, with the subset kept on the device and the items
gathered there, `data.kind: shapenet_completion_device` (optional `data.cache_dir` keeps the decoded clouds between runs).

    python -m cloud_transformers_amd.train_completion EXP -c configs/inpainting.yaml [--gpus N] [--eval]

The config is the reference's YAML as it is (`data.category_path`, `data.partial_path`, `data.gt_path`, `data.n_renders`,
`data.input_size`, `data.gt_size`, `data.batch_size`, `data.batch_size_val`); `data.kind` is filled in.

- training: batches prepared on the device (data/completion.py CompletionBatches), EMD + Chamfer loss, one validation per
  epoch (`Trainer.validate`: <exp>/completion_val.jsonl, `generator_best_0.t7` on a new minimum).
- `--eval` (eval_inpainting.py:163-226): restore `restore.generator`, then the TEST subset in batches of one: dense =
  reconstruction / 2, `Metrics.get` (F-Score@0.01, Chamfer x 1000) and the dense Chamfer loss x 1000 per sample, averaged
  per taxonomy and overall; the table is printed and written to <exp>/completion_test.json.  With `data.batch_size_test`
  above 1 (not a key of the reference) the subset goes through in batches of that many clouds: `Metrics.get_batch` on the
  device, the sums per taxonomy in a `metrics.TableMeter`, one copy at the end.
- `--gpus N > 1`: N ranks through `launch.spawn_ranks`, one process group over RCCL (training only)."""
import argparse
import json
import os
import sys

import torch

COMPLETION_DATA = {"kind": "shapenet_completion", "n_renders": 1, "input_size": 2048, "gt_size": 16384, "seed": 0}
BATCH_SIZE_TEST = 1     # `data.batch_size_test` where the config lacks it: --eval in batches of one, as eval_inpainting.py:163
COMPLETION_TRAIN = {"val_emd_eps": 0.004, "val_emd_iters": 3000, "emd_eps": 0.005, "emd_iters": 50}


def completion_config(cfg):
    """A copy of `cfg` with the protocol's defaults (train_inpainter.py:186-192, :267-269) under the keys it lacks;
    `data.batch_size_val` defaults to `data.batch_size`."""
    from .protocols import with_defaults
    return with_defaults(cfg, COMPLETION_DATA, COMPLETION_TRAIN)


def eval_batch_size(cfg):
    """`data.batch_size_test` of a config, BATCH_SIZE_TEST where it is absent (`completion_config` leaves the key alone: the
    dictionary it returns for a config without it is what it was before the key existed)."""
    k = int(cfg.get("data", {}).get("batch_size_test", BATCH_SIZE_TEST))
    if k < 1:
        raise ValueError("data.batch_size_test is %d: at least 1" % k)
    return k


def _resident_items(resident, generator):
    """The TEST subset of a DeviceShapeNetCompletion in batches of one, shaped as the host loader's batches: rendering 0, the
    partial cloud sampled, gt as stored (data/completion.py completion_gather with gt_scale 1)."""
    from .data.completion import completion_gather
    for i in range(len(resident)):
        item = torch.full((1,), i, dtype=torch.int64, device=resident.device)
        partial, gt = completion_gather(resident, item, False, generator, gt_scale=1.0)
        yield [resident.taxonomy_ids[i]], [resident.model_ids[i]], {"partial_cloud": partial, "gtcloud": gt}


def _resident_batches(resident, generator, k):
    """`_resident_items` in batches of `k` items (the last one smaller): one completion_gather per batch."""
    from .data.completion import completion_gather
    order = torch.arange(len(resident), dtype=torch.int64).to(resident.device, non_blocking=True)
    for i0 in range(0, len(resident), k):
        i1 = min(i0 + k, len(resident))
        partial, gt = completion_gather(resident, order[i0:i1], False, generator, gt_scale=1.0)
        yield resident.taxonomy_ids[i0:i1], resident.model_ids[i0:i1], {"partial_cloud": partial, "gtcloud": gt}


def _evaluate_batched(model, cfg, device, generator, resident, k):
    """The TEST subset in batches of `k` clouds (the last one smaller), without a host read inside the loop: per batch one
    completion_items call, one model forward and `Metrics.get_batch` (two nearest-neighbour passes; the dense loss is a column
    of the first); the per-taxonomy sums stay on the device in a TableMeter whose row indices are built on the host from the
    ids, which are host data.  One copy at the end -> the dictionary `evaluate` returns, taxonomies in the order they first
    appear."""
    from .data.completion import DatasetSubset, collate_fn, completion_items, shapenet_loader
    from .graphs import eval_forward
    from .metrics import Metrics, TableMeter
    if resident is not None:
        every_id = list(resident.taxonomy_ids)
        loader = _resident_batches(resident, generator, k)
    else:
        ds = shapenet_loader(cfg["data"]).get_dataset(DatasetSubset.TEST)
        every_id = [sample["taxonomy_id"] for sample in ds.file_list]
        loader = torch.utils.data.DataLoader(ds, batch_size=k, num_workers=int(cfg["data"].get("num_workers", 0)), collate_fn=collate_fn,
                                             shuffle=False)
    rows = {}
    for t in every_id:
        rows.setdefault(t, len(rows))
    meter = TableMeter(len(rows), 3, device)            # columns: F-Score, Chamfer x 1000, dense loss x 1000
    was_training = model.training
    model.eval()
    forward = eval_forward(model, cfg)          # `train.hip_graph_val`: a HIP graph per batch shape
    with torch.no_grad():
        for taxonomy_ids, _model_ids, data in loader:
            ids = [t if isinstance(t, str) else t.item() for t in taxonomy_ids]
            gt = data["gtcloud"].to(device, non_blocking=True)
            part, noise, _ = completion_items(data["partial_cloud"].to(device, non_blocking=True), gt.shape[1], scale=2.0,
                                              generator=generator)
            out = forward(noise, part.permute(0, 2, 1)[:, :, None])
            rec = out[0] if isinstance(out, (tuple, list)) else out
            dense = (rec / 2)[:, :, 0].permute(0, 2, 1).contiguous()
            row = torch.tensor([rows[t] for t in ids], dtype=torch.int64).to(device, non_blocking=True)
            meter.update(row, Metrics.get_batch(dense, gt, with_dense=True))
    model.train(was_training)
    counts, sums = meter.result()
    total = int(counts.sum())
    mean = lambda v, c: [float(x) / c if c else 0.0 for x in v]      # noqa: E731  (AverageMeter.avg of nothing is 0)
    return {"names": Metrics.names(),
            "taxonomies": {str(t): {"count": int(counts[r]), "avg": mean(sums[r, :2], int(counts[r]))} for t, r in rows.items() if counts[r]},
            "overall": {"count": total, "avg": mean(sums[:, :2].sum(axis=0), total)},
            "dense_loss": mean(sums[:, 2:].sum(axis=0), total)[0]}


def evaluate(model, cfg, device, exp_dir=None, generator=None, verbose=True, resident=None, batch_size=None):
    """test_net of eval_inpainting.py:132-230 -> {"names": metric names, "taxonomies": {id: {"count", "avg"}}, "overall":
    {"count", "avg"}, "dense_loss": mean dense Chamfer x 1000}; printed as the reference prints it and, with `exp_dir`,
    written to <exp_dir>/completion_test.json.  `resident`: the TEST subset as a DeviceShapeNetCompletion, read instead of
    the files.  `batch_size` (default: `data.batch_size_test`, 1): above 1 the subset is taken in batches of that many
    clouds and the metrics stay on the device until the end (`_evaluate_batched`); the model's draws then depend on the
    batch, so the table is that of another sample of the noise, not the batch-of-one table bit for bit."""
    from .data.completion import DatasetSubset, collate_fn, completion_items, shapenet_loader
    from .graphs import eval_forward
    from .metrics import AverageMeter, ChamferDistance, Metrics
    if generator is None:
        generator = torch.Generator(device=device).manual_seed(int(cfg["data"].get("seed", 0)) * 1000003 + 104729)
    if batch_size is None:
        batch_size = eval_batch_size(cfg)
    if int(batch_size) > 1:
        res = _evaluate_batched(model, cfg, device, generator, resident, int(batch_size))
        return _report(res, exp_dir, verbose)
    if resident is not None:
        loader = _resident_items(resident, generator)
    else:
        ds = shapenet_loader(cfg["data"]).get_dataset(DatasetSubset.TEST)
        loader = torch.utils.data.DataLoader(ds, batch_size=1, num_workers=int(cfg["data"].get("num_workers", 0)), collate_fn=collate_fn,
                                             shuffle=False)
    was_training = model.training
    model.eval()
    forward = eval_forward(model, cfg, verbose=verbose)          # `train.hip_graph_val`: a HIP graph per batch shape
    chamfer_dist = ChamferDistance()
    test_losses, test_metrics, category_metrics = AverageMeter(["DenseLoss"]), AverageMeter(Metrics.names()), {}
    with torch.no_grad():
        for taxonomy_id, model_id, data in loader:
            taxonomy_id = taxonomy_id[0] if isinstance(taxonomy_id[0], str) else taxonomy_id[0].item()
            gt = data["gtcloud"].to(device)
            part, noise, _ = completion_items(data["partial_cloud"].to(device), gt.shape[1], scale=2.0, generator=generator)
            out = forward(noise, part.permute(0, 2, 1)[:, :, None])
            rec = out[0] if isinstance(out, (tuple, list)) else out
            dense = (rec / 2)[:, :, 0].permute(0, 2, 1).contiguous()
            test_losses.update([chamfer_dist(dense, gt).item() * 1000])
            m = Metrics.get(dense, gt)
            test_metrics.update(m)
            category_metrics.setdefault(taxonomy_id, AverageMeter(Metrics.names())).update(m)
    model.train(was_training)
    res = {"names": Metrics.names(),
           "taxonomies": {str(t): {"count": am.count(0), "avg": am.avg()} for t, am in category_metrics.items()},
           "overall": {"count": test_metrics.count(0), "avg": test_metrics.avg()},
           "dense_loss": test_losses.avg(0)}
    return _report(res, exp_dir, verbose)


def _report(res, exp_dir, verbose):
    """The table printed as the reference prints it and, with `exp_dir`, written to <exp_dir>/completion_test.json."""
    if verbose:
        print("============================ TEST RESULTS ============================")
        print("\t".join(["Taxonomy", "#Sample"] + res["names"]))
        for t, row in res["taxonomies"].items():
            print("\t".join([t, str(row["count"])] + ["%.4f" % v for v in row["avg"]]))
        print("\t".join(["Overall", str(res["overall"]["count"])] + ["%.4f" % v for v in res["overall"]["avg"]]))
    if exp_dir is not None:
        with open(os.path.join(str(exp_dir), "completion_test.json"), "w") as f:
            json.dump(res, f, indent=1)
    return res


def _parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("exp_name")
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--eval", action="store_true", help="restore restore.generator, then the per-taxonomy table of the TEST subset")
    return ap.parse_args(argv)


def main(argv=None):
    """Train one experiment (returns the validation records of this rank) or, with --eval, evaluate it (returns the table)."""
    from . import harness, launch, parallel
    argv = list(sys.argv[1:] if argv is None else argv)
    args = _parse(argv)

    def run(dist):
        cfg = completion_config(harness.load_config(args.config))
        n_in = int(cfg["data"]["input_size"])
        if args.eval:
            if "generator" not in cfg.get("restore", {}):
                raise SystemExit("--eval needs restore.generator in the config")
            from .data.completion import DatasetSubset, shapenet_loader
            tr = harness.Trainer(cfg, "completion", n_in, dist=dist, exp_name=args.exp_name,
                                 dataset=shapenet_loader(cfg["data"]).get_dataset(DatasetSubset.TEST))
            resident = tr.loader.ds if tr.protocol.shapenet_device else None
            return evaluate(parallel._plain_module(tr.model), cfg, tr.device, exp_dir=tr.exp_dir, resident=resident)
        tr = harness.Trainer(cfg, "completion", n_in, dist=dist, exp_name=args.exp_name)
        tr.fit()
        return tr.val_records

    return launch.run_entry(__file__, argv, args.gpus, args.config, run, spawn=not args.eval)


if __name__ == "__main__":
    if __package__ in (None, ""):            # started as a file by launch.spawn_ranks
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from cloud_transformers_amd.train_completion import main as _main
        _main()
    else:
        main()
