"""Training and evaluation of the S3DIS KPConv protocol (train_segmentation_kpconv.py, eval_segmentation_kpconv.py,
datasets/s3dis_closer_train.py) on the device: the `segmentation_kpconv` task of `harness.Trainer`.

    python -m cloud_transformers_amd.train_kpconv EXP -c configs/s3dis_kpconv.yaml [--gpus N] [--eval]

The config is the reference's YAML as it is (`data.path` = the Stanford3dDataset_v1.2 folder or its parent); the keys the
reference hard-codes in its FakeCFG (train_segmentation_kpconv.py:84-114) are defaults here (`kpconv_config`).

- `KPConvData`: one epoch = a plan of `data.num_steps` sphere picks, identical on every rank (the plan's generator is
  seeded by `data.seed`), sharded as DistributedSampler(shuffle=False) shards indices, in batches of `data.batch_size` (the
  last partial batch is dropped); items are augmented (`Augment`) from a per-rank generator.  Validation: the same over
  the validation Area, `num_votes` passes, pass v > 0 augmented, the last partial batch kept (the reference's val loader).
- `--eval`: restore `restore.generator` (and `restore.optimizer` when given), then one validation of 20 votes
  (`train.hip_graph_val: true`: forward and loss of every vote batch by HIP-graph replay, `VoteEvaluator.add` eager).
- `--gpus N > 1`: N ranks through `launch.spawn_ranks`, one process group over RCCL."""
import argparse
import math
import os
import sys

import torch

ALL_AREAS = ["Area_%d" % k for k in range(1, 7)]


def kpconv_config(cfg):
    """A copy of `cfg` with the protocol's defaults (protocols.KPConv `DATA` / `TRAIN`: train_segmentation_kpconv.py:84-114,
    :240-266) under the keys it lacks."""
    from .protocols import KPConv
    return KPConv.config(cfg)


def load_kpconv_areas(cfg, train=True, device=None):
    """(train Areas or None, validation Areas) of `data.path`: `data.test_area` validates, the other Areas 1-6 train;
    subsampled at `data.sampleDl` (on `device` when one is given: the same arrays) and cached under <data.path>/processed."""
    from .data.s3dis_kpconv import load_areas
    data = kpconv_config(cfg)["data"]
    test = str(data["test_area"])
    kw = dict(sampleDl=float(data["sampleDl"]), cache_dir=os.path.join(str(data["path"]), "processed"), device=device)
    val = load_areas(data["path"], [test], **kw)
    return (load_areas(data["path"], [a for a in ALL_AREAS if a != test], **kw) if train else None), val


def shard_batches(n, rank, world, batch_size, drop_last=True):
    """Index batches of rank `rank` over items 0..n-1: DistributedSampler(shuffle=False)'s order (its wrap-around padding to a
    multiple of `world` included), cut into batches of `batch_size`; `drop_last` drops the last partial batch."""
    num_samples = int(math.ceil(n / world))
    total = num_samples * world
    idx = list(range(n))
    pad = total - n
    idx += (idx * int(math.ceil(pad / n)))[:pad] if pad > 0 else []
    mine = idx[rank:total:world]
    out = [mine[i:i + batch_size] for i in range(0, len(mine), batch_size)]
    if drop_last and out and len(out[-1]) < batch_size:
        out.pop()
    return out


def masked_cross_entropy(pred, labels, mask):
    """MaskedCrossEntropy (s3dis_closer_train.py:11-18): sum(CE * mask) / sum(mask)."""
    m = mask.float()
    return (torch.nn.functional.cross_entropy(pred, labels, reduction="none") * m).sum() / m.sum()


class KPConvData:
    """Samplers, augmentation and the vote evaluator of one rank.  `areas`: (train Areas or None, validation Areas); an
    iteration over the object is one training epoch of (points, mask, features, labels) batches on `device`."""

    def __init__(self, cfg, device, dist=None, areas=None):
        from . import parallel
        from .data.s3dis_kpconv import Augment, SphereSampler, VoteEvaluator
        cfg = kpconv_config(cfg)
        data = cfg["data"]
        self.device = torch.device(device)
        self.dist = dist
        self.rank = dist.get_rank() if parallel._active(dist) else 0
        self.world = parallel.world_size(dist)
        self.B, self.N, self.steps = int(data["batch_size"]), int(data["num_points"]), int(data["num_steps"])
        train_areas, val_areas = areas if areas is not None else load_kpconv_areas(cfg)
        seed = int(data["seed"])
        F, r = int(data["input_features_dim"]), float(data["in_radius"])

        def gen(k):
            return torch.Generator(device=self.device).manual_seed(seed * 1000003 + k)

        self.train = None
        if train_areas is not None:
            self.train = SphereSampler(train_areas, self.N, in_radius=r, input_features_dim=F, color_drop=float(data["color_drop"]),
                                       device=self.device, generator=gen(0))
        self.val = SphereSampler(val_areas, self.N, in_radius=r, input_features_dim=F, color_drop=float(data["val_color_drop"]),
                                 device=self.device, generator=gen(1))
        self.train_gen, self.val_gen = gen(16 + 2 * self.rank), gen(17 + 2 * self.rank)       # per rank: the items' draws
        self.augment = Augment()
        self.evaluator = VoteEvaluator(val_areas, num_classes=int(data["num_classes"]), device=self.device)

    def __iter__(self):
        cloud, picks = self.train.plan(self.steps)
        for rows in shard_batches(self.steps, self.rank, self.world, self.B):
            sel = torch.tensor(rows, dtype=torch.int64, device=self.device)
            points, mask, features, labels, _, _ = self.train.items(cloud[sel], picks[sel], self.augment, generator=self.train_gen)
            yield points, mask, features, labels

    def validate(self, model, num_votes, epoch, step=None):
        """validate() of s3dis_closer_train.py:70-167: the vote sums and counts restart, the running logits go on; one record
        per pass: mean loss, part / running-sub / sub / full IoUs and their means (sums, counts and the part confusion
        summed over the ranks first).  `step`: (points, mask, features, labels) -> (pred, masked cross-entropy) of `model`,
        called per batch in its place (the harness passes its validation step, eager or replayed as a HIP graph; `pred` may
        be a graph's static output: `VoteEvaluator.add` consumes it before the next batch)."""
        from . import parallel
        ev = self.evaluator
        ev.reset_votes()
        ev.projections()
        was_training = model.training
        model.eval()
        records = []
        with torch.no_grad():
            for v in range(int(num_votes)):
                ev.start_pass()
                cloud, picks = self.val.plan(self.steps)
                loss = torch.zeros(2, dtype=torch.float64, device=self.device)       # sum of batch losses * batch size, items
                for rows in shard_batches(self.steps, self.rank, self.world, self.B, drop_last=False):
                    sel = torch.tensor(rows, dtype=torch.int64, device=self.device)
                    points, mask, features, labels, cl, inds = self.val.items(cloud[sel], picks[sel], self.augment if v > 0 else None,
                                                                              generator=self.val_gen)
                    if step is None:
                        pred = model(points, mask, features)
                        batch_loss = masked_cross_entropy(pred, labels, mask)
                    else:
                        pred, batch_loss = step(points, mask, features, labels)
                    loss[0] += batch_loss.double() * len(rows)
                    loss[1] += len(rows)
                    ev.add(pred, mask, cl, inds)
                if parallel._active(self.dist):
                    self.dist.all_reduce(loss)
                red = ev.synced(self.dist)
                rec = {"epoch": epoch, "vote": v, "loss": float(loss[0] / loss[1])}
                for name, (ious, miou) in (("part", red.part_ious()), ("running_sub", red.sub_ious(running=True)),
                                           ("sub", red.sub_ious()), ("full", red.full_ious())):
                    rec[name + "_ious"] = [float(x) for x in ious]
                    rec[name + "_miou"] = float(miou)
                records.append(rec)
        model.train(was_training)
        return records


def _parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("exp_name")
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--eval", action="store_true", help="restore, then one validation of train.final_votes (20) votes")
    return ap.parse_args(argv)


def main(argv=None):
    """Train (or with --eval, evaluate) one experiment; returns the validation records of this rank (rank 0 writes them to
    <exp>/kpconv_val.jsonl)."""
    from . import harness, launch
    argv = list(sys.argv[1:] if argv is None else argv)
    args = _parse(argv)

    def run(dist):
        cfg = kpconv_config(harness.load_config(args.config))
        areas = load_kpconv_areas(cfg, train=not args.eval, device=torch.device("cuda", torch.cuda.current_device()))
        tr = harness.Trainer(cfg, "segmentation_kpconv", int(cfg["data"]["num_classes"]), dist=dist, exp_name=args.exp_name,
                             dataset=areas)
        if args.eval:
            return tr.validate(int(cfg["train"]["final_votes"]), "Last")
        tr.fit()
        return tr.val_records

    return launch.run_entry(__file__, argv, args.gpus, args.config, run)              # (--eval runs on N ranks too)


if __name__ == "__main__":
    if __package__ in (None, ""):            # started as a file by launch.spawn_ranks
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from cloud_transformers_amd.train_kpconv import main as _main
        _main()
    else:
        main()
