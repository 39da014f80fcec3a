"""The ScanObjectNN classification protocol's data path on the device (datasets/scanobjectnn.py:87-125,
train_classification.py:65-90,194-197,333-350): the split is uploaded once, a batch is one gather launch.

- `DeviceScanObjectNN(dataset, device)`: the points, byte mask and labels of a `data.datasets.ScanObjectNN` (whose host
  centring and normalisation stay as they are: they run once and are the reference's bits) as device tensors.
- `scan_items_from_draws`: the raw `ct_scan_items` launch (include/cloudct.h) on explicit draws; a pure function.
- `scan_items`: the draws of one batch from one generator on the device, then the launch; no host synchronisation.
- `ScanBatches`: one iteration = one epoch of `(pcd [B, 3, 1, N], label [B], mask [B, N])` on the device, in the order of
  torch's own `DistributedSampler`.
- `ClassificationMeter`: cls_acc, seg_acc and the per-class m_acc of train_classification.py:333-350 from count tensors.
"""
import math

import torch
from torch.utils.data.distributed import DistributedSampler


class DeviceScanObjectNN(object):
    """`data` f32[M, P, 3], `mask` u8[M, P] (0 background, 1 object) and `label` i64[M] of a `data.datasets.ScanObjectNN` on
    `device`, uploaded once (the main split is about 0.3 GB)."""

    def __init__(self, dataset, device):
        self.device = torch.device(device)
        self.data = torch.as_tensor(dataset.data, dtype=torch.float32).contiguous().to(self.device)
        self.mask = torch.as_tensor(dataset.mask != 0).to(torch.uint8).contiguous().to(self.device)
        self.label = torch.as_tensor(dataset.label).reshape(-1).to(torch.int64).contiguous().to(self.device)
        M, P, three = self.data.shape
        if three != 3 or tuple(self.mask.shape) != (M, P) or tuple(self.label.shape) != (M,):
            raise ValueError("ScanObjectNN arrays: data [M, P, 3], mask [M, P], label [M]; got %s %s %s"
                             % (tuple(self.data.shape), tuple(self.mask.shape), tuple(self.label.shape)))
        self.num_points = P

    def __len__(self):
        return self.data.shape[0]


def scan_items_from_draws(ds, item, perm, rot, jit, N, sigma=0.01, clip=0.05, out=None):
    """ct_scan_items (include/cloudct.h) on explicit draws: item i64[B], perm i64[B, P] or None, rot f32[B, 2] = (cos, sin) and
    jit f32[B, N, 3], both or neither -> (points f32[B, 3, N], mask f32[B, N], label i64[B]).  `out`: the three tensors to write
    (contiguous, on the device; any alignment).  A pure function of its arguments."""
    from .. import _lib
    from ..ops import _dev, _on, _ptr, _stream
    _dev(ds.data, item, perm, rot, jit)
    dev = ds.data.device
    M, P, N = len(ds), ds.num_points, int(N)
    B = item.shape[0]
    if item.dim() != 1 or item.dtype != torch.int64:
        raise TypeError("scan_items: item is int64 [B]")
    if perm is not None and (perm.dtype != torch.int64 or tuple(perm.shape) != (B, P)):
        raise ValueError("scan_items: perm is int64 [B, P] = [%d, %d]; got %s %s" % (B, P, perm.dtype, tuple(perm.shape)))
    if (rot is None) != (jit is None):
        raise ValueError("scan_items: rot and jit are given both or neither")
    if rot is not None and (rot.dtype != torch.float32 or jit.dtype != torch.float32 or tuple(rot.shape) != (B, 2)
                            or tuple(jit.shape) != (B, N, 3)):
        raise ValueError("scan_items: rot is float32 [B, 2], jit float32 [B, N, 3]; got %s %s" % (tuple(rot.shape), tuple(jit.shape)))
    item, perm, rot, jit = [None if t is None else t.contiguous() for t in (item, perm, rot, jit)]
    if out is None:
        out = (torch.empty(B, 3, N, dtype=torch.float32, device=dev), torch.empty(B, N, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.int64, device=dev))
    points, mask, label = out
    for t, shape, dtype in ((points, (B, 3, N), torch.float32), (mask, (B, N), torch.float32), (label, (B,), torch.int64)):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError("scan_items: out is contiguous (f32[B, 3, N], f32[B, N], i64[B]) on %s" % dev)
    with _on(dev):
        _lib.check(_lib.load().ct_scan_items(ds.data.data_ptr(), ds.mask.data_ptr(), ds.label.data_ptr(), M, P, item.data_ptr(),
                                             _ptr(perm), _ptr(rot), _ptr(jit), float(sigma), float(clip), B, N, points.data_ptr(),
                                             mask.data_ptr(), label.data_ptr(), _stream(dev)), "ct_scan_items")
    return points, mask, label


def scan_draws(B, P, N, train, device, generator=None):
    """The draws of one batch from `generator` on `device`, in this order: the subsample keys rand(B, P) when N < P (their
    argsort is `perm`: its first N entries are N points without replacement), then with `train` the jitter randn(B, N, 3),
    then the angle rand(B) * 2 pi, returned as (cos, sin).  -> (perm | None, rot | None, jit | None)."""
    perm = rot = jit = None
    if N < P:
        perm = torch.argsort(torch.rand(B, P, device=device, generator=generator), dim=1)
    if train:
        jit = torch.randn(B, N, 3, device=device, generator=generator)
        angle = torch.rand(B, device=device, generator=generator) * (2 * math.pi)
        rot = torch.stack([torch.cos(angle), torch.sin(angle)], dim=1)
    return perm, rot, jit


def scan_items(ds, item, N=None, train=False, generator=None, sigma=0.01, clip=0.05):
    """(points f32[B, 3, N], mask f32[B, N], label i64[B]) of the clouds `item` i64[B] (on the device): what the reference's
    `ScanObjectNN(train=train, subsample=N)[i]` items give after the collate and the `permute` — with `train`, jitter clipped to
    `clip` and one rotation about y per cloud; with N < P, N points without replacement.  The draws are `scan_draws`'; the
    jitter is drawn per kept point (the reference draws it for all P and keeps N: the same distribution).  No host
    synchronisation."""
    N = ds.num_points if N is None else int(N)
    with torch.no_grad():
        perm, rot, jit = scan_draws(item.shape[0], ds.num_points, N, train, ds.data.device, generator)
        return scan_items_from_draws(ds, item, perm, rot, jit, N, sigma, clip)


class ScanBatches(object):
    """One iteration is one epoch of device batches `(pcd f32[B, 3, 1, N], label i64[B], mask f32[B, N])` of a
    DeviceScanObjectNN.  The epoch's order is `torch.utils.data.distributed.DistributedSampler(range(len(ds)), world, rank,
    shuffle=train, seed=seed)` after `set_epoch` (shuffling and the padding of the shards are torch's), uploaded once per
    epoch; `drop_last` drops a ragged last batch as a DataLoader does.  `subsample` = N (None: all P points).  The items'
    draws come from a device generator seeded by `seed` and the rank.  `last_items` is the index tensor of the batch just
    yielded (a view of the epoch's order on the device)."""

    def __init__(self, ds, batch_size, train=False, seed=0, rank=0, world=1, drop_last=False, subsample=None, sigma=0.01, clip=0.05):
        self.ds, self.batch_size, self.train, self.drop_last = ds, int(batch_size), bool(train), bool(drop_last)
        self.N = ds.num_points if subsample is None else int(subsample)
        self.sigma, self.clip = float(sigma), float(clip)
        self.sampler = DistributedSampler(range(len(ds)), num_replicas=int(world), rank=int(rank), shuffle=self.train, seed=int(seed))
        self.generator = None
        if ds.device.type == "cuda":
            self.generator = torch.Generator(device=ds.device).manual_seed(int(seed) * 1000003 + int(rank))
        self.last_items = None

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def set_epoch(self, epoch):
        self.sampler.set_epoch(int(epoch))

    def epoch_order(self):
        """The cloud indices of this rank's epoch, batch after batch (host list)."""
        order = list(self.sampler)
        return order[:len(self) * self.batch_size]

    def __iter__(self):
        order = torch.tensor(self.epoch_order(), dtype=torch.int64).to(self.ds.device, non_blocking=True)
        for k in range(len(self)):
            item = order[k * self.batch_size:(k + 1) * self.batch_size]
            points, mask, label = scan_items(self.ds, item, self.N, self.train, self.generator, self.sigma, self.clip)
            self.last_items = item
            yield points[:, :, None], label, mask


class ClassificationMeter(object):
    """The counts behind train_classification.py:333-350, kept as one int64 tensor on the device the predictions live on:
    cls_acc = correct / seen, seg_acc = correct mask points / mask points (a point is predicted object when
    sigmoid(mask_pred[:, 0, 0]) > 0.5), m_acc = mean over the classes of correct_c / total_c.  `reduce(dist)` all-reduces the
    counts over the ranks (in place of the reference's pickled all_gather).  A class absent from the split makes its accuracy,
    and so m_acc, NaN — the reference's 0 / 0 division does the same."""

    def __init__(self, n_classes):
        self.n = int(n_classes)
        self.counts = None              # [correct, seen, correct_seg, seen_seg, correct_c ..., total_c ...]

    def update(self, class_pred, mask_pred, labels, mask):
        with torch.no_grad():
            if self.counts is None:
                self.counts = torch.zeros(4 + 2 * self.n, dtype=torch.int64, device=class_pred.device)
            labels = labels.long()
            hit = (class_pred.argmax(dim=1) == labels).long()
            seg = ((torch.sigmoid(mask_pred[:, 0, 0]) > 0.5) == (mask != 0)).long().sum()
            head = torch.stack([hit.sum(), torch.full_like(seg, labels.numel()), seg, torch.full_like(seg, mask.numel())])
            self.counts[:4] += head
            self.counts[4:4 + self.n].index_add_(0, labels, hit)
            self.counts[4 + self.n:].index_add_(0, labels, torch.ones_like(hit))

    def reduce(self, dist):
        if self.counts is not None:
            dist.all_reduce(self.counts)

    def result(self):
        """{"cls_acc", "seg_acc", "m_acc", "class_acc": [n_classes]} as python floats (one device-to-host copy)."""
        c = self.counts.tolist() if self.counts is not None else [0] * (4 + 2 * self.n)

        def div(a, b):
            return a / b if b else float("nan")

        per = [div(c[4 + k], c[4 + self.n + k]) for k in range(self.n)]
        return {"cls_acc": div(c[0], c[1]), "seg_acc": div(c[2], c[3]), "m_acc": sum(per) / len(per), "class_acc": per}
