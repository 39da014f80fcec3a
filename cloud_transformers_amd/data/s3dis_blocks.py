"""The S3DIS 1x1 m block protocol's data path on the device (datasets/s3dis_v2.py:494-574, train_segmentation.py:77-105,
175-205,244-288): the split is uploaded once, a batch is one launch, the confusion matrix is filled where the predictions are.

- `DeviceS3DISBlocks(dataset, device)`: columns 0..5 and the labels of a `data.datasets.Indoor3DSemSeg` as device tensors.
- `block_items_from_draws`: the raw `ct_block_items` launch (include/cloudct.h) on explicit draws; a pure function.
- `block_draws`: the draws of one batch from one generator on the device, in a fixed order; no host synchronisation.
- `block_items`: the draws, then the launch.
- `BlockBatches`: one iteration = one epoch of `(pcd [B, 6, 1, N], labels [B, N])` on the device, in the order of torch's own
  `DistributedSampler`.
- `SegmentationMeter`: the confusion matrix of train_segmentation.py:198-205 through `ct_seg_confusion`, and
  `return_metrics_dict`'s numbers from it (datasets/S3DIS_tools/iou_util_new.py).
"""
import math

import torch
from torch.utils.data.distributed import DistributedSampler

# datasets/s3dis_v2.py class_order — NOT s3dis_kpconv.LABEL_TO_NAMES, which has chair before table
CLASS_NAMES = ("ceiling", "floor", "wall", "beam", "column", "window", "door", "table", "chair", "sofa", "bookcase", "board",
               "clutter")


class DeviceS3DISBlocks(object):
    """`data` f32[M, P, 6] (x, y, z, r, g, b) and `label` u8[M, P] of a `data.datasets.Indoor3DSemSeg` on `device`, uploaded once
    (the training Areas: 16733 blocks of 4096 points, 1.6 GB + 69 MB).  `length` is the host dataset's `len()`: its
    `data_precent` cuts the epoch, not the arrays."""

    def __init__(self, dataset, device):
        self.device = torch.device(device)
        points = torch.as_tensor(dataset.points)
        self.data = points[:, :, :6].to(torch.float32).contiguous().to(self.device)
        self.label = torch.as_tensor(dataset.labels).to(torch.uint8).contiguous().to(self.device)
        M, P, six = self.data.shape
        if six != 6 or tuple(self.label.shape) != (M, P):
            raise ValueError("S3DIS blocks: points [M, P, >= 6], labels [M, P]; got %s %s" % (tuple(points.shape), tuple(self.label.shape)))
        self.num_points = P
        self.length = len(dataset) if hasattr(dataset, "__len__") else M

    def __len__(self):
        return self.data.shape[0]


def block_items_from_draws(ds, item, perm, aug, jit, cjit, N, sigma=0.01, clip=0.05, cstd=0.05, out=None):
    """ct_block_items (include/cloudct.h) on explicit draws: item i64[B], perm i64[B, N] or None, aug f32[B, 16], jit f32[B, N, 3]
    and cjit f32[B, N, 3], all three or none -> (points f32[B, 6, N], labels i64[B, N]).  `out`: the two tensors to write
    (contiguous, on the device; any alignment).  A pure function of its arguments."""
    from .. import _lib
    from ..ops import _dev, _on, _ptr, _stream
    _dev(ds.data, item, perm, aug, jit, cjit)
    dev = ds.data.device
    M, P, N = len(ds), ds.num_points, int(N)
    B = item.shape[0]
    if item.dim() != 1 or item.dtype != torch.int64:
        raise TypeError("block_items: item is int64 [B]")
    if perm is not None and (perm.dtype != torch.int64 or tuple(perm.shape) != (B, N)):
        raise ValueError("block_items: perm is int64 [B, N] = [%d, %d]; got %s %s" % (B, N, perm.dtype, tuple(perm.shape)))
    given = [t is not None for t in (aug, jit, cjit)]
    if any(given) != all(given):
        raise ValueError("block_items: aug, jit and cjit are given all three or none")
    if aug is not None:
        for t, shape, name in ((aug, (B, 16), "aug"), (jit, (B, N, 3), "jit"), (cjit, (B, N, 3), "cjit")):
            if t.dtype != torch.float32 or tuple(t.shape) != shape:
                raise ValueError("block_items: %s is float32 %s; got %s %s" % (name, list(shape), t.dtype, tuple(t.shape)))
    item, perm, aug, jit, cjit = [None if t is None else t.contiguous() for t in (item, perm, aug, jit, cjit)]
    if out is None:
        out = (torch.empty(B, 6, N, dtype=torch.float32, device=dev), torch.empty(B, N, dtype=torch.int64, device=dev))
    points, labels = out
    for t, shape, dtype in ((points, (B, 6, N), torch.float32), (labels, (B, N), torch.int64)):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError("block_items: out is contiguous (f32[B, 6, N], i64[B, N]) on %s" % dev)
    with _on(dev):
        _lib.check(_lib.load().ct_block_items(ds.data.data_ptr(), ds.label.data_ptr(), M, P, item.data_ptr(), _ptr(perm), _ptr(aug),
                                              _ptr(jit), _ptr(cjit), float(sigma), float(clip), float(cstd), B, N,
                                              points.data_ptr(), labels.data_ptr(), _stream(dev)), "ct_block_items")
    return points, labels


def block_draws(B, N, train, aug, device, generator=None, ratio=0.1, hue_max=0.5, sat_max=0.2):
    """The draws of one batch from `generator` on `device`, in this order:

    1. rand(B, N), whose argsort is `perm` (the loader shuffles every item, validation included);
    and, when `train and aug`,
    2. u = rand(B, 14): angle = 2 pi u0; scale = 0.8 + 0.4 u1..3; the mirror's sign = -1 where u4 < 0.5; auto-contrast taken
       where u5 < 0.2 with w = u6; translation taken where u7 < 0.95 with shift = (u8..10 - 0.5) * 2 * ratio; colour jitter
       taken where u11 < 0.95; hue = (u12 - 0.5) * 2 * hue_max; saturation = 1 + (u13 - 0.5) * 2 * sat_max;
    3. jit = randn(B, N, 3);
    4. cjit = randn(B, N, 3).
    The stage choices are made on the device (torch.where); nothing is read back.  -> (perm, aug f32[B, 16] | None, jit | None,
    cjit | None) with `aug` laid out as include/cloudct.h has it."""
    perm = torch.argsort(torch.rand(B, N, device=device, generator=generator), dim=1)
    if not (train and aug):
        return perm, None, None, None
    u = torch.rand(B, 14, device=device, generator=generator)
    jit = torch.randn(B, N, 3, device=device, generator=generator)
    cjit = torch.randn(B, N, 3, device=device, generator=generator)
    angle = u[:, 0] * (2 * math.pi)
    one, zero = torch.ones_like(angle), torch.zeros_like(angle)
    scale = 0.8 + 0.4 * u[:, 1:4]
    sign = torch.where(u[:, 4] < 0.5, -one, one)
    translated = u[:, 7] < 0.95
    shift = torch.where(translated[:, None], (u[:, 8:11] - 0.5) * (2 * ratio), zero[:, None])
    cols = [torch.cos(angle), torch.sin(angle), scale[:, 0] * sign, scale[:, 1], scale[:, 2],
            torch.where(u[:, 5] < 0.2, u[:, 6], -one), shift[:, 0], shift[:, 1], shift[:, 2],
            translated.to(u.dtype), (u[:, 11] < 0.95).to(u.dtype), (u[:, 12] - 0.5) * (2 * hue_max),
            1 + (u[:, 13] - 0.5) * (2 * sat_max), zero, zero, zero]
    return perm, torch.stack(cols, dim=1), jit, cjit


def block_items(ds, item, N=None, train=False, aug=False, generator=None, sigma=0.01, clip=0.05, cstd=0.05, ratio=0.1, hue_max=0.5,
                sat_max=0.2):
    """(points f32[B, 6, N], labels i64[B, N]) of the blocks `item` i64[B] (on the device): what the reference's
    `Indoor3DSemSeg(num_points=N, train=train, aug=aug)[i]` items give after the collate and the `permute` — the block's first N
    points shuffled and, with `train and aug`, the eight transforms on `block_draws`' draws.  No host synchronisation."""
    N = ds.num_points if N is None else int(N)
    with torch.no_grad():
        perm, a, jit, cjit = block_draws(item.shape[0], N, train, aug, ds.data.device, generator, ratio, hue_max, sat_max)
        return block_items_from_draws(ds, item, perm, a, jit, cjit, N, sigma, clip, cstd)


class BlockBatches(object):
    """One iteration is one epoch of device batches `(pcd f32[B, 6, 1, N], labels i64[B, N])` of a DeviceS3DISBlocks.  The epoch's
    order is `torch.utils.data.distributed.DistributedSampler(range(length), world, rank, shuffle=train, seed=seed)` after
    `set_epoch` (shuffling and the padding of the shards are torch's) with length = int(len(ds) * data_percent), as
    `Indoor3DSemSeg.__len__` cuts it; `drop_last` drops a ragged last batch as a DataLoader does.  Validation (`train=False`, or
    `aug=False`) draws the shuffle but no augmentation.  The items' draws come from a device generator seeded by `seed` and
    the rank.  `last_items` is the index tensor of the batch just yielded (a view of the epoch's order on the device)."""

    def __init__(self, ds, batch_size, num_points=None, train=False, aug=False, seed=0, rank=0, world=1, drop_last=False,
                 data_percent=None, sigma=0.01, clip=0.05, cstd=0.05, ratio=0.1, hue_max=0.5, sat_max=0.2):
        self.ds, self.batch_size, self.train, self.aug = ds, int(batch_size), bool(train), bool(aug)
        self.drop_last = bool(drop_last)
        self.N = ds.num_points if num_points is None else int(num_points)
        self.params = (float(sigma), float(clip), float(cstd), float(ratio), float(hue_max), float(sat_max))
        self.length = ds.length if data_percent is None else int(len(ds) * float(data_percent))
        self.sampler = DistributedSampler(range(self.length), num_replicas=int(world), rank=int(rank), shuffle=self.train, seed=int(seed))
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
        """The block indices of this rank's epoch, batch after batch (host list)."""
        order = list(self.sampler)
        return order[:len(self) * self.batch_size]

    def __iter__(self):
        order = torch.tensor(self.epoch_order(), dtype=torch.int64).to(self.ds.device, non_blocking=True)
        for k in range(len(self)):
            item = order[k * self.batch_size:(k + 1) * self.batch_size]
            points, labels = block_items(self.ds, item, self.N, self.train, self.aug, self.generator, *self.params)
            self.last_items = item
            yield points[:, :, None], labels


class SegmentationMeter(object):
    """The confusion matrix of train_segmentation.py:175,198-205 as one int64 tensor `conf` [n_classes, n_classes] (rows truth,
    columns prediction) on the device the predictions live on, filled by `ct_seg_confusion` — the predictions are never copied
    to the host — and `return_metrics_dict`'s numbers from it.  `reduce(dist)` all-reduces the counts over the ranks (in place of
    the reference's pickled all_gather).  `names`: the classes' names for the `iou_<name>` keys (default: the block protocol's
    13, else the class index)."""

    def __init__(self, n_classes, names=None):
        self.n = int(n_classes)
        if names is None:
            names = CLASS_NAMES if self.n == len(CLASS_NAMES) else tuple(str(k) for k in range(self.n))
        assert len(names) == self.n
        self.names = tuple(names)
        self.conf = None

    def update(self, pred, labels):
        """pred f32[B, C, N] or [B, C, 1, N] (the model's output), labels i64[B, N].  One launch, no synchronisation."""
        from .. import _lib
        from ..ops import _dev, _on, _stream
        with torch.no_grad():
            if pred.dim() == 4:
                pred = pred[:, :, 0]
            _dev(pred, labels)
            B, C, N = pred.shape
            if C != self.n or tuple(labels.shape) != (B, N) or pred.dtype != torch.float32 or labels.dtype != torch.int64:
                raise ValueError("SegmentationMeter: pred f32[B, %d, N], labels i64[B, N]; got %s %s %s %s"
                                 % (self.n, pred.dtype, tuple(pred.shape), labels.dtype, tuple(labels.shape)))
            if self.conf is None:
                self.conf = torch.zeros(self.n, self.n, dtype=torch.int64, device=pred.device)
            pred, labels = pred.detach().contiguous(), labels.contiguous()
            with _on(pred.device):
                _lib.check(_lib.load().ct_seg_confusion(pred.data_ptr(), labels.data_ptr(), B, C, N, self.conf.data_ptr(),
                                                        _stream(pred.device)), "ct_seg_confusion")

    def reset(self):
        if self.conf is not None:
            self.conf.zero_()

    def reduce(self, dist):
        if self.conf is not None:
            dist.all_reduce(self.conf)

    def result(self):
        """iou_util_new.return_metrics_dict: {"overall_acc", "mean_class_acc", "iou_<name>" ..., "mean_iou"} as python floats, in
        the reference's key order (one device-to-host copy).  Its quirks are kept: an IoU's divisor is 1 when the diagonal entry
        is 0, mean_iou divides by the number of classes with a non-empty row or column (NaN when there is none), mean_class_acc
        divides each diagonal entry by max(1, row sum) and the sum by n_classes."""
        n = self.n
        m = [[float(v) for v in row] for row in (self.conf.tolist() if self.conf is not None else [[0] * n] * n)]
        diag = [m[i][i] for i in range(n)]
        rows = [sum(m[i][j] for j in range(n) if j != i) for i in range(n)]
        cols = [sum(m[j][i] for j in range(n) if j != i) for i in range(n)]
        total = sum(sum(row) for row in m)
        out = {"overall_acc": sum(diag) / (total if total != 0 else 1)}
        acc = 0.0
        for i in range(n):
            acc = acc + diag[i] / max(1, sum(m[i]))
        out["mean_class_acc"] = acc / n
        iou = [diag[i] / (diag[i] + rows[i] + cols[i] if diag[i] != 0 else 1) for i in range(n)]
        for name, v in zip(self.names, iou):
            out["iou_" + name] = v
        seen = sum(1 for i in range(n) if sum(m[i]) + sum(m[j][i] for j in range(n)) != 0)
        out["mean_iou"] = sum(iou) / seen if seen else float("nan")
        return out
