"""Approximate Earth Mover's Distance (auction algorithm) on MI355X — counterpart of
the reference's `emd_linear/emd_module.py` (`emdFunction` :29-70, `emdModule` :72-77)
with the pybind11 `emd.forward/backward` calls (emd.cpp:28-31) replaced by the C ABI
entry points ct_emd_fwd / ct_emd_bwd.

Inputs: xyz1 (prediction), xyz2 (ground truth), both [B, n, 3] normalised to [0, 1];
n a multiple of 1024, B <= 512.  Returns (dist [B,n] squared distance to the assigned
target, assignment [B,n] int32).  Only xyz1 receives a gradient; the gradient wrt xyz2
is zeros, as in the reference (emd_module.py:66-70).  The twelve scratch tensors the
reference allocates per call (emd_module.py:41-54) are one opaque workspace here, and
tensors stay on the device of the inputs (the reference hard-codes 'cuda').

`emd_with_counts`, `emdModule`'s optional count, `loss_emd_counts` and the routing helper `emd_distance` lift the two shape
restrictions (ct_emd_fwd_counts / ct_emd_bwd_counts): any n, and clouds of different lengths in one batch, their row counts
read on the device.  The reference has no counterpart; `emdFunction` and `emdModule()(a, b, eps, iters)` are unchanged.
"""
import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from .ops import _dev, _ptr, _stream, _on


class emdFunction(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, iters):
        batchsize, n, _ = xyz1.size()
        _, m, _ = xyz2.size()
        assert n == m
        assert xyz1.size()[0] == xyz2.size()[0]
        assert n % 1024 == 0
        assert batchsize <= 512
        _dev(xyz1, xyz2)
        xyz1 = xyz1.contiguous().float()
        xyz2 = xyz2.contiguous().float()
        dev = xyz1.device
        dist = torch.empty(batchsize, n, device=dev, dtype=torch.float32)
        assignment = torch.empty(batchsize, n, device=dev, dtype=torch.int32)
        lib = _lib.load()
        nws = lib.ct_emd_workspace_bytes(batchsize, n)
        ws = torch.empty(nws, device=dev, dtype=torch.uint8)
        with _on(dev):
            _lib.check(lib.ct_emd_fwd(_ptr(xyz1), _ptr(xyz2), _ptr(dist), _ptr(assignment), _ptr(ws), nws,
                                      batchsize, n, float(eps), int(iters), _stream()), "ct_emd_fwd")
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.mark_non_differentiable(assignment)
        return dist, assignment

    @staticmethod
    def backward(ctx, graddist, gradidx):
        xyz1, xyz2, assignment = ctx.saved_tensors
        graddist = graddist.contiguous()
        gradxyz1 = torch.empty_like(xyz1)
        gradxyz2 = torch.zeros_like(xyz2)
        lib = _lib.load()
        B, n, _ = xyz1.shape
        with _on(xyz1.device):
            _lib.check(lib.ct_emd_bwd(_ptr(xyz1), _ptr(xyz2), _ptr(graddist), _ptr(assignment), _ptr(gradxyz1),
                                      B, n, _stream()), "ct_emd_bwd")
        return gradxyz1, gradxyz2, None, None


def _count_arg(count, B, n, dev):
    """An optional int32 [B] tensor of per-cloud row counts on the clouds' device -> the tensor (contiguous) or None."""
    if count is None:
        return None
    if not torch.is_tensor(count) or count.dtype != torch.int32 or tuple(count.shape) != (B,):
        raise TypeError("emd_with_counts: count is an int32 tensor [B] = [%d] of counts in [0, %d], or None" % (B, n))
    if count.device != dev:
        raise ValueError("emd_with_counts: count is on %s, the clouds are on %s" % (count.device, dev))
    return count.contiguous()


class EmdWithCountsFunction(Function):
    """emdFunction for any n and for clouds of different lengths in one batch (ct_emd_fwd_counts / ct_emd_bwd_counts): cloud b
    is the rows [0, count[b]) of xyz1 and of xyz2 (count: int32 [B] on the clouds' device, read on the device only — no
    synchronisation; None: every row).  Rows below the count carry the auction of that pair of clouds alone; rows at or
    beyond it get dist 0, assignment -1 and an exact zero gradient, and their contents are never read.  The count is not
    differentiable and xyz2 gets zeros, as in emdFunction.  With count None and n a multiple of 1024 the dense entry points
    run: the same bits at their full speed."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, iters, count):
        batchsize, n, _ = xyz1.size()
        _, m, _ = xyz2.size()
        assert n == m
        assert xyz1.size()[0] == xyz2.size()[0]
        assert batchsize <= 512
        count = _count_arg(count, batchsize, n, xyz1.device)
        _dev(xyz1, xyz2, count)
        xyz1 = xyz1.contiguous().float()
        xyz2 = xyz2.contiguous().float()
        dev = xyz1.device
        dist = torch.empty(batchsize, n, device=dev, dtype=torch.float32)
        assignment = torch.empty(batchsize, n, device=dev, dtype=torch.int32)
        lib = _lib.load()
        nws = lib.ct_emd_workspace_bytes(batchsize, n)
        ws = torch.empty(nws, device=dev, dtype=torch.uint8)
        dense = count is None and n % 1024 == 0
        with _on(dev):
            if dense:
                _lib.check(lib.ct_emd_fwd(_ptr(xyz1), _ptr(xyz2), _ptr(dist), _ptr(assignment), _ptr(ws), nws,
                                          batchsize, n, float(eps), int(iters), _stream()), "ct_emd_fwd")
            else:
                _lib.check(lib.ct_emd_fwd_counts(_ptr(xyz1), _ptr(xyz2), _ptr(count), _ptr(dist), _ptr(assignment), _ptr(ws), nws,
                                                 batchsize, n, float(eps), int(iters), _stream()), "ct_emd_fwd_counts")
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.count, ctx.dense = count, dense
        ctx.mark_non_differentiable(assignment)
        return dist, assignment

    @staticmethod
    def backward(ctx, graddist, gradidx):
        xyz1, xyz2, assignment = ctx.saved_tensors
        graddist = graddist.contiguous()
        gradxyz1 = torch.empty_like(xyz1)
        gradxyz2 = torch.zeros_like(xyz2)
        lib = _lib.load()
        B, n, _ = xyz1.shape
        with _on(xyz1.device):
            if ctx.dense:
                _lib.check(lib.ct_emd_bwd(_ptr(xyz1), _ptr(xyz2), _ptr(graddist), _ptr(assignment), _ptr(gradxyz1),
                                          B, n, _stream()), "ct_emd_bwd")
            else:
                _lib.check(lib.ct_emd_bwd_counts(_ptr(xyz1), _ptr(xyz2), _ptr(ctx.count), _ptr(graddist), _ptr(assignment),
                                                 _ptr(gradxyz1), B, n, _stream()), "ct_emd_bwd_counts")
        return gradxyz1, gradxyz2, None, None, None


def emd_with_counts(xyz1, xyz2, eps, iters, count=None):
    """(dist [B,n], assignment [B,n] int32) of clouds xyz1, xyz2 [B,n,3] for any n, cloud b having count[b] rows (int32 [B]
    device tensor; None: every row) — see EmdWithCountsFunction."""
    return EmdWithCountsFunction.apply(xyz1, xyz2, eps, iters, count)


class EmdWithInfoFunction(Function):
    """The same auction through ct_emd_fwd_tail: a cloud whose bidder list has become short enough (by default: empty — the
    measured crossover) is finished by one workgroup in one launch, and `info` int32 [B, 2] says what
    the auction came to: info[b, 0] the first iteration that began without a bidder (iters: none did), info[b, 1] the bidders
    the last iteration force-assigned (0 exactly when the auction finished).  dist and assignment are those of
    emdFunction / EmdWithCountsFunction bit for bit, and so is the gradient."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, iters, count, tail_from):
        batchsize, n, _ = xyz1.size()
        _, m, _ = xyz2.size()
        assert n == m
        assert xyz1.size()[0] == xyz2.size()[0]
        assert batchsize <= 512
        lib = _lib.load()
        if not lib.ct_emd_tail_supported(batchsize, n):
            raise ValueError("emd_with_info: B = %d, n = %d is not a shape of ct_emd_fwd_tail (B <= 512, n <= 16384)" % (batchsize, n))
        count = _count_arg(count, batchsize, n, xyz1.device)
        _dev(xyz1, xyz2, count)
        xyz1 = xyz1.contiguous().float()
        xyz2 = xyz2.contiguous().float()
        dev = xyz1.device
        dist = torch.empty(batchsize, n, device=dev, dtype=torch.float32)
        assignment = torch.empty(batchsize, n, device=dev, dtype=torch.int32)
        info = torch.empty(batchsize, 2, device=dev, dtype=torch.int32)
        nws = lib.ct_emd_tail_workspace_bytes(batchsize, n)
        ws = torch.empty(nws, device=dev, dtype=torch.uint8)
        with _on(dev):
            _lib.check(lib.ct_emd_fwd_tail(_ptr(xyz1), _ptr(xyz2), _ptr(count), _ptr(dist), _ptr(assignment), _ptr(info), _ptr(ws), nws,
                                           batchsize, n, float(eps), int(iters), -1 if tail_from is None else int(tail_from),
                                           _stream()), "ct_emd_fwd_tail")
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.count, ctx.dense = count, count is None and n % 1024 == 0
        ctx.mark_non_differentiable(assignment, info)
        return dist, assignment, info

    @staticmethod
    def backward(ctx, graddist, gradidx, gradinfo):
        return EmdWithCountsFunction.backward(ctx, graddist, gradidx) + (None,)


def emd_with_info(xyz1, xyz2, eps, iters, count=None, tail_from=None):
    """(dist [B,n], assignment [B,n] int32, info [B,2] int32) — see EmdWithInfoFunction.  count: int32 [B] device tensor or None;
    tail_from: the iteration after which the first tail launch is enqueued (None: the library's default).  Raises ValueError
    where ct_emd_tail_supported declines the shape."""
    return EmdWithInfoFunction.apply(xyz1, xyz2, eps, iters, count, tail_from)


def emd_tail_supported(B, n):
    return bool(_lib.load().ct_emd_tail_supported(int(B), int(n)))


def emd_distance(xyz1, xyz2, eps, iters, count=None, tail=False):
    """The EMD call of the training loops: emdFunction — its preconditions, bits and speed — where it applies (no count, n a
    multiple of 1024), EmdWithCountsFunction otherwise.  tail=True: the same (dist, assignment) through emd_with_info where
    its shape is supported; the default is the call described above, launch for launch."""
    if tail and emd_tail_supported(xyz1.size(0), xyz1.size(1)):
        return emd_with_info(xyz1, xyz2, eps, iters, count)[:2]
    if count is None and xyz1.size(1) % 1024 == 0:
        return emdFunction.apply(xyz1, xyz2, eps, iters)
    return EmdWithCountsFunction.apply(xyz1, xyz2, eps, iters, count)


def loss_emd_counts(pc_1, pc_2, eps, iters, count=None, tail=False):
    """The EMD loss of train_inpainter.py:189 for clouds [B, 3, 1, N] of different lengths: per cloud, the mean of sqrt(dist)
    over its count[b] rows; then the mean over the batch.  A count of None stands for every row.  The rows at or beyond a
    count are masked BEFORE the root (the root's derivative at their stored 0 is inf, and inf * 0 = NaN).  (A cloud with a
    zero count has no mean: its term, and the loss, is NaN, as torch's mean of nothing.)  tail: as in emd_distance."""
    from .chamfer import _to_bn3
    dist, _ = emd_distance(_to_bn3(pc_1), _to_bn3(pc_2), eps, iters, count, tail=tail)
    if count is None:
        return torch.sqrt(dist).mean(1).mean()
    n = dist.size(1)
    rows = count.clamp(0, n)
    valid = torch.arange(n, device=dist.device)[None] < rows[:, None]
    root = torch.sqrt(torch.where(valid, dist, torch.ones_like(dist)))
    return torch.mean(torch.where(valid, root, torch.zeros_like(root)).sum(dim=1) / rows.to(dist.dtype))


class emdModule(nn.Module):
    def forward(self, input1, input2, eps, iters, count=None):
        """With `count` (int32 [B] on the device): `emd_with_counts`; without, the reference's call and its preconditions."""
        if count is None:
            return emdFunction.apply(input1, input2, eps, iters)
        return emd_with_counts(input1, input2, eps, iters, count)
