"""Chamfer distance on MI355X — counterpart of the reference's
`chamfer_extension/dist_chamfer.py` (ChamferFunction :10-56, ChamferDist :59-64,
loss_chamfer :67-76, loss_chamfer_adj :80-89, loss_chamder_2d :92-98), with the
pybind11 `chamfer.forward/backward` calls (chamfer_cuda.cpp:30-33) replaced by
the C ABI entry points ct_chamfer_fwd / ct_chamfer_bwd.  `chamfer_with_counts`,
`ChamferDist`'s optional counts and `loss_chamfer_counts` take clouds of different
lengths in one batch (ct_chamfer_fwd_counts / ct_chamfer_bwd_counts); the reference
has no counterpart (utils/grdnet_utils.py:18-21 drops padding rows at B == 1 only).

Differences from the reference that are NOT observable in the results: outputs
are allocated on the device (the reference allocates on the CPU and copies,
dist_chamfer.py:25-34), kernels run on torch's current stream, and a nonzero
status raises instead of being ignored (dist_chamfer.py:36).
"""
import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from . import determinism as _det
from .ops import _dev, _ptr, _stream, _on


class ChamferWithIndicesFunction(Function):
    """(dist1, dist2, idx1, idx2): the nearest-neighbour indices too (int32, lowest index on ties) — what metrics.py and
    chamfer_with_indices use.  `ChamferFunction` below keeps the reference's two outputs."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        assert xyz1.device == xyz2.device
        assert xyz1.size(0) == xyz2.size(0)
        assert xyz1.size(2) == 3 and xyz2.size(2) == 3
        assert xyz1.is_contiguous() and xyz2.is_contiguous()
        assert xyz1.dtype == torch.float32 and xyz2.dtype == torch.float32
        _dev(xyz1, xyz2)
        B, n, _ = xyz1.size()
        _, m, _ = xyz2.size()
        dev = xyz1.device
        dist1 = torch.empty(B, n, device=dev, dtype=torch.float32)
        dist2 = torch.empty(B, m, device=dev, dtype=torch.float32)
        idx1 = torch.empty(B, n, device=dev, dtype=torch.int32)
        idx2 = torch.empty(B, m, device=dev, dtype=torch.int32)
        lib = _lib.load()
        with _on(dev):
            _lib.check(lib.ct_chamfer_fwd(_ptr(xyz1), _ptr(xyz2), _ptr(dist1), _ptr(dist2), _ptr(idx1), _ptr(idx2),
                                          B, n, m, _stream()), "ct_chamfer_fwd")
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, graddist1, graddist2, _gi1, _gi2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        B, n, _ = xyz1.size()
        m = xyz2.size(1)
        graddist1 = graddist1.contiguous()
        graddist2 = graddist2.contiguous()
        gradxyz1 = torch.empty_like(xyz1)
        gradxyz2 = torch.empty_like(xyz2)
        lib = _lib.load()
        _det.push(lib)          # deterministic mode: the ordered form of the kernel (one wave per destination row)
        with _on(xyz1.device):
            _lib.check(lib.ct_chamfer_bwd(_ptr(xyz1), _ptr(xyz2), _ptr(graddist1), _ptr(graddist2),
                                          _ptr(idx1), _ptr(idx2), _ptr(gradxyz1), _ptr(gradxyz2),
                                          B, n, m, _stream()), "ct_chamfer_bwd")
        return gradxyz1, gradxyz2


def _count_arg(count, B, rows, dev, name):
    """An optional int32 [B] device tensor of per-cloud row counts -> (tensor kept alive or None, pointer or None)."""
    if count is None:
        return None, None
    if not torch.is_tensor(count) or count.dtype != torch.int32 or tuple(count.shape) != (B,):
        raise TypeError("chamfer_with_counts: %s is an int32 tensor [B] = [%d] of counts in [0, %d], or None" % (name, B, rows))
    _dev(count)
    if count.device != dev:
        raise ValueError("chamfer_with_counts: %s is on %s, the clouds are on %s" % (name, count.device, dev))
    count = count.contiguous()
    return count, _ptr(count)


class ChamferWithCountsFunction(Function):
    """ChamferWithIndicesFunction for clouds of different lengths in one batch (ct_chamfer_fwd_counts / ct_chamfer_bwd_counts):
    cloud b of xyz1 is its rows [0, count1[b]), of xyz2 its rows [0, count2[b]); a count of None means every row.  Rows below
    the count carry the bits the dense op returns for that pair alone; rows at or beyond it get dist 0, idx -1 and an exact
    zero gradient, and their contents are never read.  The counts are not differentiable."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, count1, count2):
        assert xyz1.device == xyz2.device
        assert xyz1.size(0) == xyz2.size(0)
        assert xyz1.size(2) == 3 and xyz2.size(2) == 3
        assert xyz1.is_contiguous() and xyz2.is_contiguous()
        assert xyz1.dtype == torch.float32 and xyz2.dtype == torch.float32
        _dev(xyz1, xyz2)
        B, n, _ = xyz1.size()
        _, m, _ = xyz2.size()
        dev = xyz1.device
        count1, c1 = _count_arg(count1, B, n, dev, "count1")
        count2, c2 = _count_arg(count2, B, m, dev, "count2")
        dist1 = torch.empty(B, n, device=dev, dtype=torch.float32)
        dist2 = torch.empty(B, m, device=dev, dtype=torch.float32)
        idx1 = torch.empty(B, n, device=dev, dtype=torch.int32)
        idx2 = torch.empty(B, m, device=dev, dtype=torch.int32)
        lib = _lib.load()
        with _on(dev):
            _lib.check(lib.ct_chamfer_fwd_counts(_ptr(xyz1), _ptr(xyz2), c1, c2, _ptr(dist1), _ptr(dist2), _ptr(idx1), _ptr(idx2),
                                                 B, n, m, _stream()), "ct_chamfer_fwd_counts")
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        ctx.counts = (count1, count2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, graddist1, graddist2, _gi1, _gi2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        count1, count2 = ctx.counts
        B, n, _ = xyz1.size()
        m = xyz2.size(1)
        graddist1 = graddist1.contiguous()
        graddist2 = graddist2.contiguous()
        gradxyz1 = torch.empty_like(xyz1)
        gradxyz2 = torch.empty_like(xyz2)
        lib = _lib.load()
        _det.push(lib)          # deterministic mode: the ordered form, with each cloud's own n and m
        with _on(xyz1.device):
            _lib.check(lib.ct_chamfer_bwd_counts(_ptr(xyz1), _ptr(xyz2), None if count1 is None else _ptr(count1),
                                                 None if count2 is None else _ptr(count2), _ptr(graddist1), _ptr(graddist2),
                                                 _ptr(idx1), _ptr(idx2), _ptr(gradxyz1), _ptr(gradxyz2),
                                                 B, n, m, _stream()), "ct_chamfer_bwd_counts")
        return gradxyz1, gradxyz2, None, None


class ChamferFunction:
    """The reference's interface (chamfer_extension/dist_chamfer.py:10-56): `dist1, dist2 = ChamferFunction.apply(xyz1, xyz2)`
    — TWO outputs, as its own callers unpack them (utils/grdnet_utils.py:22, dist_chamfer.py:62)."""

    @staticmethod
    def apply(xyz1, xyz2):
        d1, d2, _, _ = ChamferWithIndicesFunction.apply(xyz1, xyz2)
        return d1, d2


class ChamferDist(nn.Module):
    """forward(input1 [B,n,3], input2 [B,m,3]) -> (dist1 [B,n], dist2 [B,m]) squared NN distances."""

    def forward(self, input1, input2, count1=None, count2=None):
        """With `count1` / `count2` (int32 [B] on the device): `chamfer_with_counts`' distances, zero at the rows at or
        beyond a cloud's count."""
        if count1 is None and count2 is None:
            return ChamferFunction.apply(input1, input2)
        d1, d2, _, _ = ChamferWithCountsFunction.apply(input1, input2, count1, count2)
        return d1, d2


def chamfer_with_indices(xyz1, xyz2):
    """(dist1, dist2, idx1, idx2) — indices are int32, lowest index on ties."""
    return ChamferWithIndicesFunction.apply(xyz1, xyz2)


def chamfer_with_counts(xyz1, xyz2, count1=None, count2=None):
    """(dist1, dist2, idx1, idx2) of clouds xyz1 [B,n,3], xyz2 [B,m,3] whose cloud b has count1[b] / count2[b] rows (int32 [B]
    device tensors; None: all rows) — see ChamferWithCountsFunction."""
    return ChamferWithCountsFunction.apply(xyz1, xyz2, count1, count2)


def _to_bn3(pc):
    # pc is [B, 3, 1, N] in the training scripts (train_inpainter.py:190-192)
    return pc[:, :, 0].permute(0, 2, 1).contiguous()


def loss_chamfer(pc_1, pc_2):
    dist_1, dist_2 = ChamferDist()(_to_bn3(pc_1), _to_bn3(pc_2))
    return torch.mean(dist_1) + torch.mean(dist_2)


def loss_chamfer_counts(pc_1, pc_2, count1, count2):
    """loss_chamfer for clouds of different lengths: per cloud, the mean of dist1 over its count1[b] rows plus the mean of
    dist2 over its count2[b] rows; then the mean over the batch.  A count of None stands for every row.  (A cloud with a
    zero count has no mean: its term, and the loss, is NaN, as torch's mean of nothing.)"""
    dist_1, dist_2 = ChamferDist()(_to_bn3(pc_1), _to_bn3(pc_2), count1, count2)
    n1 = dist_1.size(1) if count1 is None else count1.to(dist_1.dtype)
    n2 = dist_2.size(1) if count2 is None else count2.to(dist_2.dtype)
    return torch.mean(dist_1.sum(dim=1) / n1 + dist_2.sum(dim=1) / n2)


def loss_chamfer_adj(pc_1, pc_2):
    """PCN-style: mean of square roots, halved."""
    dist_1, dist_2 = ChamferDist()(_to_bn3(pc_1), _to_bn3(pc_2))
    return (torch.mean(torch.sqrt(dist_1)) + torch.mean(torch.sqrt(dist_2))) / 2


def loss_chamder_2d(pc_1, pc_2):
    """2-D clouds are lifted to z = 0 (name kept as the reference spells it)."""
    z1 = torch.zeros(pc_1.size(0), 1, 1, pc_1.size(-1), device=pc_1.device, dtype=pc_1.dtype)
    z2 = torch.zeros(pc_2.size(0), 1, 1, pc_2.size(-1), device=pc_2.device, dtype=pc_2.dtype)
    return loss_chamfer(torch.cat([pc_1, z1], dim=1), torch.cat([pc_2, z2], dim=1))
