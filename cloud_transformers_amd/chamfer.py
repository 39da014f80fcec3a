"""Chamfer distance on MI355X — counterpart of the reference's
`chamfer_extension/dist_chamfer.py` (ChamferFunction :10-56, ChamferDist :59-64,
loss_chamfer :67-76, loss_chamfer_adj :80-89, loss_chamder_2d :92-98), with the
pybind11 `chamfer.forward/backward` calls (chamfer_cuda.cpp:30-33) replaced by
the C ABI entry points ct_chamfer_fwd / ct_chamfer_bwd.

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


class ChamferFunction:
    """The reference's interface (chamfer_extension/dist_chamfer.py:10-56): `dist1, dist2 = ChamferFunction.apply(xyz1, xyz2)`
    — TWO outputs, as its own callers unpack them (utils/grdnet_utils.py:22, dist_chamfer.py:62)."""

    @staticmethod
    def apply(xyz1, xyz2):
        d1, d2, _, _ = ChamferWithIndicesFunction.apply(xyz1, xyz2)
        return d1, d2


class ChamferDist(nn.Module):
    """forward(input1 [B,n,3], input2 [B,m,3]) -> (dist1 [B,n], dist2 [B,m]) squared NN distances."""

    def forward(self, input1, input2):
        return ChamferFunction.apply(input1, input2)


def chamfer_with_indices(xyz1, xyz2):
    """(dist1, dist2, idx1, idx2) — indices are int32, lowest index on ties."""
    return ChamferWithIndicesFunction.apply(xyz1, xyz2)


def _to_bn3(pc):
    # pc is [B, 3, 1, N] in the training scripts (train_inpainter.py:190-192)
    return pc[:, :, 0].permute(0, 2, 1).contiguous()


def loss_chamfer(pc_1, pc_2):
    dist_1, dist_2 = ChamferDist()(_to_bn3(pc_1), _to_bn3(pc_2))
    return torch.mean(dist_1) + torch.mean(dist_2)


def loss_chamfer_adj(pc_1, pc_2):
    """PCN-style: mean of square roots, halved."""
    dist_1, dist_2 = ChamferDist()(_to_bn3(pc_1), _to_bn3(pc_2))
    return (torch.mean(torch.sqrt(dist_1)) + torch.mean(torch.sqrt(dist_2))) / 2


def loss_chamder_2d(pc_1, pc_2):
    """2-D clouds are lifted to z = 0 (name kept as the reference spells it)."""
    z1 = torch.zeros(pc_1.size(0), 1, 1, pc_1.size(-1), device=pc_1.device, dtype=pc_1.dtype)
    z2 = torch.zeros(pc_2.size(0), 1, 1, pc_2.size(-1), device=pc_2.device, dtype=pc_2.dtype)
    return loss_chamfer(torch.cat([pc_1, z1], dim=1), torch.cat([pc_2, z2], dim=1))
