"""Frozen-statistics fine-tuning: hold every norm's running statistics still while the rest of the model trains.

`freeze_norms(model)` puts every BatchNorm of `model` (1d, 2d, 3d and SyncBatchNorm) in eval mode and marks it; a marked
norm stays in eval mode through later `model.train()` calls, so its running statistics and `num_batches_tracked` never
move and — under data parallelism — it exchanges no statistics.  Marked BatchNorm1d / SyncBatchNorm layers of the MHCT
blocks run on the fused kernels, forward (ct_bn_eval_group_fwd) and backward (ct_bn_eval_group_bwd); the 2d / 3d norms
and the model files' own stems and heads are frozen all the same and run by torch.

The mark is two plain instance attributes: no parameter, no buffer, so state-dict keys are unchanged, and
`copy.deepcopy` carries it along.  Apply it AFTER `torch.nn.SyncBatchNorm.convert_sync_batchnorm`: the conversion builds
new modules and would drop it.
"""
import torch
from torch.nn.modules.batchnorm import _BatchNorm


class _StayEval:
    """Stands in for a marked norm's `train`: whatever mode is asked for, the norm stays in eval mode.  (An object, not a
    closure: deepcopy and pickle rebuild it around the copied module.)"""

    def __init__(self, module):
        self.module = module

    def __call__(self, mode=True):
        torch.nn.Module.train(self.module, False)
        return self.module


def _norms(model):
    return [m for m in model.modules() if isinstance(m, _BatchNorm)]


def freeze_norms(model, affine=False):
    """Freeze the running statistics of every BatchNorm of `model`; returns `model`.  With affine=True the norms' weight and
    bias stop taking gradients as well (their previous requires_grad flags are remembered for unfreeze_norms).  Apply after
    convert_sync_batchnorm and after wrapping for data parallelism."""
    for m in _norms(model):
        m.__dict__["_ct_frozen"] = True
        m.__dict__["train"] = _StayEval(m)
        torch.nn.Module.train(m, False)
        if affine and m.affine and "_ct_frozen_affine" not in m.__dict__:
            m.__dict__["_ct_frozen_affine"] = (m.weight.requires_grad, m.bias.requires_grad)
            m.weight.requires_grad_(False)
            m.bias.requires_grad_(False)
    return model


def unfreeze_norms(model):
    """Undo freeze_norms: the marks go, the requires_grad flags come back, and every norm takes the mode of `model`."""
    for m in _norms(model):
        if not m.__dict__.pop("_ct_frozen", False):
            continue
        m.__dict__.pop("train", None)
        flags = m.__dict__.pop("_ct_frozen_affine", None)
        if flags is not None:
            m.weight.requires_grad_(flags[0])
            m.bias.requires_grad_(flags[1])
        m.train(model.training)
    return model


def norms_frozen(model):
    """True when `model` has norms and all are frozen, False when none is, "partial" otherwise."""
    marks = [bool(m.__dict__.get("_ct_frozen", False)) for m in _norms(model)]
    if marks and all(marks):
        return True
    return "partial" if any(marks) else False
