"""CPU-side checks of frozen-statistics norms: the header declares ct_bn_eval_bwd_item / ct_bn_eval_group_bwd and names the
entry point in the version comment, the library rejects bad arguments before anything touches a device, freeze_norms /
unfreeze_norms / norms_frozen behave on a plain torch model, and the eligibility functions keep everything but a marked,
eval-mode norm on a device off the new path."""
import copy
import ctypes
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def test_header_declares_the_struct_and_the_entry_point(lib):
    from cloud_transformers_amd import _lib
    text = open(os.path.join(ROOT, "include", "cloudct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    struct = re.search(r"typedef struct \{([^}]*)\} ct_bn_eval_bwd_item;", code)
    assert struct is not None
    fields = re.findall(r"(\w+)\s*;", struct.group(1))
    assert fields == [name for name, _ in _lib.BnEvalBwdItem._fields_]              # the ctypes struct, field for field
    assert fields == ["x", "x_batch_stride", "weight", "bias", "running_mean", "running_var", "gy", "gy_batch_stride", "gx",
                      "gx_batch_stride", "g_weight", "g_bias", "amax_out", "C", "eps", "relu"]
    assert re.search(r"int ct_bn_eval_group_bwd\(const ct_bn_eval_bwd_item\* items, int n, int B, int N, ct_stream_t s\);", code)
    version_comment = text[:text.index("#define CT_ABI_VERSION")]
    assert "ct_bn_eval_group_bwd" in version_comment[version_comment.rindex("/*"):]
    assert re.search(r"#define CT_ABI_VERSION\s+3\b", text) and lib.ct_abi_version() == 3      # additive: no bump
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ct_bn_eval_group_bwd") and "ct_bn_eval_group_bwd" in _lib.SIGNATURES


def test_argument_checks_without_gpu(lib):
    from cloud_transformers_amd import _lib
    buf = ctypes.create_string_buffer(64)                        # never dereferenced: every call below is refused first
    p = ctypes.cast(buf, ctypes.c_void_p).value
    B, C, N = 2, 8, 64

    def call(x=p, xbs=0, w=p, b=p, rm=p, rv=p, gy=p, gybs=0, gx=p, gxbs=0, gw=p, gb=p, C=C, eps=1e-5, B=B, N=N):
        it = _lib.BnEvalBwdItem(x=x, x_batch_stride=xbs, weight=w, bias=b, running_mean=rm, running_var=rv, gy=gy,
                                gy_batch_stride=gybs, gx=gx, gx_batch_stride=gxbs, g_weight=gw, g_bias=gb, C=C, eps=eps, relu=1)
        return lib.ct_bn_eval_group_bwd(ctypes.addressof(it), 1, B, N, None)

    for name in ("x", "w", "b", "rm", "rv", "gy"):                                  # a null required pointer
        assert call(**{name: None}) == -1, name
    assert call(gw=None) == -1 and call(gb=None) == -1                              # only one of g_weight / g_bias
    assert call(gx=None, gw=None, gb=None) == -1                                    # nothing asked for
    assert call(xbs=C * N - 1) == -1 and call(gybs=C * N - 1) == -1 and call(gxbs=C * N - 1) == -1 and call(xbs=-4) == -1
    assert call(eps=-1e-5) == -1 and call(eps=float("nan")) == -1
    assert call(B=0) == -1 and call(N=0) == -1 and call(B=-1) == -1 and call(C=0) == -1
    assert call(B=1 << 16, N=1 << 15) == -1                                         # B*N = 2^31
    items = (_lib.BnEvalBwdItem * 9)()
    for e in items:
        e.x = e.weight = e.bias = e.running_mean = e.running_var = e.gy = e.gx = e.g_weight = e.g_bias = p
        e.C, e.eps, e.relu = C, 1e-5, 1
    addr = ctypes.addressof(items)
    assert lib.ct_bn_eval_group_bwd(None, 2, B, N, None) == -1
    assert lib.ct_bn_eval_group_bwd(addr, 0, B, N, None) == -1
    assert lib.ct_bn_eval_group_bwd(addr, 9, B, N, None) == -1
    assert lib.ct_bn_eval_group_bwd(addr, 2, 0, N, None) == -1
    items[1].g_bias = None                                                          # a bad item that is not the first
    assert lib.ct_bn_eval_group_bwd(addr, 2, B, N, None) == -1
    items[1].g_bias = p
    items[1].gy_batch_stride = C * N - 1
    assert lib.ct_bn_eval_group_bwd(addr, 2, B, N, None) == -1


def _model():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv1d(4, 8, 1), nn.BatchNorm1d(8), nn.ReLU(), nn.Unflatten(2, (4, 4)), nn.Conv2d(8, 6, 1),
                         nn.BatchNorm2d(6), nn.Unflatten(3, (2, 2)), nn.BatchNorm3d(6), nn.Flatten(2), nn.SyncBatchNorm(6))


def test_freeze_unfreeze_and_report_on_a_plain_torch_model():
    from cloud_transformers_amd import freeze_norms, norms_frozen, unfreeze_norms
    model = _model()
    norms = [m for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    assert len(norms) == 4 and norms_frozen(model) is False
    keys = list(model.state_dict())
    assert freeze_norms(model) is model and norms_frozen(model) is True
    assert all(not m.training for m in norms) and model[0].training                 # the norms only
    model.train()                                                                   # a marked norm stays in eval mode
    assert model.training and model[0].training and all(not m.training for m in norms)
    model.eval()
    model.train(True)
    assert all(not m.training for m in norms)
    assert all(m.weight.requires_grad and m.bias.requires_grad for m in norms)      # affine=False: the parameters still train
    assert list(model.state_dict()) == keys                                         # no parameter, no buffer
    twin = copy.deepcopy(model)                                                     # the marks travel
    assert norms_frozen(twin) is True
    twin.train()
    twin_norms = [m for m in twin.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    assert all(not m.training for m in twin_norms) and all(a is not b for a, b in zip(norms, twin_norms))
    unfreeze_norms(twin)                                                            # ... and undoing the copy leaves the original
    assert norms_frozen(twin) is False and norms_frozen(model) is True
    assert all(m.training for m in twin_norms) and all(not m.training for m in norms)
    unfreeze_norms(model)
    assert norms_frozen(model) is False and all(m.training for m in norms)
    model.eval()
    assert all(not m.training for m in norms)
    freeze_norms(model[1])                                                          # one norm of several
    assert norms_frozen(model) == "partial"
    assert norms_frozen(nn.Linear(2, 2)) is False


def test_affine_flags_are_remembered_and_restored():
    from cloud_transformers_amd import freeze_norms, unfreeze_norms
    model = _model()
    model[1].bias.requires_grad_(False)                                             # a flag that was off before
    before = {n: p.requires_grad for n, p in model.named_parameters()}
    freeze_norms(model, affine=True)
    freeze_norms(model, affine=True)                                                # twice: the first memory is kept
    norms = [m for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    assert all(not m.weight.requires_grad and not m.bias.requires_grad for m in norms)
    assert model[0].weight.requires_grad and model[4].weight.requires_grad          # nothing but the norms
    twin = copy.deepcopy(model)
    unfreeze_norms(twin)
    assert {n: p.requires_grad for n, p in twin.named_parameters()} == before
    unfreeze_norms(model)
    assert {n: p.requires_grad for n, p in model.named_parameters()} == before


def test_a_frozen_training_step_leaves_the_statistics_bit_unchanged():
    from cloud_transformers_amd import freeze_norms
    model = nn.Sequential(*list(_model())[:-1])                                     # (SyncBatchNorm has no CPU forward in training)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.running_mean.uniform_(-1, 1)
                m.running_var.uniform_(0.5, 2)
    freeze_norms(model).train()
    stats = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    assert len(stats) == 9
    x = torch.randn(3, 4, 16, requires_grad=True)
    model(x).square().sum().backward()
    assert x.grad is not None and model[1].weight.grad is not None and float(model[1].weight.grad.abs().max()) > 0
    now = model.state_dict()
    assert all(torch.equal(v, now[k]) for k, v in stats.items())


def test_eligibility_is_false_off_the_frozen_path():
    from cloud_transformers_amd import freeze_norms, ops
    x = torch.zeros(2, 8, 64)
    marked = freeze_norms(nn.BatchNorm1d(8))
    assert ops.norm_frozen(marked) and not ops.norm_frozen(nn.BatchNorm1d(8).eval())
    assert not ops.bn_frozen_eligible(marked, x)                                    # a CPU tensor
    convs = [nn.Conv1d(8, 6, 1, bias=False) for _ in range(2)]
    kbs, vbs = [freeze_norms(nn.BatchNorm1d(2)) for _ in range(2)], [freeze_norms(nn.BatchNorm1d(4)) for _ in range(2)]
    assert not ops.union_keys_values_frozen_eligible(x, convs, kbs, vbs)            # a CPU tensor
    assert ops.records_gradients(x, marked.weight) and not ops.records_gradients(x, None)
    with torch.no_grad():
        assert not ops.records_gradients(x, marked.weight)
    if torch.cuda.is_available():
        xc = x.cuda()
        marked = marked.cuda()
        convs, kbs, vbs = [c.cuda() for c in convs], [b.cuda() for b in kbs], [b.cuda() for b in vbs]
        assert ops.bn_frozen_eligible(marked, xc) and ops.union_keys_values_frozen_eligible(xc, convs, kbs, vbs)
        assert not ops.bn_frozen_eligible(nn.BatchNorm1d(8).cuda().eval(), xc)      # unmarked
        assert not ops.bn_frozen_eligible(nn.BatchNorm1d(8).cuda().train(), xc)     # training
        marked.training = True                                                      # a marked norm forced out of eval mode
        assert not ops.bn_frozen_eligible(marked, xc)
        marked.training = False
        plain = nn.BatchNorm1d(2).cuda().eval()
        assert not ops.union_keys_values_frozen_eligible(xc, convs, [kbs[0], plain], vbs)
        switch = ops.BN_FROZEN
        ops.BN_FROZEN = False
        try:
            assert not ops.bn_frozen_eligible(marked, xc) and not ops.union_keys_values_frozen_eligible(xc, convs, kbs, vbs)
        finally:
            ops.BN_FROZEN = switch
    # the switch and the mark come first, so they are checked where no device is needed too
    switch = ops.BN_FROZEN
    ops.BN_FROZEN = False
    try:
        assert not ops.bn_frozen_eligible(marked.cpu(), x)
    finally:
        ops.BN_FROZEN = switch


def test_bound_rehearsal_on_the_cpu():
    """The elementwise gx bound and the order-free bound on the sums of tests/test_bn_frozen_gpu.py, rehearsed without a device:
    the kernel's operation order restated in fp32 against float64, at that file's rounding shapes, the cancellation case
    included; the mask is the fp32 forward's, as on the device."""
    from tests.test_bn_frozen_gpu import ROUNDING, _float_case, _ref64

    for B, C, N, offset in ROUNDING:
        for relu in (False, True):
            p = _float_case(B, C, N, offset)
            m, w, b = (p[k][None, :, None] for k in ("rm", "w", "b"))
            rs = (1.0 / torch.sqrt(p["rv"] + p["eps"]))[None, :, None]
            xh = (p["x"] - m) * rs
            mask = (xh * w + b > 0) if relu else None
            ref = _ref64(p, mask)
            g = p["gy"] if mask is None else p["gy"] * mask
            assert bool((((g * (w * rs)).double() - ref["gx"]).abs() <= ref["gx_bound"]).all()), (B, C, N, offset, relu)
            assert bool(((g.sum((0, 2)).double() - ref["gb"]).abs() <= ref["gb_bound"]).all()), (B, C, N, offset, relu)
            assert bool((((g * xh).sum((0, 2)).double() - ref["gw"]).abs() <= ref["gw_bound"]).all()), (B, C, N, offset, relu)
