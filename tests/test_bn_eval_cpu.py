"""CPU-side checks of the eval-mode BatchNorm path: the two ct_bn_eval_* symbols are exported and reject bad arguments
before anything touches a device, and ops.bn_eval_eligible keeps CPU tensors, training-mode norms and norms without
running statistics on the modules' own path."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def test_symbols_are_exported(lib):
    from cloud_transformers_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ct_bn_eval_supported", "ct_bn_eval_group_fwd"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.ct_bn_eval_supported(6, 48, 8192) == 1
    assert lib.ct_bn_eval_supported(1, 3, 1) == 1                # one value per channel: legal without a variance
    assert lib.ct_bn_eval_supported(2, 3, 1001) == 1
    assert lib.ct_bn_eval_supported(0, 3, 8) == 0 and lib.ct_bn_eval_supported(2, 0, 8) == 0 and lib.ct_bn_eval_supported(2, 3, 0) == 0
    assert lib.ct_bn_eval_supported(1 << 16, 3, 1 << 15) == 0   # B*N = 2^31


def test_argument_checks_without_gpu(lib):
    from cloud_transformers_amd import _lib
    buf = ctypes.create_string_buffer(64)                        # never dereferenced: every call below is refused first
    p = ctypes.cast(buf, ctypes.c_void_p).value
    B, C, N = 2, 8, 64

    def call(x=p, xbs=0, w=p, b=p, rm=p, rv=p, res=None, rbs=0, y=p, ybs=0, B=B, N=N):
        it = _lib.BnFwdItem(x=x, x_batch_stride=xbs, weight=w, bias=b, running_mean=rm, running_var=rv, residual=res,
                            residual_batch_stride=rbs, y=y, y_batch_stride=ybs, C=C, eps=1e-5, relu=1)
        return lib.ct_bn_eval_group_fwd(ctypes.addressof(it), 1, B, N, None)

    assert call(x=None) == -1 and call(w=None) == -1 and call(b=None) == -1 and call(y=None) == -1
    assert call(rm=None) == -1 and call(rv=None) == -1 and call(rm=None, rv=None) == -1
    assert call(xbs=C * N - 1) == -1 and call(ybs=C * N - 1) == -1 and call(res=p, rbs=C * N - 1) == -1
    assert call(B=0) == -1 and call(N=0) == -1 and call(B=-1) == -1
    items = (_lib.BnFwdItem * 9)()
    for e in items:
        e.x = e.weight = e.bias = e.running_mean = e.running_var = e.y = p
        e.C, e.eps, e.relu = C, 1e-5, 1
    addr = ctypes.addressof(items)
    assert lib.ct_bn_eval_group_fwd(None, 2, B, N, None) == -1
    assert lib.ct_bn_eval_group_fwd(addr, 0, B, N, None) == -1
    assert lib.ct_bn_eval_group_fwd(addr, 9, B, N, None) == -1
    assert lib.ct_bn_eval_group_fwd(addr, 2, 0, N, None) == -1
    items[1].y_batch_stride = C * N - 1
    assert lib.ct_bn_eval_group_fwd(addr, 2, B, N, None) == -1
    items[1].y_batch_stride = 0
    items[1].running_mean = None
    assert lib.ct_bn_eval_group_fwd(addr, 2, B, N, None) == -1


def test_bn_eval_eligible_is_false_off_the_fused_path():
    from cloud_transformers_amd import ops
    x = torch.zeros(2, 8, 64)
    with torch.no_grad():
        assert not ops.bn_eval_eligible(torch.nn.BatchNorm1d(8).eval(), x)                       # a CPU tensor
        if torch.cuda.is_available():
            xc = x.cuda()
            assert ops.bn_eval_eligible(torch.nn.BatchNorm1d(8).cuda().eval(), xc)
            assert not ops.bn_eval_eligible(torch.nn.BatchNorm1d(8).cuda().train(), xc)
            assert not ops.bn_eval_eligible(torch.nn.BatchNorm1d(8, track_running_stats=False).cuda().eval(), xc)
    # the norm's own conditions, checked where no device is needed
    with torch.no_grad():
        assert not ops._bn_eval_norm_ok(torch.nn.BatchNorm1d(8).train(), 2, 8, 64)
        assert not ops._bn_eval_norm_ok(torch.nn.BatchNorm1d(8, track_running_stats=False).eval(), 2, 8, 64)
        assert not ops._bn_eval_norm_ok(torch.nn.BatchNorm1d(8, affine=False).eval(), 2, 8, 64)
        assert not ops._bn_eval_norm_ok(torch.nn.BatchNorm2d(8).eval(), 2, 8, 64)
        assert not ops._bn_eval_norm_ok(torch.nn.BatchNorm1d(8).eval(), 2, 4, 64)                  # channels of another norm
        assert ops._bn_eval_norm_ok(torch.nn.BatchNorm1d(8).eval(), 2, 8, 64)
    # with something to record the forward-only path steps aside
    bn = torch.nn.BatchNorm1d(8).eval()
    assert not ops._records_nothing(x, bn.weight, bn.bias, None)
    with torch.no_grad():
        assert ops._records_nothing(x, bn.weight, bn.bias, None)
    bn.requires_grad_(False)
    assert ops._records_nothing(x, bn.weight, bn.bias, None) and not ops._records_nothing(x.clone().requires_grad_(True), bn.weight)


def test_bound_rehearsal_on_the_cpu():
    """The 2^-20 bound of tests/test_bn_eval_gpu.py, rehearsed without a device: torch's fp32 F.batch_norm(training=False)
    against float64 holds it at that file's shapes, and so does the kernel's operation order restated in fp32
    (((x - m) * rstd) * w + b, one rounding each), the cancellation case included — where the x * scale + shift form of
    the same affine misses it by two orders of magnitude, which is what the case is there to catch."""
    import torch.nn.functional as F
    from tests.test_bn_eval_gpu import CASES, _norm, _ref64

    def worst(y, ref, bound):
        return float(((y.double() - ref).abs() / bound.clamp_min(1e-300)).max())

    for B, C, N, relu, with_res, offset in CASES:
        torch.manual_seed(B * 100 + C)
        bn = _norm(C, B * 100 + C, offset)
        x = bn.running_mean[None, :, None] + torch.randn(B, C, N) if offset else torch.randn(B, C, N) * 3 + 0.7
        res = torch.randn(B, C, N) if with_res else None
        ref, bound = _ref64(bn, x, relu, res)
        m, v, w, b = bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach()

        def finish(y):
            y = torch.relu(y) if relu else y
            return y if res is None else y + res

        rstd = 1.0 / torch.sqrt(v + bn.eps)
        ordered = finish(((x - m[None, :, None]) * rstd[None, :, None]) * w[None, :, None] + b[None, :, None])
        assert worst(ordered, ref, bound) <= 1.0, (B, C, N, offset)
        scale = w * rstd
        folded = finish(x * scale[None, :, None] + (b - m * scale)[None, :, None])
        if offset:
            assert worst(folded, ref, bound) > 10.0                # the form the issue rules out is caught
        else:
            assert worst(finish(F.batch_norm(x, m, v, w, b, False, 0.0, bn.eps)), ref, bound) <= 1.0, (B, C, N)
