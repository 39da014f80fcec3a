"""CPU-side checks of the norms-in-the-GEMM-epilogue path: ct_pw_gemm_rs_norm and its length query are declared in
include/cloudct.h and bound in _lib.py with the same number of arguments, bad arguments are refused before anything touches a
device, and ops.pw_norm_eligible keeps CPU tensors, training-mode norms, inputs that require grad and ops.PW_NORM = False on
the old path."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def test_symbols_are_declared_and_bound_with_matching_arity(lib):
    from cloud_transformers_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cloudct.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, arity in (("ct_pw_gemm_rs_norm", 17), ("ct_pw_gemm_norm_amax_len", 3)):
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(raw, name)
    assert lib.ct_pw_gemm_norm_amax_len(2, 164, 132) == 8 and lib.ct_pw_gemm_norm_amax_len(8, 512, 4096) == 1024
    assert lib.ct_pw_gemm_norm_amax_len(64, 4096, 4096) == 0 and lib.ct_pw_gemm_norm_amax_len(0, 8, 8) == 0


def test_argument_checks_without_gpu(lib):
    from cloud_transformers_amd import _lib
    buf = ctypes.create_string_buffer(64)                        # never dereferenced: every call below is refused first
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    B, Co, Ci, N = 2, 16, 8, 64

    def call(n=2, w=p, x=p, Co=Co, N=N, **kw):
        items = (_lib.BnFwdItem * 9)()
        for e in items:
            e.weight = e.bias = e.running_mean = e.running_var = e.y = p
            e.C, e.eps, e.relu = 8, 1e-5, 1
        for k, v in kw.items():
            setattr(items[1], k, v)
        return lib.ct_pw_gemm_rs_norm(w, x, ctypes.addressof(items), n, None, None, 0, 0, None, 0, None, 0, B, Co, Ci, N, None)

    assert call(n=0) == -1 and call(n=9) == -1 and call(n=1) == -1 and call(n=3) == -1      # 1, 3: sum of C != Co
    assert call(w=None) == -1 and call(x=None) == -1 and call(w=p + 4) == -1
    assert call(y=None) == -1 and call(weight=None) == -1 and call(bias=None) == -1
    assert call(running_mean=None) == -1 and call(running_var=None) == -1
    assert call(eps=-1.0) == -1 and call(amax_out=p) == -1 and call(C=0) == -1
    assert call(y_batch_stride=8 * N - 4) == -1 and call(residual_batch_stride=8 * N - 4) == -1
    assert call(y_batch_stride=8 * N + 2) == -1 and call(y=p + 4) == -1 and call(residual=p + 4) == -1
    assert call(N=N - 2) == -1 and call(Co=Co + 2) == -1


def test_pw_norm_eligible_is_false_off_the_fused_path():
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers.pointwise import PointwiseConv1d
    conv = PointwiseConv1d(128, 128, kernel_size=1, bias=False)
    x = torch.zeros(2, 128, 64)
    with torch.no_grad():
        assert not ops.pw_norm_eligible(conv, [torch.nn.BatchNorm1d(128).eval()], x)             # a CPU tensor
        assert not ops.pw_norm_eligible(conv, [torch.nn.BatchNorm1d(128).train()], x)
    assert not ops.pw_norm_eligible(conv, [torch.nn.BatchNorm1d(128).eval()], x.clone().requires_grad_(True))
    # the shape and switch rule, which needs no device
    assert ops.PW_NORM and ops.BN_EVAL
    assert ops._pw_norm_takes(128, 128, 64, 1, ops.PW_FWD) and ops._pw_norm_takes(352, 128, 1024, 8, ops.PW_FWD)
    assert not ops._pw_norm_takes(64, 128, 64, 1, ops.PW_FWD) and ops._pw_norm_takes(28, 16, 1024, 2)     # under one row tile
    assert not ops._pw_norm_takes(14, 16, 1024, 2) and not ops._pw_norm_takes(128, 128, 64, 9, ops.PW_FWD)
    assert not ops._pw_norm_takes(128, 128, 64, 0, ops.PW_FWD)
    for switch in ("PW_NORM", "BN_EVAL"):
        setattr(ops, switch, False)
        try:
            assert not ops._pw_norm_takes(128, 128, 64, 1, ops.PW_FWD)
        finally:
            setattr(ops, switch, True)
    if not torch.cuda.is_available():
        return
    conv, xc = conv.cuda(), x.cuda()
    ev = torch.nn.BatchNorm1d(128).cuda().eval()
    halves = [torch.nn.BatchNorm1d(64).cuda().eval(), torch.nn.BatchNorm1d(64).cuda().eval()]
    with torch.no_grad():
        assert ops.pw_norm_eligible(conv, [ev], xc) and ops.pw_norm_eligible(conv, halves, xc)
        assert ops.pw_norm_eligible(conv, [ev], xc, residual=torch.zeros_like(xc))
        assert not ops.pw_norm_eligible(conv, [torch.nn.BatchNorm1d(128).cuda().train()], xc)   # a training-mode norm
        assert not ops.pw_norm_eligible(conv, [torch.nn.Identity()], xc)                         # not a norm at all
        assert not ops.pw_norm_eligible(conv, halves[:1], xc)                                    # norms that do not cover the rows
        assert not ops.pw_norm_eligible(conv, [torch.nn.BatchNorm1d(8).cuda().eval()] * 16, xc)  # more than a table holds
        assert not ops.pw_norm_eligible(PointwiseConv1d(128, 128, kernel_size=1, bias=True).cuda(), [ev], xc)
        assert not ops.pw_norm_eligible(PointwiseConv1d(128, 64, kernel_size=1, bias=False).cuda(), halves[:1], xc)   # under one row tile
        assert ops.pw_norm_eligible(PointwiseConv1d(128, 64, kernel_size=1, bias=False).cuda(), halves[:1], xc, mode=None)
        for switch in ("PW_NORM", "BN_EVAL"):
            setattr(ops, switch, False)
            try:
                assert not ops.pw_norm_eligible(conv, [ev], xc)
            finally:
                setattr(ops, switch, True)
    assert not ops.pw_norm_eligible(conv, [ev], xc)                                              # grad mode on, parameters require grad
    conv.requires_grad_(False)
    ev.requires_grad_(False)
    assert ops.pw_norm_eligible(conv, [ev], xc)
    assert not ops.pw_norm_eligible(conv, [ev], xc.clone().requires_grad_(True))                 # an input that requires grad
    assert not ops.pw_norm_eligible(conv, [ev], xc, residual=torch.zeros_like(xc).requires_grad_(True))
