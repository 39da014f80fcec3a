"""CPU-side checks of the norms-in-the-Slice-write-out path: ct_slice_fwd_norm / ct_mhct_core_fwd_norm and their length queries
are declared in include/cloudct.h and bound in _lib.py with the same number of arguments, bad arguments are refused before
anything touches a device, the switch ops.SLICE_NORM is off unless CLOUDCT_SLICE_NORM=1, and ops.slice_norm_eligible keeps CPU
tensors, training-mode norms and recorded gradients on the old path."""
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
    for name, arity in (("ct_slice_fwd_norm", 13), ("ct_slice_fwd_norm_amax_len", 6), ("ct_mhct_core_fwd_norm", 20),
                        ("ct_mhct_core_fwd_norm_amax_len", 6)):
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(raw, name)
    # the fused entry points take the plain ones' arguments with `out` replaced by (norm, amax_out)
    assert len(_lib.SIGNATURES["ct_slice_fwd_norm"][1]) == len(_lib.SIGNATURES["ct_slice_fwd"][1]) + 1
    assert len(_lib.SIGNATURES["ct_mhct_core_fwd_norm"][1]) == len(_lib.SIGNATURES["ct_mhct_core_fwd"][1]) + 1


def test_length_queries_count_the_workgroups_of_the_plain_plan(lib):
    from cloud_transformers_amd import _lib
    W2, W3 = _lib.int_array((32, 32)), _lib.int_array((8, 8, 8))
    q = lib.ct_slice_fwd_norm_amax_len
    try:
        # one channel chunk per plane, the cloud cut towards one workgroup per CU (N / split >= 256)
        lib.ct_debug_set_flags(_lib.DEBUG_FORCE_HOT)
        assert q(2, 2, 8, 1024, 2, W2) == 2 * 2 * 4
        assert q(2, 2, 8, 1024, 3, W3) == 2 * 2 * 2 * 4                                  # 3D, few planes: two chunks of four channels
        assert q(2, 2, 16, 1024, 2, _lib.int_array((64, 64))) == 2 * 2 * 4 * 4          # four chunks of four channels
        lib.ct_debug_set_flags(_lib.DEBUG_NO_HOT)
        assert q(2, 2, 8, 1024, 2, W2) == 2 * 2 * 8 * 4                                  # few planes: single-channel chunks
        lib.ct_debug_set_flags(0)
        assert q(2, 1, 3, 2048, 2, _lib.int_array((256, 256))) == 2 * 8                  # the tile stays in memory: one chunk, N in eight
        assert q(2, 2, 5, 1022, 2, W2) == 2 * 2 * 5 * 2                                  # 1022 / 4 < 256: N in two
        assert q(0, 2, 8, 1024, 2, W2) == 0 and q(2, 2, 8, 1024, 4, W2) == 0 and q(2, 2, 8, 1024, 2, None) == 0
        assert q(4096, 16, 4, 1024, 2, W2) == 0                                          # 65536 planes: more than a GEMM folds
    finally:
        lib.ct_debug_set_flags(0)
    qc = lib.ct_mhct_core_fwd_norm_amax_len
    W16 = _lib.int_array((16, 16))
    try:
        for S in (1, 2, 4):
            lib.ct_debug_set_core(S << 8)
            assert qc(2, 4, 16, 2048, 2, W16) == 2 * 4 * S and qc(2, 4, 32, 2048, 3, W3) == 2 * 4 * S
        assert qc(2, 4, 8, 2048, 2, W16) == 0 and qc(2, 4, 16, 2046, 2, W16) == 0         # not a core shape
    finally:
        lib.ct_debug_set_core(0)


def _item(p, C, **kw):
    from cloud_transformers_amd import _lib
    it = _lib.BnFwdItem()
    it.weight = it.bias = it.running_mean = it.running_var = it.y = p
    it.C, it.eps, it.relu = C, 1e-5, 1
    for k, v in kw.items():
        setattr(it, k, v)
    return it


def test_argument_checks_without_gpu(lib):
    from cloud_transformers_amd import _lib
    buf = ctypes.create_string_buffer(64)                        # never dereferenced: every call below is refused first
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    B, H, C, N = 2, 2, 8, 1024

    def call(keys=p, grid=p, pad=None, pad_dtype=0, amax=None, B=B, H=H, C=C, N=N, dim=2, W=(32, 32), no_item=False, item_C=16, **kw):
        it = _item(p, item_C, **kw)
        return lib.ct_slice_fwd_norm(keys, grid, pad, pad_dtype, None if no_item else ctypes.addressof(it), amax, B, H, C, N, dim,
                                     None if W is None else _lib.int_array(W), None)

    assert call(keys=None) == -1 and call(grid=None) == -1 and call(no_item=True) == -1 and call(W=None) == -1
    assert call(y=None) == -1 and call(weight=None) == -1 and call(bias=None) == -1
    assert call(running_mean=None) == -1 and call(running_var=None) == -1
    assert call(C=15) == -1 and call(H=1) == -1                                           # norm->C != H*C
    assert call(eps=-1.0) == -1 and call(eps=float("nan")) == -1
    assert call(y_batch_stride=16 * N - 4) == -1 and call(y_batch_stride=-1) == -1
    assert call(residual=p) == -1 and call(amax_out=p) == -1
    assert call(pad=None, pad_dtype=1) == -1 and call(pad=p, pad_dtype=7) == -1 and call(dim=4) == -1 and call(N=0) == -1
    # maxima only where the launch is the one the query planned (16-byte aligned tensors and stride) and the length is not 0
    assert call(amax=p, keys=p + 4) == -1 and call(amax=p, y=p + 4) == -1 and call(amax=p, grid=p + 4) == -1
    assert call(amax=p, y_batch_stride=16 * N + 2) == -1 and call(amax=p + 2) == -1
    assert lib.ct_slice_fwd_norm_amax_len(4096, 16, 4, N, 2, _lib.int_array((32, 32))) == 0
    assert call(amax=p, B=4096, H=16, C=4, item_C=64) == -1                               # more partials than a GEMM folds

    def core(keys=p, feat=p, w=p, amax=None, ws=p, ws_bytes=1 << 30, C=16, N=2048, W=(16, 16), no_item=False, pad=None, pad_dtype=0, **kw):
        it = _item(p, 4 * C, **kw)
        return lib.ct_mhct_core_fwd_norm(keys, feat, pad, pad_dtype, w, None, None if no_item else ctypes.addressof(it), amax, None, None,
                                         None, ws, ws_bytes, 2, 4, C, N, len(W), _lib.int_array(W), None)

    assert core(keys=None) == -1 and core(feat=None) == -1 and core(w=None) == -1 and core(no_item=True) == -1
    assert core(y=None) == -1 and core(weight=None) == -1 and core(bias=None) == -1
    assert core(running_mean=None) == -1 and core(running_var=None) == -1 and core(C=64) == -1
    assert core(eps=-1.0) == -1 and core(eps=float("nan")) == -1 and core(residual=p) == -1 and core(amax_out=p) == -1
    assert core(y_batch_stride=64 * 2048 - 4) == -1 and core(y_batch_stride=64 * 2048 + 2) == -1
    assert core(y=p + 4) == -1 and core(keys=p + 4) == -1 and core(amax=p + 2) == -1
    assert core(C=8, W=(16, 16)) == -1 and core(N=2046) == -1 and core(pad_dtype=1) == -1      # what ct_mhct_core_fwd refuses
    assert core(ws=None) == -3 and core(ws_bytes=16) == -3                                      # CT_EWORKSPACE, as the plain entry point


def test_switch_is_off_by_default_and_eligibility_is_false_off_the_fused_path():
    from cloud_transformers_amd import ops
    assert os.environ.get("CLOUDCT_SLICE_NORM", "0") == "1" or ops.SLICE_NORM is False
    keys, grid = torch.zeros(2, 4, 64), torch.zeros(2, 16, 8, 8)
    ev = torch.nn.BatchNorm1d(16).eval()
    with torch.no_grad():
        assert not ops.slice_norm_eligible(ev, keys, grid)                    # the switch is off
    saved = ops.SLICE_NORM
    ops.SLICE_NORM = True
    try:
        with torch.no_grad():
            assert not ops.slice_norm_eligible(ev, keys, grid)                # CPU tensors
            assert not ops.slice_norm_eligible(torch.nn.BatchNorm1d(16).train(), keys, grid)
            assert not ops.slice_norm_plannable(ev, keys, 64) and not ops.slice_norm_plannable(torch.nn.BatchNorm1d(16).train(), keys, 64)
        assert not ops.slice_norm_eligible(ev, keys, grid.clone().requires_grad_(True))
        if not torch.cuda.is_available():
            return
        kc, gc, evc = keys.cuda(), grid.cuda(), torch.nn.BatchNorm1d(16).cuda().eval()
        with torch.no_grad():
            assert ops.slice_norm_eligible(evc, kc, gc) and ops.slice_norm_plannable(evc, kc, 64)
            assert not ops.slice_norm_eligible(torch.nn.BatchNorm1d(16).cuda().train(), kc, gc)            # training mode
            assert not ops.slice_norm_eligible(torch.nn.BatchNorm1d(8).cuda().eval(), kc, gc)              # not the channels of the grid
            assert not ops.slice_norm_eligible(torch.nn.Identity(), kc, gc)                                # not a norm at all
            assert not ops.slice_norm_eligible(torch.nn.BatchNorm1d(16, affine=False).cuda().eval(), kc, gc)
            assert not ops.slice_norm_eligible(evc, torch.zeros(2, 4, 62).cuda(), gc)                      # N % 4
            assert not ops.slice_norm_eligible(evc, torch.zeros(2, 4, 65).cuda()[:, :, 1:], gc)            # not contiguous / aligned
            assert not ops.slice_norm_eligible(evc, kc, gc.double())
            for switch in ("SLICE_NORM", "BN_EVAL"):
                setattr(ops, switch, False)
                try:
                    assert not ops.slice_norm_eligible(evc, kc, gc)
                finally:
                    setattr(ops, switch, True)
        assert not ops.slice_norm_eligible(evc, kc, gc)                       # grad mode on, parameters require grad
        evc.requires_grad_(False)
        assert ops.slice_norm_eligible(evc, kc, gc)
        assert not ops.slice_norm_eligible(evc, kc, gc.clone().requires_grad_(True))       # recorded gradients
        assert not ops.slice_norm_eligible(evc, kc.clone().requires_grad_(True), gc)
    finally:
        ops.SLICE_NORM = saved
