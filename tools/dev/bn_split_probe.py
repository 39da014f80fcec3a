"""Training BatchNorm forward / backward at B8 N4096 for the channel counts of the blocks: the one-workgroup-per-channel kernels
(ct_bn_group_fwd / _bwd on a table of one norm) against the split statistics + apply kernels (ct_bn_group_stats_fwd +
ct_bn_group_apply_fwd, ct_bn_group_reduce_bwd + ct_bn_group_apply_bwd on the same table, as the SyncBatchNorm path uses them,
with world = 1); us per call, HIP events."""
import os, sys, ctypes
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from cloud_transformers_amd import _lib
from cloud_transformers_amd.ops import _ptr, _stream
lib = _lib.load()
def t(fn, iters=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3
B, N = 8, 4096
for C in (32, 48, 64, 128, 256, 512, 768, 1024):
    x = torch.randn(B, C, N, device="cuda"); y = torch.empty_like(x); gy = torch.randn_like(x); gx = torch.empty_like(x)
    w = torch.rand(C, device="cuda") + 0.5; b = torch.randn(C, device="cuda")
    rm = torch.zeros(C, device="cuda"); rv = torch.ones(C, device="cuda"); nbt = torch.zeros(1, device="cuda", dtype=torch.int64)
    mean = torch.empty(C, device="cuda"); rstd = torch.empty(C, device="cuda")
    gw = torch.empty(C, device="cuda"); gb = torch.empty(C, device="cuda")
    loc = torch.empty(2 * C + 1, device="cuda"); cnt = torch.empty(1, device="cuda")
    sums = torch.empty(2 * C, device="cuda")
    fi = _lib.BnFwdItem(x=_ptr(x), weight=_ptr(w), bias=_ptr(b), running_mean=_ptr(rm), running_var=_ptr(rv), num_batches_tracked=_ptr(nbt),
                        y=_ptr(y), save_mean=_ptr(mean), save_rstd=_ptr(rstd), C=C, eps=1e-5, momentum=0.1, relu=1)
    bi = _lib.BnBwdItem(x=_ptr(x), weight=_ptr(w), bias=_ptr(b), save_mean=_ptr(mean), save_rstd=_ptr(rstd), gy=_ptr(gy), gx=_ptr(gx),
                        g_weight=_ptr(gw), g_bias=_ptr(gb), C=C, relu=1)
    fa, ba = ctypes.addressof(fi), ctypes.addressof(bi)
    one_f = lambda: _lib.check(lib.ct_bn_group_fwd(fa, 1, B, N, _stream()), "f")
    one_b = lambda: _lib.check(lib.ct_bn_group_bwd(ba, 1, B, N, _stream()), "b")
    def split_f():
        _lib.check(lib.ct_bn_group_stats_fwd(fa, 1, 0, 1, B, N, _ptr(loc), _stream()), "s")
        _lib.check(lib.ct_bn_group_apply_fwd(fa, 1, 0, 1, B, N, _ptr(loc), 1, _ptr(cnt), _stream()), "a")
    def split_b():
        _lib.check(lib.ct_bn_group_reduce_bwd(ba, 1, 0, 1, B, N, _ptr(sums), None, _stream()), "r")
        _lib.check(lib.ct_bn_group_apply_bwd(ba, 1, 0, 1, B, N, _ptr(sums), _ptr(cnt), _stream()), "ab")
    of, ob = t(one_f), t(one_b)
    y1 = y.clone(); gx1 = gx.clone()
    sf, sb = t(split_f), t(split_b)
    mb = B * C * N * 4 / 1e6
    print("C%4d (%5.1f MB): one kernel fwd %5.1f bwd %5.1f us | split fwd %5.1f bwd %5.1f us | max diff y %.1e gx %.1e" % (
        C, mb, of, ob, sf, sb, float((y - y1).abs().max()), float((gx - gx1).abs().max())), flush=True)
