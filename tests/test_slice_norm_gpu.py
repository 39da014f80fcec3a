"""ct_slice_fwd_norm / ct_mhct_core_fwd_norm: the eval-mode norm (+ ReLU) of a head's sliced features applied in the store of the
kernel that produces them.

The pin: every output element holds exactly the bits of ct_slice_fwd (ct_mhct_core_fwd) into a dense scratch tensor followed by
ct_bn_eval_group_fwd with the same item (torch.equal) — for every gather family ct_slice_fwd can choose (its tag plus "+norm"),
with and without ReLU, into a dense output and into a channel range of a wider tensor whose other channels stay untouched; the
per-workgroup partial maxima fill the queried length and fold to max |y|.  The norm's parameters are drawn so that a folded
scale / shift would show (running means of ~1e3 on some channels, variances from 1e-6 to 10, weights of both signs).  Then the
argument checks, and the routing in ops / layers.multihead_ct: with ops.SLICE_NORM on and off the blocks and the whole segmenter
produce the same bits, with no ct_bn_eval_group_fwd launch left in a union block."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import raster_families as F

pytestmark = pytest.mark.gpu

FILL = 7.0          # what every output holds before a call
EPS = 1e-5


def _libs():
    from cloud_transformers_amd import _lib
    return _lib, _lib.load()


def _norm_params(C, seed):
    """The issue's draws: |running_mean| ~ 1e3 on every third channel, running_var log-uniform over 1e-6 .. 10, weight of mixed
    sign."""
    g = torch.Generator().manual_seed(seed)
    rm = torch.rand(C, generator=g) * 2 - 1
    rm[::3] *= 1e3
    rv = 10.0 ** (torch.rand(C, generator=g) * 7 - 6)
    rv[0], rv[-1] = 1e-6, 10.0
    w = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    w[0], w[-1] = abs(float(w[0])), -abs(float(w[-1]))
    b = torch.rand(C, generator=g) - 0.5
    return dict(w=w.cuda(), b=b.cuda(), rm=rm.cuda(), rv=rv.cuda(), eps=EPS)


def _item(par, C, relu, x, y_view, amax=None):
    """A _bn_eval_item-style dict (ops._bn_fwd_table); x: the dense scratch tensor the reference norm reads, or None."""
    return dict(x=None if x is None else x.data_ptr(), xbs=0, C=C, relu=relu, res=None, rbs=0, y=y_view.data_ptr(),
                ybs=y_view.stride(0), amax=amax, **par)


def _output(B, HC, N, wide):
    """(the tensor that owns the memory, the [B, HC, N] view the call writes): dense, or channels [8, 8 + HC) of [B, HC + 20, N]."""
    if wide:
        owner = torch.full((B, HC + 20, N), FILL, device="cuda")
        return owner, owner[:, 8:8 + HC]
    owner = torch.full((B, HC, N), FILL, device="cuda")
    return owner, owner


# (id, tag, B, H, C, N, W, pad, flags): the issue's cases per family
RASTER_CASES = [
    ("ci_32sq", "gather_ci", 2, 2, 8, 1024, (32, 32), "f32", F.FORCE_HOT),
    ("ci_64sq_chunks", "gather_ci", 2, 2, 16, 1024, (64, 64), None, F.FORCE_HOT),
    ("ci3_8cube", "gather_ci3", 2, 2, 8, 1024, (8, 8, 8), "i32", F.FORCE_HOT),
    ("ci3_16cube_chunks", "gather_ci3", 2, 2, 16, 1024, (16, 16, 16), None, F.FORCE_HOT),
    ("quad_32sq", "gather_quad", 2, 2, 8, 1024, (32, 32), None, F.NO_HOT),
    ("generic_256sq", "gather_generic", 2, 1, 3, 2048, (256, 256), "f32", 0),
    ("generic_c5_n1022", "gather_generic", 2, 2, 5, 1022, (32, 32), None, 0),
]
_raster_cache = {}


def _raster_inputs(case):
    """keys, grid, pad, the norm's parameters and ct_slice_fwd's dense result under the case's flags — computed once per case
    and shared by its four runs, which leave them unchanged."""
    cid, tag, B, H, C, N, W, pad_kind, flags = case
    if cid not in _raster_cache:
        L, lib = _libs()
        from cloud_transformers_amd.ops import _ptr, _stream
        g = torch.Generator().manual_seed(len(cid) * 131 + C)
        keys = torch.tanh(torch.randn(B, H * len(W), N, generator=g)).cuda()
        grid = torch.randn(B, H * C, *W, generator=g).cuda()
        pad, code = None, L.PAD_NONE
        if pad_kind == "f32":
            pad, code = (torch.rand(B, N, generator=g) > 0.25).float().cuda(), L.PAD_F32
        elif pad_kind == "i32":
            pad, code = (torch.rand(B, N, generator=g) > 0.25).to(torch.int32).cuda(), L.PAD_I32
        scratch = torch.full((B, H * C, N), FILL, device="cuda")
        lib.ct_debug_set_flags(flags)
        try:
            rc = lib.ct_slice_fwd(_ptr(keys), _ptr(grid), _ptr(pad), code, _ptr(scratch), B, H, C, N, len(W), L.int_array(W), _stream())
            plain_tag = lib.ct_debug_last_launch().decode()
        finally:
            lib.ct_debug_set_flags(0)
        assert rc == 0 and plain_tag == tag, (rc, plain_tag)
        _raster_cache[cid] = (keys, grid, pad, code, _norm_params(H * C, 17 + C), scratch)
    return _raster_cache[cid]


def _slice_norm(case, keys, grid, pad, code, item, amax):
    L, lib = _libs()
    from cloud_transformers_amd import ops
    cid, tag, B, H, C, N, W, pad_kind, flags = case
    arr = ops._bn_fwd_table([item])
    lib.ct_debug_set_flags(flags)
    try:
        rc = lib.ct_slice_fwd_norm(ops._ptr(keys), ops._ptr(grid), ops._ptr(pad), code, ops._at(arr, 0), ops._ptr(amax), B, H, C, N,
                                   len(W), L.int_array(W), ops._stream())
        got_tag = lib.ct_debug_last_launch().decode()
    finally:
        lib.ct_debug_set_flags(0)
    torch.cuda.synchronize()
    return rc, got_tag


@pytest.mark.parametrize("wide", [False, True], ids=["dense", "wide"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", RASTER_CASES, ids=[c[0] for c in RASTER_CASES])
def test_same_bits_as_slice_followed_by_the_eval_norm(case, relu, wide):
    L, lib = _libs()
    from cloud_transformers_amd import ops
    cid, tag, B, H, C, N, W, pad_kind, flags = case
    keys, grid, pad, code, par, scratch = _raster_inputs(case)
    HC = H * C
    # the reference: ct_bn_eval_group_fwd on ct_slice_fwd's dense result, into the same kind of output
    ref_owner, ref_view = _output(B, HC, N, wide)
    ref_slots = torch.full((HC,), -1.0, device="cuda")
    arr = ops._bn_fwd_table([_item(par, HC, relu, scratch, ref_view, amax=ref_slots.data_ptr())])
    assert lib.ct_bn_eval_group_fwd(ops._at(arr, 0), 1, B, N, ops._stream()) == 0
    # the fused call
    lib.ct_debug_set_flags(flags)
    try:
        n_len = lib.ct_slice_fwd_norm_amax_len(B, H, C, N, len(W), L.int_array(W))
    finally:
        lib.ct_debug_set_flags(0)
    assert 0 < n_len <= 32768
    slots = torch.full((n_len + 4,), -1.0, device="cuda")
    owner, view = _output(B, HC, N, wide)
    rc, got_tag = _slice_norm(case, keys, grid, pad, code, _item(par, HC, relu, None, view), slots)
    assert rc == 0 and got_tag == tag + "+norm", (rc, got_tag)
    assert torch.equal(owner, ref_owner), (cid, float((owner - ref_owner).abs().max()))      # the owners: nothing outside the range is touched
    assert bool((view != FILL).any())
    if wide:
        assert bool((owner[:, :8] == FILL).all()) and bool((owner[:, 8 + HC:] == FILL).all())
    part, tail = slots[:n_len], slots[n_len:]
    print("%s relu=%d: %d partial maxima, fold %.6g; per-channel fold %.6g" % (cid, relu, n_len, float(part.max()), float(ref_slots.max())))
    assert bool((tail == -1.0).all())                                       # nothing written past the queried length
    assert bool(torch.isfinite(part).all()) and bool((part >= 0).all())     # every slot written
    assert torch.equal(part.max(), view.abs().max()) and torch.equal(part.max(), ref_slots.max())


def test_no_maxima_asked_for_gives_the_same_bits():
    case = RASTER_CASES[0]
    cid, tag, B, H, C, N, W, pad_kind, flags = case
    keys, grid, pad, code, par, scratch = _raster_inputs(case)
    outs = []
    for slots in (None, torch.empty(64, device="cuda")):
        owner, view = _output(B, H * C, N, False)
        rc, _ = _slice_norm(case, keys, grid, pad, code, _item(par, H * C, 1, None, view), slots)
        assert rc == 0
        outs.append(owner)
    assert torch.equal(outs[0], outs[1])


def test_unaligned_output_takes_the_generic_kernel_like_slice_fwd():
    """y and its stride enter the alignment test where `out` does: an output 4 bytes off a 16-byte boundary sends ct_slice_fwd to
    the generic kernel, and the norm entry with it — same bits; maxima cannot be asked for there."""
    L, lib = _libs()
    from cloud_transformers_amd import ops
    case = RASTER_CASES[4]
    cid, tag, B, H, C, N, W, pad_kind, flags = case
    keys, grid, pad, code, par, _ = _raster_inputs(case)
    HC = H * C
    flat = torch.full((B * HC * N + 1,), FILL, device="cuda")
    scratch = flat[1:].view(B, HC, N)
    lib.ct_debug_set_flags(flags)
    try:
        assert lib.ct_slice_fwd(ops._ptr(keys), ops._ptr(grid), None, code, ops._ptr(scratch), B, H, C, N, 2, L.int_array(W), ops._stream()) == 0
        assert lib.ct_debug_last_launch().decode() == "gather_generic"
    finally:
        lib.ct_debug_set_flags(0)
    ref = torch.full((B, HC, N), FILL, device="cuda")
    aligned = scratch.clone()
    arr = ops._bn_fwd_table([_item(par, HC, 1, aligned, ref)])
    assert lib.ct_bn_eval_group_fwd(ops._at(arr, 0), 1, B, N, ops._stream()) == 0
    got_flat = torch.full((B * HC * N + 1,), FILL, device="cuda")
    got = got_flat[1:].view(B, HC, N)
    rc, got_tag = _slice_norm(case, keys, grid, pad, code, _item(par, HC, 1, None, got), None)
    assert rc == 0 and got_tag == "gather_generic+norm", (rc, got_tag)
    assert torch.equal(got, ref) and float(got_flat[0]) == FILL
    rc, _ = _slice_norm(case, keys, grid, pad, code, _item(par, HC, 1, None, got), torch.empty(256, device="cuda"))
    assert rc == -1


def test_bad_arguments_are_refused_and_write_nothing():
    L, lib = _libs()
    from cloud_transformers_amd import ops
    case = RASTER_CASES[0]
    cid, tag, B, H, C, N, W, pad_kind, flags = case
    keys, grid, pad, code, par, _ = _raster_inputs(case)
    HC = H * C
    owner, view = _output(B, HC, N, True)
    slots = torch.full((64,), -1.0, device="cuda")
    good = _item(par, HC, 1, None, view)

    def call(item=good, keys_p=keys.data_ptr(), grid_p=grid.data_ptr(), pad_p=pad.data_ptr(), code=code, amax=slots.data_ptr(),
             H=H, C=C, N=N, W=W, no_item=False):
        arr = ops._bn_fwd_table([item])
        rc = lib.ct_slice_fwd_norm(keys_p, grid_p, pad_p, code, None if no_item else ops._at(arr, 0), amax, B, H, C, N, len(W),
                                   L.int_array(W), ops._stream())
        torch.cuda.synchronize()
        return rc, bool((owner == FILL).all()) and bool((slots == -1.0).all())

    def edit(**kw):
        it = dict(good)
        it.update(kw)
        return it

    bad = {
        "no keys": dict(keys_p=None), "no grid": dict(grid_p=None), "no item": dict(no_item=True), "no pad with a dtype": dict(pad_p=None),
        "no y": dict(item=edit(y=None)), "no weight": dict(item=edit(w=None)), "no bias": dict(item=edit(b=None)),
        "no running_mean": dict(item=edit(rm=None)), "no running_var": dict(item=edit(rv=None)),
        "norm C != H*C": dict(item=edit(C=HC - 1)), "H*C != norm C": dict(H=1),
        "negative eps": dict(item=edit(eps=-1e-5)), "nan eps": dict(item=edit(eps=float("nan"))),
        "stride below H*C*N": dict(item=edit(ybs=HC * N - 4)), "negative stride": dict(item=edit(ybs=-4)),
        "residual": dict(item=edit(res=keys.data_ptr())), "per-item amax_out": dict(item=edit(amax=slots.data_ptr())),
        "amax_out, y not 16-byte aligned": dict(item=edit(y=good["y"] + 4)),
        "amax_out, stride not 16-byte aligned": dict(item=edit(ybs=good["ybs"] + 2)),
        "amax_out, keys not aligned": dict(keys_p=keys.data_ptr() + 4), "amax_out not aligned": dict(amax=slots.data_ptr() + 2),
        "bad pad dtype": dict(code=7), "bad dim": dict(W=(32,)), "N = 0": dict(N=0),
    }
    for what, kw in bad.items():
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, (what, rc, untouched)
    lib.ct_debug_set_flags(flags)
    try:
        rc, untouched = call()                               # and the good call goes through
    finally:
        lib.ct_debug_set_flags(0)
    assert rc == 0 and not untouched


# ---- the plane-resident core ----

@pytest.fixture
def core_flags():
    _, lib = _libs()
    yield lib.ct_debug_set_core
    lib.ct_debug_set_core(0)


def _core_call(norm_item, keys, feat, padt, code, w, bias, out, amax, B, H, C, N, dim, W):
    """ct_mhct_core_fwd (out) or ct_mhct_core_fwd_norm (norm_item, amax) on a fresh workspace -> status word"""
    L, lib = _libs()
    from cloud_transformers_amd import ops
    Wa = L.int_array([W] * dim)
    nws = lib.ct_mhct_core_workspace_bytes(B, H, C, N, dim, Wa)
    ws = torch.full((nws,), 0xAB, device="cuda", dtype=torch.uint8)
    L.check(lib.ct_mhct_core_workspace_init(ops._ptr(ws), nws, B, H, C, N, dim, Wa, ops._stream()), "ct_mhct_core_workspace_init")
    occ = torch.full((), -1, device="cuda", dtype=torch.int64)
    if norm_item is None:
        rc = lib.ct_mhct_core_fwd(ops._ptr(keys), ops._ptr(feat), ops._ptr(padt), code, ops._ptr(w), ops._ptr(bias), ops._ptr(out), None,
                                  None, ops._ptr(occ), ops._ptr(ws), nws, B, H, C, N, dim, Wa, ops._stream())
    else:
        arr = ops._bn_fwd_table([norm_item])
        rc = lib.ct_mhct_core_fwd_norm(ops._ptr(keys), ops._ptr(feat), ops._ptr(padt), code, ops._ptr(w), ops._ptr(bias), ops._at(arr, 0),
                                       ops._ptr(amax), None, None, ops._ptr(occ), ops._ptr(ws), nws, B, H, C, N, dim, Wa, ops._stream())
    assert rc == 0, rc
    st = ctypes.c_int(-1)
    L.check(lib.ct_mhct_core_status(ops._ptr(ws), nws, B, H, C, N, dim, Wa, ctypes.byref(st), ops._stream()), "ct_mhct_core_status")
    torch.cuda.synchronize()
    return st.value, int(occ)


@pytest.mark.parametrize("dim,W,C", [(2, 32, 16), (2, 16, 16), (3, 8, 32)])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("pad_kind", [None, "f32"])
def test_core_same_bits_as_the_core_followed_by_the_eval_norm(core_flags, dim, W, C, S, pad_kind):
    from tests.test_mhct_core_gpu import make_inputs
    from cloud_transformers_amd.ops import _pad_args
    L, lib = _libs()
    from cloud_transformers_amd import ops
    core_flags(S << 8)
    B, H, N = 2, 4, 2048
    HC = H * C
    keys, feat, w, bias, _, pad = (None if t is None else t.cuda().contiguous() for t in make_inputs(B, H, C, N, dim, 300 + S, pad_kind))
    padt, code = _pad_args(pad, B, N)
    par = _norm_params(HC, 40 + C + dim)
    scratch = torch.full((B, HC, N), FILL, device="cuda")
    st, occ_ref = _core_call(None, keys, feat, padt, code, w, bias, scratch, None, B, H, C, N, dim, W)
    assert st == 0
    n_len = lib.ct_mhct_core_fwd_norm_amax_len(B, H, C, N, dim, L.int_array([W] * dim))
    assert n_len == B * H * S
    for relu, wide in ((1, False), (0, True)):
        ref_owner, ref_view = _output(B, HC, N, wide)
        arr = ops._bn_fwd_table([_item(par, HC, relu, scratch, ref_view)])
        assert lib.ct_bn_eval_group_fwd(ops._at(arr, 0), 1, B, N, ops._stream()) == 0
        owner, view = _output(B, HC, N, wide)
        slots = torch.full((n_len + 4,), -1.0, device="cuda")
        st, occ = _core_call(_item(par, HC, relu, None, view), keys, feat, padt, code, w, bias, None, slots, B, H, C, N, dim, W)
        assert st == 0 and occ == occ_ref
        assert torch.equal(owner, ref_owner), (relu, wide, float((owner - ref_owner).abs().max()))
        part = slots[:n_len]
        assert bool((slots[n_len:] == -1.0).all()) and bool(torch.isfinite(part).all()) and bool((part >= 0).all())
        assert torch.equal(part.max(), view.abs().max())


# ---- routing: ops and the blocks ----

NEW = ("ct_slice_fwd_norm", "ct_mhct_core_fwd_norm")


def _union_core_and_raster(seed=12):
    """A union block whose first head takes the plane-resident core (16^2, 16 features) and whose second a raster family (8^3, 8
    features: 32 planes at B2, the channel-interleaved gather)."""
    from cloud_transformers_amd.layers.multihead_ct import MultiHeadUnion
    from tests.test_eval_blocks_gpu import _randomise_norms
    torch.manual_seed(seed)
    blk = MultiHeadUnion(128, [16, 8], [16, 8], [2, 3], [16, 16]).cuda().eval()
    return _big_means(_randomise_norms(blk, seed + 1))


def _big_means(module):
    """The heads' `after` norms (`after.0` of a MultiHead: the norm on its Slice output) with the issue's draws on top of
    _randomise_norms: means of ~1e3 on some channels, variances from 1e-6 to 10, weights of both signs."""
    from torch import nn
    with torch.no_grad():
        for name, m in module.named_modules():
            if isinstance(m, nn.BatchNorm1d) and (name == "after.0" or name.endswith(".after.0")):
                par = _norm_params(m.num_features, 5 + m.num_features)
                m.running_mean.copy_(par["rm"])
                m.running_var.copy_(par["rv"])
                m.weight.copy_(par["w"])
    return module


def _on_off(run):
    """(result with ops.SLICE_NORM on, its call counts; the same with it off)."""
    from cloud_transformers_amd import ops
    from tests.test_pw_norm_gpu import _Calls
    assert ops.BN_EVAL and ops.PW_NORM
    saved, out = ops.SLICE_NORM, []
    try:
        for switch in (True, False):
            ops.SLICE_NORM = switch
            with torch.no_grad(), _Calls("ct_bn_eval_group_fwd", *NEW) as c:
                res = run()
            out += [res, c.n]
    finally:
        ops.SLICE_NORM = saved
    return out


def test_union_block_same_bits_and_no_norm_launch():
    from tests.test_eval_blocks_gpu import _inputs
    blk = _union_core_and_raster()
    x, pcd = _inputs(2, 128, 1024)
    on, n_on, off, n_off = _on_off(lambda: blk(x, pcd)[0])
    assert n_on == {"ct_bn_eval_group_fwd": 0, "ct_slice_fwd_norm": 1, "ct_mhct_core_fwd_norm": 1}, n_on
    assert n_off == {"ct_bn_eval_group_fwd": 1, "ct_slice_fwd_norm": 0, "ct_mhct_core_fwd_norm": 0}, n_off      # today's: the join
    assert torch.equal(on, off)
    assert bool(torch.isfinite(on).all())


def test_union_join_carries_partials_of_one_maximum():
    """The concatenation the heads' launches fill is tagged with ONE 1-D buffer whose fold is max |joined| — the scale the
    projection that reads it would get from ct_amax_f32."""
    from cloud_transformers_amd import ops
    from tests.test_eval_blocks_gpu import _inputs
    blk = _union_core_and_raster()
    x, pcd = _inputs(2, 128, 1024)
    seen = []
    real = blk._slice_norm_join
    blk._slice_norm_join = lambda targets, pres: seen.append(real(targets, pres)) or seen[-1]
    saved = ops.SLICE_NORM
    ops.SLICE_NORM = True
    try:
        with torch.no_grad():
            blk(x, pcd)
    finally:
        ops.SLICE_NORM = saved
        del blk._slice_norm_join
    joined = seen[0]
    tag = joined._ct_amax[0]
    assert tag.dim() == 1 and joined._ct_amax[1] == joined._version
    assert bool(torch.isfinite(tag).all()) and bool((tag >= 0).all()) and torch.equal(tag.max(), joined.abs().max())


def test_single_head_same_bits_and_no_norm_launch():
    from cloud_transformers_amd.layers.multihead_ct import MultiHead
    from tests.test_eval_blocks_gpu import _inputs, _randomise_norms
    torch.manual_seed(3)
    blk = _big_means(_randomise_norms(MultiHead(16, 4, 16, 8, 2, 4).cuda().eval(), 4))
    x, pcd = _inputs(2, 16, 1024)
    on, n_on, off, n_off = _on_off(lambda: blk(x, pcd)[0])
    assert n_on == {"ct_bn_eval_group_fwd": 0, "ct_slice_fwd_norm": 1, "ct_mhct_core_fwd_norm": 0}, n_on
    assert n_off == {"ct_bn_eval_group_fwd": 1, "ct_slice_fwd_norm": 0, "ct_mhct_core_fwd_norm": 0}, n_off      # today's: `after`
    assert torch.equal(on, off)
    tag = on._ct_amax[0]
    assert tag.dim() == 1 and torch.equal(tag.max(), on.abs().max())


def test_with_gradients_or_in_training_the_new_entry_points_are_never_called():
    from cloud_transformers_amd import ops
    from tests.test_eval_blocks_gpu import _inputs
    from tests.test_pw_norm_gpu import _Calls
    blk = _union_core_and_raster()
    x, pcd = _inputs(2, 128, 1024)
    saved = ops.SLICE_NORM
    ops.SLICE_NORM = True
    try:
        with _Calls(*NEW) as c:
            out, _ = blk(x.clone().requires_grad_(True), pcd)          # eval mode, gradients recorded
            assert out.requires_grad
            blk(x, pcd)                                                # eval mode, parameters that require grad
            blk.train()
            with torch.no_grad():
                blk(x, pcd)                                            # training mode
            blk.eval()
            ops.BN_EVAL = False
            try:
                with torch.no_grad():
                    blk(x, pcd)                                        # the eval kernels switched off
            finally:
                ops.BN_EVAL = True
        assert c.n == {k: 0 for k in NEW}, c.n
    finally:
        ops.SLICE_NORM = saved


def test_eval_forward_replays_from_a_captured_graph_with_forked_heads():
    from cloud_transformers_amd import ops
    from tests.test_eval_blocks_gpu import _inputs
    from tests.test_pw_norm_gpu import _Calls
    blk = _union_core_and_raster()
    x, pcd = _inputs(2, 128, 1024)
    saved = ops.SLICE_NORM
    ops.SLICE_NORM = True
    try:
        with torch.no_grad():
            want = blk(x, pcd)[0].clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    blk(x, pcd)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with _Calls("ct_bn_eval_group_fwd", *NEW) as c:
                with torch.cuda.graph(g):               # (the heads run on forked streams while capturing: HEAD_STREAMS "auto")
                    out = blk(x, pcd)[0]
            assert c.n == {"ct_bn_eval_group_fwd": 0, "ct_slice_fwd_norm": 1, "ct_mhct_core_fwd_norm": 1}, c.n
            for _ in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, want)
    finally:
        ops.SLICE_NORM = saved


def test_whole_segmenter_same_bits_with_the_switch_on_and_off():
    from tests.test_zoo_gpu import _model
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zoo_segmenter_forward.npz"))
    net = _model(int(gold["seed"])).eval()
    cloud = torch.from_numpy(gold["cloud"]).cuda()
    on, n_on, off, n_off = _on_off(lambda: net(cloud))
    assert n_on["ct_slice_fwd_norm"] + n_on["ct_mhct_core_fwd_norm"] > 0 and n_off["ct_slice_fwd_norm"] + n_off["ct_mhct_core_fwd_norm"] == 0
    assert n_on["ct_bn_eval_group_fwd"] < n_off["ct_bn_eval_group_fwd"], (n_on, n_off)
    assert torch.equal(on, off)
