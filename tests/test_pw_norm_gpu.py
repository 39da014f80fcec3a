"""ct_pw_gemm_rs_norm: the eval-mode norms of a pointwise projection applied in the GEMM's epilogue.

The pin: every output holds exactly the bits of ct_pw_gemm_rs into a scratch tensor followed by ct_bn_eval_group_fwd with the
same items (torch.equal), at a shape whose item boundaries fall inside MFMA blocks, wave blocks and across the row tile; the
fold of the per-workgroup partial maxima equals the fold of the reference's per-channel maxima.  Then: a float64 sanity
check under the GEMM's bound of tests/test_pw_gemm_gpu.py carried through the affine plus the affine's own bound of
tests/test_bn_eval_gpu.py; the argument checks; and the routing in ops / layers.multihead_ct — with ops.PW_NORM on and off
the blocks and the whole segmenter produce the same bits, with one ct_bn_eval_group_fwd launch per union block instead of
three."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, CI, CO, N = 2, 40, 164, 132            # two row tiles (the second: 36 rows), two column tiles (4 columns), a partial last K-step
FILL = 7.0                                # what every output holds before a call


def _params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(w=(torch.rand(C, generator=g) + 0.5).cuda(), b=(torch.rand(C, generator=g) - 0.5).cuda(),
                rm=(torch.rand(C, generator=g) * 2 - 1).cuda(), rv=(torch.rand(C, generator=g) * 1.5 + 0.5).cuda(), eps=1e-5)


def _operands(seed=1, Co=CO):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(Co, CI, generator=g) / CI ** 0.5).cuda()
    x = torch.randn(B, CI, N, generator=g).cuda()
    return W, x


class _Case:
    """The items of one call: per item its parameters, relu, an output (contiguous, or a channel range of a wider tensor) and
    an optional residual (contiguous, or a channel slice of a wider tensor)."""

    def __init__(self, Cs, relus, wide_y=None, res=None, res_slice=None, seed=3):
        g = torch.Generator().manual_seed(seed)
        self.Cs, self.relus = Cs, relus
        self.par = [_params(C, seed * 10 + i) for i, C in enumerate(Cs)]
        self.wide_y, self.res = wide_y, {}
        for i in (res or ()):
            self.res[i] = torch.randn(B, Cs[i], N, generator=g).cuda()
        for i in (res_slice or ()):
            self.res[i] = torch.randn(B, Cs[i] + 8, N, generator=g).cuda()[:, 8:]

    def outputs(self):
        """(the tensors that own the memory, the [B, C, N] views the items write)."""
        owners, views = [], []
        for i, C in enumerate(self.Cs):
            if i == self.wide_y:
                t = torch.full((B, C + 12, N), FILL, device="cuda")
                owners.append(t)
                views.append(t[:, 4:4 + C])
            else:
                t = torch.full((B, C, N), FILL, device="cuda")
                owners.append(t)
                views.append(t)
        return owners, views

    def items(self, views, x=None, amax=None):
        """_bn_eval_item-style dicts; x: the [B, Co, N] tensor whose channel ranges the reference norms read."""
        out, c0 = [], 0
        for i, (C, v) in enumerate(zip(self.Cs, views)):
            r = self.res.get(i)
            out.append(dict(x=None if x is None else x.data_ptr() + c0 * N * 4, xbs=0 if x is None else x.size(1) * N, C=C,
                            relu=self.relus[i], res=None if r is None else r.data_ptr(), rbs=0 if r is None else r.stride(0),
                            y=v.data_ptr(), ybs=v.stride(0), amax=None if amax is None else amax.data_ptr() + 4 * c0,
                            **self.par[i]))
            c0 += C
        return out


CASES = {
    "plain": lambda: _Case((6, 22, 36, 100), (1, 0, 1, 0)),
    "relu_swapped": lambda: _Case((6, 22, 36, 100), (0, 1, 0, 1)),
    "wide_y": lambda: _Case((6, 22, 36, 100), (1, 0, 1, 1), wide_y=2),
    "residual_slice": lambda: _Case((6, 22, 36, 100), (1, 1, 0, 1), res=(1,), res_slice=(3,)),
    "n1": lambda: _Case((164,), (1,), res=(0,)),
    "n8": lambda: _Case((6, 22, 36, 4, 8, 40, 44, 4), (1, 0, 1, 0, 1, 1, 0, 1), wide_y=5, res=(2,), res_slice=(6,)),
}


def _fused(W, x, items, want_amax=True, n=None, Co=None, amax_a="rows"):
    from cloud_transformers_amd import _lib, ops
    lib = _lib.load()
    Co = W.size(0) if Co is None else Co
    am_w = ops.prep_weight(W, False)[0][0] if amax_a == "rows" else ops.amax(W)
    am_x = ops.amax(x)
    n_out = lib.ct_pw_gemm_norm_amax_len(B, Co, N)
    slots = torch.full((n_out,), -1.0, device="cuda") if want_amax else None
    arr = ops._bn_fwd_table(items)
    rc = lib.ct_pw_gemm_rs_norm(W.data_ptr(), x.data_ptr(), ops._at(arr, 0), len(items) if n is None else n,
                                None if slots is None else slots.data_ptr(), am_w.data_ptr(), am_w.numel(),
                                ops._rows_of(am_w, Co), am_x.data_ptr(), am_x.numel(), None, 0, B, Co, CI, N, ops._stream())
    return rc, slots


def _reference(W, x, case):
    """ct_pw_gemm_rs into a scratch tensor, then ct_bn_eval_group_fwd with the same items."""
    from cloud_transformers_amd import _lib, ops
    lib = _lib.load()
    scratch = ops.pw_gemm(ops.PW_FWD, W, x, ops.prep_weight(W, False)[0][0], ops.amax(x), B, CO, CI, N)
    owners, views = case.outputs()
    slots = torch.full((CO,), -1.0, device="cuda")
    arr = ops._bn_fwd_table(case.items(views, x=scratch, amax=slots))
    assert lib.ct_bn_eval_group_fwd(ops._at(arr, 0), len(case.Cs), B, N, ops._stream()) == 0
    return owners, views, slots, scratch


@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bits_as_the_gemm_followed_by_the_eval_norm(name):
    from cloud_transformers_amd import _lib
    assert _lib.load().ct_pw_gemm_norm_amax_len(B, CO, N) == 2 * 2 * B
    W, x = _operands()
    case = CASES[name]()
    ref_owners, _, ref_slots, _ = _reference(W, x, case)
    owners, views = case.outputs()
    rc, slots = _fused(W, x, case.items(views))
    torch.cuda.synchronize()
    assert rc == 0
    for i, (got, want) in enumerate(zip(owners, ref_owners)):            # the owners: nothing outside a channel range is touched
        assert torch.equal(got, want), (name, i, float((got - want).abs().max()))
    assert all(bool((v != FILL).any()) for v in views)
    fold = float(slots.max())
    print("%s: fold of %d partial maxima %.6f, of %d per-channel maxima %.6f" % (name, slots.numel(), fold, CO, float(ref_slots.max())))
    assert bool((slots >= 0).all()) and fold == float(ref_slots.max()) == max(float(v.abs().max()) for v in views)


def test_per_tensor_weight_maxima_and_no_amax_out_give_the_same_bits():
    """rows_a = 0 (partials of one maximum for W) and amax_out = NULL are the same epilogue."""
    from cloud_transformers_amd import ops
    W, x = _operands(seed=4)
    case = CASES["plain"]()
    scratch = ops.pw_gemm(ops.PW_FWD, W, x, ops.amax(W), ops.amax(x), B, CO, CI, N)
    ref_owners, ref_views = case.outputs()
    ops._bn_eval_group(case.items(ref_views, x=scratch), B, N)
    owners, views = case.outputs()
    rc, _ = _fused(W, x, case.items(views), want_amax=False, amax_a="tensor")
    assert rc == 0
    for got, want in zip(owners, ref_owners):
        assert torch.equal(got, want)


def test_matches_float64_within_the_gemm_bound_carried_through_the_affine():
    """|err| <= BOUND * (|W| |x|) * rstd * |w|  (the GEMM's bound of tests/test_pw_gemm_gpu.py, through the affine's slope)
                + 2^-20 * (|v - m| * rstd * |w| + |b| + |res|)  (the affine's own bound of tests/test_bn_eval_gpu.py)."""
    from tests.test_pw_gemm_gpu import BOUND
    W, x = _operands(seed=2)
    case = CASES["residual_slice"]()
    owners, views = case.outputs()
    rc, _ = _fused(W, x, case.items(views))
    assert rc == 0
    Wd, xd = W.double().cpu(), x.double().cpu()
    v, mag = torch.matmul(Wd, xd), torch.matmul(Wd.abs(), xd.abs())
    c0 = 0
    for i, (C, y) in enumerate(zip(case.Cs, views)):
        p = {k: (t.double().cpu()[None, :, None] if torch.is_tensor(t) else t) for k, t in case.par[i].items()}
        rstd = 1.0 / torch.sqrt(p["rv"] + p["eps"])
        vi = v[:, c0:c0 + C]
        ref = (vi - p["rm"]) * rstd * p["w"] + p["b"]
        bound = BOUND * mag[:, c0:c0 + C] * rstd * p["w"].abs() + 2.0 ** -20 * ((vi - p["rm"]).abs() * rstd * p["w"].abs() + p["b"].abs())
        if case.relus[i]:
            ref = torch.relu(ref)
        if i in case.res:
            r = case.res[i].double().cpu()
            ref, bound = ref + r, bound + 2.0 ** -20 * r.abs()
        err = (y.double().cpu() - ref).abs()
        print("item %d: max |err| %.3e, worst err / bound %.3f" % (i, float(err.max()), float((err / bound).max())))
        assert bool((err <= bound).all()), (i, float(err.max()), float((err / bound).max()))
        c0 += C


def test_bad_arguments_are_refused_and_write_nothing():
    from cloud_transformers_amd import _lib, ops
    lib = _lib.load()
    W, x = _operands()
    case = CASES["residual_slice"]()
    owners, views = case.outputs()
    good = case.items(views)
    slots_len = lib.ct_pw_gemm_norm_amax_len(B, CO, N)

    def call(items=good, n=None, w=W.data_ptr(), xp=x.data_ptr(), Co=CO, Nn=N, rows_a=CO, per_item_amax=None, want_amax=True):
        am_w, am_x = ops.prep_weight(W, False)[0][0], ops.amax(x)
        slots = torch.full((slots_len,), -1.0, device="cuda")
        items = [dict(it) for it in items]
        if per_item_amax is not None:
            items[0]["amax"] = per_item_amax
        arr = ops._bn_fwd_table(items)
        rc = lib.ct_pw_gemm_rs_norm(w, xp, ops._at(arr, 0), len(items) if n is None else n, slots.data_ptr() if want_amax else None,
                                    am_w.data_ptr(), am_w.numel(), rows_a, am_x.data_ptr(), am_x.numel(), None, 0, B, Co, CI, Nn,
                                    ops._stream())
        torch.cuda.synchronize()
        untouched = all(bool((o == FILL).all()) for o in owners) and bool((slots == -1.0).all())
        return rc, untouched

    def edit(i, **kw):
        items = [dict(it) for it in good]
        items[i].update(kw)
        return items

    nine = good + good + [good[0]]
    bad = {
        "n = 0": dict(n=0), "n = 9": dict(items=nine),
        "sum C < Co": dict(items=good[:3]), "sum C > Co": dict(items=edit(3, C=104)), "C = 0": dict(items=edit(0, C=0)),
        "no y": dict(items=edit(1, y=None)), "no weight": dict(items=edit(1, w=None)), "no bias": dict(items=edit(1, b=None)),
        "no running_mean": dict(items=edit(2, rm=None)), "no running_var": dict(items=edit(2, rv=None)),
        "negative eps": dict(items=edit(0, eps=-1e-5)), "nan eps": dict(items=edit(0, eps=float("nan"))),
        "y stride below C*N": dict(items=edit(2, ybs=36 * N - 4)), "residual stride below C*N": dict(items=edit(1, rbs=22 * N - 4)),
        "y stride not a multiple of 4": dict(items=edit(2, ybs=36 * N + 2)),
        "residual stride not a multiple of 4": dict(items=edit(1, rbs=22 * N + 2)),
        "y not 16-byte aligned": dict(items=edit(0, y=good[0]["y"] + 4)),
        "residual not 16-byte aligned": dict(items=edit(1, res=good[1]["res"] + 4)),
        "per-item amax_out": dict(per_item_amax=x.data_ptr()),
        "w not aligned": dict(w=W.data_ptr() + 4), "x not aligned": dict(xp=x.data_ptr() + 4), "no w": dict(w=None), "no x": dict(xp=None),
        "N % 4": dict(Nn=N - 2), "Co % 4": dict(items=edit(3, C=98), Co=CO - 2), "rows_a != Co": dict(rows_a=CO - 4),
    }
    for what, kw in bad.items():
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, (what, rc, untouched)
    assert lib.ct_pw_gemm_rs_norm(W.data_ptr(), x.data_ptr(), None, 4, None, None, 0, 0, None, 0, None, 0, B, CO, CI, N, ops._stream()) == -1
    # more partial maxima than a GEMM folds: the query says 0 and an amax_out is refused
    assert lib.ct_pw_gemm_norm_amax_len(64, 4096, 4096) == 0 and lib.ct_pw_gemm_norm_amax_len(8, 512, 4096) == 4 * 32 * 8
    rc, untouched = call()                                   # and the good call goes through
    assert rc == 0 and not untouched


# ---- routing: ops and the blocks ----

class _Calls:
    """Counts the calls of the library's entry points named in `names` while active (as tests/test_bn_eval_gpu.py wraps
    ct_bn_eval_group_fwd)."""

    def __init__(self, *names):
        self.names, self.n = names, {k: 0 for k in names}

    def __enter__(self):
        from cloud_transformers_amd import _lib
        self.lib, self.real = _lib.load(), {}
        for k in self.names:
            self.real[k] = real = getattr(self.lib, k)
            setattr(self.lib, k, lambda *a, _k=k, _f=real: (self.n.__setitem__(_k, self.n[_k] + 1), _f(*a))[1])
        return self

    def __exit__(self, *exc):
        for k, f in self.real.items():
            setattr(self.lib, k, f)
        return False


def _on_off(run):
    """(result with ops.PW_NORM on, its call counts, module-norm calls; the same with it off)."""
    from cloud_transformers_amd import ops
    from tests.test_eval_blocks_gpu import _CountNorms
    assert ops.PW_NORM and ops.BN_EVAL
    out = []
    try:
        for switch in (True, False):
            ops.PW_NORM = switch
            with torch.no_grad(), _CountNorms() as mods, _Calls("ct_bn_eval_group_fwd", "ct_pw_gemm_rs_norm") as c:
                res = run()
            out += [res, c.n, mods.calls]
    finally:
        ops.PW_NORM = True
    return out


def test_union_block_same_bits_one_norm_launch_instead_of_three():
    from tests.test_eval_blocks_gpu import _inputs, _union
    blk = _union()
    x, pcd = _inputs(2, 128, 1024)
    on, n_on, mods_on, off, n_off, mods_off = _on_off(lambda: blk(x, pcd)[0])
    assert n_on == {"ct_bn_eval_group_fwd": 1, "ct_pw_gemm_rs_norm": 2}, n_on          # the join | the projections, `after`
    assert n_off == {"ct_bn_eval_group_fwd": 3, "ct_pw_gemm_rs_norm": 0}, n_off
    assert mods_on == 0 and mods_off == 0
    assert torch.equal(on, off)
    # the block's output carries partial maxima the next block's GEMM folds to the same scale as the per-channel ones
    tag = on._ct_amax[0]
    assert tag.dim() == 1 and float(tag.max()) == float(on.abs().max()) == float(off._ct_amax[0].max())


def test_union_block_with_projected_shortcut_still_one_module_norm():
    from tests.test_eval_blocks_gpu import _inputs, _union
    blk = _union(model_dim_out=64)
    x, pcd = _inputs(2, 128, 1024)
    on, n_on, mods_on, off, n_off, mods_off = _on_off(lambda: blk(x, pcd)[0])
    assert mods_on == 1 and mods_off == 1                    # shortcut_bn: one module call, whatever the switch says
    assert n_on["ct_pw_gemm_rs_norm"] >= 1 and n_off["ct_pw_gemm_rs_norm"] == 0
    assert torch.equal(on, off)


@pytest.mark.parametrize("heads,fuses", [(4, True), (2, False)])
def test_single_head(heads, fuses):
    """heads 4: the projection has 28 output rows, a shape the kernel takes — one fused call (the unfused path runs the
    library GEMM there, so the two agree within the fused-versus-plain bound of tests/test_eval_blocks_gpu.py); heads 2: 14
    rows, no GEMM shape — the old path, whatever the switch says."""
    from cloud_transformers_amd.layers.multihead_ct import MultiHead
    from tests.test_eval_blocks_gpu import _agree, _inputs, _randomise_norms
    torch.manual_seed(3)
    blk = _randomise_norms(MultiHead(16, 4, 16, 8, 2, heads).cuda().eval(), 4)
    x, pcd = _inputs(2, 16, 1024)
    on, n_on, mods_on, off, n_off, mods_off = _on_off(lambda: blk(x, pcd)[0])
    assert mods_on == 0 and mods_off == 0
    assert n_on["ct_pw_gemm_rs_norm"] == (1 if fuses else 0) and n_off["ct_pw_gemm_rs_norm"] == 0
    assert n_on["ct_bn_eval_group_fwd"] == (1 if fuses else 2) and n_off["ct_bn_eval_group_fwd"] == 2
    if fuses:
        _agree(on, off)
    else:
        assert torch.equal(on, off)


def test_pool_head_fuses_its_projection():
    from cloud_transformers_amd.layers.multihead_ct import MultiHeadPool
    from tests.test_eval_blocks_gpu import _agree, _inputs, _randomise_norms
    torch.manual_seed(3)
    blk = _randomise_norms(MultiHeadPool(16, 4, 8, 2, 4).cuda().eval(), 4)
    x, pcd = _inputs(2, 16, 1024)
    on, n_on, _, off, n_off, _ = _on_off(lambda: blk(x, pcd)[0])
    assert n_on == {"ct_bn_eval_group_fwd": 0, "ct_pw_gemm_rs_norm": 1} and n_off == {"ct_bn_eval_group_fwd": 1, "ct_pw_gemm_rs_norm": 0}
    _agree(on, off)


def test_with_gradients_the_fused_entry_point_is_never_called():
    from tests.test_eval_blocks_gpu import _inputs, _union
    blk = _union()
    x, pcd = _inputs(2, 128, 1024)
    x.requires_grad_(True)
    with _Calls("ct_pw_gemm_rs_norm", "ct_bn_eval_group_fwd") as c:
        out, _ = blk(x, pcd)
    assert c.n == {"ct_pw_gemm_rs_norm": 0, "ct_bn_eval_group_fwd": 0}, c.n
    assert out.requires_grad


def test_eval_forward_replays_from_a_captured_graph():
    from tests.test_eval_blocks_gpu import _inputs, _union
    blk = _union()
    x, pcd = _inputs(2, 128, 1024)
    with torch.no_grad():
        want = blk(x, pcd)[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                blk(x, pcd)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with _Calls("ct_pw_gemm_rs_norm") as c:
            with torch.cuda.graph(g):
                out = blk(x, pcd)[0]
        assert c.n["ct_pw_gemm_rs_norm"] == 2
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)


def test_whole_segmenter_same_bits_with_the_switch_on_and_off():
    from tests.test_zoo_gpu import _model
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zoo_segmenter_forward.npz"))
    net = _model(int(gold["seed"])).eval()
    cloud = torch.from_numpy(gold["cloud"]).cuda()
    on, n_on, _, off, n_off, _ = _on_off(lambda: net(cloud))
    assert n_on["ct_pw_gemm_rs_norm"] == 24 and n_off["ct_pw_gemm_rs_norm"] == 0, (n_on, n_off)     # twelve blocks, two calls each
    assert n_on["ct_bn_eval_group_fwd"] == n_off["ct_bn_eval_group_fwd"] - 24
    assert torch.equal(on, off)
