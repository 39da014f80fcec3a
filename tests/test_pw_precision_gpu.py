"""The "high" precision mode of the pointwise GEMMs (include/cloudct.h: CT_PW_PRECISION_HIGH — one f16 MFMA term per operand,
fp32 accumulation): the header's error bound against float64 products in every arrangement, the 4097 witness that tells the
two modes apart, exact integer data (layout), the default mode's bits untouched by the switch, the epilogues' bit
equalities within the mode, and the mode carried through the autograd layer, a union block and a captured graph.

Every tolerance is the header's bound (f16's 11-bit significand and subnormal spacing) or a bit equality."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS_ACC = 2.0e-6                                   # tests/test_pw_gemm_gpu.py: BOUND, the three-term mode's whole allowance
REL = 2.0 ** -10 + 2.0 ** -22 + EPS_ACC            # include/cloudct.h, CT_PW_PRECISION_HIGH
SUB = 2.0 ** -37

# (B, Co, Ci, N): one partial tile and K-step | ragged everywhere, K no multiple of 32 or 64 | ragged, several tiles |
# several full K-steps and tiles, B > 1
SHAPES = [(1, 4, 4, 4), (3, 52, 36, 260), (1, 260, 44, 1028), (2, 208, 512, 1024)]
SCALES = [(1.0, 1.0), (1e-7, 1.0), (1e6, 1e-5), (1.0, 1e-30)]


def _needs_split16():
    from cloud_transformers_amd import ops
    if ops.PW_GEMM != "split16":
        pytest.skip("the precision mode belongs to ct_pw_gemm (CLOUDCT_PW_GEMM=split16)")


@pytest.fixture(autouse=True)
def _split16_and_clean_mode():
    _needs_split16()
    from cloud_transformers_amd import precision
    prev = precision.get_mode()
    precision.set_matmul_precision("highest")
    yield
    precision.set_matmul_precision(prev)


def _high():
    import cloud_transformers_amd as ct
    return ct.matmul_precision("high")


def _rs(mode, a, b, am_a, am_b, B, Co, Ci, N):
    """ct_pw_gemm_rs itself, in the library's current mode; 2-D maxima are per-row maxima (ops._rows_of)."""
    from cloud_transformers_amd import _lib, ops
    lib = _lib.load()
    out = torch.empty((B, Co, N) if mode == 0 else (B, Ci, N) if mode in (1, 3) else (Co, Ci), device="cuda")
    nbytes = lib.ct_pw_gemm_workspace_bytes(mode, B, Co, Ci, N)
    ws = torch.empty(max(nbytes, 16) // 4, device="cuda")
    rows_a = ops._rows_of(am_a, Co if mode in (0, 2) else Ci) if mode != 1 else 0
    rows_b = ops._rows_of(am_b, Ci) if mode == 2 else 0
    rc = lib.ct_pw_gemm_rs(mode, a.data_ptr(), b.data_ptr(), out.data_ptr(), am_a.data_ptr(), am_a.numel(), rows_a, am_b.data_ptr(),
                           am_b.numel(), rows_b, ws.data_ptr(), nbytes, B, Co, Ci, N, ops._stream())
    assert rc == 0, rc
    return out


def _product(mode, W, x, gy):
    """The product of `mode` with per-row maxima where the arrangement has them: rows of W (0), of W^T (3), channels of g_y
    and x (2); the data gradient from W (1) keeps one scale per operand."""
    from cloud_transformers_amd import ops
    Co, Ci = W.shape
    B, _, N = x.shape
    (rowmax, colmax), Wt = ops.prep_weight(W, True)
    if mode == 0:
        return _rs(0, W, x, rowmax, ops.amax(x), B, Co, Ci, N)
    if mode == 1:
        return _rs(1, W, gy, ops.amax(W), ops.amax(gy), B, Co, Ci, N)
    if mode == 3:
        return _rs(3, Wt, gy, colmax, ops.amax(gy), B, Co, Ci, N)
    return _rs(2, gy, x, ops.amax_rows(gy), ops.amax_rows(x), B, Co, Ci, N)


def _bound(mode, W, x, gy):
    """(float64 product, the header's bound per output) for _product's scales: M_a / M_b are the row's own maxima wherever
    per-row scales apply, the tensor's otherwise."""
    Wd, xd, gd = W.double(), x.double(), gy.double()
    if mode == 0:
        ref, mag = torch.matmul(Wd, xd), torch.matmul(Wd.abs(), xd.abs())
        Ma, sa = Wd.abs().amax(1)[None, :, None], Wd.abs().sum(1)[None, :, None]
        Mb, sb = xd.abs().max(), xd.abs().sum(1, keepdim=True)
    elif mode in (1, 3):
        ref, mag = torch.matmul(Wd.t(), gd), torch.matmul(Wd.abs().t(), gd.abs())
        Ma = Wd.abs().amax(0)[None, :, None] if mode == 3 else Wd.abs().max()
        sa = Wd.abs().sum(0)[None, :, None]
        Mb, sb = gd.abs().max(), gd.abs().sum(1, keepdim=True)
    else:
        ref = torch.matmul(gd, xd.transpose(1, 2)).sum(0)
        mag = torch.matmul(gd.abs(), xd.abs().transpose(1, 2)).sum(0)
        Ma, sa = gd.abs().amax(dim=(0, 2))[:, None], gd.abs().sum(dim=(0, 2))[:, None]
        Mb, sb = xd.abs().amax(dim=(0, 2))[None, :], xd.abs().sum(dim=(0, 2))[None, :]
    return ref, REL * mag + SUB * (Ma * sb + Mb * sa)


@functools.lru_cache(maxsize=None)
def _operands(shape, scales=(1.0, 1.0)):
    """W, x, g_y of a case, made once and never modified (the float64 references are cached with them: _reference)."""
    B, Co, Ci, N = shape
    g = torch.Generator(device="cuda").manual_seed(B * 7 + Co)
    W = torch.randn(Co, Ci, device="cuda", generator=g) / Ci ** 0.5
    x = torch.randn(B, Ci, N, device="cuda", generator=g)
    gy = torch.randn(B, Co, N, device="cuda", generator=g)
    if scales != (1.0, 1.0):
        # a spread inside one tensor as well (tests/test_pw_gemm_gpu.py: test_operand_magnitudes)
        x[:, ::3] *= 2.0 ** -12
        gy[:, 1::5] *= 2.0 ** -10
    return W, x, gy


@functools.lru_cache(maxsize=None)
def _reference(shape, scales, mode):
    W, x, gy = _scaled(shape, scales, mode)
    return _bound(mode, W, x, gy)


def _scaled(shape, scales, mode):
    """The case's operands with the first / second operand of `mode` at the magnitudes `scales`."""
    W, x, gy = _operands(shape, scales)
    if mode == 0:
        return W * scales[0], x * scales[1], gy
    if mode in (1, 3):
        return W * scales[0], x, gy * scales[1]
    return W, x * scales[1], gy * scales[0]


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_high_is_within_the_headers_bound_of_the_float64_product(mode, shape, scales):
    W, x, gy = _scaled(shape, scales, mode)
    ref, bound = _reference(shape, scales, mode)
    with _high():
        out = _product(mode, W, x, gy)
    err = (out.double() - ref).abs()
    print("mode %d %s %s: worst err / bound %.3f" % (mode, shape, scales, float((err / bound.clamp_min(1e-300)).max())))
    assert torch.isfinite(out).all()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


def _witness(mode, B=2, Co=132, Ci=36, N=260):
    """A product whose every non-zero output is 4097 exactly in "highest" and 4096 in "high" (f16's spacing at the scaled
    value is 4 units of the operand: 4097 is no tie): one operand is zero but for one 4097.0, the other is all ones."""
    from cloud_transformers_amd import ops
    if mode == 2:
        gy = torch.zeros(B, Co, N, device="cuda")
        gy[1, 5, 77] = 4097.0
        x = torch.ones(B, Ci, N, device="cuda")
        out = ops.pw_gemm(2, gy, x, ops.amax_rows(gy), ops.amax_rows(x), B, Co, Ci, N)
        hit = out[5]
    else:
        W = torch.zeros(Co, Ci, device="cuda")
        W[5, 7] = 4097.0
        if mode == 0:
            x = torch.ones(B, Ci, N, device="cuda")
            out = ops.pw_gemm(0, W, x, ops.amax(W), ops.amax(x), B, Co, Ci, N)
            hit = out[:, 5]
        else:
            gy = torch.ones(B, Co, N, device="cuda")
            if mode == 1:
                out = ops.pw_gemm(1, W, gy, ops.amax(W), ops.amax(gy), B, Co, Ci, N)
            else:
                (_, colmax), Wt = ops.prep_weight(W, True)
                out = ops.pw_gemm(3, Wt, gy, colmax, ops.amax(gy), B, Co, Ci, N)
            hit = out[:, 7]
    values = hit.unique().tolist()
    assert len(values) == 1 and int((out != 0).sum()) == hit.numel(), (values, int((out != 0).sum()))
    return values[0]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_the_mode_is_really_on_and_really_off(mode):
    import cloud_transformers_amd as ct
    assert _witness(mode) == 4097.0
    with _high():
        assert _witness(mode) == 4096.0
    assert _witness(mode) == 4097.0
    with ct.matmul_precision("medium"):              # served by the "high" kernels
        assert _witness(mode) == 4096.0
    assert _witness(mode) == 4097.0


@pytest.mark.parametrize("wide", ["first", "second"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_integers_up_to_2048_are_exact_in_high(mode, wide):
    """Layout pin: integers |v| <= 2048 are f16 values under any power-of-two scale, so one term carries them whole and any
    slip in a fragment, swizzle or output map shows as a wrong integer.  Exact fp32 accumulation needs sum_k |a b| < 2^24: one
    operand spans the whole [-2048, 2048], the other [-32, 32] (K <= 64: at most 2^22), and each operand takes the wide
    role once."""
    B, Co, Ci, N = {0: (2, 132, 60, 260), 1: (2, 60, 132, 260), 3: (2, 60, 132, 260), 2: (2, 132, 136, 28)}[mode]
    g = torch.Generator(device="cuda").manual_seed(5 + mode)

    def ints(shape, role):
        top = 2048 if role == wide else 32
        t = torch.randint(-top, top + 1, shape, device="cuda", generator=g).float()
        t.view(-1)[:2] = torch.tensor([float(top), -float(top)], device="cuda")
        return t

    W = ints((Co, Ci), "first" if mode != 2 else "none")
    x = ints((B, Ci, N), "second" if mode in (0, 2) else "none")
    gy = ints((B, Co, N), "second" if mode in (1, 3) else "first" if mode == 2 else "none")
    ref, _ = _bound(mode, W, x, gy)
    with _high():
        out = _product(mode, W, x, gy)
    assert torch.equal(out.double(), ref)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_the_default_is_untouched_by_the_switch(mode):
    W, x, gy = _operands((3, 52, 36, 260))
    before = _product(mode, W, x, gy)
    with _high():
        inside = _product(mode, W, x, gy)
    after = _product(mode, W, x, gy)
    assert torch.equal(before, after)
    assert not torch.equal(before, inside)


@pytest.mark.parametrize("shape", [(3, 52, 36, 260), (2, 208, 512, 1024)])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_addend_epilogue_is_the_product_plus_the_addend_bit_for_bit_in_high(mode, shape):
    from cloud_transformers_amd import ops
    B, Co, Ci, N = shape
    W, x, gy = _operands(shape)
    (rowmax, colmax), Wt = ops.prep_weight(W, True)
    a, b, am_a, am_b = ((W, x, rowmax, ops.amax(x)) if mode == 0 else (W, gy, ops.amax(W), ops.amax(gy)) if mode == 1
                        else (Wt, gy, colmax, ops.amax(gy)))
    with _high():
        plain = _rs(mode, a, b, am_a, am_b, B, Co, Ci, N)
        add = torch.randn(plain.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 3
        fused = ops.pw_gemm(mode, a, b, am_a, am_b, B, Co, Ci, N, addend=add)
    assert torch.equal(fused, plain + add)
    assert not torch.equal(plain, _rs(mode, a, b, am_a, am_b, B, Co, Ci, N))        # (and `plain` was a one-term product)


@pytest.mark.parametrize("shape,split", [((3, 52, 36, 260), 20), ((2, 208, 512, 1024), 100)])
def test_norm_epilogue_is_the_product_then_the_eval_norm_bit_for_bit_in_high(shape, split):
    """ct_pw_gemm_rs_norm with two items that split Co at a row that is no multiple of 32, against ct_pw_gemm_rs into scratch
    followed by ct_bn_eval_group_fwd with the same items, both in "high"."""
    from cloud_transformers_amd import _lib, ops
    lib = _lib.load()
    B, Co, Ci, N = shape
    assert split % 32 != 0
    W, x, _ = _operands(shape)
    Cs = (split, Co - split)
    g = torch.Generator().manual_seed(Co)
    par = [dict(w=(torch.rand(C, generator=g) + 0.5).cuda(), b=(torch.rand(C, generator=g) - 0.5).cuda(),
                rm=(torch.rand(C, generator=g) * 2 - 1).cuda(), rv=(torch.rand(C, generator=g) * 1.5 + 0.5).cuda(), eps=1e-5) for C in Cs]
    res = torch.randn(B, Cs[1], N, generator=g).cuda()

    def items(outs, src):
        c0, out = 0, []
        for i, (C, y) in enumerate(zip(Cs, outs)):
            out.append(dict(x=None if src is None else src.data_ptr() + c0 * N * 4, xbs=0 if src is None else Co * N, C=C, relu=1 - i,
                            res=res.data_ptr() if i == 1 else None, rbs=0, y=y.data_ptr(), ybs=0, amax=None, **par[i]))
            c0 += C
        return out

    rowmax, am_x = ops.prep_weight(W, False)[0][0], ops.amax(x)
    want = [torch.full((B, C, N), 7.0, device="cuda") for C in Cs]
    got = [torch.full((B, C, N), 7.0, device="cuda") for C in Cs]
    with _high():
        scratch = _rs(0, W, x, rowmax, am_x, B, Co, Ci, N)
        arr = ops._bn_fwd_table(items(want, scratch))
        assert lib.ct_bn_eval_group_fwd(ops._at(arr, 0), 2, B, N, ops._stream()) == 0
        arr = ops._bn_fwd_table(items(got, None))
        assert lib.ct_pw_gemm_rs_norm(W.data_ptr(), x.data_ptr(), ops._at(arr, 0), 2, None, rowmax.data_ptr(), rowmax.numel(), Co,
                                      am_x.data_ptr(), am_x.numel(), None, 0, B, Co, Ci, N, ops._stream()) == 0
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b), float((a - b).abs().max())
    assert not torch.equal(scratch, _rs(0, W, x, rowmax, am_x, B, Co, Ci, N))


def test_weight_gradient_is_reproducible_in_high():
    W, x, gy = _operands((2, 208, 512, 1024))          # four K chunks per cloud: slabs and the fixed-order fold
    with _high():
        a = _product(2, W, x, gy)
        b = _product(2, W, x, gy)
    assert torch.equal(a, b)


def test_zeros_nan_and_inf_reach_the_same_outputs_as_in_highest():
    from cloud_transformers_amd import ops
    B, Co, Ci, N = 1, 128, 36, 260
    x = torch.randn(B, Ci, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    Wz = torch.zeros(Co, Ci, device="cuda")
    W = torch.randn(Co, Ci, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    xn = x.clone()
    xn[0, 3, 17] = float("nan")
    xn[0, 5, 100] = float("inf")

    def both():
        return (ops.pw_gemm(0, Wz, x, ops.amax(Wz), ops.amax(x), B, Co, Ci, N), ops.pw_gemm(0, W, xn, ops.amax(W), ops.amax(xn), B, Co, Ci, N))

    z_hi, y_hi = both()
    with _high():
        z, y = both()
    assert torch.equal(z, torch.zeros_like(z)) and torch.equal(z_hi, z)
    assert torch.isnan(y[0, :, 17]).all() and not torch.isfinite(y[0, :, 100]).any()
    assert torch.equal(torch.isfinite(y), torch.isfinite(y_hi))
    assert int((~torch.isfinite(y)).sum()) == 2 * Co


@pytest.mark.parametrize("depth", [16, 24, 40])
def test_a_row_far_below_the_tensors_maximum_keeps_the_modes_bound(depth):
    """Per-row scales in the weight gradient: channels of g_y and of x 2^-depth below their tensor's maximum stay within the
    bound of THEIR OWN maxima."""
    W, x, gy = _operands((3, 52, 36, 260))
    x, gy = x.clone(), gy.clone()
    gy[:, 2::9] *= 2.0 ** -depth
    x[:, 1::11] *= 2.0 ** -depth
    ref, bound = _bound(2, W, x, gy)
    with _high():
        out = _product(2, W, x, gy)
    err = (out.double() - ref).abs()
    assert torch.isfinite(out).all() and bool((out[2::9] != 0).any())
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


def test_pointwise_layer_keeps_the_forwards_mode_in_its_backward():
    """PointwiseConv1d(128, 132, 1) on [2, 128, 260]: the forward inside the scope, the backward outside it.  Bound: the
    header's, with the tensors' maxima for M (an upper bound of any row's), plus the fp32 rounding of the bias add."""
    import cloud_transformers_amd as ct
    from cloud_transformers_amd.layers.pointwise import PointwiseConv1d
    torch.manual_seed(0)
    B, Ci, Co, N = 2, 128, 132, 260
    layer = PointwiseConv1d(Ci, Co, 1).cuda()
    ref = torch.nn.Conv1d(Ci, Co, 1).cuda().double()
    ref.load_state_dict({k: v.double() for k, v in layer.state_dict().items()})
    x = torch.randn(B, Ci, N, device="cuda", requires_grad=True)
    xd = x.detach().double().requires_grad_(True)
    cot = torch.randn(B, Co, N, device="cuda")
    with ct.matmul_precision("high"):
        y = layer(x)
    assert ct.get_matmul_precision() == "highest"
    y.backward(cot)
    yd = ref(xd)
    yd.backward(cot.double())
    Wd, cd = ref.weight.detach()[:, :, 0], cot.double()
    xa, ca, Wa = xd.detach().abs(), cd.abs(), Wd.abs()
    MW, Mx, Mc = Wa.max(), xa.max(), ca.max()
    b_y = REL * torch.matmul(Wa, xa) + SUB * (MW * xa.sum(1, keepdim=True) + Mx * Wa.sum(1)[None, :, None]) + 2.0 ** -24 * yd.detach().abs()
    b_x = REL * torch.matmul(Wa.t(), ca) + SUB * (MW * ca.sum(1, keepdim=True) + Mc * Wa.sum(0)[None, :, None])
    b_w = REL * torch.matmul(ca, xa.transpose(1, 2)).sum(0) + SUB * (Mc * xa.sum(dim=(0, 2))[None, :] + Mx * ca.sum(dim=(0, 2))[:, None])
    for name, got, want, bound in (("y", y.detach(), yd.detach(), b_y), ("g_x", x.grad, xd.grad, b_x),
                                   ("g_w", layer.weight.grad[:, :, 0], ref.weight.grad[:, :, 0], b_w)):
        err = (got.double() - want).abs()
        print("%s: worst err / bound %.3f, err / (2e-6 * sum|ab|) %.1f" % (name, float((err / bound).max()), float((err / bound).max()) * REL / EPS_ACC))
        assert bool((err <= bound).all()), (name, float((err / bound).max()))
    # the witness through the layer's own backward: x = 1, one 4097 in g_y -> that row of g_w is 4096 where the forward ran
    # in "high" (the backward runs outside the scope), 4097 where it ran in the default mode
    seed = torch.zeros(B, Co, N, device="cuda")
    seed[1, 9, 33] = 4097.0
    ones = torch.ones(B, Ci, N, device="cuda", requires_grad=True)
    for scope, want in ((ct.matmul_precision("high"), 4096.0), (ct.matmul_precision("highest"), 4097.0)):
        layer.weight.grad = None
        ones.grad = None
        with scope:
            out = layer(ones)
        with ct.matmul_precision("highest" if want == 4096.0 else "high"):      # the other mode while the backward runs
            out.backward(seed)
        row = layer.weight.grad[9, :, 0]
        assert bool((row == want).all()), (want, row.unique().tolist())


def test_union_block_in_eval_same_bits_with_the_norm_epilogue_on_and_off_in_high():
    from cloud_transformers_amd import ops
    from tests.test_eval_blocks_gpu import _inputs, _union
    blk = _union()
    x, pcd = _inputs(2, 128, 256)
    assert ops.PW_NORM and ops.BN_EVAL
    res = {}
    try:
        for switch in (True, False):
            ops.PW_NORM = switch
            with torch.no_grad(), _high():
                res[switch] = blk(x, pcd)[0]
    finally:
        ops.PW_NORM = True
    with torch.no_grad():
        default = blk(x, pcd)[0]
    assert torch.isfinite(res[True]).all()
    assert torch.equal(res[True], res[False])
    assert not torch.equal(res[True], default)           # the block did run one-term products


def test_a_captured_graph_keeps_the_mode_it_was_recorded_in():
    from cloud_transformers_amd import ops
    B, Co, Ci, N = 2, 132, 36, 260
    W = torch.zeros(Co, Ci, device="cuda")
    W[5, 7] = 4097.0
    x = torch.ones(B, Ci, N, device="cuda")
    am_w, am_x = ops.amax(W), ops.amax(x)
    with _high():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.pw_gemm(0, W, x, am_w, am_x, B, Co, Ci, N)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = ops.pw_gemm(0, W, x, am_w, am_x, B, Co, Ci, N)
    assert float(ops.pw_gemm(0, W, x, am_w, am_x, B, Co, Ci, N)[0, 5, 0]) == 4097.0      # the scope has ended
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert bool((out[:, 5] == 4096.0).all()) and int((out != 0).sum()) == B * N
