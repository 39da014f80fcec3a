"""GPU checks of the backward of the eval-mode norm (ct_bn_eval_group_bwd) and of its entry points in ops (bn_frozen,
split_bn_frozen, join_bn_relu_frozen, union_keys_values_frozen).

Exact coverage runs on integer-valued data (running_var = 1 and eps = 0, so rstd is exactly 1; |x - mean| <= 10, |weight|
<= 3, |bias| <= 4, |gy| <= 4): every product and every sum is an integer below 2^24 (at most 80000 terms of at most 40), so
fp32 holds them exactly in ANY order and the results must equal an int64 computation on the host bit for bit.

Rounding runs on random data against float64 on the host.  With rs = 1 / sqrt(var + eps) and the mask taken from what the
forward stored (the contract: an element passes iff the forward stored a positive value):
* gx = g' * (w * rs): the kernel's rs is within 2 ulp (4 * 2^-24 relative), w * rs rounds once and so does the product with
  g', so |err| <= 6 * 2^-24 * |g'| * |w| * rs to first order; the tests allow 2^-21 of that product (1.33x margin).  (The
  way the docstring of tests/test_bn_eval_gpu.py bounds the forward: count the roundings, allow the next power of two.)
* g_bias = sum g': the terms are the inputs themselves, and M - 1 additions in any order err by at most
  (M - 1) * 2^-24 * sum |g'| to first order (M = B * N).
* g_weight = sum g' * xh: a term carries the roundings of x - mean, rs (4 units), (x - mean) * rs and g' * xh, seven units of
  2^-24 in all, before the M - 1 additions.
  Both sums are held to (M + 8) * 2^-24 * sum |terms|, which covers any summation order.
Where |running_mean| >> |x - running_mean| (the cancellation case) these bounds are small against |x|: a kernel that did
not subtract the mean first would miss them."""
import copy
import ctypes

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1), (2, 5, 256), (3, 7, 1001), (4, 32, 512), (2, 4, 40000)]       # the last: a channel beyond the registers
ROUNDING = [(4, 32, 512, 0.0), (3, 7, 1001, 0.0), (4, 32, 512, 50.0), (3, 7, 1001, 50.0)]
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _int_case(B, C, N, seed):
    """Integer-valued inputs (int64, CPU); channel 0 has weight 0 (key_bn.weight starts at zero in every block)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)      # noqa: E731
    case = dict(x=r(-8, 8, B, C, N), gy=r(-4, 4, B, C, N), w=r(-3, 3, C), b=r(-4, 4, C), rm=r(-2, 2, C))
    case["w"][0] = 0
    if C > 1:
        case["w"][1] = -2
    return case


def _int_ref(case, relu):
    """int64 on the host: gx, g_weight, g_bias, max |gx| per channel, and the forward's value before the residual."""
    x, gy = case["x"], case["gy"]
    w, b, rm = (case[k][None, :, None] for k in ("w", "b", "rm"))
    xh = x - rm
    o = xh * w + b
    g = torch.where(o > 0, gy, torch.zeros_like(gy)) if relu else gy
    gx = g * w
    return dict(gx=gx.float(), gw=(g * xh).sum((0, 2)).float(), gb=g.sum((0, 2)).float(), amax=gx.abs().amax((0, 2)).float(),
                y=(o.clamp_min(0) if relu else o).float())


def _dev(case):
    d = {k: v.float().cuda() for k, v in case.items()}
    d["rv"] = torch.ones_like(d["w"])
    d["eps"] = 0.0
    return d


def _item(d, relu, x=None, xbs=0, gy=None, gybs=0, gx=None, gxbs=0, gw=None, gb=None, amax=None):
    """One ct_bn_eval_bwd_item for ops._bn_eval_bwd_table: x / gy / gx are data pointers (default: the case's own tensors)."""
    return dict(x=d["x"].data_ptr() if x is None else x, xbs=xbs, C=d["w"].numel(), w=d["w"], b=d["b"], rm=d["rm"], rv=d["rv"],
                eps=d["eps"], relu=int(relu), gy=d["gy"].data_ptr() if gy is None else gy, gybs=gybs, gx=gx, gxbs=gxbs, gw=gw, gb=gb,
                amax=amax)


def _launch(items, B, N):
    from cloud_transformers_amd import _lib, ops
    arr = ops._bn_eval_bwd_table(items)
    rc = _lib.load().ct_bn_eval_group_bwd(ops._at(arr, 0), len(items), B, N, ops._stream())
    assert rc == 0, rc


def _outs(B, C, N):
    """NaN-filled gx, g_weight, g_bias, amax: a value the kernel did not write cannot pass for one it did."""
    return (torch.full((B, C, N), NAN, device="cuda"), torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda"),
            torch.full((C,), NAN, device="cuda"))


def _all_asked(d, relu, B, N):
    C = d["w"].numel()
    gx, gw, gb, am = _outs(B, C, N)
    return _item(d, relu, gx=gx.data_ptr(), gw=gw, gb=gb, amax=am.data_ptr()), (gx, gw, gb, am)


def _equal(got, ref, what):
    gx, gw, gb, am = got
    assert torch.equal(gx.cpu(), ref["gx"]), what + ": gx"
    assert torch.equal(gw.cpu(), ref["gw"]), what + ": g_weight"
    assert torch.equal(gb.cpu(), ref["gb"]), what + ": g_bias"
    assert am is None or torch.equal(am.cpu(), ref["amax"]), what + ": amax"


def _frozen_norm(C, seed, mean_offset=0.0):
    """A BatchNorm1d off its initial values, marked frozen (tests/test_bn_eval_gpu.py's _norm)."""
    from cloud_transformers_amd import freeze_norms
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm1d(C, eps=1e-5)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(C, generator=g) - 0.5)
        bn.running_mean.copy_(torch.rand(C, generator=g) * 2 - 1 + mean_offset)
        bn.running_var.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
    return freeze_norms(bn)


def _stats(*mods):
    return [t.clone() for m in mods for sub in m.modules() if isinstance(sub, nn.modules.batchnorm._BatchNorm)
            for t in (sub.running_mean, sub.running_var, sub.num_batches_tracked)]


def _agree(got, want, what=""):
    """The project's fused-versus-plain bar (tests/test_eval_blocks_gpu.py)."""
    tol = 1e-4 * max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print("%s max |fused - modules| %.3e (bound %.3e)" % (what, err, tol))
    assert got.shape == want.shape and err <= tol, (what, err, tol)


# ---------------------------------------------------------------------------------------------------------------------
# exact coverage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("B,C,N", SHAPES)
def test_exact_on_integer_data(B, C, N, relu):
    from cloud_transformers_amd import ops
    case = _int_case(B, C, N, 1000 * B + C)
    ref = _int_ref(case, relu)
    d = _dev(case)

    # contiguous, everything asked for
    item, got = _all_asked(d, relu, B, N)
    _launch([item], B, N)
    _equal(got, ref, "contiguous")

    # x a channel slice of a wider tensor, gy a channel range of a concatenation's cotangent, gx into a range of a wider tensor
    wx = torch.full((B, C + 3, N), 99.0, device="cuda")
    wgy = torch.full((B, C + 5, N), -77.0, device="cuda")
    wgx = torch.full((B, C + 4, N), 7.0, device="cuda")
    wx[:, 2:2 + C], wgy[:, 4:4 + C] = d["x"], d["gy"]
    _, gw, gb, am = _outs(B, C, N)
    _launch([_item(d, relu, x=wx.data_ptr() + 2 * N * 4, xbs=(C + 3) * N, gy=wgy.data_ptr() + 4 * N * 4, gybs=(C + 5) * N,
                   gx=wgx.data_ptr() + 1 * N * 4, gxbs=(C + 4) * N, gw=gw, gb=gb, amax=am.data_ptr())], B, N)
    _equal((wgx[:, 1:1 + C], gw, gb, am), ref, "slices")
    assert bool((wgx[:, :1] == 7.0).all()) and bool((wgx[:, 1 + C:] == 7.0).all())                # nothing outside the range

    # frozen affine parameters: no sums (a pure stream, cut over workgroups at the long shape), no maxima
    gx = _outs(B, C, N)[0]
    _launch([_item(d, relu, gx=gx.data_ptr())], B, N)
    assert torch.equal(gx.cpu(), ref["gx"]), "null sums"
    # ... and the same from a base that is not 16-byte aligned: float by float, cut differently
    flat_x, flat_gx = torch.empty(B * C * N + 1, device="cuda"), torch.full((B * C * N + 1,), NAN, device="cuda")
    flat_x[1:] = d["x"].flatten()
    _launch([_item(d, relu, x=flat_x.data_ptr() + 4, gx=flat_gx.data_ptr() + 4)], B, N)
    assert torch.equal(flat_gx[1:].view(B, C, N).cpu(), ref["gx"]) and bool(torch.isnan(flat_gx[0])), "null sums, unaligned"

    # the input needs no gradient: sums only
    _, gw, gb, _ = _outs(B, C, N)
    _launch([_item(d, relu, gw=gw, gb=gb)], B, N)
    assert torch.equal(gw.cpu(), ref["gw"]) and torch.equal(gb.cpu(), ref["gb"]), "null gx"

    # through autograd, with and without a residual in the forward (it changes y, never the mask)
    bn = nn.BatchNorm1d(C, eps=0.0).cuda().eval()
    with torch.no_grad():
        bn.weight.copy_(d["w"]), bn.bias.copy_(d["b"]), bn.running_mean.copy_(d["rm"])
    before = _stats(bn)
    for with_res in (False, True):
        x = d["x"].clone().requires_grad_(True)
        res = torch.randint(-5, 6, (B, C, N)).float().cuda().requires_grad_(True) if with_res else None
        bn.zero_grad()
        y = ops.bn_frozen(x, bn, relu=relu, residual=res)
        assert torch.equal(y.detach().cpu(), ref["y"] + (res.detach().cpu() if with_res else 0)), "forward"
        y.backward(d["gy"])
        _equal((x.grad, bn.weight.grad, bn.bias.grad, None), ref, "autograd, residual %s" % with_res)
        assert not with_res or torch.equal(res.grad, d["gy"])                  # the residual's cotangent is gy itself
    assert all(torch.equal(a, b) for a, b in zip(before, _stats(bn)))


@pytest.mark.parametrize("B,C,N", SHAPES)
def test_a_table_of_three_norms_equals_the_three_alone(B, C, N):
    """Three norms of different C in one launch against the same three launched alone: equal bits, and both the host's."""
    cases = [_int_case(B, c, N, 50 + c) for c in (C, 2 * C + 1, 2)]
    refs = [_int_ref(c, relu) for c, relu in zip(cases, (True, False, True))]
    devs = [_dev(c) for c in cases]
    table = [_all_asked(d, relu, B, N) for d, relu in zip(devs, (True, False, True))]
    _launch([item for item, _ in table], B, N)
    for (_, got), d, relu, ref in zip(table, devs, (True, False, True), refs):
        item, alone = _all_asked(d, relu, B, N)
        _launch([item], B, N)
        _equal(got, ref, "in the table")
        assert all(torch.equal(a, b) for a, b in zip(got, alone))


@pytest.mark.parametrize("B,C,N", [(4, 32, 512), (3, 7, 1001), (2, 4, 40000)])
def test_bits_do_not_depend_on_the_neighbours_or_the_run(B, C, N):
    """Random data, where the order of the additions shows: a norm gives the same sums and maxima alone, inside a table, beside
    a neighbour whose rows are not 16-byte addressable (the float4 choice is per item), and from run to run."""
    torch.manual_seed(N)
    devs = []
    for c in (C, 5, C + 1):
        devs.append(dict(x=torch.randn(B, c, N, device="cuda") * 2, gy=torch.randn(B, c, N, device="cuda"), w=torch.randn(c, device="cuda"),
                         b=torch.randn(c, device="cuda") * 0.3, rm=torch.randn(c, device="cuda") * 0.5,
                         rv=torch.rand(c, device="cuda") + 0.5, eps=1e-5))
    item, alone = _all_asked(devs[0], True, B, N)
    _launch([item], B, N)
    item, again = _all_asked(devs[0], True, B, N)
    _launch([item], B, N)
    assert all(torch.equal(a, b) for a, b in zip(alone, again))
    flat = torch.empty(B * 5 * N + 1, device="cuda")                          # the neighbour's x starts 4 bytes off
    flat[1:] = devs[1]["x"].flatten()
    first, in_table = _all_asked(devs[0], True, B, N)
    second, keep_second = _all_asked(devs[1], False, B, N)
    second["x"] = flat.data_ptr() + 4
    third, keep_third = _all_asked(devs[2], True, B, N)
    _launch([second, first, third], B, N)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(alone, in_table))
    assert not bool(torch.isnan(alone[0]).any()) and float(alone[1].abs().max()) > 0


def test_nine_norms_through_ops_run_one_launch_each():
    """More than BN_GROUP_MAX norms: one ct_bn_eval_group_bwd launch of n = 1 per norm, as _bn_runs rules."""
    from cloud_transformers_amd import _lib, ops
    B, N, Cs = 2, 260, (3, 4, 5, 6, 7, 8, 9, 10, 12)
    cases = [_int_case(B, c, N, 70 + c) for c in Cs]
    refs = [_int_ref(c, True) for c in cases]
    bns, xs = [], []
    for c, case in zip(Cs, cases):
        bn = nn.BatchNorm1d(c, eps=0.0).cuda().eval()
        with torch.no_grad():
            bn.weight.copy_(case["w"].float()), bn.bias.copy_(case["b"].float()), bn.running_mean.copy_(case["rm"].float())
        bns.append(bn)
        xs.append(case["x"].float().cuda().requires_grad_(True))
    lib = _lib.load()
    real, calls = lib.ct_bn_eval_group_bwd, []
    lib.ct_bn_eval_group_bwd = lambda items, n, *a: (calls.append(n), real(items, n, *a))[1]
    try:
        y = ops.join_bn_relu_frozen(xs, bns)
        assert torch.equal(y.detach().cpu(), torch.cat([r["y"] for r in refs], dim=1))
        y.backward(torch.cat([c["gy"] for c in cases], dim=1).float().cuda())
    finally:
        lib.ct_bn_eval_group_bwd = real
    assert calls == [1] * len(Cs), calls
    for x, bn, ref in zip(xs, bns, refs):
        _equal((x.grad, bn.weight.grad, bn.bias.grad, None), ref, "C = %d" % bn.num_features)


# ---------------------------------------------------------------------------------------------------------------------
# rounding, mask
# ---------------------------------------------------------------------------------------------------------------------
def _float_case(B, C, N, offset):
    """Random fp32 inputs on the CPU; offset: running_mean = offset + ..., x = running_mean + N(0, 1) — the cancellation case."""
    g = torch.Generator().manual_seed(B * 100 + C + int(offset))
    rm = torch.rand(C, generator=g) * 2 - 1 + offset
    noise = torch.randn(B, C, N, generator=g)
    x = rm[None, :, None] + noise if offset else noise * 3 + 0.7
    w = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()     # both signs, none zero
    gy = torch.randn(B, C, N, generator=g)
    gy = torch.where(gy.abs() < 0.1, torch.full_like(gy, 0.1), gy)                                         # none zero
    return dict(x=x, gy=gy, w=w, b=torch.rand(C, generator=g) - 0.5, rm=rm, rv=torch.rand(C, generator=g) * 1.5 + 0.5, eps=1e-5)


def _ref64(p, mask):
    """float64 on the host from the fp32 inputs; mask (bool [B,C,N] or None): where the forward stored a positive value."""
    x, gy = p["x"].double(), p["gy"].double()
    w, rm = p["w"].double()[None, :, None], p["rm"].double()[None, :, None]
    rs = (1.0 / torch.sqrt(p["rv"].double() + p["eps"]))[None, :, None]
    M = x.size(0) * x.size(2)
    g = gy if mask is None else gy * mask.double()
    xh = (x - rm) * rs
    unit = 2.0 ** -24
    return dict(gx=g * (w * rs), gx_bound=(g * (w * rs)).abs() * 2.0 ** -21,
                gb=g.sum((0, 2)), gb_bound=(M + 8) * unit * g.abs().sum((0, 2)),
                gw=(g * xh).sum((0, 2)), gw_bound=(M + 8) * unit * (g * xh).abs().sum((0, 2)))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("B,C,N,offset", ROUNDING)
def test_rounding_against_float64(B, C, N, offset, relu):
    from cloud_transformers_amd import ops
    p = _float_case(B, C, N, offset)
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in p.items()}
    mask = None
    if relu:                                    # what the forward stored decides which elements pass
        y = torch.empty(B, C, N, device="cuda")
        ops._bn_eval_group([dict(x=d["x"].data_ptr(), xbs=0, C=C, w=d["w"], b=d["b"], rm=d["rm"], rv=d["rv"], eps=d["eps"], relu=1,
                                 res=None, rbs=0, y=y.data_ptr(), ybs=0, amax=None)], B, N)
        mask = (y > 0).cpu()
        assert 0.2 < float(mask.float().mean()) < 0.8
    ref = _ref64(p, mask)
    item, (gx, gw, gb, am) = _all_asked(d, relu, B, N)
    _launch([item], B, N)
    for name, got in (("gx", gx), ("gw", gw), ("gb", gb)):
        err = (got.cpu().double() - ref[name]).abs()
        worst = float((err / ref[name + "_bound"].clamp_min(1e-300)).max())
        print("%s %s: max |err| %.3e, worst err / bound %.3f" % ((B, C, N, offset, relu), name, float(err.max()), worst))
        assert bool((err <= ref[name + "_bound"]).all()), (name, float(err.max()), worst)
    assert torch.equal(am, gx.abs().amax((0, 2)))                              # the maxima of the values as stored


@pytest.mark.parametrize("B,C,N,offset", ROUNDING)
def test_mask_is_the_forward_s(B, C, N, offset):
    """relu on, no residual, no zero in gy or the weights: gx is zero exactly where the forward stored a zero."""
    from cloud_transformers_amd import ops
    p = _float_case(B, C, N, offset)
    bn = nn.BatchNorm1d(C, eps=p["eps"]).cuda().eval()
    with torch.no_grad():
        bn.weight.copy_(p["w"]), bn.bias.copy_(p["b"]), bn.running_mean.copy_(p["rm"]), bn.running_var.copy_(p["rv"])
    x = p["x"].cuda().requires_grad_(True)
    y = ops.bn_frozen(x, bn, relu=True)
    with torch.no_grad():
        assert torch.equal(y, ops.bn_eval(x.detach(), bn, relu=True))          # the eval function's launch, the same bits
    y.backward(p["gy"].cuda())
    zeros = y.detach() == 0
    assert 0.2 < float(zeros.float().mean()) < 0.8
    assert torch.equal(x.grad == 0, zeros)


# ---------------------------------------------------------------------------------------------------------------------
# autograd through the ops against torch modules in eval mode
# ---------------------------------------------------------------------------------------------------------------------
def _grads(outs, cots, leaves):
    return torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cots)), leaves, allow_unused=True)


def _params(mods):
    return [p for m in mods for p in m.parameters()]


def _compare(run_fused, run_plain, inputs, fused_mods, what):
    """Forward and every gradient of run_fused(inputs, fused_mods) against run_plain(inputs', unmarked eval copies)."""
    from cloud_transformers_amd import norms_frozen, unfreeze_norms
    plain_mods = copy.deepcopy(fused_mods)
    for m in plain_mods:
        unfreeze_norms(m)
        m.eval()
        assert norms_frozen(m) is False
    before = _stats(*fused_mods)
    a = [t.clone().requires_grad_(True) for t in inputs]
    b = [t.clone().requires_grad_(True) for t in inputs]
    got, want = run_fused(a, fused_mods), run_plain(b, plain_mods)
    torch.manual_seed(1)
    cots = [torch.randn_like(o) for o in want]
    for i, (g, w) in enumerate(zip(got, want)):
        _agree(g.detach(), w.detach(), "%s output %d" % (what, i))
    g_got = _grads(got, cots, a + _params(fused_mods))
    g_want = _grads(want, cots, b + _params(plain_mods))
    names = ["input %d" % i for i in range(len(a))] + [n for m in fused_mods for n, _ in m.named_parameters()]
    assert len(g_got) == len(g_want) == len(names)
    for name, g, w in zip(names, g_got, g_want):
        assert (g is None) == (w is None), name
        if g is not None:
            _agree(g, w, "%s grad %s" % (what, name))
    assert all(torch.equal(s, t) for s, t in zip(before, _stats(*fused_mods)))          # statistics, num_batches_tracked


@pytest.mark.parametrize("relu,with_res", [(True, False), (True, True), (False, False)])
def test_bn_frozen_matches_the_module(relu, with_res):
    from cloud_transformers_amd import ops
    torch.manual_seed(2)
    B, C, N = 4, 32, 512
    bn = _frozen_norm(C, 11).cuda()
    inputs = [torch.randn(B, C, N, device="cuda") * 2 + 0.3] + ([torch.randn(B, C, N, device="cuda")] if with_res else [])

    def fused(t, mods):
        assert ops.bn_frozen_eligible(mods[0], t[0], residual=t[1] if with_res else None)
        return [ops.bn_frozen(t[0], mods[0], relu=relu, residual=t[1] if with_res else None)]

    def plain(t, mods):
        y = mods[0](t[0])
        y = torch.relu(y) if relu else y
        return [y + t[1] if with_res else y]

    _compare(fused, plain, inputs, [bn], "bn_frozen relu=%s res=%s" % (relu, with_res))


@pytest.mark.parametrize("B,Ca,Cb,N", [(4, 12, 40, 1024), (3, 3, 5, 1001)])
def test_split_bn_frozen_matches_the_modules_on_split_views(B, Ca, Cb, N):
    from cloud_transformers_amd import ops
    torch.manual_seed(3)
    mods = [_frozen_norm(Ca, 31).cuda(), _frozen_norm(Cb, 32).cuda()]

    def fused(t, mods):
        assert ops.bn_frozen_eligible(mods[0], t[0], Ca) and ops.bn_frozen_eligible(mods[1], t[0], Cb)
        return list(ops.split_bn_frozen(t[0], mods[0], mods[1]))

    def plain(t, mods):
        a, b = torch.split(t[0], [Ca, Cb], dim=1)
        return [mods[0](a), mods[1](b)]

    _compare(fused, plain, [torch.randn(B, Ca + Cb, N, device="cuda") * 2 + 0.3], mods, "split_bn_frozen N=%d" % N)


@pytest.mark.parametrize("N", [1024, 1022])
def test_join_bn_relu_frozen_matches_cat_of_the_modules(N):
    from cloud_transformers_amd import ops
    torch.manual_seed(4)
    B, Cs = 4, (16, 24)
    mods = [_frozen_norm(c, 40 + c).cuda() for c in Cs]

    def fused(t, mods):
        return [ops.join_bn_relu_frozen(t, mods)]

    def plain(t, mods):
        return [torch.cat([torch.relu(m(x)) for m, x in zip(mods, t)], dim=1)]

    _compare(fused, plain, [torch.randn(B, c, N, device="cuda") * 2 - 0.2 for c in Cs], mods, "join_bn_relu_frozen N=%d" % N)


@pytest.mark.parametrize("passthrough", [False, True])
@pytest.mark.parametrize("Cin,spec", [(32, [(12, 16), (6, 40)]), (128, [(48, 128), (48, 128)])])
def test_union_keys_values_frozen_matches_per_head_modules(Cin, spec, passthrough):
    """The specs of tests/test_bn_eval_gpu.py::test_union_keys_values_eval_equals_per_head_modules, with gradients: one stacked GEMM
    and its two gradient GEMMs around the 2n frozen norms against conv_i -> split -> key_bn_i / values_bn_i in eval mode;
    passthrough: x is an output of the node too and its cotangent rides the data gradient's epilogue."""
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers.pointwise import PointwiseConv1d
    torch.manual_seed(8)
    B, N, n = 4, 512, len(spec)
    convs = [PointwiseConv1d(Cin, ck + cv, kernel_size=1, bias=False).cuda() for ck, cv in spec]
    kbs = [_frozen_norm(ck, 80 + i).cuda() for i, (ck, _) in enumerate(spec)]
    vbs = [_frozen_norm(cv, 90 + i).cuda() for i, (_, cv) in enumerate(spec)]

    def fused(t, mods):
        convs, kbs, vbs = mods[:n], mods[n:2 * n], mods[2 * n:]
        assert ops.union_keys_values_frozen_eligible(t[0], convs, kbs, vbs)
        if passthrough:
            skip, kvs = ops.union_keys_values_frozen(t[0], convs, kbs, vbs, passthrough=True)
            return [skip] + [o for kv in kvs for o in kv]
        return [o for kv in ops.union_keys_values_frozen(t[0], convs, kbs, vbs) for o in kv]

    def plain(t, mods):
        convs, kbs, vbs = mods[:n], mods[n:2 * n], mods[2 * n:]
        outs = [t[0] * 1.0] if passthrough else []
        for conv, kb, vb, (ck, cv) in zip(convs, kbs, vbs, spec):
            a, b = torch.split(conv(t[0]), [ck, cv], dim=1)
            outs += [kb(a.contiguous()), vb(b.contiguous())]
        return outs

    _compare(fused, plain, [torch.randn(B, Cin, N, device="cuda")], convs + kbs + vbs, "union Cin=%d passthrough=%s" % (Cin, passthrough))


def test_frozen_affine_parameters_take_no_gradient_and_ask_for_no_sums():
    """affine=True: the norms' parameters do not require grad — ct_bn_eval_group_bwd gets null g_weight / g_bias and the input
    gradient carries the bits of the run with trainable parameters."""
    from cloud_transformers_amd import _lib, freeze_norms, ops
    torch.manual_seed(5)
    B, C, N = 4, 32, 512
    bn = _frozen_norm(C, 13).cuda()
    x0, gy = torch.randn(B, C, N, device="cuda"), torch.randn(B, C, N, device="cuda")
    x = x0.clone().requires_grad_(True)
    ops.bn_frozen(x, bn).backward(gy)
    want = x.grad.clone()
    assert bn.weight.grad is not None and bn.bias.grad is not None
    bn.zero_grad(set_to_none=True)
    freeze_norms(bn, affine=True)
    lib = _lib.load()
    real, seen = lib.ct_bn_eval_group_bwd, []

    def spy(items, n, *a):
        it = ctypes.cast(ctypes.c_void_p(items), ctypes.POINTER(_lib.BnEvalBwdItem))[0]
        seen.append((it.g_weight, it.g_bias, bool(it.gx)))
        return real(items, n, *a)

    lib.ct_bn_eval_group_bwd = spy
    try:
        x = x0.clone().requires_grad_(True)
        ops.bn_frozen(x, bn).backward(gy)
    finally:
        lib.ct_bn_eval_group_bwd = real
    assert seen == [(None, None, True)], seen
    assert bn.weight.grad is None and bn.bias.grad is None and torch.equal(x.grad, want)
