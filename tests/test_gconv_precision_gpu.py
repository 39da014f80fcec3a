"""CT_GCONV_PRECISION_HIGH on the GPU, straight through the C ABI unless said otherwise: the documented bound (include/cloudct.h)
against float64 on every branch of the quad and K-split kernels, the integer probe that shows the mode took effect and only where
the planner says it covers, the default mode untouched, zeros / NaN / inf, the bit equalities within the mode, the layer's
backward-data in its forward's mode, graph capture, Trainer.fit.

The probe (as tests/test_pw_precision_gpu.py): 4097 = 2^12 + 1 needs 13 significand bits, so under its scale 2 the one-term kernel
rounds it to 8192 / 2 = 4096 while fp32 keeps 4097; every other operand is 0 or 1, so nothing else rounds."""
import contextlib
import threading

import pytest
import torch

from tests import gconv_families as F
from tests import gconv_precision_common as C
from tests import test_gconv_families_gpu as T
from tests.test_gconv_families_gpu import bound, inputs, reference

pytestmark = pytest.mark.gpu

PROBE_COVERED = [(2, 3, 16, 16, (32, 32)), (1, 2, 16, 16, (16, 16, 16)), (1, 2, 64, 64, (8, 8, 8)), (1, 2, 32, 32, (40, 32))]
PROBE_UNCOVERED = [(2, 4, 4, 4, (16, 16)), (1, 1, 5, 7, (9, 11))]          # four-channel, one-position


def _lib():
    from cloud_transformers_amd import _lib as L
    return L.load()


@contextlib.contextmanager
def _high():
    lib = _lib()
    assert lib.ct_get_gconv_precision() == 0
    lib.ct_set_gconv_precision(1)
    try:
        yield
    finally:
        lib.ct_set_gconv_precision(0)
    assert lib.ct_get_gconv_precision() == 0


def _covers(p, s):
    from cloud_transformers_amd import _lib as L
    return L.load().ct_gconv_precision_covers(p, s[0], s[1], s[2], s[3], len(s[4]), L.int_array(list(s[4])))


def _run(api, shape, ops, bias=True):
    """one call through the families test's guarded buffers -> (the output tensor, the tag)"""
    rc, tag, outs, every = T.call(api, shape, ops, bias=bias)
    assert rc == F.CT_OK, (api, shape, rc)
    assert all(t.guards_intact() for t in every), (api, shape, "wrote outside a tensor")
    out = outs["y" if api == F.FWD else "g_x"].view
    return out, tag


def _check_bound(shape, ops, bwd, scale=1.0):
    x, w, b, cin, cout = C.as_forward(shape, ops, bwd, scale)
    ref, bnd = C.high_bound(shape, x, w, b, cin, cout)
    dev = {k: (v * scale if k in ("x", "w", "g_y") else v) for k, v in ops.items()}
    with _high():
        got, _ = _run(F.BWD if bwd else F.FWD, shape, dev)
    assert torch.isfinite(got).all()
    ratio = float(((got.double().cpu() - ref).abs() / bnd).max())
    print("%s %s scale %g: worst err / bound %.3f" % (C.shape_id(shape), "bwd" if bwd else "fwd", scale, ratio))
    assert ratio <= 1.0, (shape, bwd, scale, ratio)


@pytest.mark.parametrize("shape", C.FWD_SHAPES, ids=C.shape_id)
def test_forward_stays_inside_the_bound(shape):
    assert _covers(0, shape) == 1
    _check_bound(shape, inputs(shape, "scaled"), False)


@pytest.mark.parametrize("shape", C.BWD_SHAPES, ids=C.shape_id)
def test_backward_data_stays_inside_the_bound(shape):
    assert _covers(1, shape) == 1
    _check_bound(shape, inputs(shape, "scaled"), True)


@pytest.mark.parametrize("shape", [(1, 3, 16, 48, (8, 8)), (3, 2, 48, 40, (4, 8, 8))], ids=C.shape_id)
@pytest.mark.parametrize("scale", [2.0 ** 20, 2.0 ** -20])
def test_operands_beyond_the_f16_range(shape, scale):
    _check_bound(shape, inputs(shape, "scaled"), False, scale)


def _probe(shape, bwd):
    """one 4097 in the input, one weight tap 1 (the centre tap of (co 1, ci 2) of the last group) -> the output element it reaches"""
    B, G, Cin, Cout, W = shape
    d = len(W)
    pos = tuple(e // 2 for e in W)
    ops = {"x": torch.zeros(B, G * Cin, *W), "w": torch.zeros(G * Cout, Cin, *([3] * d)), "b": torch.zeros(G * Cout),
           "g_y": torch.zeros(B, G * Cout, *W)}
    co, ci = (G - 1) * Cout + 1, 2
    ops["w"][(co, ci) + (1,) * d] = 1.0
    ops["g_y" if bwd else "x"][(B - 1, co if bwd else (G - 1) * Cin + ci) + pos] = 4097.0
    out, tag = _run(F.BWD if bwd else F.FWD, shape, ops)
    at = (B - 1, (G - 1) * Cin + ci if bwd else co) + pos
    assert int((out != 0).sum()) == 1, "the probe reaches one output"
    return float(out[at]), tag


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("shape", PROBE_COVERED + PROBE_UNCOVERED, ids=C.shape_id)
def test_the_mode_took_effect_and_only_where_covered(shape, bwd):
    covered = shape in PROBE_COVERED
    assert _covers(int(bwd), shape) == int(covered)
    v0, tag0 = _probe(shape, bwd)
    with _high():
        v1, tag1 = _probe(shape, bwd)
    assert v0 == 4097.0
    assert v1 == (4096.0 if covered else 4097.0), (shape, v1)
    assert tag1 == tag0 and tag0 != ""


@pytest.mark.parametrize("row", ["dense3d_ragged_channels", "ksplit_one_64_8cube", "quad_16_32sq"])
def test_every_variant_of_a_family_notes_the_plain_calls_tags(row):
    """one launch function per family picks among plain / NORM / F16 / NORM + F16 after it has noted the tags: the four calls on a
    shape note the same string, the row's (dense has no F16 variant: the mode changes nothing there; 8^3 has the four spans the
    K-split one-term kernel asks for; 16 input channels per group are the quad one's threshold)"""
    from tests import test_gconv_norm_gpu as N
    r = next(r for r in F.ROWS if r.id == row)
    shape = (r.B, r.G, r.Cin, r.Cout, r.W)
    assert _covers(0, shape) == (0 if row.startswith("dense") else 1)
    ops = inputs(shape, "plain")
    tags = {"plain": _run(F.FWD, shape, ops, bias=r.bias)[1], "norm": N._fused(shape, "norm_relu")[1]}
    with _high():
        tags["high"] = _run(F.FWD, shape, ops, bias=r.bias)[1]
        rc, tags["norm+high"], y = N._fused(shape, "normed_skip_relu")
    assert rc == F.CT_OK and y.guards_intact()
    assert tags == dict.fromkeys(tags, r.tag), tags


@pytest.mark.parametrize("shape", [(2, 3, 16, 16, (32, 32)), (1, 2, 64, 64, (8, 8, 8))], ids=C.shape_id)
def test_default_untouched_by_a_high_call(shape):
    ops = inputs(shape, "scaled")
    before = {api: _run(api, shape, ops)[0].clone() for api in (F.FWD, F.BWD)}
    with _high():
        high = {api: _run(api, shape, ops)[0].clone() for api in (F.FWD, F.BWD)}
    assert _lib().ct_get_gconv_precision() == 0
    ref = reference(shape, "scaled", True, only=("y", "g_x"))
    for api, key in ((F.FWD, "y"), (F.BWD, "g_x")):
        after = _run(api, shape, ops)[0]
        assert torch.equal(before[api], after)
        assert not torch.equal(high[api], after)
        r, mag, K = ref[key]
        assert bool(((after.double().cpu() - r).abs() <= bound(mag, K)).all())


@pytest.mark.parametrize("shape", [(1, 3, 16, 48, (8, 8)), (1, 2, 16, 16, (16, 16, 16)), (3, 2, 48, 40, (4, 8, 8))], ids=C.shape_id)
def test_zeros_nan_and_inf(shape):
    B, G, Cin, Cout, W = shape
    ops = dict(inputs(shape, "plain"))
    ones = [1] * len(W)
    zero_x = dict(ops, x=torch.zeros_like(ops["x"]))
    zero_row = dict(ops, w=ops["w"].clone())
    zero_row["w"][Cout + 3] = 0.0
    special = dict(ops, x=ops["x"].clone())
    pos = tuple(e // 2 for e in W)
    special["x"][(0, 1) + pos] = float("nan")
    special["x"][(B - 1, G * Cin - 1) + tuple(e // 2 - 1 for e in W)] = float("inf")
    want = _run(F.FWD, shape, special)[0]
    with _high():
        z = _run(F.FWD, shape, zero_x)[0]
        r = _run(F.FWD, shape, zero_row)[0]
        s = _run(F.FWD, shape, special)[0]
    assert torch.equal(z.cpu(), ops["b"].reshape(1, -1, *ones).expand_as(z).contiguous())
    assert torch.equal(r[:, Cout + 3].cpu(), ops["b"][Cout + 3].expand_as(r[:, Cout + 3]).contiguous())
    assert torch.isfinite(r).all()
    assert torch.equal(torch.isnan(s), torch.isnan(want)) and torch.equal(torch.isinf(s), torch.isinf(want))
    assert 0 < int((~torch.isfinite(s)).sum()) < s.numel() // 2


@pytest.mark.parametrize("shape", [(1, 3, 16, 48, (8, 8)), (3, 2, 48, 40, (4, 8, 8))], ids=C.shape_id)
def test_fwd_norm_is_the_composed_sequence_bit_for_bit_in_high(shape):
    from cloud_transformers_amd import _lib as L, ops as O
    from tests import test_gconv_norm_gpu as N
    lib = L.load()
    c = N._case(shape)
    B, G, Cin, Cout, W = shape
    with _high():
        scratch = torch.empty(B, G * Cout, *W, device="cuda")
        L.check(lib.ct_gconv_fwd(c["x"].data_ptr(), c["w"].data_ptr(), c["b"].data_ptr() if c["b"] is not None else None,
                                 scratch.data_ptr(), B, G, Cin, Cout, len(W), L.int_array(W), O._stream()), "ct_gconv_fwd")
        tag = lib.ct_debug_last_launch().decode()
        for variant in ("norm_relu", "identity_skip_relu", "normed_skip_relu"):
            rc, ftag, y = N._fused(shape, variant)
            assert rc == F.CT_OK and ftag == tag and y.guards_intact()
            if "skip" not in variant:
                want = N._bn_eval(scratch, c["n"], c["eps"], True)
            else:
                t = N._bn_eval(c["skip"], c["sn"], c["seps"], False) if variant == "normed_skip_relu" else c["skip"]
                want = torch.relu(torch.add(N._bn_eval(scratch, c["n"], c["eps"], False), t))
            assert torch.equal(y.view, want), (variant, int((y.view != want).sum()))
    assert not torch.equal(scratch, N._plain(shape)[0])                  # (and the scratch was a one-term result)


@pytest.mark.parametrize("shape", [(2, 3, 16, 16, (32, 32)), (1, 2, 16, 16, (16, 16, 16)), (1, 2, 64, 64, (16, 16, 16)),
                                   (1, 1, 64, 64, (64, 64))], ids=C.shape_id)
def test_two_runs_are_bit_equal(shape):
    ops = inputs(shape, "scaled")
    with _high():
        for api in (F.FWD, F.BWD):
            assert torch.equal(_run(api, shape, ops)[0], _run(api, shape, ops)[0])


@pytest.mark.parametrize("dim", [2, 3])
def test_layer_backward_keeps_the_forwards_mode(dim):
    """GroupedConv{2,3}d, 2 groups of 16 -> 16 channels: the forward inside the scope, .backward() outside it and on a second
    thread.  x holds one 4097 and the weights one tap 1, the cotangent one 4097: y and g_x show the probe."""
    import cloud_transformers_amd as ct
    from cloud_transformers_amd.layers.gconv import GroupedConv2d, GroupedConv3d
    W = (16, 16) if dim == 2 else (8, 8, 8)
    pos = tuple(e // 2 for e in W)
    layer = (GroupedConv2d if dim == 2 else GroupedConv3d)(32, 32, 3, padding=1, groups=2).cuda()
    with torch.no_grad():
        layer.weight.zero_()
        layer.bias.zero_()
        layer.weight[(17, 2) + (1,) * dim] = 1.0
    seed = torch.zeros(2, 32, *W, device="cuda")
    seed[(1, 17) + pos] = 4097.0
    xin = torch.rand(2, 32, *W, device="cuda")
    g_w = {}
    for mode, other, want in (("high", "highest", 4096.0), ("highest", "high", 4097.0)):
        x = torch.zeros(2, 32, *W, device="cuda")
        x[(1, 18) + pos] = 4097.0
        x.requires_grad_(True)
        layer.weight.grad = None
        with ct.conv_precision(mode):
            y = layer(x)
        assert float(y.detach()[(1, 17) + pos]) == want
        assert ct.get_conv_precision() == "highest"
        with ct.conv_precision(other):                   # the other mode while the backward runs, on another thread
            t = threading.Thread(target=lambda: y.backward(seed))
            t.start()
            t.join()
        assert float(x.grad[(1, 18) + pos]) == want and int((x.grad != 0).sum()) == 1
        # the weight gradient is fp32 in every mode: random operands, the same bits whichever mode the forward ran in
        layer.weight.grad = None
        xr = xin.clone().requires_grad_(True)
        with ct.conv_precision(mode):
            yr = layer(xr)
        yr.backward(torch.ones_like(yr) * 0.37)
        g_w[mode] = layer.weight.grad.clone()
    assert torch.equal(g_w["high"], g_w["highest"])
    assert _lib().ct_get_gconv_precision() == 0


def test_a_captured_graph_keeps_the_mode_it_was_recorded_in():
    import cloud_transformers_amd as ct
    from cloud_transformers_amd.layers.gconv import GroupedConv2d
    layer = GroupedConv2d(32, 32, 3, padding=1, groups=2).cuda()
    with torch.no_grad():
        layer.weight.zero_()
        layer.bias.zero_()
        layer.weight[17, 2, 1, 1] = 1.0
    x = torch.zeros(2, 32, 16, 16, device="cuda")
    x[1, 18, 8, 8] = 4097.0
    with torch.no_grad(), ct.conv_precision("high"):
        layer(x)                                         # (the library is loaded and the plan's LDS attribute set before the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = layer(x)
    with torch.no_grad():
        assert float(layer(x)[1, 17, 8, 8]) == 4097.0    # the scope has ended
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert float(out[1, 17, 8, 8]) == 4096.0 and int((out != 0).sum()) == 1


def test_trainer_config_switch_is_in_force_inside_fit_and_gone_after():
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import harness as H
    from cloud_transformers_amd.layers.gconv import GroupedConv2d
    layer = GroupedConv2d(32, 32, 3, padding=1, groups=2).cuda()
    with torch.no_grad():
        layer.weight.zero_()
        layer.bias.zero_()
        layer.weight[17, 2, 1, 1] = 1.0
    x = torch.zeros(2, 32, 16, 16, device="cuda")
    x[1, 18, 8, 8] = 4097.0

    def probe():
        with torch.no_grad():
            return float(layer(x)[1, 17, 8, 8])

    class Stub:
        cfg = {"train": {"conv_precision": "high"}}

        def _fit(self, max_iters, hip_graph, log_each):
            return [probe()]

    assert probe() == 4097.0
    assert H.Trainer.fit(Stub(), max_iters=1) == [4096.0]
    assert probe() == 4097.0 and ct.get_conv_precision() == "highest" and _lib().ct_get_gconv_precision() == 0
