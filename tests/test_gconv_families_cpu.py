"""The table of grouped-convolution kernel families (tests/gconv_families.py) names every launch tag of csrc/ct_gconv.hip: the string
literals passed to note() are exactly the tags its rows cover or mark unreachable; the rows are well formed (the library plans
without a GPU); and the float64 reference / magnitude helpers and the element-wise bound of tests/test_gconv_families_gpu.py hold
for a plain fp32 convolution on the CPU (the bound does not reject a correct fp32 result)."""
import os

import pytest
import torch

from tests import gconv_families as F
from tests import test_gconv_families_gpu as T
from tests.test_raster_families_cpu import note_literals

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cloud_transformers_amd", "csrc", "ct_gconv.hip")


def _tags():
    with open(SRC) as f:
        return note_literals(f.read())


def test_every_note_literal_has_a_row_and_every_row_a_literal():
    tags = _tags()
    assert len(tags) >= 25, sorted(tags)
    covered = F.covered_tags()
    assert not tags - covered, "launch tags without a row in tests/gconv_families.py: %s" % sorted(tags - covered)
    assert not covered - tags, "rows naming tags csrc/ct_gconv.hip no longer has: %s" % sorted(covered - tags)


def test_removing_a_row_or_adding_a_literal_is_caught():
    with open(SRC) as f:
        text = f.read()
    tags = note_literals(text)
    assert "x_new" not in tags
    assert note_literals(text + '\nvoid f() { note("x_new"); }') - F.covered_tags() == {"x_new"}
    for drop in ("ksplit_items2", "wrw_tiles", "onepos_msplit", "dense2d", "bias_grad"):
        rest = set(F.UNREACHABLE)
        for r in F.ROWS:
            if drop not in r.tag.split("+"):
                rest.update(t for t in r.tag.split("+") if t)
        assert drop in tags - rest, drop


def test_every_launch_site_is_tagged():
    """as many note() calls as kernel launches would be too strict (macros launch template variants); what must hold is that every
    function that launches a kernel also notes a tag"""
    import re
    with open(SRC) as f:
        text = f.read()
    host = text[text.index("bool plan_tiles_min_halo"):]
    bodies = re.split(r"\n(?=(?:int|bool|size_t|template <typename K>\nint) \w+\()", host)
    launchers = [b for b in bodies if "hipLaunchKernelGGL" in b]
    assert len(launchers) == 13      # one per family: six forward, six weight-gradient, and ct_gconv_bwd_weight's own bias_grad
    for b in launchers:
        assert re.search(r"(?<![\w.])note\(", b), b.split("{")[0]


def test_rows_are_well_formed():
    from cloud_transformers_amd import _lib
    _lib.build()
    lib = _lib.load()
    ids = [r.id for r in F.ROWS]
    assert len(ids) == len(set(ids))
    for r in F.ROWS:
        assert r.api in _lib.SIGNATURES and r.api in (F.FWD, F.BWD, F.WRW), r
        assert len(r.W) in (2, 3) and min(r.B, r.G, r.Cin, r.Cout, *r.W) >= 1, r
        assert r.Cin >= 3, "a row needs an all-zero input channel next to its 1e-4 .. 1e4 channels"
        assert set(r.offset4) <= {"x", "w", "y", "g_y", "g_x"}, r
        assert (r.ws in ("query", None, "short")) and (r.api == F.WRW or r.ws is None), r
        assert r.rc in (F.CT_OK, F.CT_EINVAL, F.CT_EWORKSPACE) and (r.rc == F.CT_OK or r.tag == ""), r
        Wa = _lib.int_array(r.W)
        shape = (r.B, r.G, r.Cin, r.Cout, r.W)
        assert lib.ct_gconv_supported(r.B, r.G, r.Cin, r.Cout, len(r.W), Wa) == (0 if shape == F.NOPLAN else 1), r
        if r.ws in ("query", "short"):
            assert lib.ct_gconv_bwd_weight_workspace_bytes(r.B, r.G, r.Cin, r.Cout, len(r.W), Wa) > 0, r
        if r.ws == "short":
            assert lib.ct_gconv_bwd_weight_workspace_bytes(r.B, r.G, r.Cin, r.Cout, len(r.W), Wa) >= 32, r
        if shape != F.NOPLAN:
            # the reference of a row takes about a second on the host (one row needs >= 2 M positions: c4_mfma3_by_size)
            macs = r.B * r.G * r.Cin * r.Cout * 3 ** len(r.W) * T.volume(r.W)
            assert macs <= (1 << 30) or r.id == "c4_mfma3_by_size", (r.id, macs)
    assert lib.ct_gconv_supported(*F.NOPLAN_WRW[:4], len(F.NOPLAN_WRW[4]), _lib.int_array(F.NOPLAN_WRW[4])) == 0
    noplan = [r for r in F.ROWS if (r.B, r.G, r.Cin, r.Cout, r.W) == F.NOPLAN]
    assert {r.api for r in noplan} == {F.FWD, F.BWD, F.WRW}
    assert all(r.rc in (F.CT_OK, F.CT_EINVAL) for r in noplan) and any(r.rc == F.CT_EINVAL for r in noplan)
    # the four-channel unaligned weight-gradient rows ask for CT_OK with the queried workspace
    c4u = [r for r in F.ROWS if r.api == F.WRW and r.Cin == 4 and r.offset4]
    assert len(c4u) >= 2 and all(r.rc == F.CT_OK and r.ws == "query" and r.W[-1] % 4 == 0 for r in c4u)
    assert {r.offset4 for r in c4u} >= {("x",), ("g_y",)}


def test_debug_bits_are_documented_in_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "cloudct.h")) as f:
        text = f.read()
    doc = text[text.index("Test hook of the grouped convolution"):text.index("void ct_debug_set_gconv")]
    for word in ("bit 0", "bit 1", "bit 2", "bits 8..15"):
        assert word in doc, word


BY_SIZE = next((r.B, r.G, r.Cin, r.Cout, r.W) for r in F.ROWS if r.id == "c4_mfma3_by_size")
HOST_SHAPES = [s for s in F.shapes() if s != BY_SIZE]      # (the >= 2 M-position shape: the same kernels as the small four-channel ones)


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=[T.shape_id(s) for s in HOST_SHAPES])
def test_bound_accepts_a_plain_fp32_convolution_and_integers_are_exact(shape):
    """For every shape of the table: torch's own fp32 CPU convolution and its gradients stay inside the element-wise bound on the
    scaled inputs (the bound is a worst-case one: it must never reject a correct fp32 sum) and equal float64 exactly on the integer
    inputs; the inputs and the float64 reference reproduce themselves."""
    assert len(HOST_SHAPES) == len(F.shapes()) - 1
    for kind in ("scaled", "int"):
        ops = T.inputs(shape, kind)
        ref = T.reference(shape, kind, bias=True)
        if shape in (HOST_SHAPES[0], HOST_SHAPES[-1], F.NOPLAN):
            assert all(torch.equal(ops[k], v) for k, v in T.make_inputs(shape, kind).items())
            again = T.reference(shape, kind, bias=True, cached=False)
            for k in ref:
                assert torch.equal(ref[k][0], again[k][0]) and torch.equal(ref[k][1], again[k][1]), (k, kind)
        got = T.fp32_cpu(shape, ops)
        for k, (want, mag, K) in ref.items():
            if kind == "int":
                assert float(mag.max()) < 2 ** 24
                assert torch.equal(got[k].double(), want), (k, shape)
            else:
                worst = float(((got[k].double() - want).abs() / T.bound(mag, K)).max())
                assert worst <= 1.0, (k, shape, worst)


def test_backward_operator_is_autograd():
    """the references ask aten::convolution_backward for single cotangents; it is what autograd runs for conv2d / conv3d"""
    for shape in ((2, 2, 5, 7, (6, 9)), (1, 2, 4, 6, (3, 4, 5))):
        ops = {k: v.double() for k, v in T.make_inputs(shape, "plain").items()}
        x, w, b = (ops[k].clone().requires_grad_(True) for k in ("x", "w", "b"))
        y = T._conv(len(shape[4]))(x, w, b, padding=1, groups=shape[1])
        want = torch.autograd.grad(y, (x, w, b), ops["g_y"])
        got = T._all_three(shape, ops["x"], ops["w"], ops["b"], ops["g_y"])
        assert torch.equal(got["y"], y.detach())
        for k, g in zip(("g_x", "g_w", "g_b"), want):
            assert torch.equal(got[k], g), k


class _Host:
    """stands in for a device tensor of tests/test_gconv_families_gpu.py: check_against reads `.view`"""

    def __init__(self, t):
        self.view = t


def _mutants(shape, ops):
    """fp32 CPU results with the slips the bars are there for: a flipped tap, a border row dropped, one small-magnitude channel
    off by 1e-3 of itself, one element left unwritten"""
    flipped = dict(ops, w=ops["w"].flip(-1))
    yield "tap flip", T.fp32_cpu(shape, flipped)["y"]
    y = T.fp32_cpu(shape, ops)["y"]
    x0 = ops["x"].clone()
    x0[..., 0, :] = 0                                              # the first row of the volume never reached the halo
    yield "border row", T.fp32_cpu(shape, dict(ops, x=x0))["y"]
    small = y.clone()
    c = int(y.abs().flatten(2).max(-1).values.min(0).values.argmin())
    small[:, c] *= 1.001
    yield "small channel", small
    hole = y.clone()
    hole.view(-1)[-1] = float("nan")
    yield "unwritten", hole


@pytest.mark.parametrize("kind", ["scaled", "int"])
def test_the_bars_reject_the_slips_they_are_there_for(kind):
    shape = (2, 2, 8, 8, (6, 12))
    ops = T.inputs(shape, kind)
    ref = T.reference(shape, kind, True, ("y",))
    T.check_against({"y": _Host(T.fp32_cpu(shape, ops)["y"])}, ref, "clean", exact=kind == "int")
    for name, y in _mutants(shape, ops):
        if kind == "int" and name == "small channel":
            continue                                               # (every channel of the integer pass has the same magnitude)
        with pytest.raises(AssertionError):
            T.check_against({"y": _Host(y)}, ref, name, maxnorm=False, exact=kind == "int")
