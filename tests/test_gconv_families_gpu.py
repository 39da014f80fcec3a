"""Every row of tests/gconv_families.py on the GPU, straight through the C ABI: the launch tag and return code, guard bands
around every output, a float64 reference with an element-wise and a max-norm bar, exact integers, reproducibility of the
workspace reductions, and one sweep over 4-byte offsets of x / g_y / w for every shape of the table.

Inputs (seeded CPU generators, the same for all rows):
  "scaled"  x / g_y channels of magnitudes 1e-4 .. 1e4, one input channel per group identically zero, the faces of the volume
            (first and last index on every axis) times 1e3 — a halo or border-mask slip is the largest term, not the smallest;
            weights and bias plain randn (no symmetry: a tap flip or a transposed bank shows)
  "plain"   randn everywhere: the project's max-norm bars bite in the bulk
  "int"     integers -4 .. 4: every partial sum is an integer below 2^24, so fp32 must equal float64 exactly in any order

The bars, none measured on the code under test:
  element-wise  |got - ref| <= (K + 2) * 2^-24 * mag + tiny, mag = the same convolution of |x| and |w| (+ |bias|), or of |g_y| and
                |x| for the gradients, K = the number of terms of one output: the textbook worst-case bound of an fp32 sum of K
                products in any order (it holds for the float-atomics rows too).  tests/test_gconv_families_cpu.py shows that
                torch's fp32 CPU convolution stays inside it.
  max-norm      the bars of tests/test_gconv_gpu.py: 2e-5 (y, g_x) and 5e-5 (g_w, g_bias) of max(1, max |ref|).
"""
import itertools
import zlib

import pytest
import torch
import torch.nn.functional as Fn

from tests import gconv_families as F

pytestmark = pytest.mark.gpu

GUARD = 256                     # floats of sentinel before and after every tensor handed to the library
SENTINEL = -12345.5
U = 2.0 ** -24                  # unit roundoff of fp32
TINY = 1e-30
MAXNORM = {"y": 2e-5, "g_x": 2e-5, "g_w": 5e-5, "g_b": 5e-5}


def volume(W):
    v = 1
    for e in W:
        v *= e
    return v


def shape_id(s):
    return "B%d_G%d_%dto%d_%s" % (s[0], s[1], s[2], s[3], "x".join(map(str, s[4])))


def _conv(dim):
    return Fn.conv3d if dim == 3 else Fn.conv2d


def _faces(t):
    for ax in range(2, t.dim()):
        idx = [slice(None)] * t.dim()
        for e in (0, -1):
            idx[ax] = e
            t[tuple(idx)] *= 1e3
    return t


def make_inputs(shape, kind):
    """x f32[B, G*Cin, *W], w f32[G*Cout, Cin, 3^d], b f32[G*Cout], g_y f32[B, G*Cout, *W] on the CPU"""
    B, G, Cin, Cout, W = shape
    d = len(W)
    gen = torch.Generator().manual_seed(zlib.crc32(repr((shape, kind)).encode()))
    if kind == "int":
        ri = lambda *s: torch.randint(-4, 5, s, generator=gen).float()      # noqa: E731
        return {"x": ri(B, G * Cin, *W), "w": ri(G * Cout, Cin, *([3] * d)), "b": ri(G * Cout), "g_y": ri(B, G * Cout, *W)}
    rn = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
    x, w, b, g_y = rn(B, G, Cin, *W), rn(G * Cout, Cin, *([3] * d)), rn(G * Cout), rn(B, G * Cout, *W)
    if kind == "scaled":
        x *= (10.0 ** torch.linspace(-4, 4, Cin)).reshape(1, 1, Cin, *([1] * d))
        x[:, :, 1] = 0
        g_y *= (10.0 ** torch.linspace(-4, 4, G * Cout)).reshape(1, -1, *([1] * d))
        x, g_y = _faces(x), _faces(g_y)
    else:
        assert kind == "plain"
    return {"x": x.reshape(B, G * Cin, *W).contiguous(), "w": w, "b": b, "g_y": g_y}


def _all_three(shape, x, w, b, g_y, only=("y", "g_x", "g_w", "g_b")):
    """y, g_x, g_w, g_b of one convolution by torch's conv and the backward autograd runs for it (aten::convolution_backward, asked
    for the wanted cotangents only), in the dtype of the operands"""
    G, d = shape[1], len(shape[4])
    out = {}
    if "y" in only:
        out["y"] = _conv(d)(x, w, b, padding=1, groups=G)
    mask = ["g_x" in only, "g_w" in only, "g_b" in only]
    if any(mask):
        grads = torch.ops.aten.convolution_backward(g_y, x, w, [b.numel()], [1] * d, [1] * d, [1] * d, False, [0] * d, G, mask)
        out.update((k, g) for k, g, m in zip(("g_x", "g_w", "g_b"), grads, mask) if m)
    return {k: out[k] for k in only}


_PARTS = (("y",), ("g_x",), ("g_w", "g_b"))      # what one entry point writes
_cache = {}


def inputs(shape, kind):
    """make_inputs, computed once per (shape, kind) and shared by the rows and the sweep"""
    key = ("in", shape, kind)
    if key not in _cache:
        _cache[key] = make_inputs(shape, kind)
    return _cache[key]


def reference(shape, kind, bias, only=("y", "g_x", "g_w", "g_b"), magnitudes=True, cached=True):
    """key -> (float64 result, magnitude, K) of the fp32 operands inputs(shape, kind); y without the bias term where bias is False
    (magnitudes=False: None in their place, for a pass that holds the max-norm bars only).  Each entry point's outputs are computed
    once per (shape, kind) and kept: the rows of one shape and the sweep share them."""
    B, G, Cin, Cout, W = shape
    d = len(W)
    K = {"y": Cin * 3 ** d + (1 if bias else 0), "g_x": Cout * 3 ** d, "g_w": B * volume(W), "g_b": B * volume(W)}
    ops, dbl = inputs(shape, kind), None
    out = {}
    for part in _PARTS:
        if not set(part) & set(only):
            continue
        for what in ("ref", "mag") if magnitudes else ("ref",):
            key = (what, shape, kind, bias if part == ("y",) else True, part)
            if key not in _cache or not cached:
                if dbl is None:
                    dbl = {k: v.double() for k, v in ops.items()}
                    if not bias:
                        dbl["b"] = torch.zeros_like(dbl["b"])
                t = dbl if what == "ref" else {k: v.abs() for k, v in dbl.items()}
                _cache[key] = _all_three(shape, t["x"], t["w"], t["b"], t["g_y"], part)
            for k in part:
                out.setdefault(k, {})[what] = _cache[key][k]
    return {k: (out[k]["ref"], out[k].get("mag"), K[k]) for k in only}


def fp32_cpu(shape, ops):
    return _all_three(shape, ops["x"], ops["w"], ops["b"], ops["g_y"])


def bound(mag, K):
    return (K + 2) * U * mag + TINY


# ---- the device side ----

class Banded:
    """a tensor inside a larger buffer: GUARD floats of SENTINEL before and after it, optionally 4 bytes past a 16-byte boundary"""

    def __init__(self, shape, off4, src=None):
        n = volume(shape)
        self.buf = torch.full((n + 2 * GUARD + 4,), SENTINEL, device="cuda", dtype=torch.float32)
        self.start = GUARD + (1 if off4 else 0)
        self.view = self.buf[self.start:self.start + n].view(*shape)
        assert self.view.data_ptr() % 16 == (4 if off4 else 0)
        if src is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(src)
        self.n = n

    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        a, b = self.buf[:self.start], self.buf[self.start + self.n:]
        return bool((a == SENTINEL).all()) and bool((b == SENTINEL).all())


def call(api, shape, ops, bias=True, ws="query", offset4=(), flags=0):
    """-> (rc, tag, {key: Banded output}, [every Banded of the call])"""
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.ops import _stream
    lib = _lib.load()
    B, G, Cin, Cout, W = shape
    d = len(W)
    Wa = _lib.int_array(W)
    off = lambda name: name in offset4                                      # noqa: E731
    lib.ct_debug_set_gconv(flags)
    try:
        if api == F.FWD:
            x, w, b = Banded(ops["x"].shape, off("x"), ops["x"]), Banded(ops["w"].shape, off("w"), ops["w"]), Banded(ops["b"].shape, False, ops["b"])
            y = Banded(ops["g_y"].shape, off("y"))
            rc = lib.ct_gconv_fwd(x.ptr(), w.ptr(), b.ptr() if bias else None, y.ptr(), B, G, Cin, Cout, d, Wa, _stream())
            outs, every = {"y": y}, [x, w, b, y]
        elif api == F.BWD:
            g_y, w = Banded(ops["g_y"].shape, off("g_y"), ops["g_y"]), Banded(ops["w"].shape, off("w"), ops["w"])
            g_x = Banded(ops["x"].shape, off("g_x"))
            rc = lib.ct_gconv_bwd_data(g_y.ptr(), w.ptr(), g_x.ptr(), B, G, Cin, Cout, d, Wa, _stream())
            outs, every = {"g_x": g_x}, [g_y, w, g_x]
        else:
            x, g_y = Banded(ops["x"].shape, off("x"), ops["x"]), Banded(ops["g_y"].shape, off("g_y"), ops["g_y"])
            g_w, g_b = Banded(ops["w"].shape, False), Banded(ops["b"].shape, False)
            need = lib.ct_gconv_bwd_weight_workspace_bytes(B, G, Cin, Cout, d, Wa)
            nbytes = {"query": need, None: 0, "short": need // 2}[ws]
            wsb = Banded((max(nbytes // 4, 1),), False) if nbytes else None
            rc = lib.ct_gconv_bwd_weight(x.ptr(), g_y.ptr(), g_w.ptr(), g_b.ptr() if bias else None, wsb.ptr() if wsb else None,
                                         nbytes, B, G, Cin, Cout, d, Wa, _stream())
            outs, every = {"g_w": g_w}, [x, g_y, g_w, g_b] + ([wsb] if wsb else [])
            if bias:
                outs["g_b"] = g_b
        torch.cuda.synchronize()
        tag = lib.ct_debug_last_launch().decode()
    finally:
        lib.ct_debug_set_gconv(0)
    return rc, tag, outs, every


def check_against(outs, ref, label, elementwise=True, maxnorm=True, exact=False):
    for k, o in outs.items():
        got = o.view.cpu()
        assert not torch.isnan(got).any(), (label, k, "an element was left unwritten")
        want, mag, K = ref[k]
        got = got.double()
        if exact:
            assert float(mag.max()) < 2 ** 24, (label, k)
            assert torch.equal(got, want), (label, k, int((got != want).sum()), "wrong integers")
            continue
        err = (got - want).abs()
        if elementwise:
            ratio = err / bound(mag, K)
            worst = float(ratio.max())
            print("%s %s: element-wise %.3f of the bound" % (label, k, worst))
            assert worst <= 1.0, (label, k, worst, "at", int(ratio.argmax()))
        if maxnorm:
            rel = float(err.max()) / max(1.0, float(want.abs().max()))
            print("%s %s: max-norm %.2e (bar %.0e)" % (label, k, rel, MAXNORM[k]))
            assert rel <= MAXNORM[k], (label, k, rel)


@pytest.fixture(autouse=True)
def _flags_reset():
    yield
    from cloud_transformers_amd import _lib
    _lib.load().ct_debug_set_gconv(0)


@pytest.mark.parametrize("r", F.ROWS, ids=[r.id for r in F.ROWS])
def test_row(r):
    shape = (r.B, r.G, r.Cin, r.Cout, r.W)
    only = {F.FWD: ("y",), F.BWD: ("g_x",), F.WRW: ("g_w", "g_b")}[r.api]
    for kind in ("scaled", "plain", "int"):
        ops = inputs(shape, kind)
        rc, tag, outs, every = call(r.api, shape, ops, r.bias, r.ws, r.offset4, r.flags)
        label = "%s[%s]" % (r.id, kind)
        print(label, "rc", rc, "tag", tag)
        assert rc == r.rc, (label, rc)
        assert tag == r.tag, (label, tag)
        for t in every:
            assert t.guards_intact(), (label, "wrote outside a tensor")
        if rc != F.CT_OK:
            for k, o in outs.items():                            # a refused call leaves its outputs as they were
                assert bool(torch.isnan(o.view).all()), (label, k)
            continue
        ref = reference(shape, kind, r.bias, only, magnitudes=kind != "plain")
        check_against(outs, ref, label, elementwise=kind == "scaled", maxnorm=kind != "int", exact=kind == "int")
        if r.api == F.WRW and kind == "scaled" and not any(t in r.tag for t in F.ATOMICS_TAGS):
            rc2, tag2, outs2, _ = call(r.api, shape, ops, r.bias, r.ws, r.offset4, r.flags)
            assert (rc2, tag2) == (rc, tag)
            for k in outs:
                assert torch.equal(outs[k].view, outs2[k].view), (label, k, "not bitwise reproducible")


def test_no_plan_shape_returns_ok_or_einval_and_einval_writes_nothing():
    rows = [r for r in F.ROWS if (r.B, r.G, r.Cin, r.Cout, r.W) == F.NOPLAN]
    assert {r.api for r in rows} == {F.FWD, F.BWD, F.WRW}
    assert all(r.rc in (F.CT_OK, F.CT_EINVAL) for r in rows) and any(r.rc == F.CT_EINVAL for r in rows)
    ops = inputs(F.NOPLAN, "plain")
    seen = set()
    for api in (F.FWD, F.BWD, F.WRW):
        for offset4 in ((), ("x",), ("g_y",), ("w",), ("y",), ("g_x",)):
            rc, tag, outs, every = call(api, F.NOPLAN, ops, True, "query", offset4)
            seen.add(rc)
            assert rc in (F.CT_OK, F.CT_EINVAL), (api, offset4, rc)
            assert all(t.guards_intact() for t in every)
            if rc == F.CT_EINVAL:
                assert tag in ("", "bwd_data"), (api, offset4, tag)
                assert all(bool(torch.isnan(o.view).all()) for o in outs.values()), (api, offset4)
    assert F.CT_EINVAL in seen
    # rows of 1001 floats: no ring (W % 4 != 0) and no tile plan for the weight gradient, which must not have zeroed g_w by then
    ops = inputs(F.NOPLAN_WRW, "plain")
    for bias in (True, False):
        rc, tag, outs, every = call(F.WRW, F.NOPLAN_WRW, ops, bias, None)
        assert (rc, tag) == (F.CT_EINVAL, "")
        assert all(t.guards_intact() for t in every)
        assert all(bool(torch.isnan(t.view).all()) for t in every[2:4]), "a refused weight gradient wrote g_w or g_bias"


SWEEP = [s for s in F.shapes() if s != F.NOPLAN]


@pytest.mark.parametrize("shape", SWEEP, ids=[shape_id(s) for s in SWEEP])
def test_offsets_sweep(shape):
    """include/cloudct.h asks for no alignment: with any of x, g_y, w four bytes past a 16-byte boundary and the queried workspace,
    the three entry points return CT_OK and meet the bounds (the shape ct_gconv_supported refuses has a test of its own)."""
    ops = inputs(shape, "scaled")
    ref = reference(shape, "scaled", True)
    for n in range(4):
        for subset in itertools.combinations(("x", "g_y", "w"), n):
            for api in (F.FWD, F.BWD, F.WRW):
                used = {F.FWD: ("x", "w"), F.BWD: ("g_y", "w"), F.WRW: ("x", "g_y")}[api]
                if n and not set(subset) & set(used):
                    continue                                    # the same call as the aligned one
                if set(subset) - set(used):
                    continue                                    # ... as a smaller subset's
                rc, tag, outs, every = call(api, shape, ops, True, "query", subset)
                label = "%s offset %s (%s)" % (api, subset, tag)
                assert rc == F.CT_OK, (label, rc)
                assert all(t.guards_intact() for t in every), label
                check_against(outs, ref, label)
