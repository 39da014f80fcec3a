"""CPU-side checks of the norms-in-the-convolution-write-out path: ct_gconv_fwd_norm and ct_gconv_fwd_norm_supported are declared
in include/cloudct.h, exported and bound in _lib.py with the same number of arguments; the support query is 1 exactly on the rows of
tests/gconv_families.py whose forward takes the K-split, quad or dense kernels and 0 on the four-channel and one-position ones;
bad arguments are refused before anything touches a device; and the Res / Basic blocks keep the modules' path on CPU tensors.

One pair of cases asked of the query cannot hold together: 1 on every ct_gconv_fwd row without offset4 whose tag starts with
`ksplit`, and 0 on NOPLAN — the row `noplan_fwd_aligned` is both (NOPLAN's 16-byte-aligned forward runs on the tiled
K-split kernel; only its one-position form and with it ct_gconv_supported have no plan).  The library's rule decides — 1 exactly
where the planner takes one of the three families for aligned tensors — so NOPLAN is 1 here; the shape without any forward plan
for the write-out that is asserted 0 instead is NOPLAN_WRW (rows of 1001 floats: the one-position form)."""
import ctypes
import os
import re

import pytest
import torch

from tests import gconv_families as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = F.CT_EINVAL


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def test_symbols_are_declared_and_bound_with_matching_arity(lib):
    from cloud_transformers_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cloudct.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, arity in (("ct_gconv_fwd_norm", 15), ("ct_gconv_fwd_norm_supported", 6)):
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(raw, name)
    # the plain forward's arguments + (norm, skip, skip_norm, relu); the query takes ct_gconv_supported's
    assert len(_lib.SIGNATURES["ct_gconv_fwd_norm"][1]) == len(_lib.SIGNATURES["ct_gconv_fwd"][1]) + 4
    assert _lib.SIGNATURES["ct_gconv_fwd_norm_supported"] == _lib.SIGNATURES["ct_gconv_supported"]
    assert ctypes.sizeof(_lib.GconvNorm) == 40                       # four pointers, a float, padding
    assert re.search(r"typedef struct \{[^}]*running_var;\s*float eps;\s*\}\s*ct_gconv_norm;", text)
    assert lib.ct_abi_version() == 3                                 # additive exports do not bump it


def _supported(lib, B, G, Cin, Cout, W):
    from cloud_transformers_amd import _lib
    return lib.ct_gconv_fwd_norm_supported(B, G, Cin, Cout, len(W), _lib.int_array(W))


def test_supported_follows_the_forward_families(lib):
    rows = [r for r in F.ROWS if r.api == F.FWD and not r.offset4]
    fused = [r for r in rows if r.tag.startswith(("ksplit", "quad", "dense"))]
    plain = [r for r in rows if r.tag.startswith(("c4_", "onepos"))]
    assert len(fused) >= 18 and len(plain) >= 16 and len(fused) + len(plain) == len(rows)
    assert {r.tag.split("+")[0] for r in fused} >= {"ksplit_one_dma", "ksplit_one_elem", "ksplit_tiled_dma", "ksplit_tiled_elem",
                                                     "quad_256", "quad_1024", "dense2d", "dense3d"}
    for r in fused:
        assert _supported(lib, r.B, r.G, r.Cin, r.Cout, r.W) == 1, r.id
    for r in plain:
        assert _supported(lib, r.B, r.G, r.Cin, r.Cout, r.W) == 0, r.id
    # the debug bits move a shape between families that both carry the write-out, or between two that do not
    try:
        for flags in (F.ksplit_from(20), F.C4_FORCE_MFMA, F.C4_NO_MFMA):
            lib.ct_debug_set_gconv(flags)
            assert _supported(lib, 1, 2, 20, 24, (8, 8)) == 1 and _supported(lib, 1, 3, 4, 4, (5, 7, 16)) == 0
    finally:
        lib.ct_debug_set_gconv(0)
    # (see the module's docstring) NOPLAN's aligned forward is the tiled K-split kernel; NOPLAN_WRW has rows of 1001 floats
    assert next(r for r in F.ROWS if r.id == "noplan_fwd_aligned").tag.startswith("ksplit_tiled_elem")
    assert _supported(lib, *F.NOPLAN) == 1
    assert _supported(lib, *F.NOPLAN_WRW) == 0
    # not a shape at all
    assert _supported(lib, 0, 2, 64, 64, (8, 8, 8)) == 0 and _supported(lib, 1, 2, 64, 64, (8, 8, 8, 8)) == 0
    assert lib.ct_gconv_fwd_norm_supported(1, 2, 64, 64, 3, None) == 0


def _norm(p, **kw):
    from cloud_transformers_amd import _lib
    n = _lib.GconvNorm(p, p, p, p, 1e-5)
    for k, v in kw.items():
        setattr(n, k, v)
    return n


def test_argument_checks_without_gpu(lib):
    from cloud_transformers_amd import _lib
    buf = ctypes.create_string_buffer(64)                        # never dereferenced: every call below is refused first
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15

    def call(x=p, w=p, conv_bias=None, norm="default", skip=None, skip_norm=None, relu=1, y=p, shape=(1, 2, 64, 64, (8, 8, 8)), W="shape",
             **kw):
        n = _norm(p, **kw) if norm == "default" else norm
        B, G, Cin, Cout, Ws = shape
        Wa = _lib.int_array(Ws) if W == "shape" else W
        return lib.ct_gconv_fwd_norm(x, w, conv_bias, None if n is None else ctypes.addressof(n), skip,
                                     None if skip_norm is None else ctypes.addressof(skip_norm), relu, y, B, G, Cin, Cout, len(Ws), Wa,
                                     None)

    # a null required pointer
    assert call(x=None) == EINVAL and call(w=None) == EINVAL and call(y=None) == EINVAL and call(norm=None) == EINVAL
    assert call(W=None) == EINVAL
    for field in ("weight", "bias", "running_mean", "running_var"):
        assert call(**{field: None}) == EINVAL, field
        assert call(skip=p, skip_norm=_norm(p, **{field: None})) == EINVAL, field
    # skip_norm without skip
    assert call(skip_norm=_norm(p)) == EINVAL
    # eps < 0 or NaN, of either norm
    assert call(eps=-1.0) == EINVAL and call(eps=float("nan")) == EINVAL
    assert call(skip=p, skip_norm=_norm(p, eps=-1e-9)) == EINVAL and call(skip=p, skip_norm=_norm(p, eps=float("nan"))) == EINVAL
    # tensors off the 16-byte grid
    assert call(x=p + 4) == EINVAL and call(w=p + 4) == EINVAL and call(y=p + 4) == EINVAL and call(skip=p + 4) == EINVAL
    # shapes without the write-out: four-channel groups, the one-position form, no shape at all
    for r in F.ROWS:
        if r.api == F.FWD and not r.offset4 and r.tag.startswith(("c4_", "onepos")):
            assert call(shape=(r.B, r.G, r.Cin, r.Cout, r.W)) == EINVAL, r.id
    assert call(shape=F.NOPLAN_WRW) == EINVAL
    assert call(shape=(0, 2, 64, 64, (8, 8, 8))) == EINVAL and call(shape=(1, 2, 64, 64, (8, 8, 8, 8))) == EINVAL


@pytest.mark.parametrize("name,args,shape", [("Res2DBlock", (8, 16, 2), (2, 8, 6, 8)), ("Res2DBlock", (16, 16, 2), (1, 16, 4, 4)),
                                             ("Res3DBlock", (8, 16, 2), (1, 8, 4, 4, 4)), ("Basic3DBlock", (8, 8, 3, 2), (1, 8, 2, 4, 4)),
                                             ("Basic2DBlock", (8, 8, 3, 2), (1, 8, 4, 4))])
def test_blocks_on_cpu_tensors_keep_the_module_path(name, args, shape):
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers import grouped_conv as G
    assert ops.GCONV_NORM is (os.environ.get("CLOUDCT_GCONV_NORM", "1") != "0")
    torch.manual_seed(0)
    block = getattr(G, name)(*args).eval()
    norms = [m for m in block.modules() if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d))]
    for bn in norms:
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(*shape)
    calls = []
    hooks = [bn.register_forward_hook(lambda m, i, o: calls.append(m)) for bn in norms]
    try:
        with torch.no_grad():
            convs = [m for m in block.modules() if isinstance(m, torch.nn.modules.conv._ConvNd) and m.kernel_size[0] == 3]
            assert not ops.gconv_norm_eligible(convs[0], norms[0], x)
            got = block(x)
            if name.startswith("Res"):
                want = torch.relu(block.res_branch(x) + block.skip_con(x))
            else:
                want = block.block(x)
    finally:
        for h in hooks:
            h.remove()
    assert len(calls) == 2 * len(norms) and torch.equal(got, want)
