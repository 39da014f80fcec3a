"""The eval-mode norms of the grouped-conv Res blocks in the convolution's write-out (ct_gconv_fwd_norm) on the GPU.

1. Bit equality through the C ABI: on every shape of the K-split, quad and dense families below, four variants (norm + ReLU, norm
   alone, norm + identity skip + ReLU, norm + normed skip + ReLU) are torch.equal with the sequence the header's contract names —
   ct_gconv_fwd into a scratch tensor, ct_bn_eval_group_fwd on it, the same on the skip, torch.add, torch.relu — y pre-filled
   with NaN between guard bands, and the launch tag is the plain forward's for the same arguments.
2. One shape per family against a float64 convolution and the formula, within 1e-4 * max(1, max |want|) (the fused-versus-plain
   bound of tests/test_blocks_gpu.py).
3. Res / Basic blocks in eval mode under no_grad: no BatchNorm2d / BatchNorm3d.forward call with the switch on, 3 / 2 / 1 with
   ops.GCONV_NORM off, the two outputs within the bound of 2; the classifier's after_pool3d tail likewise.
4. Eval with gradients and training mode keep the modules' path.
5. A Res block's eval forward captured in a graph and replayed on fresh inputs equals the eager result bit for bit.
"""
import ctypes
import zlib

import pytest
import torch
from torch import nn

from tests import gconv_families as F
from tests import test_gconv_families_gpu as T

pytestmark = pytest.mark.gpu

SHAPES = {
    "ksplit": [(1, 2, 64, 64, (8, 8, 8)), (1, 2, 64, 64, (4, 4, 4)), (1, 2, 64, 64, (16, 16, 16)), (3, 2, 48, 40, (4, 8, 8)),
               (1, 2, 32, 16, (40, 32)), (1, 1, 64, 64, (64, 64))],
    "quad": [(2, 3, 16, 16, (32, 32)), (1, 3, 16, 48, (8, 8)), (1, 2, 16, 16, (8, 256)), (1, 1, 16, 16, (101, 32)),
             (1, 2, 16, 16, (16, 16, 16))],
    "dense": [(2, 3, 40, 24, (2, 2, 2)), (2, 3, 24, 40, (2, 2, 2)), (3, 2, 5, 7, (2, 2)), (70, 1, 8, 6, (2, 2, 2))],
}
ALL = [(fam, s) for fam, ss in SHAPES.items() for s in ss]
VARIANTS = ("norm_relu", "norm", "identity_skip_relu", "normed_skip_relu")


def _row(shape):
    """the plain forward's row of the shape (aligned tensors, no debug bits): its tag and whether it passes a bias"""
    rows = [r for r in F.ROWS if r.api == F.FWD and not r.offset4 and not r.flags and (r.B, r.G, r.Cin, r.Cout, r.W) == shape]
    assert len(rows) == 1, shape
    return rows[0]


def _stats(C, seed):
    """(weight, bias, running_mean, running_var) on the device: means in +-0.5, variances in [0.5, 2], weights in +-[0.5, 1.5] with
    every third one negative and one exactly 0, biases in +-0.5"""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: torch.rand(C, generator=g) * (hi - lo) + lo                 # noqa: E731
    w = u(0.5, 1.5)
    w[::3] *= -1
    w[C // 2] = 0.0
    return tuple(t.cuda() for t in (w, u(-0.5, 0.5), u(-0.5, 0.5), u(0.5, 2.0)))


def _norm_struct(stats, eps):
    from cloud_transformers_amd import _lib
    return _lib.GconvNorm(stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), stats[3].data_ptr(), eps)


def _bn_eval(x, stats, eps, relu):
    """ct_bn_eval_group_fwd of x [B, C, *W] viewed as [B, C, volume] into a new tensor"""
    from cloud_transformers_amd import _lib, ops
    B, C = x.shape[:2]
    N = x[0, 0].numel()
    y = torch.empty_like(x)
    arr = ops._bn_fwd_table([dict(x=x.data_ptr(), xbs=0, C=C, w=stats[0], b=stats[1], rm=stats[2], rv=stats[3], eps=eps,
                                  relu=int(relu), res=None, rbs=0, y=y.data_ptr(), ybs=0)])
    _lib.check(_lib.load().ct_bn_eval_group_fwd(ops._at(arr, 0), 1, B, N, ops._stream()), "ct_bn_eval_group_fwd")
    return y


_cases = {}


def _case(shape):
    """device operands of a shape, made once: x, w, bias (or None, as the family's row), skip, the two norms' statistics"""
    if shape not in _cases:
        B, G, Cin, Cout, W = shape
        host = T.make_inputs(shape, "plain")
        seed = zlib.crc32(repr(shape).encode())
        _cases[shape] = dict(x=host["x"].cuda(), w=host["w"].cuda(), b=host["b"].cuda() if _row(shape).bias else None,
                             skip=(host["g_y"] * 8.0).cuda(), n=_stats(G * Cout, seed), sn=_stats(G * Cout, seed + 1),
                             eps=1e-5, seps=1e-3)
    return _cases[shape]


def _fused(shape, variant):
    """-> (rc, tag, the Banded y) of one ct_gconv_fwd_norm call"""
    from cloud_transformers_amd import _lib, ops
    lib = _lib.load()
    c = _case(shape)
    B, G, Cin, Cout, W = shape
    y = T.Banded((B, G * Cout) + tuple(W), False)
    norm = _norm_struct(c["n"], c["eps"])
    snorm = _norm_struct(c["sn"], c["seps"])
    skip = c["skip"] if "skip" in variant else None
    rc = lib.ct_gconv_fwd_norm(c["x"].data_ptr(), c["w"].data_ptr(), c["b"].data_ptr() if c["b"] is not None else None,
                               ctypes.addressof(norm), skip.data_ptr() if skip is not None else None,
                               ctypes.addressof(snorm) if variant == "normed_skip_relu" else None, int(variant.endswith("relu")),
                               y.ptr(), B, G, Cin, Cout, len(W), _lib.int_array(W), ops._stream())
    torch.cuda.synchronize()
    return rc, lib.ct_debug_last_launch().decode(), y


def _plain(shape):
    """-> (the plain forward's output, its tag), computed once per shape"""
    from cloud_transformers_amd import _lib, ops
    c = _case(shape)
    if "plain" not in c:
        lib = _lib.load()
        B, G, Cin, Cout, W = shape
        y = torch.empty(B, G * Cout, *W, device="cuda")
        _lib.check(lib.ct_gconv_fwd(c["x"].data_ptr(), c["w"].data_ptr(), c["b"].data_ptr() if c["b"] is not None else None,
                                    y.data_ptr(), B, G, Cin, Cout, len(W), _lib.int_array(W), ops._stream()), "ct_gconv_fwd")
        torch.cuda.synchronize()
        c["plain"] = (y, lib.ct_debug_last_launch().decode())
    return c["plain"]


def _composed(shape, variant):
    """the sequence of the header's contract"""
    c = _case(shape)
    relu = variant.endswith("relu")
    scratch, _ = _plain(shape)
    if "skip" not in variant:
        return _bn_eval(scratch, c["n"], c["eps"], relu)
    o = _bn_eval(scratch, c["n"], c["eps"], False)
    t = _bn_eval(c["skip"], c["sn"], c["seps"], False) if variant == "normed_skip_relu" else c["skip"]
    o = torch.add(o, t)
    return torch.relu(o) if relu else o


@pytest.mark.parametrize("fam,shape", ALL, ids=["%s-%s" % (f, T.shape_id(s)) for f, s in ALL])
def test_bit_equal_with_the_composed_sequence(fam, shape):
    from cloud_transformers_amd import _lib
    row = _row(shape)
    assert row.tag.startswith(fam)
    assert _lib.load().ct_gconv_fwd_norm_supported(*shape[:4], len(shape[4]), _lib.int_array(shape[4])) == 1
    _, plain_tag = _plain(shape)
    assert plain_tag == row.tag
    for variant in VARIANTS:
        rc, tag, y = _fused(shape, variant)
        label = "%s[%s]" % (row.id, variant)
        assert rc == F.CT_OK, (label, rc)
        assert tag == plain_tag, (label, tag)
        assert y.guards_intact(), (label, "wrote outside y")
        got = y.view
        assert not torch.isnan(got).any(), (label, "an element was left unwritten")
        want = _composed(shape, variant)
        assert torch.isfinite(want).all()
        if variant.endswith("relu"):
            clipped = float((want == 0).float().mean())
            print("%s: %.2f of the values clipped" % (label, clipped))
            assert 0.2 < clipped < 0.8, (label, clipped)
        else:
            assert float((want < 0).float().mean()) > 0.2
        diff = int((got != want).sum())
        assert torch.equal(got, want), (label, diff, "elements differ from the composed sequence")


@pytest.mark.parametrize("fam", list(SHAPES))
def test_against_a_float64_convolution_and_the_formula(fam):
    shape = SHAPES[fam][0]
    c = _case(shape)
    G, d = shape[1], len(shape[4])
    b = c["b"].double().cpu() if c["b"] is not None else None
    v = T._conv(d)(c["x"].double().cpu(), c["w"].double().cpu(), b, padding=1, groups=G)

    def bn(t, stats, eps):
        w, be, mu, var = (s.double().cpu().reshape(1, -1, *([1] * d)) for s in stats)
        return ((t - mu) * (1.0 / torch.sqrt(var + eps))) * w + be

    want = torch.relu(bn(v, c["n"], c["eps"]) + bn(c["skip"].double().cpu(), c["sn"], c["seps"]))
    rc, _, y = _fused(shape, "normed_skip_relu")
    assert rc == F.CT_OK
    tol = 1e-4 * max(1.0, float(want.abs().max()))
    err = float((y.view.double().cpu() - want).abs().max())
    print("%s: max |fused - float64| %.3e (bound %.3e)" % (T.shape_id(shape), err, tol))
    assert err <= tol, (err, tol)


# ---- the blocks ----

class _CountNorms:
    """Counts the calls of nn.BatchNorm2d / nn.BatchNorm3d.forward (the module path of a norm) while active."""

    def __enter__(self):
        self.calls = 0
        base = nn.modules.batchnorm._BatchNorm
        self.real = base.forward
        outer = self

        def forward(module, x):
            if isinstance(module, (nn.BatchNorm2d, nn.BatchNorm3d)):
                outer.calls += 1
            return outer.real(module, x)

        base.forward = forward
        return self

    def __exit__(self, *exc):
        nn.modules.batchnorm._BatchNorm.forward = self.real
        return False


def _randomise_norms(block, seed):
    g = torch.Generator().manual_seed(seed)
    for m in block.modules():
        if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
            C = m.num_features
            with torch.no_grad():
                m.running_mean.copy_(torch.rand(C, generator=g) - 0.5)
                m.running_var.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
                m.weight.copy_((torch.rand(C, generator=g) + 0.5) * (1 - 2 * (torch.arange(C) % 3 == 0).float()))
                m.bias.copy_(torch.rand(C, generator=g) - 0.5)
    return block


def _both_paths(block, x):
    """(result with the switch on, module-norm calls there, result with ops.GCONV_NORM = False, calls there)"""
    from cloud_transformers_amd import ops
    assert ops.GCONV_NORM and ops.BN_EVAL
    with torch.no_grad():
        with _CountNorms() as new:
            got = block(x)
        ops.GCONV_NORM = False
        try:
            with _CountNorms() as old:
                want = block(x)
        finally:
            ops.GCONV_NORM = True
    torch.cuda.synchronize()
    return got, new.calls, want, old.calls


def _agree(got, want):
    tol = 1e-4 * max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print("max |fused - module path| %.3e (bound %.3e)" % (err, tol))
    assert got.shape == want.shape and torch.isfinite(got).all() and err <= tol, (err, tol)


BLOCKS = [
    ("Res3DBlock", (64, 128, 2), (2, 64, 8, 8, 8), 3),
    ("Res3DBlock", (128, 128, 2), (2, 128, 4, 4, 4), 2),
    ("Res3DBlock", (128, 128, 2), (2, 128, 2, 2, 2), 2),
    ("Res2DBlock", (32, 64, 2), (2, 32, 16, 16), 3),
    ("Basic3DBlock", (64, 64, 3, 2), (2, 64, 8, 8, 8), 1),
    ("Res2DBlock", (8, 8, 2), (2, 8, 16, 16), 2),                   # four-channel groups: the composed route
]


def _block(name, args, seed=3):
    from cloud_transformers_amd.layers import grouped_conv as G
    torch.manual_seed(seed)
    return _randomise_norms(getattr(G, name)(*args), seed + 1).cuda().eval()


@pytest.mark.parametrize("name,args,xshape,module_calls", BLOCKS,
                         ids=["%s%s-%s" % (n, "_".join(map(str, a)), "x".join(map(str, s[2:]))) for n, a, s, _ in BLOCKS])
def test_blocks_launch_no_norm_and_agree_with_the_module_path(name, args, xshape, module_calls):
    from cloud_transformers_amd import _lib
    block = _block(name, args)
    x = torch.randn(*xshape, generator=torch.Generator().manual_seed(11)).cuda()
    got, new_calls, want, old_calls = _both_paths(block, x)
    assert new_calls == 0, new_calls
    assert old_calls == module_calls, old_calls
    _agree(got, want)
    groups = args[-1]
    fused = _lib.load().ct_gconv_fwd_norm_supported(xshape[0], groups, args[1] // groups, args[1] // groups, len(xshape) - 2,
                                                    _lib.int_array(xshape[2:]))
    assert fused == (0 if args[1] // groups == 4 else 1)


def test_classifier_tail_agrees_with_its_module_path():
    from cloud_transformers_amd.layers.grouped_conv import Pool3DBlock, Res3DBlock
    torch.manual_seed(5)
    tail = nn.Sequential(Res3DBlock(512, 1024, groups=16), Pool3DBlock(2), Res3DBlock(1024, 1024, groups=16),
                         Pool3DBlock(2), Res3DBlock(1024, 1024, groups=16), nn.AdaptiveAvgPool3d((1, 1, 1)))
    tail = _randomise_norms(tail, 6).cuda().eval()
    x = torch.randn(2, 512, 8, 8, 8, generator=torch.Generator().manual_seed(7)).cuda()
    got, new_calls, want, old_calls = _both_paths(tail, x)
    assert new_calls == 0 and old_calls == 3 + 2 + 2, (new_calls, old_calls)
    _agree(got, want)


# ---- paths that stay as they are ----

def test_eval_with_gradients_keeps_the_module_path():
    block = _block("Res3DBlock", (64, 128, 2))
    x = torch.randn(2, 64, 4, 4, 4, generator=torch.Generator().manual_seed(2)).cuda().requires_grad_()
    with _CountNorms() as n:
        out = block(x)
    assert n.calls == 3, n.calls
    out.sum().backward()
    assert torch.isfinite(x.grad).all()
    grads = [p.grad for p in block.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)


def test_training_mode_keeps_the_module_path_and_updates_the_statistics():
    block = _block("Res3DBlock", (64, 128, 2)).train()
    before = block.res_branch[1].running_mean.clone()
    x = torch.randn(2, 64, 4, 4, 4, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad(), _CountNorms() as n:
        block(x)
    assert n.calls == 3, n.calls
    assert not torch.equal(block.res_branch[1].running_mean, before)


# ---- graph capture ----

def test_a_captured_res_block_replays_bit_for_bit_on_fresh_inputs():
    block = _block("Res3DBlock", (64, 128, 2))
    fresh = lambda seed: torch.randn(2, 64, 8, 8, 8, generator=torch.Generator().manual_seed(seed)).cuda()      # noqa: E731
    static = fresh(20)
    with torch.no_grad():
        # warm-up (library choices of the skip GEMM, allocator) on the current stream: a stream of its own would come out of
        # torch's round-robin pool of 32 handles, and tests/test_graph_replay_gpu.py compares its streams' handles with the
        # capture stream's — this file leaves the pool where it found it
        for _ in range(2):
            block(static)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with _CountNorms() as n, torch.cuda.graph(g):
            out = block(static)
        assert n.calls == 0
        for seed in (21, 22):
            x = fresh(seed)
            static.copy_(x)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, block(x)), seed
