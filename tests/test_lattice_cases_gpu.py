"""The lattice and so3 kernels (csrc/ct_lattice.hip) at the shapes where they can go wrong, against tests/lattice_ref.py (float64,
written out by hand, pinned on the oracle's autograd by tests/test_lattice_ref_cpu.py):

  1  exact arithmetic: inputs on a binary grid make every product and partial sum exact in float32, so keys and every gradient
     equal the reference bit for bit — through the workspace (ordered sums) and through the NULL-workspace atomics;
  2  float64 parity at every shape, each cotangent alone and both, keys to a bound derived from their own magnitudes;
  3  the key statistics to the one-pass formula's bound: centred keys, off-centre keys, one stretch of a row far from the rest;
  4  the so3 arithmetic inside the lattice launches against the stand-alone kernels, bit for bit;
  5  strided inputs;  6  a NaN stays where it belongs;  7  launch after launch at different grid sizes.

Every case prints the ratio of what it measured to its bound before it asserts."""
import types

import pytest
import torch

from tests import lattice_ref as L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of float32

SHAPES = [
    (1, 1, 1),          # one point, one head; nwg = 1; n-1 of the variance with 2 or 3 keys
    (1, 3, 255),        # one short of a 256-point step in forward, backward and the finish half of the tail (3N vs 256)
    (2, 5, 256),        # exactly one 256-point step
    (2, 5, 257),        # one past it: a second forward workgroup of one point, backward nbx = 2
    (1, 2, 5000),       # few rows: 20 forward workgroups per row, ragged last one; backward nwg = 20 (> 16, not a multiple)
    (8, 16, 1300),      # ppw = 512: workgroups [0,512) [512,1024) [1024,1300), the loop runs twice, ragged end; nwg = 48
    (4, 64, 700),       # ppw = 512, two workgroups per row, the second ragged; H = 64
    (3, 70, 40),        # H > 64; rows shorter than a wave's worth of a workgroup; nwg * H = 210 for the g_kscale tree
]
_ids = ["B%d-H%d-N%d" % s for s in SHAPES]


def fwd_plan(B, H, N):
    """(workgroups per row, points per workgroup) of lattice_fwd_kernel: lattice_fwd_nbx of csrc/ct_lattice.hip restated"""
    rows, max_nbx = B * H, (N + 255) // 256
    nbx = max(1, min((512 + rows - 1) // rows, max_nbx))
    ppw = ((N + nbx - 1) // nbx + 255) // 256 * 256
    return (N + ppw - 1) // ppw, ppw


# ---------------------------------------------------------------------------
# inputs, GPU runs, checks
# ---------------------------------------------------------------------------
def _inputs(B, H, N, dim, use_scales, use_kscale, seed):
    """random inputs as in tests/test_lattice_gpu.py, on the CPU"""
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(
        B=B, H=H, N=N, dim=dim,
        xyz=torch.rand(B, 3, N, generator=g) * 2 - 1,
        res=torch.randn(B, H * 3, N, generator=g) * 0.3,
        log_R=torch.randn(H, 3, generator=g),
        shift=torch.randn(H, 3, generator=g) * 0.1,
        scales=(1 + 0.2 * torch.randn(H, dim, generator=g)) if use_scales else None,
        kscale=torch.tensor(0.7) if use_kscale else None,
        cot_k=torch.randn(B, H * dim, N, generator=g) * 0.1,
        cot_l=torch.randn(B, H * dim, N, generator=g))


def _leaf(t):
    return None if t is None else t.clone().cuda().requires_grad_(True)


def _forward(inp, path, with_stats=False):
    """path "fused": ops.lattice_so3 (the so3 map inside the launches); "split": ops.so3_exp, then ops.lattice on its R"""
    from cloud_transformers_amd import ops
    t = types.SimpleNamespace(xyz=_leaf(inp.xyz), res=_leaf(inp.res), log_R=_leaf(inp.log_R), shift=_leaf(inp.shift),
                              scales=_leaf(inp.scales), kscale=_leaf(inp.kscale), R=None)
    if path == "fused":
        out = ops.lattice_so3(t.xyz, t.res, t.log_R, t.shift, t.scales, t.kscale, inp.dim, with_stats=with_stats)
    else:
        t.R = ops.so3_exp(t.log_R)
        out = ops.lattice(t.xyz, t.res, t.R, t.shift, t.scales, t.kscale, inp.dim, with_stats)
    t.keys, t.lattice = out[0], out[1]
    t.stats = out[2].cpu() if with_stats else None
    return t


def _backward(t, cot_k, cot_l):
    """gradients of sum(keys cot_k) + sum(lattice cot_l), either None: autograd then hands the op None for that output"""
    terms = [(o * c.cuda()).sum() for o, c in ((t.keys, cot_k), (t.lattice, cot_l)) if c is not None]
    names = [n for n in ("xyz", "res", "R", "shift", "scales", "kscale", "log_R") if getattr(t, n) is not None]
    grads = torch.autograd.grad(sum(terms), [getattr(t, n) for n in names], retain_graph=True)
    return {"g_" + n: g.cpu() for n, g in zip(names, grads)}


def _reference(inp, t, path, cot_k=None, cot_l=None):
    """on the split path the reference rotates with the float32 R the kernel was given"""
    kw = dict(log_R=inp.log_R) if path == "fused" else dict(R=t.R.detach())
    ref = L.lattice_ref(inp.xyz, inp.res, inp.shift, inp.dim, scales=inp.scales, kscale=inp.kscale, g_keys=cot_k, g_lattice=cot_l, **kw)
    if path == "split" and (cot_k is not None or cot_l is not None):
        ref.g_log_R = L.so3_grad(inp.log_R, ref.g_R)
    return ref


def _check_values(t, ref, what):
    """keys: 10 * 2^-24 * M, M = sum_c (|xyz| + |kscale res| + |shift|) |R| |scales| — eight roundings to first order (three in
    p, three in the dot product, one in the scale, one in the float32 R of the fused path), 10 for the second order."""
    err = (t.keys.detach().cpu().double() - ref.keys).abs()
    bound = 10 * U * ref.keys_mag
    print("%s keys: worst err / bound = %.3f" % (what, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (what, float(err.max()))
    err = float((t.lattice.detach().cpu().double() - ref.lattice).abs().max())
    assert err <= 2e-5, (what, "lattice", err)


def _check_grads(got, ref, what):
    for name, g in got.items():
        if name == "g_R" and ref.g_R is None:
            continue
        r = getattr(ref, name)
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        err, tol = float((g.double() - r).abs().max()), 1e-4 * max(1.0, float(r.abs().max()))
        print("%s %s: err / tol = %.3g" % (what, name, err / tol))
        assert err <= tol, (what, name, err)


def _check_stats(stats, ref, inp, what):
    """mean and unbiased variance from float32 workgroup partials of (sum k, sum k^2), finished in double by the one-pass formula.
    A partial is a chain of (ppw / 256) * dim additions per thread and a short tree; with m = (ppw / 256) * dim + 20 roundings:
    |mean - ref| <= m 2^-24 mean|k|,  |var - ref| <= 3 m 2^-24 mean(k^2) n / (n - 1): relative to mean(k^2), not to the variance."""
    n = ref.keys.numel()
    m = fwd_plan(inp.B, inp.H, inp.N)[1] // 256 * inp.dim + 20
    mean_bound = m * U * float(ref.mean_abs)
    var_bound = 3 * m * U * float(ref.mean_sq) * n / (n - 1)
    e_mean, e_var = abs(float(stats[0]) - float(ref.mean)), abs(float(stats[1]) - float(ref.var))
    print("%s statistics: mean err / bound = %.3g, var err / bound = %.3g, var bound / var = %.3g"
          % (what, e_mean / mean_bound, e_var / var_bound, var_bound / max(float(ref.var), 1e-300)))
    assert bool(torch.isfinite(stats).all()), (what, stats)
    assert e_mean <= mean_bound, (what, "mean", e_mean, mean_bound)
    assert e_var <= var_bound, (what, "var", e_var, var_bound)


# ---------------------------------------------------------------------------
# 1. exact arithmetic
# ---------------------------------------------------------------------------
def _exact_inputs(B, H, N, dim, use_scales, use_kscale, gmax, seed):
    """signed permutation matrices, multiples of 1/4 in [-2, 2], scales in {0.5, 1, 2}, kscale 0.5, integer cotangents of the keys"""
    g = torch.Generator().manual_seed(seed)
    quarters = lambda *s: torch.randint(-8, 9, s, generator=g).float() / 4
    R = torch.zeros(H, 3, 3)
    for h in range(H):
        perm, sign = torch.randperm(3, generator=g), torch.randint(0, 2, (3,), generator=g) * 2 - 1
        R[h, torch.arange(3), perm] = sign.float()
    return types.SimpleNamespace(
        B=B, H=H, N=N, dim=dim, R=R, xyz=quarters(B, 3, N), res=quarters(B, H * 3, N), shift=quarters(H, 3),
        scales=torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (H, dim), generator=g)] if use_scales else None,
        kscale=torch.tensor(0.5) if use_kscale else None,
        g_keys=torch.randint(-gmax, gmax + 1, (B, H * dim, N), generator=g).float())


def _exact_reference(inp):
    """the reference, and the precondition on it alone: (sum of |terms|) / (granularity of a term) below 2^24 for every sum"""
    ref = L.lattice_ref(inp.xyz, inp.res, inp.shift, inp.dim, R=inp.R, scales=inp.scales, kscale=inp.kscale, g_keys=inp.g_keys)
    gran = {"g_R": 1 / 16 if inp.kscale is not None else 1 / 8, "g_scales": 1 / 8, "g_kscale": 1 / 8, "g_shift": 1 / 2, "g_xyz": 1 / 2}
    for name, q in gran.items():
        mag = getattr(ref, "abs_" + name)
        if mag is not None:
            print("B%d H%d N%d dim %d %s: sum|terms| / granularity = %.3g of %.3g" % (inp.B, inp.H, inp.N, inp.dim, name, float(mag.max()) / q, 2.0 ** 24))
            assert float(mag.max()) / q < 2.0 ** 24, name
            val = getattr(ref, name)
            assert torch.equal(val, val.float().double()) and torch.equal(val / q, (val / q).round()), name
    return ref


def _assert_exact(got, ref, what):
    for name, g in got.items():
        r = getattr(ref, name)
        assert g.shape == r.shape and torch.equal(g.double(), r), (what, name, float((g.double() - r).abs().max()))


# B, H, N, dim, scales, kscale, largest |g_keys|
EXACT = [
    (2, 3, 777, 2, True, True, 4),
    (2, 3, 777, 3, True, True, 4),
    (8, 16, 1300, 3, True, False, 2),      # with kscale at this size the g_kscale sum leaves 24 bits in the worst case
    (4, 64, 700, 2, False, False, 2),
    (3, 70, 40, 3, True, True, 4),
]
_exact_ids = ["B%d-H%d-N%d-dim%d" % c[:4] for c in EXACT]


@pytest.mark.parametrize("case", EXACT, ids=_exact_ids)
def test_exact_arithmetic_through_the_workspace(case):
    """ops.lattice (R an input), g_lattice None so that no tanh enters a gradient: the forward's row walk, the backward's 16-lane
    sums over the workgroup partials and its g_kscale tree, term by term — a dropped, doubled or misplaced term changes a bit."""
    from cloud_transformers_amd import ops
    inp = _exact_inputs(*case, seed=sum(case))
    ref = _exact_reference(inp)
    leaves = {n: _leaf(getattr(inp, n)) for n in ("xyz", "res", "R", "shift", "scales", "kscale")}
    keys, lat = ops.lattice(leaves["xyz"], leaves["res"], leaves["R"], leaves["shift"], leaves["scales"], leaves["kscale"], inp.dim)
    (keys * inp.g_keys.cuda()).sum().backward()
    assert torch.equal(keys.detach().cpu().double(), ref.keys)
    assert float((lat.detach().cpu().double() - ref.lattice).abs().max()) <= 2e-5
    _assert_exact({"g_" + n: t.grad.cpu() for n, t in leaves.items() if t is not None}, ref, case)


@pytest.mark.parametrize("case", EXACT[:3], ids=_exact_ids[:3])
def test_exact_arithmetic_through_the_null_workspace_atomics(case):
    """ct_lattice_bwd with a NULL workspace (lattice_zero_kernel, then one float atomic per workgroup and parameter), outside
    deterministic mode: atomic sums of exact terms are exact in any order."""
    from cloud_transformers_amd import _lib, ops
    from cloud_transformers_amd.ops import _ptr, _stream
    lib = _lib.load()
    inp = _exact_inputs(*case, seed=sum(case))
    ref = _exact_reference(inp)
    B, H, N, dim = inp.B, inp.H, inp.N, inp.dim
    dev = lambda t: None if t is None else t.cuda()
    xyz, res, Rm, shift, scales, g_keys = (dev(t) for t in (inp.xyz, inp.res, inp.R, inp.shift, inp.scales, inp.g_keys))
    ks = dev(inp.kscale.reshape(1)) if inp.kscale is not None else None
    keys, lat = ops.lattice(xyz, res, Rm, shift, scales, ks, dim)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    out = {"g_xyz": nan(B, 3, N), "g_res": nan(B, H * 3, N), "g_R": nan(H, 3, 3), "g_shift": nan(H, 3),
           "g_scales": nan(H, dim) if scales is not None else None, "g_kscale": nan(1) if ks is not None else None}
    assert lib.ct_get_deterministic() == 0
    rc = lib.ct_lattice_bwd(_ptr(xyz), _ptr(res), _ptr(Rm), _ptr(shift), _ptr(scales), _ptr(ks), _ptr(lat), None, _ptr(g_keys),
                            _ptr(out["g_xyz"]), _ptr(out["g_res"]), _ptr(out["g_R"]), _ptr(out["g_shift"]), _ptr(out["g_scales"]),
                            _ptr(out["g_kscale"]), None, 0, B, H, N, dim, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = {n: t.cpu() for n, t in out.items() if t is not None}
    if ks is not None:
        got["g_kscale"] = got["g_kscale"].reshape(())
    _assert_exact(got, ref, case)


# ---------------------------------------------------------------------------
# 2. float64 parity at all shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["split", "fused"])
@pytest.mark.parametrize("params", [False, True], ids=["bare", "scales-kscale"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_parity_with_float64_at_every_shape(shape, dim, params, path):
    inp = _inputs(*shape, dim, params, params, seed=7 * sum(shape) + dim + 2 * params)
    t = _forward(inp, path, with_stats=(path == "fused"))
    what = "B%d H%d N%d dim %d %s %s" % (shape + (dim, "params" if params else "bare", path))
    for name, cot_k, cot_l in (("g_keys alone", inp.cot_k, None), ("g_lattice alone", None, inp.cot_l), ("both", inp.cot_k, inp.cot_l)):
        got = _backward(t, cot_k, cot_l)
        ref = _reference(inp, t, path, cot_k, cot_l)
        if name == "g_keys alone":       # the forward's values: once
            _check_values(t, ref, what)
            if t.stats is not None:
                _check_stats(t.stats, ref, inp, what)
        _check_grads(got, ref, what + ", " + name)


# ---------------------------------------------------------------------------
# 3. statistics with a stated bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["split", "fused"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_statistics_of_centred_keys(shape, dim, path):
    """3a: ops.lattice(with_stats=True) (two launches, lattice_stats_kernel) and ops.lattice_so3(with_stats=True) (the launch's
    last workgroup) against the float64 mean and unbiased variance of the reference keys"""
    inp = _inputs(*shape, dim, True, True, seed=11 * sum(shape) + dim)
    t = _forward(inp, path, with_stats=True)
    ref = _reference(inp, t, path)
    _check_values(t, ref, "centred")
    _check_stats(t.stats, ref, inp, "centred B%d H%d N%d dim %d %s" % (shape + (dim, path)))


def _rotated(log_R, value):
    """per head the 3-vector p whose rotated coordinates p R_h are all `value`: R_h (value, value, value)"""
    return (L.so3(log_R) @ torch.full((3,), float(value), dtype=torch.float64)).float()


@pytest.mark.parametrize("path", ["split", "fused"])
def test_statistics_of_off_centre_keys(path):
    """3b: keys of mean about 3 and standard deviation about 0.05 (shift is a learned parameter: nothing keeps the keys centred).
    The bound is relative to mean(k^2) = 9, so it is a visible fraction of the variance 0.0025 — what the kernel promises."""
    inp = _inputs(8, 16, 1300, 3, False, False, seed=31)
    inp.xyz, inp.res = inp.xyz * 0.08, inp.res / 15
    inp.shift = _rotated(inp.log_R, 3.0)
    t = _forward(inp, path, with_stats=True)
    ref = _reference(inp, t, path)
    assert abs(float(ref.mean) - 3.0) < 0.05 and 0.03 < float(ref.var) ** 0.5 < 0.07, (float(ref.mean), float(ref.var))
    _check_values(t, ref, "off-centre")
    _check_stats(t.stats, ref, inp, "off-centre %s" % path)


@pytest.mark.parametrize("path", ["split", "fused"])
@pytest.mark.parametrize("start", [256, 1024], ids=["second-step-of-workgroup-0", "ragged-workgroup"])
def test_statistics_keep_every_partial(start, path):
    """3c: one 256-point stretch of one row has keys about 10, the rest about 0 (through the residual): a partial that is
    dropped, read twice or read before it is written moves the mean by 1000 bounds."""
    inp = _inputs(8, 16, 1300, 3, False, False, seed=37)
    b, h = 5, 11
    inp.res[b, 3 * h:3 * h + 3, start:start + 256] += _rotated(inp.log_R, 10.0)[h][:, None]
    t = _forward(inp, path, with_stats=True)
    ref = _reference(inp, t, path)
    stretch = ref.keys[b, 3 * h:3 * h + 3, start:start + 256]
    assert float(stretch.min()) > 6.0 and float(ref.keys.abs().mean()) < 1.0
    _check_values(t, ref, "stretch")
    _check_stats(t.stats, ref, inp, "stretch at %d %s" % (start, path))


# ---------------------------------------------------------------------------
# 4. twin arithmetic, bit for bit
# ---------------------------------------------------------------------------
def test_so3_inside_the_lattice_launches_equals_the_stand_alone_kernels_bit_for_bit():
    """so3_exp_one / so3_exp_bwd_one (inside the lattice launches) and so3_exp_fwd_kernel / so3_exp_bwd_kernel carry the same
    double arithmetic twice: 70 heads with large angles, rows below the clamp, a zero row and both sides of sqrt(eps)."""
    from cloud_transformers_amd import _lib, ops
    from cloud_transformers_amd.ops import _ptr, _stream
    lib = _lib.load()
    B, H, N, dim = 3, 70, 40, 3
    inp = _inputs(B, H, N, dim, True, True, seed=41)
    inp.log_R = L.so3_rows_70(torch.Generator().manual_seed(43))
    s = (inp.log_R.double() ** 2).sum(1)
    assert bool(((s - L.EPS).abs() > 1e-9).all()) and int((s < L.EPS).sum()) >= 10 and float(s.max()) > 3.1416 ** 2

    # the R that ct_lattice_so3_fwd writes (no statistics: no ticket needed)
    d = lambda x: x.cuda()
    R_out, keys, lat = torch.full((H, 3, 3), float("nan"), device="cuda"), torch.empty(B, H * dim, N, device="cuda"), torch.empty(B, H * dim, N, device="cuda")
    xyz, res, log_R, shift, scales, ks = d(inp.xyz), d(inp.res), d(inp.log_R), d(inp.shift), d(inp.scales), d(inp.kscale.reshape(1))
    rc = lib.ct_lattice_so3_fwd(_ptr(xyz), _ptr(res), _ptr(log_R), 1e-4, _ptr(shift), _ptr(scales), _ptr(ks), _ptr(R_out), _ptr(keys),
                                _ptr(lat), None, None, 0, None, B, H, N, dim, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    R_alone = ops.so3_exp(log_R)
    assert torch.equal(R_out, R_alone)

    fused, split = _forward(inp, "fused"), _forward(inp, "split")
    assert torch.equal(fused.keys, keys) and torch.equal(fused.lattice, lat)
    assert torch.equal(fused.keys, split.keys) and torch.equal(fused.lattice, split.lattice)
    gf, gs = _backward(fused, inp.cot_k, inp.cot_l), _backward(split, inp.cot_k, inp.cot_l)
    assert set(gs) - set(gf) == {"g_R"}
    for name, g in gf.items():       # g_log_R: so3_exp_bwd_one on the tail's g_R against So3ExpFn.backward of the same g_R
        assert torch.equal(g, gs[name]), (name, float((g - gs[name]).abs().max()))

    # and the stand-alone kernels at these rows against float64
    ref_R = L.so3(inp.log_R)
    assert float((R_alone.cpu().double() - ref_R).abs().max()) <= 2e-6
    ref_g = L.so3_grad(inp.log_R, gs["g_R"])
    assert float((gs["g_log_R"].double() - ref_g).abs().max()) <= 2e-5 * max(1.0, float(ref_g.abs().max()))
    eye = torch.eye(3, device="cuda").expand_as(R_alone)
    assert float((R_alone @ R_alone.transpose(1, 2) - eye).abs().max()) <= 1e-5


def test_so3_exp_of_no_heads():
    from cloud_transformers_amd import ops
    v = torch.empty(0, 3, device="cuda", requires_grad=True)
    Rm = ops.so3_exp(v)
    Rm.sum().backward()
    torch.cuda.synchronize()
    assert Rm.shape == (0, 3, 3) and Rm.dtype == torch.float32 and v.grad.shape == (0, 3)


# ---------------------------------------------------------------------------
# 5. inputs where they lie
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ks_shape", [(), (1,)], ids=["kscale-0dim", "kscale-1"])
@pytest.mark.parametrize("path", ["split", "fused"])
def test_views_give_the_bits_of_their_contiguous_clones(path, ks_shape):
    """xyz as a transposed [B,N,3], the residual as the first 3H channels of a wider leaf (how the blocks produce it)"""
    from cloud_transformers_amd import ops
    B, H, N, dim = 2, 5, 257, 3
    inp = _inputs(B, H, N, dim, True, True, seed=53)
    g = torch.Generator().manual_seed(59)
    points = inp.xyz.transpose(1, 2).contiguous().cuda().requires_grad_(True)                        # [B,N,3]
    wide = torch.cat([inp.res, torch.randn(B, 16, N, generator=g)], 1).cuda().requires_grad_(True)     # [B,3H+16,N]
    views = (points.transpose(1, 2), wide[:, :3 * H])
    assert not views[0].is_contiguous() and not views[1].is_contiguous()
    clones = tuple(v.detach().clone(memory_format=torch.contiguous_format).requires_grad_(True) for v in views)
    assert clones[0].is_contiguous() and clones[1].is_contiguous()
    outs = []
    for xyz, res in (views, clones):
        log_R, shift, scales = _leaf(inp.log_R), _leaf(inp.shift), _leaf(inp.scales)
        ks = _leaf(inp.kscale.reshape(ks_shape))
        if path == "fused":
            keys, lat = ops.lattice_so3(xyz, res, log_R, shift, scales, ks, dim)
        else:
            keys, lat = ops.lattice(xyz, res, ops.so3_exp(log_R), shift, scales, ks, dim)
        ((keys * inp.cot_k.cuda()).sum() + (lat * inp.cot_l.cuda()).sum()).backward()
        assert ks.grad.shape == ks_shape
        outs.append((keys.detach(), lat.detach(), log_R.grad, shift.grad, scales.grad, ks.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.equal(points.grad.transpose(1, 2), clones[0].grad)
    assert torch.equal(wide.grad[:, :3 * H], clones[1].grad)
    assert float(wide.grad[:, 3 * H:].abs().max()) == 0.0


# ---------------------------------------------------------------------------
# 6. non-finite confinement
# ---------------------------------------------------------------------------
def _same_bits(a, b):
    """torch.equal that lets NaN equal NaN"""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


@pytest.mark.parametrize("use_kscale", [False, True], ids=["bare", "kscale"])
@pytest.mark.parametrize("dim", [2, 3])
def test_a_nan_stays_at_its_point_and_poisons_its_heads_sums(dim, use_kscale):
    B, H, N = 2, 5, 257
    inp = _inputs(B, H, N, dim, True, use_kscale, seed=61 + dim)
    b, h, c, n = 1, 3, 1, 256                                     # the one point of the second workgroup
    clean = _forward(inp, "split")
    g_clean = _backward(clean, inp.cot_k, inp.cot_l)
    inp.res[b, 3 * h + c, n] = float("nan")
    bad = _forward(inp, "split")
    g_bad = _backward(bad, inp.cot_k, inp.cot_l)
    assert not any(bool(g.isnan().any()) for g in g_clean.values())

    def confined(got, want, index, name):
        mask = torch.zeros(want.shape, dtype=torch.bool)
        mask[index] = True
        got = got.detach().cpu()
        assert bool(got[mask].isnan().all()), name
        assert torch.equal(got[~mask], want.detach().cpu()[~mask]), name

    at = (b, slice(h * dim, (h + 1) * dim), n)
    confined(bad.keys, clean.keys, at, "keys")
    confined(bad.lattice, clean.lattice, at, "lattice")
    confined(g_bad["g_xyz"], g_clean["g_xyz"], (b, slice(None), n), "g_xyz")
    confined(g_bad["g_res"], g_clean["g_res"], (b, slice(3 * h, 3 * h + 3), n), "g_res")
    if use_kscale:                                               # one sum over everything
        assert bool(g_bad["g_kscale"].isnan().all())
    # sums over the head's points: poisoned (the columns of g_R that dim = 2 leaves out are products with a zero cotangent)
    confined(g_bad["g_R"][:, :, :dim], g_clean["g_R"][:, :, :dim], h, "g_R")
    confined(g_bad["g_shift"], g_clean["g_shift"], h, "g_shift")
    confined(g_bad["g_scales"], g_clean["g_scales"], h, "g_scales")
    others = [i for i in range(H) if i != h]
    assert torch.equal(g_bad["g_R"][others], g_clean["g_R"][others])


# ---------------------------------------------------------------------------
# 7. launch after launch
# ---------------------------------------------------------------------------
def test_launch_after_launch_at_different_grid_sizes():
    """ops.lattice_so3(with_stats=True) at B8 H16 N1300 three times with fresh inputs, then one point, then the large shape again:
    the ticket word and the workspaces serve grids of 384 workgroups and of 1; every launch against the reference, not the last."""
    from cloud_transformers_amd import ops
    for it, shape in enumerate([(8, 16, 1300)] * 3 + [(1, 1, 1), (8, 16, 1300)]):
        inp = _inputs(*shape, 3, True, True, seed=71 + it)
        t = _forward(inp, "fused", with_stats=True)
        got = _backward(t, inp.cot_k, inp.cot_l)
        ref = _reference(inp, t, "fused", inp.cot_k, inp.cot_l)
        what = "launch %d B%d H%d N%d" % ((it,) + shape)
        # the launch leaves its ticket (ops.LatticeSo3Fn: the last word of the stream's ticket buffer) zero for the next one: a word
        # left at 1 lets the second-to-last workgroup of the next launch finish the statistics, usually unnoticed
        assert int(ops.raster_tickets(t.keys.device, force=True)[-1]) == 0, what
        _check_values(t, ref, what)
        _check_stats(t.stats, ref, inp, what)
        _check_grads(got, ref, what)
