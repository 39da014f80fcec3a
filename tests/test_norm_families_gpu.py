"""Every kernel body of the training BatchNorm, the SyncBatchNorm exchange phases, the eval norms and AdaIN (the rows of
tests/norm_families.py) straight through the C ABI with ctypes item tables: the launch tag, and every output against float64 on
the host computed from the fp32 inputs.  Buffers, strides and the NaN prefill are the test's own.

Data: `plain` x = 3 N(0,1) + 0.7 (rank r of a multi-rank case shifted by 2r); `offset` x = 1000 + U(-1,1)_c + N(0,1), the
cancellation case (|mean| >> |x - mean|).  Weights U(0.5, 1.5) with random sign, bias U(-0.5, 0.5), gy = N(0,1).  With ReLU the
backward reference takes its mask from what the kernel's forward stored (y > 0, forward without residual): an element within
rounding of zero is decided by the forward and by nobody else.

Bounds.  u = 2^-24; mu, var, rstd, g = w rstd, xhat from float64; A = mean |x| over the channel (over all ranks); g' the masked
cotangent, m0 = mean g', m1 = mean g' xhat; M values per channel (the job's); D the summation depth read off the kernel: the
adds a value passes through.  A thread adds one item per round of its loop: ceil(items / threads) adds, the items being the
M / 4 quads of a float4 body (reg*, loop_vec, AdaIN's reg*; + 2 for the quad's own (x + y) + (z + w)) and the M floats of a
scalar one (loop_scalar, strided); then 6 shuffle steps and one add per wave (16 for the 1024-thread BatchNorm workgroup, 4 for
AdaIN's 256), + world where ranks are added.  8192 quads: D = 8 + 2 + 6 + 16 = 32.  A sum of fp32 terms of depth D errs by at
most D u sum |term| to first order.

Elementwise (the coefficients 8 are not derived worst cases: tests/test_norm_families_cpu.py holds an fp32 emulation of the
kernels to at most half of them and shows six wrong variants of the emulation outside them):
  |y  - y64 | <= u ( 8 |x - mu| |g| + 8 A |g| + 2 |b| + 2 |y64| + |res| )
  |gx - gx64| <= u |g| ( 8 (|g'| + |m0| + |xhat| |m1|) + 8 mean|g'| + |xhat| (8 mean|g' xhat| + 8 A rstd mean|g'|)
                         + (8 |xhat| + 8 A rstd) |m1| )
The A terms are the rounding of the channel mean of fp32 data (|delta mu| ~ u A): at offset 1000 they are inherent, not slack.
ReLU is 1-Lipschitz, so the forward bound is that of the value before it.

Per channel:
  mean          dmu = (D + 2) u A                          (the sum, the division)
  sum (x-mean)^2  (D + 6) u m2 + n dmu^2                   (x - mean and its square round three times; the first-order effect of
                                                           delta mean cancels because sum (x - mean) = 0, the second is n dmu^2)
  var           dvar = (D + 6) u var + sum_r n_r (4 |mean_r - mu| dmu + 4 dmu^2) / M      (the merge term n_r (mean_r - mu)^2
                                                           with both means off by dmu; one rank: 4 dmu^2 covers the line above)
  rstd          rstd (dvar / (2 (var + eps)) + 4 u)        (the device rsqrt is within 2 ulp, + eps and the division round)
  running_mean  momentum dmu + 3 u (|(1 - momentum) old| + |momentum mu|)
  running_var   momentum (dvar + 3 u var) M / (M - 1) + 3 u (|(1 - momentum) old| + momentum var M / (M - 1))
  sum g'        D u sum |g'|                               (g_bias, g_beta, sums[0:C])
  sum g' xhat   (D + 4) u sum |g' xhat| + sum |g'| dmu rstd + sum |g' xhat| drstd / rstd      (g_weight, g_gamma, sums[C:2C])
  ranks added   + world u sum_r |sum_r|
  count, num_batches_tracked, amax_out (the maxima of the stored values): exact.
The eval rows keep the bounds of tests/test_bn_eval_gpu.py and tests/test_bn_frozen_gpu.py.

Every test prints its worst error-to-bound ratio per output (`RATIO ...`); DESIGN.md records the worst per family."""
import ctypes
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import norm_families as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS, MOMENTUM = 1e-5, 0.1
NAN = float("nan")
DISTS = ("plain", "offset")
NBT0 = 5                      # num_batches_tracked before the launch
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------------
# inputs, float64 reference, bounds (host only: tests/test_norm_families_cpu.py uses them too)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_case(key, Bs, C, N, dist, integer_gy=False):
    """fp32 inputs of one norm over len(Bs) ranks of Bs[r] clouds each (computed once per key, never written to)."""
    g = np.random.default_rng(zlib.crc32(("%s %s %s %s %s" % (key, Bs, C, N, dist)).encode()))
    off = g.uniform(-1, 1, C)
    xs, gys, ress = [], [], []
    for r, B in enumerate(Bs):
        n = g.standard_normal((B, C, N))
        xs.append(f32(3 * n + 0.7 + 2 * r if dist == "plain" else 1000 + off[None, :, None] + n))
        gys.append(f32(g.choice([-2, -1, 1, 2], (B, C, N)) if integer_gy else g.standard_normal((B, C, N))))
        ress.append(f32(g.standard_normal((B, C, N))))
    case = dict(xs=xs, gys=gys, ress=ress, w=f32(g.uniform(0.5, 1.5, C) * g.choice([-1, 1], C)), b=f32(g.uniform(-0.5, 0.5, C)),
                rm=f32(g.uniform(-1, 1, C)), rv=f32(g.uniform(0.5, 2, C)))
    for v in case.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return case


def depth(M, threads, vec):
    """the adds a value passes through in a workgroup's sum of M values (module docstring); vec: a float4 body"""
    per_thread = -(-(int(M) // 4) // threads) + 2 if vec else -(-int(M) // threads)
    return per_thread + 6 + threads // 64


def bn_vecs(Bs, N, aligned=True):
    """per rank: does the training BatchNorm launch of (B_r, N) take a float4 body"""
    return [F.bn_family(B, N, aligned) != "loop_scalar" for B in Bs]


def _c(v):
    return v[None, :, None]


def forward_ref(xs, w, b, relu, vecs, ress=None, rm=None, rv=None, threads=F.BN_THREADS):
    """float64 forward of one norm over the concatenation of the ranks' batches, with every bound of the module docstring;
    vecs: per rank, whether its launch takes a float4 body (the summation depth)."""
    X = [x.astype(f64) for x in xs]
    w, b = w.astype(f64), b.astype(f64)
    n = np.array([x.shape[0] * x.shape[2] for x in X], f64)
    M, world = float(n.sum()), len(X)
    allx = np.concatenate(X, 0)
    mu = allx.mean((0, 2))
    var = ((allx - _c(mu)) ** 2).mean((0, 2))
    A = np.abs(allx).mean((0, 2))
    rstd = 1.0 / np.sqrt(var + EPS)
    D_r = [depth(k, threads, v) for k, v in zip(n, vecs)]
    D = max(D_r) + world
    dmu = (D + 2) * U * A
    local = []
    for x, k, d in zip(X, n, D_r):
        m = x.mean((0, 2))
        m2 = ((x - _c(m)) ** 2).sum((0, 2))
        m_b = (d + 2) * U * np.abs(x).mean((0, 2))
        local.append(SimpleNamespace(mean=m, mean_b=m_b, m2=m2, m2_b=(d + 6) * U * m2 + k * m_b ** 2, count=k, D=d))
    dvar = (D + 6) * U * var + sum(l.count * (4 * np.abs(l.mean - mu) * dmu + 4 * dmu ** 2) for l in local) / M
    drstd = rstd * (0.5 * dvar / (var + EPS) + 4 * U)
    g = w * rstd
    ys, y_bs = [], []
    for r, x in enumerate(X):
        y = (x - _c(mu)) * _c(g) + _c(b)
        if relu:
            y = np.maximum(y, 0.0)
        res = 0.0 if ress is None else ress[r].astype(f64)
        y = y + res
        ys.append(y)
        y_bs.append(U * (8 * np.abs(x - _c(mu)) * _c(np.abs(g)) + _c(8 * A * np.abs(g) + 2 * np.abs(b)) + 2 * np.abs(y) + np.abs(res)))
    f = SimpleNamespace(X=X, w=w, b=b, n=n, M=M, world=world, mu=mu, var=var, A=A, rstd=rstd, D=D, dmu=dmu, dvar=dvar, drstd=drstd,
                        g=g, local=local, y=ys, y_b=y_bs, relu=relu)
    if rm is not None:
        unb = var * (M / (M - 1))
        f.rm = (1 - MOMENTUM) * rm.astype(f64) + MOMENTUM * mu
        f.rm_b = MOMENTUM * dmu + 3 * U * (np.abs((1 - MOMENTUM) * rm) + np.abs(MOMENTUM * mu))
        f.rv = (1 - MOMENTUM) * rv.astype(f64) + MOMENTUM * unb
        f.rv_b = MOMENTUM * (dvar + 3 * U * var) * (M / (M - 1)) + 3 * U * (np.abs((1 - MOMENTUM) * rv) + MOMENTUM * unb)
    return f


def backward_ref(f, gys, masks):
    """float64 backward with the forward's masks (None: no ReLU) and its bounds; per rank and for the job."""
    gx, gx_b, sums = [], [], []
    gps, xhs = [], []
    for r, x in enumerate(f.X):
        gp = gys[r].astype(f64) * (1.0 if masks is None else masks[r].astype(f64))
        xh = (x - _c(f.mu)) * _c(f.rstd)
        a0, a1 = np.abs(gp).sum((0, 2)), np.abs(gp * xh).sum((0, 2))
        d = f.local[r].D
        sums.append(SimpleNamespace(s0=gp.sum((0, 2)), s1=(gp * xh).sum((0, 2)), a0=a0, a1=a1, s0_b=d * U * a0,
                                    s1_b=(d + 4) * U * a1 + a0 * f.dmu * f.rstd + a1 * f.drstd / f.rstd))
        gps.append(gp)
        xhs.append(xh)
    extra = f.world if f.world > 1 else 0
    s0, s1 = sum(s.s0 for s in sums), sum(s.s1 for s in sums)
    a0, a1 = sum(s.a0 for s in sums), sum(s.a1 for s in sums)
    gb_b = sum(s.s0_b for s in sums) + extra * U * sum(np.abs(s.s0) for s in sums)
    gw_b = sum(s.s1_b for s in sums) + extra * U * sum(np.abs(s.s1) for s in sums)
    m0, m1 = s0 / f.M, s1 / f.M
    ag, Ar = np.abs(f.g), f.A * f.rstd
    for gp, xh in zip(gps, xhs):
        axh = np.abs(xh)
        gx.append(_c(f.g) * (gp - _c(m0) - xh * _c(m1)))
        gx_b.append(U * _c(ag) * (8 * (np.abs(gp) + _c(np.abs(m0)) + axh * _c(np.abs(m1))) + _c(8 * a0 / f.M)
                                  + axh * _c(8 * a1 / f.M + 8 * Ar * a0 / f.M) + (8 * axh + _c(8 * Ar)) * _c(np.abs(m1))))
    return SimpleNamespace(gx=gx, gx_b=gx_b, sums=sums, gb=s0, gb_b=gb_b, gw=s1, gw_b=gw_b)


class Ratios:
    """worst |got - want| / bound per output; every value finite; all within `limit` at done()"""

    def __init__(self, what, strict=True):
        self.what, self.worst, self.strict = what, {}, strict      # not strict: a value that is not finite counts as ratio inf

    def add(self, name, got, want, bound):
        got = np.asarray(got, f64)
        assert got.shape == np.shape(want), (self.what, name, got.shape, np.shape(want))
        assert not self.strict or np.isfinite(got).all(), (self.what, name, "not finite")
        r = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()) if got.size else 0.0
        r = r if np.isfinite(got).all() else float("inf")
        self.worst[name] = max(self.worst.get(name, 0.0), r)

    def done(self, limit=1.0):
        print("RATIO %s %s" % (self.what, " ".join("%s=%.3f" % kv for kv in sorted(self.worst.items()))))
        bad = {k: v for k, v in self.worst.items() if not v <= limit}
        assert not bad, (self.what, bad)
        return self.worst


def compare(R, f, bw, out):
    """`out` holds lists over the ranks (y, save_mean, save_rstd; rm, rv, local, count_total, gx, sums where present) and the
    job's gb / gw; every entry present is held to its bound."""
    for r in range(len(out["y"])):
        R.add("y", out["y"][r], f.y[r], f.y_b[r])
        R.add("save_mean", out["save_mean"][r], f.mu, f.dmu)
        R.add("save_rstd", out["save_rstd"][r], f.rstd, f.drstd)
        if "rm" in out:
            R.add("running_mean", out["rm"][r], f.rm, f.rm_b)
            R.add("running_var", out["rv"][r], f.rv, f.rv_b)
        if "local" in out:
            mean, m2, count = out["local"][r]
            l = f.local[r]
            R.add("local_mean", mean, l.mean, l.mean_b)
            R.add("local_m2", m2, l.m2, l.m2_b)
            assert float(count) == l.count, (R.what, "local count", float(count), l.count)
        if "count_total" in out:
            assert float(out["count_total"][r]) == f.M, (R.what, "count_total", float(out["count_total"][r]), f.M)
        if bw is not None:
            R.add("gx", out["gx"][r], bw.gx[r], bw.gx_b[r])
            if "sums" in out:
                s = bw.sums[r]
                R.add("sums_g", out["sums"][r][0], s.s0, s.s0_b)
                R.add("sums_gxhat", out["sums"][r][1], s.s1, s.s1_b)
    if bw is not None:
        R.add("g_bias", out["gb"], bw.gb, bw.gb_b)
        R.add("g_weight", out["gw"], bw.gw, bw.gw_b)


def adain_case(row, dist, integer_gy=False):
    """an AdaIN row as a norm over B * C channels of one cloud: gamma + 1 is the weight (in float64 from the fp32 gamma)"""
    c = make_case(row.id, (1,), row.B * row.C, row.N, dist, integer_gy)
    gamma = f32(c["w"] - f32(1))
    return c, gamma, gamma.astype(f64) + 1.0


# ---------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------
def _lib_():
    from cloud_transformers_amd import _lib
    return _lib, _lib.load()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _dev(a):
    return torch.tensor(a, device="cuda")                   # (a copy: the cases are read-only)


def _place(a, shape, layout):
    """(storage, view, batch stride) of a (B, C, N) tensor: dense, one float into its storage, or channels 3 .. 3 + C of a
    NaN-filled tensor of C + 8 channels; a = None: NaN everywhere (an output)"""
    B, C, N = shape
    if layout == "slice":
        store = _nan(B, C + 8, N)
        view, bs = store[:, 3:3 + C], (C + 8) * N
    elif layout == "x_offset":
        store = _nan(B * C * N + 1)
        view, bs = store[1:].view(B, C, N), 0
    else:
        store = _nan(B, C, N)
        view, bs = store, 0
    if a is not None:
        view.copy_(_dev(a))
    return store, view, bs


def _outside_is_nan(store, C):
    return bool(torch.isnan(store[:, :3]).all()) and bool(torch.isnan(store[:, 3 + C:]).all())


def _call(lib, name, items, *args):
    arr = (type(items[0]) * len(items))(*items)
    rc = getattr(lib, name)(ctypes.addressof(arr), len(items), *args, None)
    assert rc == 0, (name, rc)
    return lib.ct_debug_last_launch().decode()


class DevBn:
    """the buffers of one training norm on one rank; every output prefilled with NaN"""

    def __init__(self, x, w, b, relu, gy=None, res=None, rm=None, rv=None, layout="dense", res_layout="dense"):
        self.shape = self.B, self.C, self.N = x.shape
        C, io = self.C, "slice" if layout == "slice" else "dense"
        self.relu = int(relu)
        self.x_store, self.x, self.xbs = _place(x, self.shape, layout)
        self.y_store, self.y, self.ybs = _place(None, self.shape, io)
        self.gy_store, self.gy, self.gybs = _place(gy, self.shape, io) if gy is not None else (None, None, 0)
        self.gx_store, self.gx, self.gxbs = _place(None, self.shape, io)
        self.res_store, self.res, self.rbs = _place(res, self.shape, res_layout) if res is not None else (None, None, 0)
        self.w, self.b = _dev(w), _dev(b)
        self.rm, self.rv = (None, None) if rm is None else (_dev(rm).clone(), _dev(rv).clone())
        self.nbt = torch.full((1,), NBT0, dtype=torch.int64, device="cuda")
        self.save_mean, self.save_rstd, self.amax_y, self.amax_gx, self.gw, self.gb = (_nan(C) for _ in range(6))

    def fwd_item(self, _lib):
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        return _lib.BnFwdItem(x=p(self.x), x_batch_stride=self.xbs, weight=p(self.w), bias=p(self.b), running_mean=p(self.rm),
                              running_var=p(self.rv), num_batches_tracked=p(self.nbt), residual=p(self.res),
                              residual_batch_stride=self.rbs, y=p(self.y), y_batch_stride=self.ybs, save_mean=p(self.save_mean), save_rstd=p(self.save_rstd),
                              amax_out=p(self.amax_y), C=self.C, eps=EPS, momentum=MOMENTUM, relu=self.relu)

    def bwd_item(self, _lib):
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        return _lib.BnBwdItem(x=p(self.x), x_batch_stride=self.xbs, weight=p(self.w), bias=p(self.b), save_mean=p(self.save_mean),
                              save_rstd=p(self.save_rstd), gy=p(self.gy), gy_batch_stride=self.gybs, gx=p(self.gx),
                              gx_batch_stride=self.gxbs, g_weight=p(self.gw), g_bias=p(self.gb), amax_out=p(self.amax_gx), C=self.C,
                              relu=self.relu)

    def outputs(self, backward=True):
        names = ["y", "save_mean", "save_rstd", "amax_y", "nbt"] + (["rm", "rv"] if self.rm is not None else [])
        names += ["gx", "gw", "gb", "amax_gx"] if backward else []
        return {k: getattr(self, k) for k in names}

    def check_exact_outputs(self, backward=True):
        assert int(self.nbt) == NBT0 + 1
        assert torch.equal(self.amax_y, self.y.abs().amax(dim=(0, 2))), "amax_out of the forward"
        if backward:
            assert torch.equal(self.amax_gx, self.gx.abs().amax(dim=(0, 2))), "amax_out of the backward"


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b, what):
    for k, v in a.items():
        assert torch.equal(v, b[k]), (what, k)


def run_train(norms, B, N, backward=True):
    _lib, lib = _lib_()
    tags = [_call(lib, "ct_bn_group_fwd", [n.fwd_item(_lib) for n in norms], B, N)]
    if backward:
        tags.append(_call(lib, "ct_bn_group_bwd", [n.bwd_item(_lib) for n in norms], B, N))
    torch.cuda.synchronize()
    return tuple(tags)


def forward_mask(case, relu, r=0):
    """where the kernel's forward (no residual, dense) stored a positive value; None without ReLU"""
    if not relu:
        return None
    d = DevBn(case["xs"][r], case["w"], case["b"], 1)
    run_train([d], d.B, d.N, backward=False)
    return _np(d.y) > 0


def train_out(d):
    return dict(y=[_np(d.y)], save_mean=[_np(d.save_mean)], save_rstd=[_np(d.save_rstd)], rm=[_np(d.rm)], rv=[_np(d.rv)],
                gx=[_np(d.gx)], gb=_np(d.gb), gw=_np(d.gw))


def run_ranks(case, Bs, C, N, relu):
    """the six steps of the exchange on one GPU; returns (the ranks' buffers, `out` for compare(), the tags by rank)"""
    _lib, lib = _lib_()
    world = len(Bs)
    devs = [DevBn(case["xs"][r], case["w"], case["b"], relu, gy=case["gys"][r], rm=case["rm"], rv=case["rv"]) for r in range(world)]
    local = [_nan(2 * C + 1) for _ in Bs]
    count = [_nan(1) for _ in Bs]
    sums = [_nan(2 * C) for _ in Bs]
    copy = [_nan(2 * C) for _ in Bs]
    tags = [[] for _ in Bs]
    for r, d in enumerate(devs):
        tags[r].append(_call(lib, "ct_bn_group_stats_fwd", [d.fwd_item(_lib)], 0, 1, Bs[r], N, local[r].data_ptr()))
    gathered = torch.cat(local)
    for r, d in enumerate(devs):
        tags[r].append(_call(lib, "ct_bn_group_apply_fwd", [d.fwd_item(_lib)], 0, 1, Bs[r], N, gathered.data_ptr(), world,
                             count[r].data_ptr()))
    for r, d in enumerate(devs):
        tags[r].append(_call(lib, "ct_bn_group_reduce_bwd", [d.bwd_item(_lib)], 0, 1, Bs[r], N, sums[r].data_ptr(), copy[r].data_ptr()))
    total = sums[0].clone()
    for s in sums[1:]:
        total = total + s                                  # fp32, in rank order: what the all_reduce does
    for r, d in enumerate(devs):
        tags[r].append(_call(lib, "ct_bn_group_apply_bwd", [d.bwd_item(_lib)], 0, 1, Bs[r], N, total.data_ptr(), count[r].data_ptr()))
    torch.cuda.synchronize()
    for r in range(world):
        assert torch.equal(sums[r], copy[r]), "sums_copy"
    L = [_np(l) for l in local]
    S = [_np(s).astype(f64) for s in copy]
    out = dict(y=[_np(d.y) for d in devs], save_mean=[_np(d.save_mean) for d in devs], save_rstd=[_np(d.save_rstd) for d in devs],
               rm=[_np(d.rm) for d in devs], rv=[_np(d.rv) for d in devs], gx=[_np(d.gx) for d in devs],
               local=[(l[:C], l[C:2 * C], l[2 * C]) for l in L], count_total=[_np(c)[0] for c in count],
               sums=[(s[:C], s[C:]) for s in S], gb=sum(s[:C] for s in S), gw=sum(s[C:] for s in S))
    bits = dict(total=total, gathered=gathered)
    for r, d in enumerate(devs):
        for k, v in d.outputs().items():
            if k not in ("gw", "gb"):                      # (the phases write the sums buffers, not the items' g_weight / g_bias)
                bits["%s%d" % (k, r)] = v
    return devs, out, tags, bits


def _phase_tags(family):
    return ["bn_fwd_" + family] * 2 + ["bn_bwd_" + family] * 2


# ---------------------------------------------------------------------------------------------------------------------
# training BatchNorm
# ---------------------------------------------------------------------------------------------------------------------
TRAIN = F.rows("bn_train")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("row", TRAIN, ids=[r.id for r in TRAIN])
def test_bn_train_row(row, dist, relu):
    case = make_case(row.id, (row.B,), row.C, row.N, dist)

    def launch():
        d = DevBn(case["xs"][0], case["w"], case["b"], relu, gy=case["gys"][0], rm=case["rm"], rv=case["rv"], layout=row.variant)
        return d, run_train([d], row.B, row.N)

    d, tags = launch()
    assert tags == row.tags
    f = forward_ref(case["xs"], case["w"], case["b"], relu, bn_vecs((row.B,), row.N, row.variant == "dense"), rm=case["rm"], rv=case["rv"])
    bw = backward_ref(f, case["gys"], [_np(d.y) > 0] if relu else None)
    R = Ratios("%s %s relu=%d %s" % (row.id, dist, relu, "+".join(tags)))
    compare(R, f, bw, train_out(d))
    R.done()
    d.check_exact_outputs()
    again, _ = launch()
    _same_bits(d.outputs(), again.outputs(), "second launch")


PHASES = F.rows("bn_phases")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("row", PHASES, ids=[r.id for r in PHASES])
def test_bn_phases_row(row, dist, relu):
    """world = 1: `gathered` is `local`; each of the four phases reports the row's body"""
    case = make_case(row.id, (row.B,), row.C, row.N, dist)
    devs, out, tags, bits = run_ranks(case, (row.B,), row.C, row.N, relu)
    assert tags[0] == [row.tags[0]] * 2 + [row.tags[1]] * 2
    f = forward_ref(case["xs"], case["w"], case["b"], relu, bn_vecs((row.B,), row.N), rm=case["rm"], rv=case["rv"])
    bw = backward_ref(f, case["gys"], [out["y"][0] > 0] if relu else None)
    R = Ratios("%s %s relu=%d %s" % (row.id, dist, relu, "+".join(row.tags)))
    compare(R, f, bw, out)
    R.done()
    devs[0].check_exact_outputs()
    _same_bits(bits, run_ranks(case, (row.B,), row.C, row.N, relu)[3], "second run")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("ranks", F.RANKS, ids=[r.id for r in F.RANKS])
def test_bn_multi_rank(ranks, dist, relu):
    """Ranks with different numbers of clouds and different means against the float64 norm over the concatenated batch."""
    case = make_case(ranks.id, ranks.Bs, ranks.C, ranks.N, dist)
    devs, out, tags, bits = run_ranks(case, ranks.Bs, ranks.C, ranks.N, relu)
    for r, fam in enumerate(ranks.families):
        assert tags[r] == _phase_tags(fam), (r, tags[r])
    f = forward_ref(case["xs"], case["w"], case["b"], relu, bn_vecs(ranks.Bs, ranks.N), rm=case["rm"], rv=case["rv"])
    assert f.M == sum(ranks.Bs) * ranks.N
    bw = backward_ref(f, case["gys"], [y > 0 for y in out["y"]] if relu else None)
    R = Ratios("%s %s relu=%d" % (ranks.id, dist, relu))
    compare(R, f, bw, out)
    R.done()
    for d in devs:
        d.check_exact_outputs()
    _same_bits(bits, run_ranks(case, ranks.Bs, ranks.C, ranks.N, relu)[3], "second run")


@pytest.mark.parametrize("entry", ["ct_bn_group_bwd", "ct_bn_group_reduce_bwd"])
@pytest.mark.parametrize("id", F.MASK_ROWS)
def test_bn_mask_is_the_forward_s(id, entry):
    """ReLU on, gy from {+-1, +-2}: every partial sum is an integer below 2^24, so g_bias must equal sum gy [y > 0] exactly."""
    row = F.by_id(id)
    case = make_case(row.id, (row.B,), row.C, row.N, "plain", True)
    if entry == "ct_bn_group_bwd":
        d = DevBn(case["xs"][0], case["w"], case["b"], 1, gy=case["gys"][0])
        assert run_train([d], row.B, row.N) == row.tags
        y, gb = _np(d.y), _np(d.gb)
    else:
        _, out, tags, _ = run_ranks(case, (row.B,), row.C, row.N, 1)
        assert tags[0] == [row.tags[0]] * 2 + [row.tags[1]] * 2
        y, gb = out["y"][0], out["sums"][0][0]
    passed = y > 0
    assert 0.2 < 1.0 - passed.mean() < 0.8, "badly chosen case: %.3f masked" % (1.0 - passed.mean())
    want = (case["gys"][0].astype(np.int64) * passed).sum((0, 2))
    assert np.array_equal(gb.astype(f64), want.astype(f64)), (gb, want)


@pytest.mark.parametrize("residual", ["dense", "slice"])
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("id", F.SLICE_ROWS)
def test_bn_channel_slices(id, dist, residual):
    """x, y, gy, gx as channel slices of wider NaN-filled tensors (batch stride (C + 8) N), ReLU on; the residual dense
    (residual_batch_stride 0) or a slice of such a tensor too (residual_batch_stride (C + 8) N)."""
    row = F.by_id(id)
    case = make_case(row.id, (row.B,), row.C, row.N, dist)
    d = DevBn(case["xs"][0], case["w"], case["b"], 1, gy=case["gys"][0], res=case["ress"][0], rm=case["rm"], rv=case["rv"], layout="slice",
              res_layout=residual)
    assert d.rbs == ((row.C + 8) * row.N if residual == "slice" else 0)
    assert run_train([d], row.B, row.N) == row.tags
    f = forward_ref(case["xs"], case["w"], case["b"], 1, bn_vecs((row.B,), row.N), ress=case["ress"], rm=case["rm"], rv=case["rv"])
    bw = backward_ref(f, case["gys"], [forward_mask(case, 1)])
    R = Ratios("slices %s %s residual=%s" % (row.id, dist, residual))
    compare(R, f, bw, train_out(d))
    R.done()
    d.check_exact_outputs()
    assert _outside_is_nan(d.y_store, row.C) and _outside_is_nan(d.gx_store, row.C)


def _table_norms(row, dist, offset_middle=False):
    out = []
    for i, C in enumerate((3, 8, 5)):
        case = make_case("%s table %d" % (row.id, i), (row.B,), C, row.N, dist)
        layout = "x_offset" if offset_middle and i == 1 else "dense"
        out.append((case, DevBn(case["xs"][0], case["w"], case["b"], i != 1, gy=case["gys"][0], rm=case["rm"], rv=case["rv"], layout=layout)))
    return out


@pytest.mark.parametrize("id", F.TABLE_ROWS)
def test_bn_table_of_three(id):
    """Three norms of C = 3, 8, 5 in one launch: the bits of the three launched alone; with the middle norm's x one float off
    the 16-byte grid the WHOLE launch takes the scalar loop kernels (vec_all is a property of the launch) and stays in bounds.
    (On the loop_scalar row the launch is scalar with or without the neighbour: the reg and loop_vec rows pin the vec_all rule.)"""
    row = F.by_id(id)
    table = _table_norms(row, "plain")
    assert run_train([d for _, d in table], row.B, row.N) == row.tags
    for (_, d), (_, alone) in zip(table, _table_norms(row, "plain")):
        assert run_train([alone], row.B, row.N) == row.tags
        _same_bits(d.outputs(), alone.outputs(), "table against alone")
        assert not any(bool(torch.isnan(v).any()) for v in d.outputs().values())
    off = _table_norms(row, "plain", offset_middle=True)
    assert run_train([d for _, d in off], row.B, row.N) == ("bn_fwd_loop_scalar", "bn_bwd_loop_scalar")
    R = Ratios("table with a misaligned neighbour %s" % row.id)
    for case, d in off:
        f = forward_ref(case["xs"], case["w"], case["b"], d.relu, [False], rm=case["rm"], rv=case["rv"])
        compare(R, f, backward_ref(f, case["gys"], [_np(d.y) > 0] if d.relu else None), train_out(d))
        d.check_exact_outputs()
    R.done()


# ---------------------------------------------------------------------------------------------------------------------
# eval BatchNorm: tags, and the bounds of tests/test_bn_eval_gpu.py / tests/test_bn_frozen_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
def eval_cut(B, N, channels, aligned=True):
    """runs per channel of ct_bn_eval_group_fwd without maxima (tests/test_bn_eval_gpu.py's _expected_split)"""
    per = B * (N // 4) if N % 4 == 0 and aligned else B * N
    return max(1, min(-(-1024 // channels), per // 2048))


def _eval_ref(case, relu):
    x, w, b = case["xs"][0].astype(f64), case["w"].astype(f64), case["b"].astype(f64)
    rm, rs = case["rm"].astype(f64), 1.0 / np.sqrt(case["rv"].astype(f64) + EPS)
    xh = (x - _c(rm)) * _c(rs)
    o = xh * _c(w) + _c(b)
    return xh, o, (np.abs(xh) * _c(np.abs(w)) + _c(np.abs(b))) * 2.0 ** -20, rs


EVAL = F.rows("bn_eval")


@pytest.mark.parametrize("with_amax", [False, True])
@pytest.mark.parametrize("row", EVAL, ids=[r.id for r in EVAL])
def test_bn_eval_row(row, with_amax):
    """norms of C and C + 2 channels in one launch; without maxima the channels of the `cut` rows are cut into runs"""
    _lib, lib = _lib_()
    assert eval_cut(row.B, row.N, 2 * row.C + 2) == row.cut
    R = Ratios("%s amax=%d %s" % (row.id, with_amax, row.tags[0]))
    devs = []
    for i, C in enumerate((row.C, row.C + 2)):
        case = make_case("%s %d" % (row.id, i), (row.B,), C, row.N, "offset" if i else "plain")
        case = dict(case, rm=f32(case["xs"][0].mean((0, 2)) + case["rm"]))          # stored statistics near the data's
        d = DevBn(case["xs"][0], case["w"], case["b"], i == 0, rm=case["rm"], rv=case["rv"])
        if not with_amax:
            d.amax_y = None
        devs.append((case, d))
    assert _call(lib, "ct_bn_eval_group_fwd", [d.fwd_item(_lib) for _, d in devs], row.B, row.N) == row.tags[0]
    torch.cuda.synchronize()
    for case, d in devs:
        _, o, bound, _ = _eval_ref(case, d.relu)
        R.add("y", _np(d.y), np.maximum(o, 0.0) if d.relu else o, bound)
        assert int(d.nbt) == NBT0 and torch.equal(d.rm, _dev(case["rm"])) and torch.equal(d.rv, _dev(case["rv"]))
        assert not with_amax or torch.equal(d.amax_y, d.y.abs().amax(dim=(0, 2)))
    R.done()


EVAL_BWD = F.rows("bn_eval_bwd")


@pytest.mark.parametrize("row", EVAL_BWD, ids=[r.id for r in EVAL_BWD])
def test_bn_eval_bwd_row(row):
    _lib, lib = _lib_()
    case = make_case(row.id, (row.B,), row.C, row.N, "plain")
    d = DevBn(case["xs"][0], case["w"], case["b"], 1, gy=case["gys"][0], rm=case["rm"], rv=case["rv"])
    d.amax_y = None
    _call(lib, "ct_bn_eval_group_fwd", [d.fwd_item(_lib)], row.B, row.N)
    p = lambda t: t.data_ptr()      # noqa: E731
    item = _lib.BnEvalBwdItem(x=p(d.x), weight=p(d.w), bias=p(d.b), running_mean=p(d.rm), running_var=p(d.rv), gy=p(d.gy), gx=p(d.gx),
                              g_weight=p(d.gw), g_bias=p(d.gb), amax_out=p(d.amax_gx), C=row.C, eps=EPS, relu=1)
    assert _call(lib, "ct_bn_eval_group_bwd", [item], row.B, row.N) == row.tags[0]
    torch.cuda.synchronize()
    xh, _, _, rs = _eval_ref(case, 1)
    g = case["gys"][0].astype(f64) * (_np(d.y) > 0)
    M = row.B * row.N
    R = Ratios("%s %s" % (row.id, row.tags[0]))
    gx = g * _c(case["w"].astype(f64) * rs)
    R.add("gx", _np(d.gx), gx, np.abs(gx) * 2.0 ** -21)
    R.add("g_bias", _np(d.gb), g.sum((0, 2)), (M + 8) * U * np.abs(g).sum((0, 2)))
    R.add("g_weight", _np(d.gw), (g * xh).sum((0, 2)), (M + 8) * U * np.abs(g * xh).sum((0, 2)))
    R.done()
    assert torch.equal(d.amax_gx, d.gx.abs().amax(dim=(0, 2)))


# ---------------------------------------------------------------------------------------------------------------------
# AdaIN: the channel is one (b, c) row, gamma + 1 the weight, beta the bias
# ---------------------------------------------------------------------------------------------------------------------
class DevAdain:
    def __init__(self, row, case, gamma, relu, layout="dense", res=None):
        self.shape = B, C, N = row.B, row.C, row.N
        io = "slice" if layout == "slice" else "dense"
        self.relu = int(relu)
        self.x_store, self.x, self.xbs = _place(case["xs"][0].reshape(B, C, N), self.shape, layout)
        self.y_store, self.y, self.ybs = _place(None, self.shape, io)
        self.gy_store, self.gy, self.gybs = _place(case["gys"][0].reshape(B, C, N), self.shape, io)
        self.gx_store, self.gx, self.gxbs = _place(None, self.shape, io)
        # res: None, or the residual's layout ("dense" / "slice")
        self.res_store, self.res, self.rbs = _place(case["ress"][0].reshape(B, C, N), self.shape, res) if res else (None, None, 0)
        self.gamma_beta = _dev(np.stack([gamma.reshape(B, C), case["b"].reshape(B, C)], axis=1))
        self.mean, self.rstd = _nan(B * C), _nan(B * C)
        self.amax_y, self.amax_gx, self.ggb = _nan(B, C), _nan(B, C), _nan(B, 2, C)

    def run(self, backward=True):
        _lib, lib = _lib_()
        B, C, N = self.shape
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        fwd = _lib.AdainFwdItem(x=p(self.x), x_batch_stride=self.xbs, gamma_beta=p(self.gamma_beta), residual=p(self.res),
                                residual_batch_stride=self.rbs, y=p(self.y), y_batch_stride=self.ybs, mean=p(self.mean), rstd=p(self.rstd),
                                amax_out=p(self.amax_y), amax_batch_stride=0, C=C, eps=EPS, relu=self.relu, gamma_beta_batch_stride=0)
        tags = [_call(lib, "ct_adain_group_fwd", [fwd], B, N)]
        if backward:
            bwd = _lib.AdainBwdItem(x=p(self.x), x_batch_stride=self.xbs, gamma_beta=p(self.gamma_beta), mean=p(self.mean),
                                    rstd=p(self.rstd), gy=p(self.gy), gy_batch_stride=self.gybs, gx=p(self.gx), gx_batch_stride=self.gxbs,
                                    g_gamma_beta=p(self.ggb), amax_out=p(self.amax_gx), amax_batch_stride=0, C=C, relu=self.relu,
                                    gamma_beta_batch_stride=0)
            tags.append(_call(lib, "ct_adain_group_bwd", [bwd], B, N))
        torch.cuda.synchronize()
        return tuple(tags)

    def outputs(self, backward=True):
        names = ["y", "mean", "rstd", "amax_y"] + (["gx", "ggb", "amax_gx"] if backward else [])
        return {k: getattr(self, k) for k in names}

    def out(self, backward=True):
        B, C, N = self.shape
        o = dict(y=[_np(self.y).reshape(1, B * C, N)], save_mean=[_np(self.mean)], save_rstd=[_np(self.rstd)])
        if backward:
            ggb = _np(self.ggb)
            o.update(gx=[_np(self.gx).reshape(1, B * C, N)], gw=ggb[:, 0].ravel(), gb=ggb[:, 1].ravel())
        return o

    def check_exact_outputs(self, backward=True):
        assert torch.equal(self.amax_y, self.y.abs().amax(dim=2)), "amax_out of the forward"
        if backward:
            assert torch.equal(self.amax_gx, self.gx.abs().amax(dim=2)), "amax_out of the backward"


def adain_mask(row, case, gamma):
    d = DevAdain(row, case, gamma, 1)
    d.run(backward=False)
    return _np(d.y).reshape(1, row.B * row.C, row.N) > 0


ADAIN = F.rows("adain")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("row", ADAIN, ids=[r.id for r in ADAIN])
def test_adain_row(row, dist, relu):
    case, gamma, w64 = adain_case(row, dist)
    backward = row.N > 1            # one point a row: xhat = 0 and d/dx is 0 * rsqrt(eps), ill-conditioned — forward only

    def launch():
        d = DevAdain(row, case, gamma, relu, layout=row.variant)
        return d, d.run(backward)

    d, tags = launch()
    assert tags == row.tags[:len(tags)]
    f = forward_ref(case["xs"], w64, case["b"], relu, [row.tags[0] != "adain_fwd_strided"], threads=F.ADAIN_THREADS)
    out = d.out(backward)
    bw = backward_ref(f, case["gys"], [out["y"][0] > 0] if relu else None) if backward else None
    R = Ratios("%s %s relu=%d %s" % (row.id, dist, relu, "+".join(tags)))
    compare(R, f, bw, out)
    R.done()
    d.check_exact_outputs(backward)
    again, _ = launch()
    _same_bits(d.outputs(backward), again.outputs(backward), "second launch")


@pytest.mark.parametrize("residual", ["dense", "slice"])
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("id", F.ADAIN_SLICE_ROWS)
def test_adain_channel_slices(id, dist, residual):
    """as test_bn_channel_slices: the residual dense, or a channel slice with residual_batch_stride (C + 8) N"""
    row = F.by_id(id)
    case, gamma, w64 = adain_case(row, dist)
    d = DevAdain(row, case, gamma, 1, layout="slice", res=residual)
    assert d.rbs == ((row.C + 8) * row.N if residual == "slice" else 0)
    assert d.run() == row.tags
    f = forward_ref(case["xs"], w64, case["b"], 1, [row.tags[0] != "adain_fwd_strided"], ress=case["ress"], threads=F.ADAIN_THREADS)
    bw = backward_ref(f, case["gys"], [adain_mask(row, case, gamma)])
    R = Ratios("slices %s %s residual=%s" % (row.id, dist, residual))
    compare(R, f, bw, d.out())
    R.done()
    d.check_exact_outputs()
    assert _outside_is_nan(d.y_store, row.C) and _outside_is_nan(d.gx_store, row.C)


@pytest.mark.parametrize("id", F.ADAIN_MASK_ROWS)
def test_adain_mask_is_the_forward_s(id):
    """g_beta[b, c] = sum_n gy [y > 0] exactly on gy from {+-1, +-2} (in place of a 2e-3 tolerance on random cotangents)"""
    row = F.by_id(id)
    case, gamma, _ = adain_case(row, "plain", True)
    d = DevAdain(row, case, gamma, 1)
    assert d.run() == row.tags
    passed = _np(d.y) > 0
    assert 0.2 < 1.0 - passed.mean() < 0.8, "badly chosen case: %.3f masked" % (1.0 - passed.mean())
    want = (case["gys"][0].reshape(passed.shape).astype(np.int64) * passed).sum(2)
    assert np.array_equal(_np(d.ggb)[:, 1].astype(f64), want.astype(f64))
