"""GPU parity of the eval-mode BatchNorm kernels (ct_bn_eval_group_fwd, tables of one and of several norms) and of their entry points in
ops (bn_eval, split_bn_eval, join_bn_relu_eval, union_keys_values_eval) against torch's eval batch norm in float64 on
the CPU, and the dispatch of layers.multihead_ct.run_after.

The elementwise bound: the kernel rounds five times in fp32 (x - m, * rstd, * w, + b, + residual) and its rstd is within
2 ulp, so |err| <= 9 * 2^-24 * (|x - m| * rstd * |w| + |b| + |res|); the tests allow 2^-20 of that sum (1.8x margin).
The x * scale + shift form of the affine misses it where |running_mean| >> |x - running_mean| (the cancellation case)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _norm(C, seed, mean_offset=0.0):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(C, eps=1e-5)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)                  # as tests/test_bnorm_gpu.py: U(0.5, 1.5), U(-0.5, 0.5)
        bn.bias.copy_(torch.rand(C, generator=g) - 0.5)
        bn.running_mean.copy_(torch.rand(C, generator=g) * 2 - 1 + mean_offset)
        bn.running_var.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
    return bn.eval()


def _ref64(bn, x, relu, res=None):
    """(float64 reference, float64 elementwise bound) of relu?(bn(x)) [+ res] for CPU tensors."""
    x = x.double()
    m, v = bn.running_mean.double(), bn.running_var.double()
    w, b = bn.weight.detach().double(), bn.bias.detach().double()
    y = F.batch_norm(x, m, v, w, b, False, 0.0, bn.eps)
    if relu:
        y = torch.relu(y)
    rstd = 1.0 / torch.sqrt(v + bn.eps)
    bound = (x - m[None, :, None]).abs() * (rstd * w.abs())[None, :, None] + b.abs()[None, :, None]
    if res is not None:
        y = y + res.double()
        bound = bound + res.double().abs()
    return y, bound * 2.0 ** -20


def _check(y, ref, bound, what=""):
    err = (y.detach().cpu().double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s max |err| %.3e, worst err / bound %.3f" % (what, float(err.max()), worst))
    assert bool((err <= bound).all()), (what, float(err.max()), worst)


CASES = [(1, 3, 1, True, False, 0.0), (2, 5, 256, False, False, 0.0), (3, 7, 1001, True, True, 0.0),
         (4, 32, 512, True, True, 0.0), (2, 4, 40000, True, False, 0.0), (8, 48, 2048, True, True, 0.0),
         (4, 32, 512, False, False, 50.0)]                                   # the last: |running_mean| >> |x - running_mean|


@pytest.mark.parametrize("B,C,N,relu,with_res,offset", CASES)
def test_bn_eval_matches_float64(B, C, N, relu, with_res, offset):
    from cloud_transformers_amd import ops
    torch.manual_seed(B * 100 + C)
    bn = _norm(C, B * 100 + C, offset)
    if offset:
        x = bn.running_mean[None, :, None] + torch.randn(B, C, N)
    else:
        x = torch.randn(B, C, N) * 3 + 0.7
    res = torch.randn(B, C, N) if with_res else None
    ref, bound = _ref64(bn, x, relu, res)
    bn = bn.cuda()
    before = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
    with torch.no_grad():
        xc, rc = x.cuda(), None if res is None else res.cuda()
        assert ops.bn_eval_eligible(bn, xc, residual=rc)
        y = ops.bn_eval(xc, bn, relu=relu, residual=rc)
    _check(y, ref, bound, "bn_eval %s" % ((B, C, N, relu, with_res, offset),))
    assert not y.requires_grad
    for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,C,N", [(4, 32, 512), (3, 7, 1001)])
@pytest.mark.parametrize("with_res", [False, True])
def test_amax_tag_is_the_maximum_of_the_stored_values(B, C, N, with_res):
    from cloud_transformers_amd import ops
    torch.manual_seed(C)
    bn = _norm(C, C).cuda()
    x = torch.randn(B, C, N, device="cuda") * 3 + 0.7
    res = torch.randn(B, C, N, device="cuda") if with_res else None
    with torch.no_grad():
        y = ops.bn_eval(x, bn, relu=True, residual=res)
    tag = ops.amax_of(y)
    assert tag is y._ct_amax[0] and tag.numel() == C
    assert torch.equal(tag.view(-1), y.abs().amax(dim=(0, 2)))


@pytest.mark.parametrize("B,Ca,Cb,N", [(4, 12, 40, 1024), (3, 3, 5, 1001)])
def test_split_bn_eval_equals_the_two_modules_on_split_views(B, Ca, Cb, N):
    from cloud_transformers_amd import ops
    torch.manual_seed(3)
    mods = [_norm(Ca, 31), _norm(Cb, 32)]
    x = torch.randn(B, Ca + Cb, N) * 2 + 0.3
    refs = [_ref64(m, part.contiguous(), False) for m, part in zip(mods, torch.split(x, [Ca, Cb], dim=1))]
    mods = [m.cuda() for m in mods]
    xc = x.cuda()
    with torch.no_grad():
        assert ops.bn_eval_eligible(mods[0], xc, Ca) and ops.bn_eval_eligible(mods[1], xc, Cb)
        outs = ops.split_bn_eval(xc, mods[0], mods[1])
    for y, (ref, bound), name in zip(outs, refs, ("first half", "second half")):
        assert y.is_contiguous()
        _check(y, ref, bound, "split_bn_eval %s N=%d" % (name, N))


@pytest.mark.parametrize("N", [1024, 1022])
def test_join_bn_relu_eval_equals_cat_of_the_modules(N):
    from cloud_transformers_amd import ops
    torch.manual_seed(4)
    B, Cs = 4, (16, 24)
    mods = [_norm(c, 40 + c) for c in Cs]
    xs = [torch.randn(B, c, N) * 2 - 0.2 for c in Cs]
    parts = [_ref64(m, x, True) for m, x in zip(mods, xs)]
    ref, bound = torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1)
    mods = [m.cuda() for m in mods]
    with torch.no_grad():
        y = ops.join_bn_relu_eval([x.cuda() for x in xs], mods)
    assert y.shape == (B, sum(Cs), N) and y.is_contiguous()
    _check(y, ref, bound, "join_bn_relu_eval N=%d" % N)
    tag = ops.amax_of(y)
    assert tag is y._ct_amax[0] and tag.numel() == sum(Cs)                   # one tag over all 40 channels
    assert torch.equal(tag.view(-1), y.abs().amax(dim=(0, 2)))


@pytest.mark.parametrize("Cin,spec", [(32, [(12, 16), (6, 40)]), (128, [(48, 128), (48, 128)])])
def test_union_keys_values_eval_equals_per_head_modules(Cin, spec):
    """One stacked GEMM + one group launch over the 2n slices against conv_i -> split -> key_bn_i / values_bn_i in eval; at
    Cin 128 the stacked product is the split-f16 GEMM, fed by the maxima tag an eval norm left on its input."""
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers.pointwise import PointwiseConv1d
    torch.manual_seed(8)
    B, N = 4, 512
    convs = [PointwiseConv1d(Cin, ck + cv, kernel_size=1, bias=False).cuda().eval() for ck, cv in spec]
    kbs = [_norm(ck, 80 + i).cuda() for i, (ck, _) in enumerate(spec)]
    vbs = [_norm(cv, 90 + i).cuda() for i, (_, cv) in enumerate(spec)]
    with torch.no_grad():
        x = ops.bn_eval(torch.randn(B, Cin, N, device="cuda"), _norm(Cin, 7).cuda(), relu=True)      # carries its maxima
        assert getattr(x, "_ct_amax", None) is not None
        assert ops.union_keys_values_eval_eligible(x, convs, kbs, vbs)
        outs = ops.union_keys_values_eval(x, convs, kbs, vbs)
        for (k, v), conv, kb, vb, (ck, cv) in zip(outs, convs, kbs, vbs, spec):
            a, b = torch.split(conv(x), [ck, cv], dim=1)
            assert torch.allclose(k, kb(a.contiguous()), rtol=1e-4, atol=1e-4)
            assert torch.allclose(v, vb(b.contiguous()), rtol=1e-4, atol=1e-4)
    x.requires_grad_(True)                                                    # something to record: not this path
    assert not ops.union_keys_values_eval_eligible(x, convs, kbs, vbs)


def test_run_after_dispatch_in_eval():
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers.multihead_ct import run_after
    torch.manual_seed(0)
    seq = torch.nn.Sequential(_norm(32, 5), torch.nn.ReLU(inplace=True)).cuda().eval()
    ref = torch.nn.Sequential(torch.nn.BatchNorm1d(32), torch.nn.ReLU()).cuda().eval()
    ref.load_state_dict(seq.state_dict())
    ev, tr = [], []
    real_eval, real_train, switch = ops.bn_eval, ops.bn_relu, ops.BN_EVAL
    ops.bn_eval = lambda *a, **k: (ev.append(1), real_eval(*a, **k))[1]
    ops.bn_relu = lambda *a, **k: (tr.append(1), real_train(*a, **k))[1]
    try:
        x = torch.randn(4, 32, 512, device="cuda")
        with torch.no_grad():
            want = ref(x)
            out = run_after(seq, x.clone())
            assert ev == [1] and not tr
            assert torch.allclose(out, want, rtol=1e-5, atol=1e-6)
            del ev[:]
            res = torch.randn_like(x)                                         # the skip connection rides the same pass
            out = run_after(seq, x.clone(), res)
            assert ev == [1] and not tr
            assert torch.allclose(out, res + want, rtol=1e-5, atol=1e-6)
            del ev[:]
        out = run_after(seq, x.clone())                                       # grad enabled, parameters require grad: the module
        assert not ev and not tr and out.requires_grad
        assert torch.allclose(out, want, rtol=1e-5, atol=1e-6)
        with torch.no_grad():
            ops.BN_EVAL = False
            out = run_after(seq, x.clone())
            assert not ev and not tr
            assert torch.allclose(out, want, rtol=1e-5, atol=1e-6)
            ops.BN_EVAL = True
            sync = torch.nn.SyncBatchNorm.convert_sync_batchnorm(
                torch.nn.Sequential(torch.nn.BatchNorm1d(32), torch.nn.ReLU())).cuda().eval()
            sync.load_state_dict(seq.state_dict())
            assert type(sync[0]) is torch.nn.SyncBatchNorm and ops.bn_eval_eligible(sync[0], x)
            out = run_after(sync, x.clone())
            assert ev == [1] and not tr
            assert torch.allclose(out, want, rtol=1e-5, atol=1e-6)
    finally:
        ops.bn_eval, ops.bn_relu, ops.BN_EVAL = real_eval, real_train, switch


def test_abi_argument_checks():
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    assert lib.ct_bn_eval_supported(8, 512, 4096) == 1
    assert lib.ct_bn_eval_supported(8, 512, 4095) == 1
    assert lib.ct_bn_eval_supported(1, 4, 1) == 1                # one value per channel is legal here
    assert lib.ct_bn_eval_supported(0, 4, 16) == 0 and lib.ct_bn_eval_supported(1, 4, 0) == 0
    assert lib.ct_bn_eval_supported(1 << 16, 4, 1 << 15) == 0   # B*N = 2^31
    buf = torch.zeros(1 << 16, device="cuda")
    p = buf.data_ptr()
    B, C, N = 2, 8, 64

    def call(x=p, xbs=0, w=p, b=p, rm=p, rv=p, res=None, rbs=0, y=p, ybs=0, B=B, N=N):
        it = _lib.BnFwdItem(x=x, x_batch_stride=xbs, weight=w, bias=b, running_mean=rm, running_var=rv, residual=res,
                            residual_batch_stride=rbs, y=y, y_batch_stride=ybs, C=C, eps=1e-5, relu=1)
        return lib.ct_bn_eval_group_fwd(ctypes.addressof(it), 1, B, N, None)

    assert call(x=None) == -1 and call(w=None) == -1 and call(b=None) == -1 and call(y=None) == -1
    assert call(rv=None) == -1 and call(rm=None) == -1           # one running buffer only
    assert call(rm=None, rv=None) == -1                          # eval has nothing to normalise with
    assert call(xbs=C * N - 4) == -1 and call(ybs=C * N - 4) == -1 and call(res=p, rbs=C * N - 4) == -1
    assert call(B=0) == -1 and call(N=0) == -1                   # B*N < 1
    items = (_lib.BnFwdItem * 9)()
    for e in items:
        e.x = e.weight = e.bias = e.running_mean = e.running_var = e.y = p
        e.C, e.eps, e.relu = C, 1e-5, 1
    addr = ctypes.addressof(items)
    assert lib.ct_bn_eval_group_fwd(addr, 0, B, N, None) == -1
    assert lib.ct_bn_eval_group_fwd(addr, 9, B, N, None) == -1
    assert lib.ct_bn_eval_group_fwd(None, 2, B, N, None) == -1
    assert lib.ct_bn_eval_group_fwd(addr, 2, 0, N, None) == -1
    items[1].running_var = None
    assert lib.ct_bn_eval_group_fwd(addr, 2, B, N, None) == -1
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                         # nothing was launched


def _expected_split(B, N, channels):
    """The runs a channel without maxima is cut into (include/cloudct.h, ct_bn_eval_group_fwd): towards 1024 workgroups in the
    launch, never below 2048 quads (floats on the scalar path) a run."""
    per = B * (N // 4) if N % 4 == 0 else B * N
    return max(1, min(-(-1024 // channels), per // 2048)), per


# (B, Ca, Cb, N, runs per channel, is the last run short): float4 rows cut evenly and with a short last run, scalar rows
# (N % 4 != 0) the same, and the shape the cut exists for (the key norms' 48 channels at B6 N8192)
CUT_CASES = [(6, 48, 64, 8192, 6, False), (3, 3, 5, 5468, 2, True), (6, 48, 64, 8190, 10, False), (3, 3, 5, 2731, 4, True)]


@pytest.mark.parametrize("B,Ca,Cb,N,runs,short", CUT_CASES)
def test_channels_cut_over_several_workgroups(B, Ca, Cb, N, runs, short):
    """Norms without maxima on long channels: every channel is cut into several runs, one workgroup each — the same
    elementwise bound on every element shows that the runs tile the channel (none skipped, none written twice wrongly)."""
    from cloud_transformers_amd import ops
    split, per = _expected_split(B, N, Ca + Cb)
    assert split == runs and split > 1 and (per % split != 0) == short
    torch.manual_seed(N)
    mods = [_norm(Ca, 51), _norm(Cb, 52)]
    x = torch.randn(B, Ca + Cb, N) * 2 + 0.3
    refs = [_ref64(m, part.contiguous(), False) for m, part in zip(mods, torch.split(x, [Ca, Cb], dim=1))]
    mods = [m.cuda() for m in mods]
    xc = x.cuda()
    with torch.no_grad():
        outs = ops.split_bn_eval(xc, mods[0], mods[1])
        single = torch.full((B, Cb, N), float("nan"), device="cuda")          # one norm, one launch: a table of one, no maxima
        ops._bn_eval_group([ops._bn_eval_item(mods[1], xc.data_ptr() + Ca * N * 4, (Ca + Cb) * N, single.data_ptr(), 0, False)], B, N)
    for y, (ref, bound), name in zip(outs, refs, ("first", "second")):
        _check(y, ref, bound, "cut %s B%d N%d runs %d" % (name, B, N, split))
    assert torch.equal(single, outs[1])              # another cut (fewer channels in the launch), the same bits
    _check(single, refs[1][0], refs[1][1], "cut, single launch B%d N%d" % (B, N))


@pytest.mark.parametrize("grouped", [True, False])
def test_more_norms_than_a_group_holds_run_one_launch_each(grouped):
    """Nine norms into one concatenation: more than BN_GROUP_MAX, so one ct_bn_eval_group_fwd launch of n = 1 per norm; with
    ops.BN_GROUP_LAUNCH off (CLOUDCT_BN_GROUP=0) two norms take the same route."""
    from cloud_transformers_amd import _lib, ops
    torch.manual_seed(6)
    B, N = 2, 260
    Cs = (3, 4, 5, 6, 7, 8, 9, 10, 12) if grouped else (16, 24)
    mods = [_norm(c, 60 + c) for c in Cs]
    xs = [torch.randn(B, c, N) for c in Cs]
    parts = [_ref64(m, x, True) for m, x in zip(mods, xs)]
    ref, bound = torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1)
    mods = [m.cuda() for m in mods]
    lib = _lib.load()
    group, calls = lib.ct_bn_eval_group_fwd, []
    lib.ct_bn_eval_group_fwd = lambda items, n, *a: (calls.append(n), group(items, n, *a))[1]
    switch = ops.BN_GROUP_LAUNCH
    ops.BN_GROUP_LAUNCH = grouped
    try:
        with torch.no_grad():
            y = ops.join_bn_relu_eval([x.cuda() for x in xs], mods)
    finally:
        lib.ct_bn_eval_group_fwd, ops.BN_GROUP_LAUNCH = group, switch
    assert calls == [1] * len(Cs), calls
    _check(y, ref, bound, "join of %d norms, one launch each" % len(Cs))
    assert torch.equal(ops.amax_of(y).view(-1), y.abs().amax(dim=(0, 2)))
