"""GPU parity of the fused training-mode BatchNorm1d + ReLU (ct_bn_group_fwd / _bwd) against torch's own
F.batch_norm + relu evaluated in float64 on the CPU: output, running statistics, and all three gradients."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _ref(x, w, b, rm, rv, eps, momentum, relu, gy):
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    b = b.double().requires_grad_(True)
    rm, rv = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(x, rm, rv, w, b, True, momentum, eps)
    if relu:
        y = torch.relu(y)
    y.backward(gy.double())
    return y.detach(), rm, rv, x.grad, w.grad, b.grad


@pytest.mark.parametrize("B,C,N,relu", [(8, 64, 4096, True), (8, 48, 2048, True), (2, 5, 256, False), (3, 7, 1000, True),
                                        (1, 3, 4, True), (8, 16, 4096, False), (16, 24, 4096, True), (3, 9, 1001, True),
                                        (2, 4, 40000, False)])
def test_bn_relu_matches_torch(B, C, N, relu):
    from cloud_transformers_amd import ops
    torch.manual_seed(B * 100 + C)
    bn = torch.nn.BatchNorm1d(C, eps=1e-5, momentum=0.1)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2)
    x = torch.randn(B, C, N) * 3 + 0.7
    gy = torch.randn(B, C, N)
    y_ref, rm_ref, rv_ref, gx_ref, gw_ref, gb_ref = _ref(x, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                                                        bn.eps, bn.momentum, relu, gy)
    bn = bn.cuda().train()
    xc = x.cuda().requires_grad_(True)
    assert ops.bn_relu_eligible(bn, xc)
    y = ops.bn_relu(xc, bn, relu=relu)
    y.backward(gy.cuda())
    tol = dict(rtol=1e-4, atol=1e-4)
    assert torch.allclose(y.detach().cpu().double(), y_ref, **tol)
    assert torch.allclose(bn.running_mean.cpu().double(), rm_ref, rtol=1e-5, atol=1e-6)
    assert torch.allclose(bn.running_var.cpu().double(), rv_ref, rtol=1e-5, atol=1e-6)
    assert int(bn.num_batches_tracked) == 1
    scale = max(1.0, float(gx_ref.abs().max()))
    assert float((xc.grad.cpu().double() - gx_ref).abs().max()) <= 1e-4 * scale
    assert torch.allclose(bn.weight.grad.cpu().double(), gw_ref, rtol=1e-4, atol=1e-3 * max(1.0, float(gw_ref.abs().max()) * 1e-1))
    assert torch.allclose(bn.bias.grad.cpu().double(), gb_ref, rtol=1e-4, atol=1e-3 * max(1.0, float(gb_ref.abs().max()) * 1e-1))


def test_run_after_dispatch():
    """The blocks' `after` stacks: BatchNorm1d + ReLU in training mode runs fused (register-resident, long-channel and
    scalar-row kernels); eval mode and SyncBatchNorm go through the modules' own forward — with the same result."""
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers.multihead_ct import run_after
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.BatchNorm1d(32), torch.nn.ReLU(inplace=True)).cuda()
    ref = torch.nn.Sequential(torch.nn.BatchNorm1d(32), torch.nn.ReLU()).cuda()
    ref.load_state_dict(seq.state_dict())
    calls = []
    real = ops.bn_relu
    ops.bn_relu = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        x = torch.randn(4, 32, 512, device="cuda")
        out = run_after(seq, x.clone())
        assert calls == [1]
        assert torch.allclose(out, ref(x), rtol=1e-4, atol=1e-5)
        assert torch.allclose(seq[0].running_var, ref[0].running_var, rtol=1e-5, atol=1e-6)
        del calls[:]
        seq.eval(), ref.eval()
        assert torch.allclose(run_after(seq, x.clone()), ref(x), rtol=1e-5, atol=1e-6) and not calls
        seq.train(), ref.train()
        odd = x[:, :, :511].contiguous()                             # rows that are not float4-addressable: scalar loop kernels
        assert torch.allclose(run_after(seq, odd.clone()), ref(odd), rtol=1e-4, atol=1e-5) and calls == [1]
        del calls[:]
        big = torch.randn(16, 32, 4096, device="cuda")              # B*N > 32768: the channel is re-read per pass
        assert torch.allclose(run_after(seq, big.clone()), ref(big), rtol=1e-4, atol=1e-5) and calls == [1]
        assert torch.allclose(seq[0].running_var, ref[0].running_var, rtol=1e-5, atol=1e-6)
        del calls[:]
        # SyncBatchNorm (what DDP training converts every norm into) takes the fused kernels too: without a process group
        # there is nothing to exchange (tests/test_syncbn_gpu.py covers the two-rank exchange)
        sync = torch.nn.SyncBatchNorm.convert_sync_batchnorm(torch.nn.Sequential(torch.nn.BatchNorm1d(32), torch.nn.ReLU())).cuda()
        assert ops.bn_relu_eligible(sync[0], x)
        assert torch.allclose(run_after(sync, x.clone()), ref(x), rtol=1e-4, atol=1e-5) and calls == [1]
    finally:
        ops.bn_relu = real


def test_abi_argument_checks():
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    assert lib.ct_bn_relu_supported(8, 512, 4096) == 1
    assert lib.ct_bn_relu_supported(16, 512, 4096) == 1          # long channels: loop kernels
    assert lib.ct_bn_relu_supported(8, 512, 4095) == 1           # rows that are not float4-addressable: scalar loops
    assert lib.ct_bn_relu_supported(1, 4, 1) == 0                # one value per channel has no variance
    buf = torch.zeros(1 << 16, device="cuda")
    p = buf.data_ptr()

    def call(B=2, N=64, **fields):
        it = _lib.BnFwdItem(**{**dict(x=p, weight=p, bias=p, y=p, save_mean=p, save_rstd=p, C=8, eps=1e-5, momentum=0.1, relu=1),
                               **fields})
        return lib.ct_bn_group_fwd(ctypes.addressof(it), 1, B, N, None)

    assert call(running_mean=p) == -1                            # one running buffer only
    assert call(x_batch_stride=8 * 64 - 4) == -1                 # batch stride < C*N
    assert call(B=1, N=1) == -1                                  # B*N < 2
    assert call(x=None) == -1
    items = (_lib.BnFwdItem * 9)()
    for e in items:
        e.x = e.weight = e.bias = e.y = e.save_mean = e.save_rstd = p
        e.C, e.eps, e.momentum, e.relu = 8, 1e-5, 0.1, 1
    addr = ctypes.addressof(items)
    assert lib.ct_bn_group_fwd(addr, 0, 2, 64, None) == -1
    assert lib.ct_bn_group_fwd(addr, 9, 2, 64, None) == -1
    assert lib.ct_bn_group_fwd(None, 1, 2, 64, None) == -1
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                         # nothing was launched


def _exchange_phases(_lib, lib, n, runs, B, N, fwd_fields, bwd_fields, Ct):
    """The four exchange phases (world = 1: `gathered` is `local`) over a table of n norms, launched as `runs` = [(first, run)];
    every output goes to a fresh buffer pre-filled with NaN.  Returns the buffers by name."""
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    Cs = [f["C"] for f in fwd_fields]
    o = dict(local=nan(2 * Ct + 1), count=nan(1), sums=nan(2 * Ct), sums_copy=nan(2 * Ct))
    for name in ("y", "gx"):
        o[name] = [nan(B, C, N) for C in Cs]
    for name in ("save_mean", "save_rstd", "amax_y", "amax_gx"):
        o[name] = [nan(C) for C in Cs]
    fwd, bwd = (_lib.BnFwdItem * n)(), (_lib.BnBwdItem * n)()
    for i in range(n):
        for k, v in fwd_fields[i].items():
            setattr(fwd[i], k, v)
        fwd[i].y, fwd[i].save_mean, fwd[i].save_rstd, fwd[i].amax_out = (o[k][i].data_ptr() for k in ("y", "save_mean", "save_rstd", "amax_y"))
        for k, v in bwd_fields[i].items():
            setattr(bwd[i], k, v)
        bwd[i].save_mean, bwd[i].save_rstd, bwd[i].gx, bwd[i].amax_out = (o[k][i].data_ptr() for k in ("save_mean", "save_rstd", "gx", "amax_gx"))
    fa, ba = ctypes.addressof(fwd), ctypes.addressof(bwd)
    for first, run in runs:
        assert lib.ct_bn_group_stats_fwd(fa, n, first, run, B, N, o["local"].data_ptr(), None) == 0
    for first, run in runs:
        assert lib.ct_bn_group_apply_fwd(fa, n, first, run, B, N, o["local"].data_ptr(), 1, o["count"].data_ptr(), None) == 0
    for first, run in runs:
        assert lib.ct_bn_group_reduce_bwd(ba, n, first, run, B, N, o["sums"].data_ptr(), o["sums_copy"].data_ptr(), None) == 0
    for first, run in runs:
        assert lib.ct_bn_group_apply_bwd(ba, n, first, run, B, N, o["sums"].data_ptr(), o["count"].data_ptr(), None) == 0
    torch.cuda.synchronize()
    return o, (fwd, bwd)


# one shape per kernel family of bn_*_launch_table: register-resident, scalar loop (N % 4 != 0), float4 loop (B*N > 32768)
@pytest.mark.parametrize("B,N", [(2, 260), (2, 259), (2, 16388)])
def test_exchange_phases_launch_a_run_of_the_table(B, N):
    """The range arguments of the four exchange phases: three norms launched as one run of three and as three runs of one
    write the same bits everywhere (the buffer layout belongs to the table, not to the launch), the whole-group result is
    torch's batch norm, and bad ranges are refused before anything is launched."""
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    torch.manual_seed(N)
    Cs = (3, 8, 5)
    Ct, n = sum(Cs), len(Cs)
    xs = [torch.randn(B, C, N, device="cuda") * 2 for C in Cs]
    ws = [torch.rand(C, device="cuda") + 0.5 for C in Cs]
    bs = [torch.randn(C, device="cuda") for C in Cs]
    gys = [torch.randn(B, C, N, device="cuda") for C in Cs]
    fwd_fields = [dict(x=x.data_ptr(), weight=w.data_ptr(), bias=b.data_ptr(), C=C, eps=1e-5, momentum=0.1, relu=1)
                  for x, w, b, C in zip(xs, ws, bs, Cs)]
    bwd_fields = [dict(x=x.data_ptr(), weight=w.data_ptr(), bias=b.data_ptr(), gy=gy.data_ptr(), C=C, relu=1)
                  for x, w, b, gy, C in zip(xs, ws, bs, gys, Cs)]
    whole, _ = _exchange_phases(_lib, lib, n, [(0, 3)], B, N, fwd_fields, bwd_fields, Ct)
    single, (fwd, bwd) = _exchange_phases(_lib, lib, n, [(0, 1), (1, 1), (2, 1)], B, N, fwd_fields, bwd_fields, Ct)
    for name in ("local", "count", "sums", "sums_copy"):
        assert not bool(torch.isnan(whole[name]).any()), name
        assert torch.equal(whole[name], single[name]), name
    for name in ("y", "save_mean", "save_rstd", "gx", "amax_y", "amax_gx"):
        for a, b in zip(whole[name], single[name]):
            assert not bool(torch.isnan(a).any()), name
            assert torch.equal(a, b), name
    assert float(whole["count"]) == B * N and torch.equal(whole["sums"], whole["sums_copy"])
    for i, (x, w, b, gy) in enumerate(zip(xs, ws, bs, gys)):
        xr = x.clone().requires_grad_(True)
        want = torch.relu(F.batch_norm(xr, None, None, w, b, True, 0.1, 1e-5))
        want.backward(gy)
        ey, egx = float((whole["y"][i] - want.detach()).abs().max()), float((whole["gx"][i] - xr.grad).abs().max())
        print("B%d N%d norm %d: max |y - torch| %.3e, max |gx - torch| %.3e" % (B, N, i, ey, egx))
        assert ey < 1e-5 and egx < 1e-5
        assert torch.equal(whole["amax_y"][i], whole["y"][i].abs().amax(dim=(0, 2)))
        assert torch.equal(whole["amax_gx"][i], whole["gx"][i].abs().amax(dim=(0, 2)))
    # bad ranges: refused by every phase, nothing launched
    probe = {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v]) for k, v in single.items()}
    fa, ba = ctypes.addressof(fwd), ctypes.addressof(bwd)
    lp, cp, sp, scp = (single[k].data_ptr() for k in ("local", "count", "sums", "sums_copy"))
    for first, run in ((1, 3), (3, 1), (0, 0), (0, 9), (-1, 1)):
        assert lib.ct_bn_group_stats_fwd(fa, n, first, run, B, N, lp, None) == -1
        assert lib.ct_bn_group_apply_fwd(fa, n, first, run, B, N, lp, 1, cp, None) == -1
        assert lib.ct_bn_group_reduce_bwd(ba, n, first, run, B, N, sp, scp, None) == -1
        assert lib.ct_bn_group_apply_bwd(ba, n, first, run, B, N, sp, cp, None) == -1
    torch.cuda.synchronize()
    for k, v in single.items():
        for a, b in zip([v] if torch.is_tensor(v) else v, [probe[k]] if torch.is_tensor(v) else probe[k]):
            assert torch.equal(a, b), k


def test_split_bn_equals_the_two_modules_on_split_views():
    """key_bn / values_bn on the halves of one tensor (layers/multihead_ct.py:89-91): values, running statistics and
    every gradient equal torch's BatchNorm1d modules applied to torch.split views."""
    from cloud_transformers_amd import ops
    torch.manual_seed(3)
    B, Ck, Cv, N = 4, 12, 40, 1024
    mods = [torch.nn.BatchNorm1d(Ck), torch.nn.BatchNorm1d(Cv)]
    with torch.no_grad():
        for m in mods:
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.5, 0.5)
    ref = [torch.nn.BatchNorm1d(Ck), torch.nn.BatchNorm1d(Cv)]
    for r, m in zip(ref, mods):
        r.load_state_dict(m.state_dict())
        r.double()
    x = torch.randn(B, Ck + Cv, N) * 2 + 0.3
    gk, gv = torch.randn(B, Ck, N), torch.randn(B, Cv, N)
    xr = x.double().requires_grad_(True)
    a, b = torch.split(xr, [Ck, Cv], dim=1)
    ya, yb = ref[0](a), ref[1](b)
    (ya * gk.double()).sum().backward(retain_graph=True)
    (yb * gv.double()).sum().backward()
    mods = [m.cuda().train() for m in mods]
    xc = x.cuda().requires_grad_(True)
    assert ops.bn_relu_eligible(mods[0], xc, Ck) and ops.bn_relu_eligible(mods[1], xc, Cv)
    ka, kb = ops.split_bn(xc, mods[0], mods[1])
    ((ka * gk.cuda()).sum() + (kb * gv.cuda()).sum()).backward()
    tol = dict(rtol=1e-4, atol=1e-4)
    assert torch.allclose(ka.detach().cpu().double(), ya.detach(), **tol) and torch.allclose(kb.detach().cpu().double(), yb.detach(), **tol)
    assert torch.allclose(xc.grad.cpu().double(), xr.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(xr.grad.abs().max())))
    for m, r in zip(mods, ref):
        assert torch.allclose(m.running_mean.cpu().double(), r.running_mean, rtol=1e-5, atol=1e-6)
        assert torch.allclose(m.running_var.cpu().double(), r.running_var, rtol=1e-5, atol=1e-6)
        assert int(m.num_batches_tracked) == 1
        assert torch.allclose(m.weight.grad.cpu().double(), r.weight.grad, rtol=1e-4, atol=1e-3)
        assert torch.allclose(m.bias.grad.cpu().double(), r.bias.grad, rtol=1e-4, atol=1e-3)
    # only one output used downstream: the other half's cotangent is None -> zeros
    xc2 = x.cuda().requires_grad_(True)
    ka2, _ = ops.split_bn(xc2, mods[0], mods[1])
    ka2.sum().backward()
    assert float(xc2.grad[:, Ck:].abs().max()) == 0.0


def test_residual_and_strided_cotangent():
    """run_after(after, x, residual): the skip connection is added inside the kernel and receives the output cotangent;
    a cotangent that is a channel slice of a wider tensor (torch.cat's backward) is read where it lies."""
    from cloud_transformers_amd.layers.multihead_ct import run_after
    torch.manual_seed(9)
    B, C, N = 4, 24, 512
    seq = torch.nn.Sequential(torch.nn.BatchNorm1d(C), torch.nn.ReLU(inplace=True)).cuda()
    ref = torch.nn.Sequential(torch.nn.BatchNorm1d(C), torch.nn.ReLU()).cuda()
    with torch.no_grad():
        seq[0].weight.uniform_(0.5, 1.5)
        seq[0].bias.uniform_(-0.5, 0.5)
    ref.load_state_dict(seq.state_dict())
    x = torch.randn(B, C, N, device="cuda")
    res = torch.randn(B, C, N, device="cuda")
    wide = torch.randn(B, C + 8, N, device="cuda")
    outs = []
    for mod, fused in ((seq, True), (ref, False)):
        xi, ri = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
        w = wide.clone().requires_grad_(True)
        y = run_after(mod, xi, ri) if fused else ri + mod(xi)
        z = torch.cat([y, w[:, :8]], dim=1)               # y's cotangent arrives as a slice of z's
        (z * wide).sum().backward()
        outs.append((y.detach(), xi.grad, ri.grad, mod[0].weight.grad.clone(), mod[0].bias.grad.clone(),
                     mod[0].running_mean.clone(), int(mod[0].num_batches_tracked)))
    for a, b in zip(outs[0][:6], outs[1][:6]):
        assert torch.allclose(a, b, rtol=1e-4, atol=2e-4), float((a - b).abs().max())
    assert outs[0][6] == outs[1][6] == 1


def test_join_bn_relu_equals_cat_of_the_modules():
    from cloud_transformers_amd import ops
    torch.manual_seed(4)
    B, N, Cs = 4, 512, (16, 40, 8)
    mods = [torch.nn.BatchNorm1d(c).cuda() for c in Cs]
    refs = [torch.nn.BatchNorm1d(c).cuda() for c in Cs]
    for m, r in zip(mods, refs):
        with torch.no_grad():
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.5, 0.5)
        r.load_state_dict(m.state_dict())
    xs = [torch.randn(B, c, N, device="cuda") for c in Cs]
    cot = torch.randn(B, sum(Cs), N, device="cuda")
    xa = [x.clone().requires_grad_(True) for x in xs]
    xb = [x.clone().requires_grad_(True) for x in xs]
    ya = ops.join_bn_relu(xa, mods)
    yb = torch.cat([torch.relu(r(x)) for r, x in zip(refs, xb)], dim=1)
    (ya * cot).sum().backward()
    (yb * cot).sum().backward()
    assert torch.allclose(ya, yb, rtol=1e-4, atol=1e-5)
    for a, b, m, r in zip(xa, xb, mods, refs):
        assert torch.allclose(a.grad, b.grad, rtol=1e-4, atol=2e-4)
        assert torch.allclose(m.weight.grad, r.weight.grad, rtol=1e-4, atol=1e-3)
        assert torch.allclose(m.bias.grad, r.bias.grad, rtol=1e-4, atol=1e-3)
        assert torch.allclose(m.running_var, r.running_var, rtol=1e-5, atol=1e-6)
        assert int(m.num_batches_tracked) == int(r.num_batches_tracked) == 1


def test_union_keys_values_equals_per_head_modules():
    """One stacked GEMM + norms for all heads (ops.union_keys_values) against conv_i -> split -> key_bn_i / values_bn_i."""
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers.pointwise import PointwiseConv1d
    torch.manual_seed(8)
    B, Cin, N = 4, 32, 512
    spec = [(12, 16), (6, 40)]                      # (3H, H*C) per head
    def build():
        torch.manual_seed(8)
        convs = [PointwiseConv1d(Cin, ck + cv, kernel_size=1, bias=False).cuda() for ck, cv in spec]
        kbs = [torch.nn.BatchNorm1d(ck).cuda() for ck, _ in spec]
        vbs = [torch.nn.BatchNorm1d(cv).cuda() for _, cv in spec]
        with torch.no_grad():
            for bn in kbs + vbs:
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.uniform_(-0.5, 0.5)
        return convs, kbs, vbs
    x0 = torch.randn(B, Cin, N, device="cuda")
    cots = [(torch.randn(B, ck, N, device="cuda"), torch.randn(B, cv, N, device="cuda")) for ck, cv in spec]
    res = []
    for fused in (True, False):
        convs, kbs, vbs = build()
        x = x0.clone().requires_grad_(True)
        if fused:
            assert ops.union_keys_values_eligible(x, convs, kbs, vbs)
            outs = ops.union_keys_values(x, convs, kbs, vbs)
        else:
            outs = []
            for conv, kb, vb, (ck, cv) in zip(convs, kbs, vbs, spec):
                a, b = torch.split(conv(x), [ck, cv], dim=1)
                outs.append((kb(a.contiguous()), vb(b.contiguous())))
        sum((k * gk).sum() + (v * gv).sum() for (k, v), (gk, gv) in zip(outs, cots)).backward()
        res.append(([t.detach() for kv in outs for t in kv], x.grad, [c.weight.grad for c in convs],
                    [bn.weight.grad for bn in kbs + vbs], [bn.bias.grad for bn in kbs + vbs],
                    [bn.running_var.clone() for bn in kbs + vbs], [int(bn.num_batches_tracked) for bn in kbs + vbs]))
    f, r = res
    for a, b in zip(f[0], r[0]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4)
    assert torch.allclose(f[1], r[1], rtol=1e-4, atol=1e-3)
    for group in (2, 3, 4):
        for a, b in zip(f[group], r[group]):
            assert torch.allclose(a, b, rtol=1e-3, atol=2e-3 * max(1.0, float(b.abs().max()))), float((a - b).abs().max())
    for a, b in zip(f[5], r[5]):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    assert f[6] == r[6] == [1, 1, 1, 1]
