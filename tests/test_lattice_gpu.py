"""GPU parity of the fused lattice kernels (rigid transform of xyz + residual, tanh) against
the CPU oracle's rigid_transform (pinned on the reference's Vol/PlaneTransformer outputs) and
its autograd, for every parameter cotangent."""
import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fused_so3", [False, True], ids=["so3-apart", "so3-inside"])
@pytest.mark.parametrize("dim,use_scales,use_kscale", [(2, False, False), (3, True, False), (2, True, True), (3, False, True)])
def test_lattice_fwd_bwd(dim, use_scales, use_kscale, fused_so3):
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers.utils import so3_exponential_map
    g = torch.Generator().manual_seed(10 * dim + use_scales + 2 * use_kscale)
    B, H, N = 2, 5, 333
    xyz = torch.rand(B, 3, N, generator=g) * 2 - 1
    res = torch.randn(B, H * 3, N, generator=g) * 0.3
    log_R = torch.randn(H, 3, generator=g)
    shift = torch.randn(H, 3, generator=g) * 0.1
    scales = (1 + 0.2 * torch.randn(H, dim, generator=g)) if use_scales else None
    kscale = torch.tensor(0.7) if use_kscale else None
    cot_l = torch.randn(B, H * dim, N, generator=g)
    cot_k = torch.randn(B, H * dim, N, generator=g) * 0.1

    leaves = [t.clone().requires_grad_(True) for t in (xyz, res, log_R, shift)]
    sc = scales.clone().requires_grad_(True) if use_scales else None
    ks = kscale.clone().requires_grad_(True) if use_kscale else None
    p = leaves[0][:, None] + (leaves[1] if ks is None else ks * leaves[1]).reshape(B, H, 3, N)
    keys_ref = R.rigid_transform(p, leaves[2], torch.zeros(H, 3) + leaves[3], sc, dim).reshape(B, H * dim, N)
    lat_ref = torch.tanh(keys_ref)
    ((lat_ref * cot_l).sum() + (keys_ref * cot_k).sum()).backward()

    dl = [t.clone().cuda().requires_grad_(True) for t in (xyz, res, log_R, shift)]
    dsc = scales.clone().cuda().requires_grad_(True) if use_scales else None
    dks = kscale.clone().cuda().requires_grad_(True) if use_kscale else None
    if fused_so3:        # ops.LatticeSo3Fn: the so3 map inside the launches, key statistics by the launch's last workgroup
        keys, lat, stats = ops.lattice_so3(dl[0], dl[1], dl[2], dl[3], dsc, dks, dim, with_stats=True)
        assert abs(float(stats[0]) - float(keys_ref.mean())) <= 1e-5 * max(1.0, abs(float(keys_ref.mean())))
        assert abs(float(stats[1]) - float(keys_ref.var())) <= 1e-4 * float(keys_ref.var())
    else:
        keys, lat = ops.lattice(dl[0], dl[1], so3_exponential_map(dl[2]), dl[3], dsc, dks, dim)
    ((lat * cot_l.cuda()).sum() + (keys * cot_k.cuda()).sum()).backward()

    def close(a, b, name, tol=2e-5):
        err = float((a.detach().cpu() - b.detach()).abs().max())
        assert err <= tol * max(1.0, float(b.abs().max())), (name, err)

    close(keys, keys_ref, "keys")
    close(lat, lat_ref, "lattice")
    for a, b, name in zip(dl, leaves, ("xyz", "residual", "log_R", "shift")):
        close(a.grad, b.grad, "g_" + name, 1e-4)
    if use_scales:
        close(dsc.grad, sc.grad, "g_scales", 1e-4)
    if use_kscale:
        close(dks.grad, ks.grad, "g_kscale", 1e-4)


def test_so3_exp_map_matches_oracle():
    """ct_so3_exp_fwd / _bwd against the oracle's Rodrigues map (pinned on the transforms golden) and its float64
    autograd, including rotations below the clamp (|v|^2 < eps: a and b stop depending on v) and a zero vector."""
    from cloud_transformers_amd.layers.utils import so3_exponential_map
    from tests.lattice_ref import so3_rows_70
    g = torch.Generator().manual_seed(5)
    v59 = torch.cat([torch.randn(40, 3, generator=g), torch.randn(8, 3, generator=g) * 3, torch.randn(8, 3, generator=g) * 1e-3,
                     torch.zeros(1, 3), torch.tensor([[0.02, 0.0, 0.0], [0.0, 0.005, 0.0]])])
    # then 70 rows: the kernels launch 64-thread workgroups, so the second one runs (rows either side of sqrt(eps) among them)
    for v in (v59, so3_rows_70(g)):
        cot = torch.randn(v.shape[0], 3, 3, generator=g)
        vr = v.double().requires_grad_(True)
        Rr = R.so3_exp(vr)
        (Rr * cot.double()).sum().backward()
        vc = v.cuda().requires_grad_(True)
        Rc = so3_exponential_map(vc)
        (Rc * cot.cuda()).sum().backward()
        assert Rc.shape == (v.shape[0], 3, 3)
        assert float((Rc.detach().cpu().double() - Rr.detach()).abs().max()) <= 2e-6
        assert float((vc.grad.cpu().double() - vr.grad).abs().max()) <= 2e-5 * max(1.0, float(vr.grad.abs().max()))
        # rotations: R R^T = I
        eye = torch.eye(3, device="cuda").expand_as(Rc)
        assert float((Rc.detach() @ Rc.detach().transpose(1, 2) - eye).abs().max()) <= 1e-5


def test_fused_lattice_statistics_over_repeated_launches():
    """The ticket word of ct_lattice_so3_fwd resets itself: many launches on one stream, fresh inputs each, every launch's key
    statistics equal the keys' own (a stale ticket or a partial read too early would show)."""
    from cloud_transformers_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    B, H, N, dim = 8, 16, 4096, 3
    for it in range(12):
        xyz = torch.rand(B, 3, N, device="cuda", generator=g) * 2 - 1
        res = torch.randn(B, H * 3, N, device="cuda", generator=g) * (0.1 + 0.05 * it)
        log_R = torch.randn(H, 3, device="cuda", generator=g)
        shift = torch.randn(H, 3, device="cuda", generator=g) * 0.1
        keys, lat, stats = ops.lattice_so3(xyz, res, log_R, shift, None, None, dim, with_stats=True)
        kd = keys.double()
        assert abs(float(stats[0]) - float(kd.mean())) <= 1e-5
        assert abs(float(stats[1]) - float(kd.var())) <= 1e-4 * float(kd.var()), it


CT_EINVAL, CT_EWORKSPACE = -1, -3       # include/cloudct.h


def test_abi_refusals_come_before_any_launch():
    """Every refused call returns its status with the outputs untouched: nothing was launched."""
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.ops import _ptr, _stream
    lib = _lib.load()
    g = torch.Generator().manual_seed(13)
    B, H, N = 2, 5, 300
    xyz, res = torch.rand(B, 3, N, generator=g).cuda(), torch.randn(B, H * 3, N, generator=g).cuda()
    log_R, shift = torch.randn(H, 3, generator=g).cuda(), torch.randn(H, 3, generator=g).cuda()
    Rm = torch.linalg.qr(torch.randn(H, 3, 3, generator=g))[0].cuda()
    scales, ks = torch.ones(H, 3).cuda(), torch.ones(1).cuda()
    lat, cot = torch.rand(B, H * 3, N, generator=g).cuda(), torch.randn(B, H * 3, N, generator=g).cuda()
    poison = lambda *s: torch.full(s, 7.0, device="cuda")
    outs = {n: poison(*s) for n, s in (("keys", (B, H * 3, N)), ("lattice", (B, H * 3, N)), ("stats", (2,)), ("R", (H, 3, 3)),
                                      ("g_xyz", (B, 3, N)), ("g_res", (B, H * 3, N)), ("g_R", (H, 3, 3)), ("g_shift", (H, 3)),
                                      ("g_scales", (H, 3)), ("g_kscale", (1,)), ("g_log_R", (H, 3)))}
    o = {n: _ptr(t) for n, t in outs.items()}
    fwd_bytes, bwd_bytes = lib.ct_lattice_fwd_workspace_bytes(B, H, N), lib.ct_lattice_bwd_workspace_bytes(B, H, N)
    assert fwd_bytes > 0 and bwd_bytes > 0
    ws = torch.zeros(max(fwd_bytes, bwd_bytes), device="cuda", dtype=torch.uint8)
    ticket = torch.zeros(1, device="cuda", dtype=torch.int32)
    s = _stream()

    def fwd(dim=3, stats=None, ws_ptr=None, ws_bytes=0):
        return lib.ct_lattice_fwd(_ptr(xyz), _ptr(res), _ptr(Rm), _ptr(shift), None, None, o["keys"], o["lattice"], stats, ws_ptr, ws_bytes,
                                  B, H, N, dim, s)

    def so3_fwd(dim=3, eps=1e-4, stats=None, ws_ptr=None, ws_bytes=0, tk=None):
        return lib.ct_lattice_so3_fwd(_ptr(xyz), _ptr(res), _ptr(log_R), eps, _ptr(shift), None, None, o["R"], o["keys"], o["lattice"], stats,
                                      ws_ptr, ws_bytes, tk, B, H, N, dim, s)

    def bwd(dim=3, g_lattice=_ptr(cot), g_keys=_ptr(cot), sc=None, g_sc=None, k=None, g_k=None, ws_ptr=_ptr(ws), ws_bytes=bwd_bytes):
        return lib.ct_lattice_bwd(_ptr(xyz), _ptr(res), _ptr(Rm), _ptr(shift), sc, k, _ptr(lat), g_lattice, g_keys, o["g_xyz"], o["g_res"],
                                  o["g_R"], o["g_shift"], g_sc, g_k, ws_ptr, ws_bytes, B, H, N, dim, s)

    def so3_bwd(dim=3, eps=1e-4):
        return lib.ct_lattice_so3_bwd(_ptr(xyz), _ptr(res), _ptr(log_R), eps, _ptr(Rm), _ptr(shift), None, None, _ptr(lat), _ptr(cot),
                                      _ptr(cot), o["g_xyz"], o["g_res"], o["g_log_R"], o["g_R"], o["g_shift"], None, None, _ptr(ws),
                                      bwd_bytes, B, H, N, dim, s)

    # both cotangents NULL
    assert bwd(g_lattice=None, g_keys=None) == CT_EINVAL
    # scales and g_scales come together
    assert bwd(sc=_ptr(scales)) == CT_EINVAL
    assert bwd(g_sc=o["g_scales"]) == CT_EINVAL
    assert bwd(k=_ptr(ks)) == CT_EINVAL and bwd(g_k=o["g_kscale"]) == CT_EINVAL      # and so do kscale and g_kscale
    # workspaces one byte short
    assert fwd(stats=o["stats"], ws_ptr=_ptr(ws), ws_bytes=fwd_bytes - 1) == CT_EWORKSPACE
    assert bwd(ws_bytes=bwd_bytes - 1) == CT_EWORKSPACE
    assert so3_fwd(stats=o["stats"], ws_ptr=_ptr(ws), ws_bytes=fwd_bytes - 1, tk=_ptr(ticket)) == CT_EWORKSPACE
    # key statistics without a ticket
    assert so3_fwd(stats=o["stats"], ws_ptr=_ptr(ws), ws_bytes=fwd_bytes, tk=None) == CT_EWORKSPACE
    # dim is 2 or 3
    for dim in (1, 4):
        assert fwd(dim=dim) == CT_EINVAL and so3_fwd(dim=dim) == CT_EINVAL and bwd(dim=dim) == CT_EINVAL and so3_bwd(dim=dim) == CT_EINVAL
    # the so3 clamp is positive
    assert so3_fwd(eps=0.0) == CT_EINVAL and so3_bwd(eps=0.0) == CT_EINVAL
    assert lib.ct_so3_exp_fwd(_ptr(log_R), o["R"], H, 0.0, s) == CT_EINVAL
    assert lib.ct_so3_exp_bwd(_ptr(log_R), _ptr(Rm), o["g_log_R"], H, 0.0, s) == CT_EINVAL
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert float((t - 7.0).abs().max()) == 0.0, name
    assert int(ticket[0]) == 0
    # and the same calls are taken once the argument is right
    assert fwd(stats=o["stats"], ws_ptr=_ptr(ws), ws_bytes=fwd_bytes) == 0 and bwd() == 0
    assert so3_fwd(stats=o["stats"], ws_ptr=_ptr(ws), ws_bytes=fwd_bytes, tk=_ptr(ticket)) == 0 and so3_bwd() == 0
    torch.cuda.synchronize()
    assert all(float((outs[n] - 7.0).abs().max()) > 0.0 for n in ("keys", "lattice", "stats", "R", "g_xyz", "g_res", "g_R", "g_shift", "g_log_R"))
    assert int(ticket[0]) == 0
