"""tests/lattice_ref.py (the hand-written float64 reference that the GPU lattice cases compare with) against float64 autograd
through oracle.ref_cpu.rigid_transform + tanh: the reference of the reference, on the CPU."""
import pytest
import torch

from oracle import ref_cpu as R
from tests import lattice_ref as L


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("cots", ["keys", "lattice", "both"])
@pytest.mark.parametrize("use_scales,use_kscale", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("dim", [2, 3])
def test_reference_equals_float64_autograd(dim, use_scales, use_kscale, cots):
    g = torch.Generator().manual_seed(100 * dim + 10 * use_scales + use_kscale)
    B, H, N = 2, 5, 37
    xyz = torch.rand(B, 3, N, generator=g, dtype=torch.float64) * 2 - 1
    res = torch.randn(B, H * 3, N, generator=g, dtype=torch.float64) * 0.3
    log_R = torch.randn(H, 3, generator=g, dtype=torch.float64)
    log_R[1] *= 1e-3                                           # below the clamp
    log_R[2] *= 3                                              # a large angle
    shift = torch.randn(H, 3, generator=g, dtype=torch.float64) * 0.1
    scales = (1 + 0.2 * torch.randn(H, dim, generator=g, dtype=torch.float64)) if use_scales else None
    kscale = torch.tensor(0.7, dtype=torch.float64) if use_kscale else None
    cot_k = torch.randn(B, H * dim, N, generator=g, dtype=torch.float64) if cots != "lattice" else None
    cot_l = torch.randn(B, H * dim, N, generator=g, dtype=torch.float64) if cots != "keys" else None

    lx, lr, lv, ls = (t.clone().requires_grad_(True) for t in (xyz, res, log_R, shift))
    sc = scales.clone().requires_grad_(True) if use_scales else None
    ks = kscale.clone().requires_grad_(True) if use_kscale else None
    p = lx[:, None] + (lr if ks is None else ks * lr).reshape(B, H, 3, N)
    keys = R.rigid_transform(p, lv, ls, sc, dim).reshape(B, H * dim, N)
    lat = torch.tanh(keys)
    loss = 0.0
    if cot_k is not None:
        loss = loss + (keys * cot_k).sum()
    if cot_l is not None:
        loss = loss + (lat * cot_l).sum()
    loss.backward()

    for form in ("log_R", "R"):
        kw = dict(log_R=log_R, eps=1e-4) if form == "log_R" else dict(R=R.so3_exp(log_R))
        ref = L.lattice_ref(xyz, res, shift, dim, scales=scales, kscale=kscale, g_keys=cot_k, g_lattice=cot_l, **kw)
        assert _rel(ref.keys, keys.detach()) <= 1e-12 and _rel(ref.lattice, lat.detach()) <= 1e-12
        assert _rel(ref.mean, keys.detach().mean()) <= 1e-12 and _rel(ref.var, keys.detach().var()) <= 1e-12
        assert _rel(ref.mean_abs, keys.detach().abs().mean()) <= 1e-12 and _rel(ref.mean_sq, (keys.detach() ** 2).mean()) <= 1e-12
        assert _rel(ref.g_xyz, lx.grad) <= 1e-12 and _rel(ref.g_res, lr.grad) <= 1e-12 and _rel(ref.g_shift, ls.grad) <= 1e-12
        if use_scales:
            assert _rel(ref.g_scales, sc.grad) <= 1e-12
        else:
            assert ref.g_scales is None and ref.abs_g_scales is None
        if use_kscale:
            assert _rel(ref.g_kscale, ks.grad) <= 1e-12
        else:
            assert ref.g_kscale is None and ref.abs_g_kscale is None
        if form == "log_R":
            assert _rel(ref.g_log_R, lv.grad) <= 1e-12
        else:
            assert ref.g_log_R is None
            assert _rel(L.so3_grad(log_R, ref.g_R, 1e-4), lv.grad) <= 1e-12      # g_R itself, through the map's autograd
        if dim == 2:
            assert float(ref.g_R[:, :, 2].abs().max()) == 0.0
        # the magnitudes bound what they are the magnitudes of
        assert bool((ref.keys.abs() <= ref.keys_mag * (1 + 1e-12)).all())
        for name in ("g_xyz", "g_shift", "g_R") + (("g_scales",) if use_scales else ()) + (("g_kscale",) if use_kscale else ()):
            val, mag = getattr(ref, name), getattr(ref, "abs_" + name)
            assert val.shape == mag.shape and bool((val.abs() <= mag * (1 + 1e-12)).all()), name


def test_sums_of_absolute_terms_by_hand():
    """One point, one head, R = I, scales 2: every magnitude can be read off."""
    xyz = torch.tensor([[[1.0], [-2.0], [0.5]]])
    res = torch.tensor([[[0.5], [0.25], [-1.0]]])
    shift = torch.tensor([[0.25, 0.0, -0.5]])
    ref = L.lattice_ref(xyz, res, shift, 3, R=torch.eye(3)[None], scales=torch.full((1, 3), 2.0), kscale=torch.tensor(0.5),
                        g_keys=torch.tensor([[[1.0], [-3.0], [2.0]]]))
    p = torch.tensor([1.5, -1.875, -0.5], dtype=torch.float64)
    assert torch.equal(ref.keys.reshape(3), 2 * p)
    assert torch.equal(ref.keys_mag.reshape(3), 2 * torch.tensor([1.5, 2.125, 1.5], dtype=torch.float64))
    gp = torch.tensor([2.0, -6.0, 4.0], dtype=torch.float64)
    assert torch.equal(ref.g_xyz.reshape(3), gp) and torch.equal(ref.abs_g_xyz.reshape(3), gp.abs())
    assert torch.equal(ref.g_res.reshape(3), 0.5 * gp) and torch.equal(ref.g_shift.reshape(3), gp)
    assert torch.equal(ref.g_R[0], p[:, None] * gp[None, :]) and torch.equal(ref.abs_g_R[0], (p[:, None] * gp[None, :]).abs())
    assert torch.equal(ref.g_scales.reshape(3), torch.tensor([1.0, -3.0, 2.0], dtype=torch.float64) * p)
    assert float(ref.g_kscale) == 2 * 0.5 - 6 * 0.25 - 4 * 1.0 and float(ref.abs_g_kscale) == 1.0 + 1.5 + 4.0
    assert float(ref.mean) == float((2 * p).mean()) and abs(float(ref.var) - float((2 * p).var())) <= 1e-15


def test_forward_plan_of_every_gpu_shape():
    """the notes beside SHAPES of tests/test_lattice_cases_gpu.py, re-derived from lattice_fwd_nbx: (workgroups per row, points
    per workgroup) of the forward, and the workgroups per head whose partials the backward's parameter sums add up"""
    from tests.test_lattice_cases_gpu import SHAPES, fwd_plan
    assert [fwd_plan(*s) for s in SHAPES] == [(1, 256), (1, 256), (1, 256), (2, 256), (20, 256), (3, 512), (2, 512), (1, 256)]
    assert fwd_plan(2, 3, 777) == (4, 256) and fwd_plan(2, 5, 333) == (2, 256) and fwd_plan(8, 16, 4096) == (4, 1024)
    assert [B * ((N + 255) // 256) for B, H, N in SHAPES] == [1, 1, 2, 4, 20, 48, 12, 3]


def test_exact_cases_leave_every_sum_inside_24_bits():
    """the precondition of the exact-arithmetic GPU cases holds on the reference alone, and the 70 so3 rows are what they say"""
    from tests.test_lattice_cases_gpu import EXACT, _exact_inputs, _exact_reference
    for case in EXACT:
        _exact_reference(_exact_inputs(*case, seed=sum(case)))
    v = L.so3_rows_70(torch.Generator().manual_seed(43))
    s = (v.double() ** 2).sum(1)
    assert v.shape == (70, 3) and bool(((s - L.EPS).abs() > 1e-9).all()) and int((s < L.EPS).sum()) == 11
    assert float(s.max()) > 3.1416 ** 2 and int((s == 0).sum()) == 1


def test_clamp_sits_at_the_float32_eps():
    """|v|^2 between float32(1e-4) and the double 1e-4 takes the live branch: the value the kernels compare with."""
    assert L.EPS < 1e-4
    s = 0.5 * (L.EPS + 1e-4)
    v = torch.tensor([[s ** 0.5, 0.0, 0.0]], dtype=torch.float64)
    g_R = torch.arange(9.0, dtype=torch.float64).reshape(1, 3, 3)
    assert not torch.equal(L.so3_grad(v, g_R), L.so3_grad(v, g_R, 1e-4))
