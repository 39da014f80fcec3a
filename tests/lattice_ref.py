"""Float64 reference of the lattice op (csrc/ct_lattice.hip), written out by hand: values, every gradient, and for each summed
output the sum of the absolute values of its terms (what a float32 sum of those terms can be held to).

    p[b,h,c,n]    = xyz[b,c,n] + kscale * res[b,h*3+c,n] + shift[h,c]
    rot[b,h,j,n]  = sum_c p[b,h,c,n] * R[h,c,j]                 j < dim
    keys          = rot * scales[h,j]
    lattice       = tanh(keys)

R is given (the split path: the float32 matrix the kernel reads) or comes from log_R through oracle.ref_cpu.so3_exp in float64,
clamped at the float32 value of eps that the library sees (ops passes eps as a C float)."""
import types

import numpy as np
import torch

from oracle import ref_cpu

EPS = float(np.float32(1e-4))      # so3 clamp as the kernels see it


def so3_rows_70(g):
    """70 float32 so3 parameter rows (a second 64-thread workgroup of the stand-alone kernels): 40 ordinary, 8 with angles
    beyond pi, 8 far below the clamp, a zero row, |v| = 0.0099 and 0.0101 either side of sqrt(eps), the rest ordinary"""
    u = torch.tensor([1.0, 2.0, 2.0]) / 3
    return torch.cat([torch.randn(40, 3, generator=g), torch.randn(8, 3, generator=g) * 3, torch.randn(8, 3, generator=g) * 1e-3,
                      torch.zeros(1, 3), 0.0099 * u[None], 0.0101 * u[None], -0.0099 * u[None, [2, 0, 1]], 0.0101 * u[None, [1, 2, 0]],
                      torch.randn(9, 3, generator=g)])


def so3(log_R, eps=EPS):
    """float64 so3 exponential map [H,3] -> [H,3,3]"""
    return ref_cpu.so3_exp(log_R.double(), eps) if log_R.shape[0] else torch.zeros(0, 3, 3, dtype=torch.float64)


def so3_grad(log_R, g_R, eps=EPS):
    """float64 gradient of <g_R, so3(log_R)> with respect to log_R, by autograd"""
    v = log_R.detach().double().requires_grad_(True)
    (ref_cpu.so3_exp(v, eps) * g_R.double()).sum().backward()
    return v.grad


def lattice_ref(xyz, res, shift, dim, R=None, log_R=None, scales=None, kscale=None, g_keys=None, g_lattice=None, eps=EPS):
    """All results in float64, as attributes: keys, lattice, keys_mag (the bound's M: sum_c (|xyz| + |kscale res| + |shift|) |R|
    |scales|), mean, var (unbiased), mean_abs, mean_sq of the keys, R; with a cotangent also g_xyz, g_res, g_R, g_shift,
    g_scales, g_kscale, g_log_R (None where their input is None) and abs_<name>: the sum of |terms| of each summed one."""
    assert (R is None) != (log_R is None) and dim in (2, 3)
    d = lambda t: None if t is None else t.detach().cpu().double()
    xyz, res, shift, scales, g_keys, g_lattice = d(xyz), d(res), d(shift), d(scales), d(g_keys), d(g_lattice)
    ks = 1.0 if kscale is None else float(d(kscale).reshape(-1)[0])
    B, _, N = xyz.shape
    H = shift.shape[0]
    Rm = d(R) if R is not None else so3(d(log_R), eps)
    sc = scales if scales is not None else torch.ones(H, dim, dtype=torch.float64)
    r = res.reshape(B, H, 3, N)
    p = xyz[:, None] + ks * r + shift[None, :, :, None]                                    # [B,H,3,N]
    Rj = Rm[:, :, :dim]                                                                    # [H,3,dim]
    rot = (p[:, :, :, None, :] * Rj[None, :, :, :, None]).sum(2)                           # [B,H,dim,N]
    keys = rot * sc[None, :, :, None]
    mag = xyz.abs()[:, None] + (ks * r).abs() + shift.abs()[None, :, :, None]
    keys_mag = (mag[:, :, :, None, :] * Rj.abs()[None, :, :, :, None]).sum(2) * sc.abs()[None, :, :, None]
    out = types.SimpleNamespace(R=Rm, keys=keys.reshape(B, H * dim, N), lattice=torch.tanh(keys).reshape(B, H * dim, N),
                                keys_mag=keys_mag.reshape(B, H * dim, N))
    n = keys.numel()
    out.mean = keys.mean()
    out.var = ((keys - out.mean) ** 2).sum() / (n - 1) if n > 1 else torch.zeros((), dtype=torch.float64)
    out.mean_abs, out.mean_sq = keys.abs().mean(), (keys * keys).mean()
    if g_keys is None and g_lattice is None:
        return out

    gk = torch.zeros_like(keys)
    if g_lattice is not None:
        gk = gk + g_lattice.reshape(B, H, dim, N) * (1.0 - torch.tanh(keys) ** 2)
    if g_keys is not None:
        gk = gk + g_keys.reshape(B, H, dim, N)
    gq = gk * sc[None, :, :, None]                                                         # cotangent of rot
    gp = (Rj[None, :, :, :, None] * gq[:, :, None, :, :]).sum(3)                           # [B,H,3,N]
    out.g_res = (ks * gp).reshape(B, H * 3, N)
    out.g_xyz, out.abs_g_xyz = gp.sum(1), gp.abs().sum(1)
    out.g_shift, out.abs_g_shift = gp.sum((0, 3)), gp.abs().sum((0, 3))
    t = p[:, :, :, None, :] * gq[:, :, None, :, :]                                         # [B,H,3,dim,N]
    out.g_R = torch.zeros(H, 3, 3, dtype=torch.float64)
    out.abs_g_R = torch.zeros(H, 3, 3, dtype=torch.float64)
    out.g_R[:, :, :dim], out.abs_g_R[:, :, :dim] = t.sum((0, 4)), t.abs().sum((0, 4))
    out.g_scales = out.abs_g_scales = out.g_kscale = out.abs_g_kscale = out.g_log_R = None
    if scales is not None:
        t = gk * rot
        out.g_scales, out.abs_g_scales = t.sum((0, 3)), t.abs().sum((0, 3))
    if kscale is not None:
        t = gp * r
        out.g_kscale, out.abs_g_kscale = t.sum(), t.abs().sum()
    if log_R is not None:
        out.g_log_R = so3_grad(d(log_R), out.g_R, eps)
    return out
