"""torch.autograd.Function wrappers over the C ABI (include/cloudct.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream;
every computation happens inside libcloudct.so.  Tensors that are not on a HIP
device raise — there is no CPU path in the product.
"""
import ctypes
import math
import os

import torch

from . import _lib
from . import determinism as _det
from . import precision as _prec


def sizes_of(tensor_size, dim):
    """int -> [W]*dim; tuple/list of len dim kept (layers/cloud_transform.py:41-46)."""
    if isinstance(tensor_size, int):
        return [tensor_size] * dim
    sizes = [int(w) for w in tensor_size]
    assert len(sizes) == dim
    return sizes


def _dev(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "cloud_transformers_amd ops need tensors on a HIP device (MI355X); "
                "got a %s tensor and there is no CPU fallback" % t.device.type)


def _stream(device=None):
    """The raw hipStream_t the launch goes to: torch's current stream of `device` (default: the current device).  Through the two
    C entry points directly: torch.cuda.current_stream().cuda_stream builds a Stream object and parses a device argument on
    every call, 9 us of host time against 0.4 — at 250-400 launches per eager model step that was 2-3 ms of a host-bound step
    (tools/dev/host_profile.py)."""
    idx = device.index if device is not None and device.index is not None else _cuda_get_device()
    return _cuda_raw_stream(idx)


# (private entry points of torch._C, present since torch 1.x; a build without them takes the public, slower route)
_cuda_get_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device
_cuda_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


class _NoSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(device):
    """Context that makes `device` current for the launch: a no-op object when it already is (the usual case;
    half the host cost of torch.cuda.device(), 0.6 vs 1.4 us per op)."""
    if device.index is None or device.index == _cuda_get_device():
        return _NO_SWITCH
    return torch.cuda.device(device)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _f32c(t):
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    return t.contiguous()


def _pad_args(pad, B, N):
    """pts_padding (B,N) float or int32 (datasets/s3dis_closer.py:330) -> (tensor, dtype code)."""
    if pad is None:
        return None, _lib.PAD_NONE
    assert pad.shape == (B, N), "pts_padding must be [batch, num_points]"
    if pad.dtype == torch.float32:
        return pad.contiguous(), _lib.PAD_F32
    if pad.dtype == torch.int32:
        return pad.contiguous(), _lib.PAD_I32
    return pad.to(torch.float32).contiguous(), _lib.PAD_F32


# ---------------------------------------------------------------------------
# Pointwise-convolution GEMMs (ct_pw_gemm: fp32 in / out, split-f16 on the matrix pipes)
# ---------------------------------------------------------------------------
PW_FWD, PW_DGRAD, PW_WGRAD, PW_DGRAD_T = 0, 1, 2, 3
# "split16": this library's kernels; "lib": rocBLAS fp32 through torch.bmm (the round-2 path, kept as the A/B switch and
# for shapes the kernel does not take: a dimension that is not a multiple of 4)
PW_GEMM = os.environ.get("CLOUDCT_PW_GEMM", "split16")


PW_BWD_STREAMS = os.environ.get("CLOUDCT_PW_BWD_STREAMS", "1") != "0"
_pw_side = {}
# streams that are themselves forks inside a capture (the heads' side streams of layers.multihead_ct._run_heads): work on them
# does not fork again — a second level of forks shared by two concurrent chains crashed hipStreamEndCapture
forked_streams = set()


def _pw_side_stream(device):
    s = _pw_side.get(device.index)
    if s is None:
        s = _pw_side[device.index] = torch.cuda.Stream(device=device)
    return s


def pw_eligible(Co, Ci, N, mode=None):
    """Whether ct_pw_gemm takes the product; with `mode`, whether it also beats the library GEMM there: an output-row
    extent under one 128-row tile leaves half the MFMA rows idle (tools/pw_gemm_bench.py: 0.7-0.95x at 64 rows)."""
    if not (PW_GEMM == "split16" and Co % 4 == 0 and Ci % 4 == 0 and N % 4 == 0 and N >= 4):
        return False
    if mode == PW_FWD:
        return Co >= 128
    if mode == PW_DGRAD:
        return Ci >= 128
    if mode == PW_WGRAD:
        return Co >= 128 and Ci >= 128
    return True


_amax_len = None


def amax(t):
    """Partial maxima of |t| for a contiguous float32 tensor: f32[ct_amax_len()], one per block of the kernel (max |t| is
    their maximum; ct_pw_gemm folds them when it starts) — the per-tensor scale of ct_pw_gemm."""
    global _amax_len
    lib = _lib.load()
    if _amax_len is None:
        _amax_len = lib.ct_amax_len()
    out = torch.empty(_amax_len, device=t.device, dtype=torch.float32)
    with _on(t.device):
        _lib.check(lib.ct_amax_f32(_ptr(t), t.numel(), _ptr(out), _stream()), "ct_amax_f32")
    return out


PW_AMAX_MAX = 32768     # partial maxima ct_pw_gemm folds per operand


def _amax_slots(C, device):
    """Maxima buffer for a producer kernel (ct_bn_group_* / ct_bn_eval_group_fwd: one slot per channel; ct_adain_group_*: one per (cloud, channel)),
    or None when the consumer could not use it (library GEMMs selected, or more slots than ct_pw_gemm folds)."""
    if PW_GEMM != "split16" or C > PW_AMAX_MAX:
        return None
    return torch.empty(C, device=device, dtype=torch.float32)


def tag_amax(t, slots):
    """Remember on tensor `t` [B, C, N] the maxima its producer left in `slots` (valid until `t` is modified in place).  The
    producers write one maximum per channel (or per (cloud, channel)): kept as a 2-D [n / C, C] view — the shape is what tells
    ct_pw_gemm_rs that these are PER-ROW maxima (a 1-D tensor holds partials of one maximum, ops.amax)."""
    if slots is not None:
        C = t.shape[1] if t.dim() == 3 else 0
        if C and slots.dim() == 1 and slots.numel() % C == 0:
            slots = slots.view(-1, C)
        t._ct_amax = (slots, t._version)
    return t


def amax_rows(t):
    """Per-channel maxima of |t| for a contiguous float32 [B, C, N] tensor, as a [1, C] tensor (ct_amax_rows_f32): what the
    weight gradient wants of an operand no producer left maxima for."""
    B, C, N = t.shape
    if C > PW_AMAX_MAX or N % 4 != 0:
        return amax(t)
    out = torch.empty(1, C, device=t.device, dtype=torch.float32)
    with _on(t.device):
        _lib.check(_lib.load().ct_amax_rows_f32(_ptr(t), B, C, N, _ptr(out), _stream()), "ct_amax_rows_f32")
    return out


def _rows_of(am, want):
    """`want` when `am` holds per-row maxima of an operand with `want` rows (2-D [.., want]), else 0 (partials of one maximum)."""
    return want if (am is not None and am.dim() == 2 and am.shape[1] == want) else 0


def amax_of(t, rows=False):
    """The operand maxima of `t` for ct_pw_gemm: what its producer left behind if `t` is unchanged since (an in-place op
    bumps `_version`), else a pass over it — ct_amax_rows_f32 (per channel) where the consumer can use per-row scales
    (`rows`: the weight gradient), ct_amax_f32 otherwise."""
    tag = getattr(t, "_ct_amax", None)
    if tag is not None and tag[1] == t._version and tag[0].device == t.device:
        return tag[0]
    return amax_rows(t) if (rows and t.dim() == 3) else amax(t)


def pw_gemm(mode, a, b, amax_a, amax_b, B, Co, Ci, N, addend=None, precision=None):
    """ct_pw_gemm on contiguous float32 tensors: PW_FWD (a = W [Co,Ci], b = x [B,Ci,N]) -> y [B,Co,N]; PW_DGRAD (a = W,
    b = g_y [B,Co,N]) -> g_x [B,Ci,N]; PW_WGRAD (a = g_y, b = x) -> g_W [Co,Ci].  amax_* from amax().  addend (contiguous,
    shaped as the output; not for PW_WGRAD): added in the kernel's epilogue (ct_pw_gemm_rs_add).  precision: None = the
    effective mode of precision.py, pushed into the library's process-wide switch ahead of the workspace query and the launch,
    which read it; or the library constant a forward remembered (a backward that runs in its forward's mode), which goes into
    the library's per-thread override around them instead."""
    lib = _lib.load()
    if precision is None:
        _prec.push(lib)
        return _pw_gemm(lib, mode, a, b, amax_a, amax_b, B, Co, Ci, N, addend)
    with _prec.forced(precision, lib):
        return _pw_gemm(lib, mode, a, b, amax_a, amax_b, B, Co, Ci, N, addend)


def _pw_gemm(lib, mode, a, b, amax_a, amax_b, B, Co, Ci, N, addend):
    dev = b.device
    if mode == PW_FWD:
        out = torch.empty(B, Co, N, device=dev, dtype=torch.float32)
    elif mode in (PW_DGRAD, PW_DGRAD_T):
        out = torch.empty(B, Ci, N, device=dev, dtype=torch.float32)
    else:
        out = torch.empty(Co, Ci, device=dev, dtype=torch.float32)
    nbytes = lib.ct_pw_gemm_workspace_bytes(mode, B, Co, Ci, N)
    ws = torch.empty(nbytes // 4, device=dev, dtype=torch.float32) if nbytes else None
    # per-row scales wherever the maxima are per row of the operand's k-contiguous arrangement (2-D: tag_amax, prep_weight)
    rows_a = _rows_of(amax_a, Co if mode in (PW_FWD, PW_WGRAD) else Ci) if mode != PW_DGRAD else 0
    rows_b = _rows_of(amax_b, Ci) if mode == PW_WGRAD else 0
    if addend is not None:
        assert mode != PW_WGRAD and addend.shape == out.shape and addend.is_contiguous() and addend.dtype == torch.float32
    with _on(dev):
        _lib.check(lib.ct_pw_gemm_rs_add(mode, _ptr(a), _ptr(b), _ptr(out), _ptr(addend), _ptr(amax_a),
                                         0 if amax_a is None else amax_a.numel(), rows_a, _ptr(amax_b),
                                         0 if amax_b is None else amax_b.numel(), rows_b, _ptr(ws), nbytes, B, Co, Ci, N, _stream()),
                   "ct_pw_gemm_rs_add")
    return out


def prep_weight(W, transpose):
    """((row maxima of |W|, column maxima), W^T or None) in ONE launch (ct_pw_prep_weight_rs): what the three products of a layer
    need of its weight — per-row scales for W in the forward ([tiles, Co]) and for W^T in the data gradient ([tiles, Ci]); falls
    back to (amax(), None) and no transpose for weights with more maxima than ct_pw_gemm_rs folds."""
    lib = _lib.load()
    Co, Ci = W.shape
    tc, tr = (Ci + 31) // 32, (Co + 31) // 32
    if tc * Co > PW_AMAX_MAX or tr * Ci > PW_AMAX_MAX:
        return (amax(W), None), None
    rowmax = torch.empty(tc, Co, device=W.device, dtype=torch.float32)
    colmax = torch.empty(tr, Ci, device=W.device, dtype=torch.float32)
    Wt = torch.empty(Ci, Co, device=W.device, dtype=torch.float32) if transpose else None
    with _on(W.device):
        _lib.check(lib.ct_pw_prep_weight_rs(_ptr(W), _ptr(Wt), _ptr(rowmax), _ptr(colmax), Co, Ci, _stream()), "ct_pw_prep_weight_rs")
    return (rowmax, colmax), Wt


def pw_forward(W, x, need_dgrad=False):
    """y[b] = W x[b] for W [Co,Ci], x [B,Ci,N] (both contiguous float32 on the device); returns (y, amax_W, amax_x, W^T) — the
    maxima (amax_W: the pair (row maxima, column maxima) of prep_weight) and, with need_dgrad, the transposed weight are reused
    by the gradients — or (y, None, None, None) from the library GEMM."""
    Co, Ci = W.shape
    B, _, N = x.shape
    if not pw_eligible(Co, Ci, N, PW_FWD):
        return torch.bmm(W.unsqueeze(0).expand(B, -1, -1), x), None, None, None
    am_w, Wt = prep_weight(W, need_dgrad and pw_eligible(Co, Ci, N, PW_DGRAD))
    am_x = amax_of(x)
    return pw_gemm(PW_FWD, W, x, am_w[0], am_x, B, Co, Ci, N), am_w, am_x, Wt


def pw_backward(W, x, g_y, am_w, am_x, need_x=True, need_w=True, am_g=None, Wt=None, add_gx=None, precision=None):
    """(g_x, g_W) of pw_forward for the cotangent g_y [B,Co,N] (contiguous); am_g: g_y's maxima where the caller has them; Wt:
    the transposed weight pw_forward made (else the data gradient writes its own through its workspace); add_gx: another
    cotangent of x (a skip connection's), added to g_x inside the data gradient's epilogue where the kernel runs it; precision:
    the library constant of the mode the forward ran in (precision.code() read there), so that a layer's three products share
    one precision wherever and whenever autograd runs this; None = the mode in effect now."""
    Co, Ci = W.shape
    B, _, N = x.shape
    mine_x = need_x and pw_eligible(Co, Ci, N, PW_DGRAD)
    mine_w = need_w and pw_eligible(Co, Ci, N, PW_WGRAD)
    if am_g is None and (mine_x or mine_w):
        am_g = amax_of(g_y, rows=mine_w)
    if torch.is_tensor(am_w):            # (a caller that kept one maxima tensor of W: partials of its maximum)
        am_w = (am_w, None)
    g_x = g_w = None

    if add_gx is not None:
        add_gx = _f32c(add_gx)

    def dgrad():
        if mine_x and Wt is not None and am_w is not None:
            # W^T's rows are W's columns: their maxima give the data gradient its per-row scales
            return pw_gemm(PW_DGRAD_T, Wt, g_y, am_w[1] if am_w[1] is not None else am_w[0], am_g, B, Co, Ci, N, addend=add_gx, precision=precision)
        if mine_x:
            return pw_gemm(PW_DGRAD, W, g_y, am_w[0] if am_w is not None else amax(W), am_g, B, Co, Ci, N, addend=add_gx, precision=precision)
        if not need_x:
            return add_gx
        g = torch.bmm(W.t().unsqueeze(0).expand(B, -1, -1), g_y)
        return g if add_gx is None else g + add_gx

    def wgrad():
        if mine_w:
            # both operands row-scaled where their maxima are per channel: a nearly-dead channel of g_y (or of x) keeps its
            # 22 bits in its own row of g_W (include/cloudct.h, ct_pw_gemm_rs)
            return pw_gemm(PW_WGRAD, g_y, x, am_g, am_x if am_x is not None else amax_of(x, rows=True), B, Co, Ci, N, precision=precision)
        return torch.bmm(g_y, x.transpose(1, 2)).sum(0) if need_w else None

    # the two gradients are independent and neither is a whole number of rounds of the chip's workgroup slots (1024 + 672
    # workgroups on 512 slots at 848 x 512): inside a HIP-graph capture they go to two streams and fill each other's tails
    if (PW_BWD_STREAMS and mine_x and mine_w and g_y.is_cuda and torch.cuda.is_current_stream_capturing()
            and _stream(g_y.device) not in forked_streams):
        cur = torch.cuda.current_stream(g_y.device)
        side = _pw_side_stream(g_y.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            g_x = dgrad()
        g_w = wgrad()
        cur.wait_stream(side)
        g_x.record_stream(cur)
    else:
        g_x, g_w = dgrad(), wgrad()
    return g_x, g_w


# ---------------------------------------------------------------------------
# DifferentiablePositions
# ---------------------------------------------------------------------------
class PositionsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, keys, W, H):
        _dev(keys)
        keys = _f32c(keys)
        dim = len(W)
        B, HD, N = keys.shape
        assert HD == H * dim
        V = 1 << dim
        lc = torch.empty(B, H, V, N, device=keys.device, dtype=torch.float32)
        idx = torch.empty(B, H, V, N, device=keys.device, dtype=torch.int64)
        lib = _lib.load()
        with _on(keys.device):
            _lib.check(lib.ct_positions_fwd(_ptr(keys), _ptr(lc), _ptr(idx), B, H, N, dim,
                                            _lib.int_array(W), _stream()), "ct_positions_fwd")
        ctx.save_for_backward(keys)
        ctx.W, ctx.H = W, H
        ctx.mark_non_differentiable(idx)
        return lc, idx

    @staticmethod
    def backward(ctx, g_lc, _g_idx):
        (keys,) = ctx.saved_tensors
        W, H = ctx.W, ctx.H
        B, _, N = keys.shape
        g_lc = _f32c(g_lc)
        g_keys = torch.empty_like(keys)
        lib = _lib.load()
        with _on(keys.device):
            _lib.check(lib.ct_positions_bwd(_ptr(keys), _ptr(g_lc), _ptr(g_keys), B, H, N, len(W),
                                            _lib.int_array(W), _stream()), "ct_positions_bwd")
        return g_keys, None, None


# ---------------------------------------------------------------------------
# fused (keys-based) Splat / Slice — the hot path
# ---------------------------------------------------------------------------
# what the mode refuses of the raster entry points (include/cloudct.h): the wording of determinism.refuse's message
_BIG_GRID_ADD = "a scatter-add onto a grid whose single-channel tile exceeds a CU's LDS: global float atomics only"
RASTER_TICKETS = os.environ.get("CLOUDCT_TICKETS", "1") != "0"      # "0": the two-launch form (A/B, debugging)
_tickets = {}


def _capturing(device):
    """Whether the current stream of `device` is recording a HIP graph.  Asked only where a per-stream state buffer is
    missing from its cache (raster_tickets, grid_occupancy_ratio, mhct_core_workspace): a buffer made DURING a capture
    lives in that graph's private pool and its zero-fill is a node of that graph alone, so it must not outlive the launch it
    was made for — cached, every later graph on the stream would use it without an init node of its own (uninitialised if
    it is replayed before the first one, or if that capture never finished), and the first graph would re-zero state other
    launches depend on at every replay."""
    with _on(device):
        return torch.cuda.is_current_stream_capturing()


def raster_tickets(device, force=False):
    """The arrival tickets of the backward raster passes (include/cloudct.h: ct_slice_bwd_tk / ct_splat_bwd_tk) for the
    CURRENT stream of `device`: a zeroed CT_TICKETS_BYTES buffer kept for the life of the process.  The kernels leave it zero,
    so it is initialised once; launches that share a buffer must be ordered, hence one buffer per stream (the heads of a
    union block run side by side on their own streams, and autograd replays every backward on its forward's stream).
    On a capturing stream that has no buffer yet the launch gets one of its own (_capturing above): allocated in the graph's
    pool, zeroed by a node of the graph, not cached — the caller keeps the tensor until its launch is enqueued.  A stream
    that ran the op eagerly before the capture (harness._capture warms up on its capture stream) keeps its cached buffer
    and the graph gains no node."""
    if not RASTER_TICKETS and not force:
        return None
    key = (device.index, _stream(device))
    t = _tickets.get(key)
    if t is None:
        t = torch.zeros(_lib.TICKETS_BYTES // 4, device=device, dtype=torch.int32)
        if not _capturing(device):
            _tickets[key] = t
    return t


class SplatKeysFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, keys, feat, pad, W, H, reduce):
        _dev(keys, feat, pad)
        keys, feat = _f32c(keys), _f32c(feat)
        dim = len(W)
        B, HC, N = feat.shape
        assert HC % H == 0 and keys.shape == (B, H * dim, N)
        C = HC // H
        padt, pad_code = _pad_args(pad, B, N)
        grid = torch.empty(B, HC, *W, device=feat.device, dtype=torch.float32)
        lib = _lib.load()
        _det.push(lib)          # (reduce="sum" onto a grid beyond a CU's LDS has float atomics only: refused in the mode)
        with _on(feat.device):
            _lib.check(_det.call(lib, "ct_splat_fwd", "ct_splat_fwd (%s)" % _BIG_GRID_ADD, _ptr(keys), _ptr(feat), _ptr(padt), pad_code,
                                 _ptr(grid), B, H, C, N, dim, _lib.int_array(W), _lib.REDUCE[reduce], _stream()),
                       "ct_splat_fwd")
        ctx.save_for_backward(keys, feat, padt, grid if reduce == "max" else None)
        ctx.meta = (W, H, C, reduce, pad_code)
        return grid

    @staticmethod
    def backward(ctx, g_grid):
        keys, feat, padt, grid = ctx.saved_tensors
        W, H, C, reduce, pad_code = ctx.meta
        dim = len(W)
        B, HC, N = feat.shape
        g_grid = _f32c(g_grid)
        g_feat = torch.empty_like(feat)
        g_keys = torch.empty_like(keys)
        lib = _lib.load()
        _det.push(lib)          # (the query below is sized by the mode)
        Wa = _lib.int_array(W)
        ws_bytes = lib.ct_splat_bwd_workspace_bytes(B, H, C, N, dim, Wa, _lib.REDUCE[reduce])
        ws = torch.empty(ws_bytes, device=feat.device, dtype=torch.uint8) if ws_bytes else None
        tk = raster_tickets(feat.device)
        with _on(feat.device):
            _lib.check(lib.ct_splat_bwd_tk(_ptr(keys), _ptr(feat), _ptr(padt), pad_code, _ptr(grid), _ptr(g_grid),
                                           _ptr(g_feat), None, _ptr(g_keys), _ptr(ws), ws_bytes, _ptr(tk),
                                           B, H, C, N, dim, Wa, _lib.REDUCE[reduce], _stream()), "ct_splat_bwd_tk")
        return g_keys, g_feat, None, None, None, None


class SliceKeysFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, keys, grid, pad, W, H):
        _dev(keys, grid, pad)
        keys, grid = _f32c(keys), _f32c(grid)
        dim = len(W)
        B, HC = grid.shape[:2]
        N = keys.shape[-1]
        assert HC % H == 0 and keys.shape == (B, H * dim, N) and list(grid.shape[2:]) == list(W)
        C = HC // H
        padt, pad_code = _pad_args(pad, B, N)
        out = torch.empty(B, HC, N, device=grid.device, dtype=torch.float32)
        lib = _lib.load()
        with _on(grid.device):
            _lib.check(lib.ct_slice_fwd(_ptr(keys), _ptr(grid), _ptr(padt), pad_code, _ptr(out),
                                        B, H, C, N, dim, _lib.int_array(W), _stream()), "ct_slice_fwd")
        ctx.save_for_backward(keys, grid, padt)
        ctx.meta = (W, H, C, pad_code)
        return out

    @staticmethod
    def backward(ctx, g_out):
        keys, grid, padt = ctx.saved_tensors
        W, H, C, pad_code = ctx.meta
        dim = len(W)
        B, _, N = keys.shape
        g_out = _f32c(g_out)
        g_grid = torch.empty_like(grid)
        g_keys = torch.empty_like(keys)
        lib = _lib.load()
        _det.push(lib)          # (off the hot shapes the key cotangents of the chunk groups are summed with atomics outside the mode)
        Wa = _lib.int_array(W)
        ws_bytes = lib.ct_slice_bwd_workspace_bytes(B, H, C, N, dim, Wa)
        ws = torch.empty(ws_bytes, device=grid.device, dtype=torch.uint8) if ws_bytes else None
        tk = raster_tickets(grid.device)
        with _on(grid.device):
            _lib.check(_det.call(lib, "ct_slice_bwd_tk", "ct_slice_bwd_tk (%s)" % _BIG_GRID_ADD, _ptr(keys), _ptr(grid), _ptr(padt), pad_code,
                                 _ptr(g_out), _ptr(g_grid), _ptr(g_keys), _ptr(ws), ws_bytes, _ptr(tk),
                                 B, H, C, N, dim, Wa, _stream()),
                       "ct_slice_bwd_tk")
        return g_keys, g_grid, None, None, None


# ---------------------------------------------------------------------------
# explicit (local_coordinate, flattened_index) Splat / Slice — API-compatible path
# ---------------------------------------------------------------------------
def _check_idx(idx):
    if idx.dtype != torch.int64:
        raise TypeError("flattened_index must be int64 (layers/cloud_transform.py:81)")
    return idx.contiguous()


class SplatLcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lc, idx, feat, pad, W, H, reduce):
        _dev(lc, idx, feat, pad)
        lc, feat, idx = _f32c(lc), _f32c(feat), _check_idx(idx)
        dim = len(W)
        B, HC, N = feat.shape
        V = 1 << dim
        assert HC % H == 0 and lc.shape == (B, H, V, N) and idx.shape == (B, H, V, N)
        C = HC // H
        padt, pad_code = _pad_args(pad, B, N)
        grid = torch.empty(B, HC, *W, device=feat.device, dtype=torch.float32)
        lib = _lib.load()
        _det.push(lib)
        with _on(feat.device):
            _lib.check(_det.call(lib, "ct_splat_lc_fwd", "ct_splat_lc_fwd (%s)" % _BIG_GRID_ADD, _ptr(lc), _ptr(idx), _ptr(feat), _ptr(padt),
                                 pad_code, _ptr(grid), B, H, C, N, dim, _lib.int_array(W), _lib.REDUCE[reduce], _stream()),
                       "ct_splat_lc_fwd")
        ctx.save_for_backward(lc, idx, feat, padt, grid if reduce == "max" else None)
        ctx.meta = (W, H, C, reduce, pad_code)
        return grid

    @staticmethod
    def backward(ctx, g_grid):
        lc, idx, feat, padt, grid = ctx.saved_tensors
        W, H, C, reduce, pad_code = ctx.meta
        dim = len(W)
        B, HC, N = feat.shape
        g_grid = _f32c(g_grid)
        g_feat = torch.empty_like(feat)
        g_lc = torch.empty_like(lc)
        lib = _lib.load()
        _det.push(lib)          # (the query below is sized by the mode)
        Wa = _lib.int_array(W)
        ws_bytes = lib.ct_splat_bwd_workspace_bytes(B, H, C, N, dim, Wa, _lib.REDUCE[reduce])
        ws = torch.empty(ws_bytes, device=feat.device, dtype=torch.uint8) if ws_bytes else None
        with _on(feat.device):
            _lib.check(lib.ct_splat_lc_bwd(_ptr(lc), _ptr(idx), _ptr(feat), _ptr(padt), pad_code, _ptr(grid),
                                           _ptr(g_grid), _ptr(g_feat), _ptr(g_lc), _ptr(ws), ws_bytes,
                                           B, H, C, N, dim, Wa, _lib.REDUCE[reduce], _stream()), "ct_splat_lc_bwd")
        return g_lc, None, g_feat, None, None, None, None


class SliceLcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lc, idx, grid, pad, W, H):
        _dev(lc, idx, grid, pad)
        lc, grid, idx = _f32c(lc), _f32c(grid), _check_idx(idx)
        dim = len(W)
        B, HC = grid.shape[:2]
        V = 1 << dim
        N = lc.shape[-1]
        assert HC % H == 0 and lc.shape == (B, H, V, N) and idx.shape == (B, H, V, N)
        assert math.prod(grid.shape[2:]) == math.prod(W)
        C = HC // H
        padt, pad_code = _pad_args(pad, B, N)
        out = torch.empty(B, HC, N, device=grid.device, dtype=torch.float32)
        lib = _lib.load()
        with _on(grid.device):
            _lib.check(lib.ct_slice_lc_fwd(_ptr(lc), _ptr(idx), _ptr(grid), _ptr(padt), pad_code, _ptr(out),
                                           B, H, C, N, dim, _lib.int_array(W), _stream()), "ct_slice_lc_fwd")
        ctx.save_for_backward(lc, idx, grid, padt)
        ctx.meta = (W, H, C, pad_code)
        return out

    @staticmethod
    def backward(ctx, g_out):
        lc, idx, grid, padt = ctx.saved_tensors
        W, H, C, pad_code = ctx.meta
        dim = len(W)
        B, _, _, N = lc.shape
        g_out = _f32c(g_out)
        g_grid = torch.empty_like(grid)
        g_lc = torch.empty_like(lc)
        lib = _lib.load()
        _det.push(lib)
        with _on(grid.device):
            _lib.check(_det.call(lib, "ct_slice_lc_bwd", "ct_slice_lc_bwd (%s)" % _BIG_GRID_ADD, _ptr(lc), _ptr(idx), _ptr(grid), _ptr(padt),
                                 pad_code, _ptr(g_out), _ptr(g_grid), _ptr(g_lc), B, H, C, N, dim, _lib.int_array(W), _stream()),
                       "ct_slice_lc_bwd")
        return g_lc, None, g_grid, None, None, None


# ---------------------------------------------------------------------------
# lattice: per-head rigid transform of (xyz + residual) and tanh, fused
# ---------------------------------------------------------------------------
class LatticeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, residual, R, shift, scales, kscale, dim, with_stats=False):
        _dev(xyz, residual, R, shift, scales, kscale)
        xyz, residual, R, shift = _f32c(xyz), _f32c(residual), _f32c(R), _f32c(shift)
        scales = _f32c(scales) if scales is not None else None
        ks = _f32c(kscale).reshape(1) if kscale is not None else None
        B, _, N = xyz.shape
        H = R.shape[0]
        assert xyz.shape[1] == 3 and residual.shape == (B, H * 3, N) and R.shape == (H, 3, 3) and shift.shape == (H, 3)
        keys = torch.empty(B, H * dim, N, device=xyz.device, dtype=torch.float32)
        lattice = torch.empty_like(keys)
        lib = _lib.load()
        stats = ws = None
        ws_bytes = 0
        if with_stats:
            stats = torch.empty(2, device=xyz.device, dtype=torch.float32)
            ws_bytes = lib.ct_lattice_fwd_workspace_bytes(B, H, N)
            ws = torch.empty(ws_bytes, device=xyz.device, dtype=torch.uint8)
        with _on(xyz.device):
            _lib.check(lib.ct_lattice_fwd(_ptr(xyz), _ptr(residual), _ptr(R), _ptr(shift), _ptr(scales), _ptr(ks),
                                          _ptr(keys), _ptr(lattice), _ptr(stats), _ptr(ws), ws_bytes, B, H, N, dim, _stream()),
                       "ct_lattice_fwd")
        ctx.save_for_backward(xyz, residual, R, shift, scales, ks, lattice)
        ctx.meta = (B, H, N, dim, kscale.shape if kscale is not None else None)
        # a block uses one of (keys, tanh(keys)) downstream: the other's cotangent stays None instead of a zero tensor that a
        # fill kernel writes and the backward kernel reads (ct_lattice_bwd takes either pointer as NULL)
        ctx.set_materialize_grads(False)
        if with_stats:
            ctx.mark_non_differentiable(stats)
            return keys, lattice, stats
        return keys, lattice

    @staticmethod
    def backward(ctx, g_keys, g_lattice, _g_stats=None):
        xyz, residual, R, shift, scales, ks, lattice = ctx.saved_tensors
        B, H, N, dim, ks_shape = ctx.meta
        if g_keys is None and g_lattice is None:
            return (None,) * 8
        g_keys = _f32c(g_keys) if g_keys is not None else None
        g_lattice = _f32c(g_lattice) if g_lattice is not None else None
        g_xyz, g_res = torch.empty_like(xyz), torch.empty_like(residual)
        g_R, g_shift = torch.empty_like(R), torch.empty_like(shift)
        g_scales = torch.empty_like(scales) if scales is not None else None
        g_ks = torch.empty_like(ks) if ks is not None else None
        lib = _lib.load()
        _det.push(lib)          # (the workspace is always passed: the parameter sums are ordered in either mode)
        with _on(xyz.device):
            ws_bytes = lib.ct_lattice_bwd_workspace_bytes(B, H, N)
            ws = torch.empty(ws_bytes, device=xyz.device, dtype=torch.uint8)
            _lib.check(lib.ct_lattice_bwd(_ptr(xyz), _ptr(residual), _ptr(R), _ptr(shift), _ptr(scales), _ptr(ks),
                                          _ptr(lattice), _ptr(g_lattice), _ptr(g_keys), _ptr(g_xyz), _ptr(g_res),
                                          _ptr(g_R), _ptr(g_shift), _ptr(g_scales), _ptr(g_ks), _ptr(ws), ws_bytes,
                                          B, H, N, dim, _stream()),
                       "ct_lattice_bwd")
        return g_xyz, g_res, g_R, g_shift, g_scales, (g_ks.reshape(ks_shape) if g_ks is not None else None), None, None


def lattice(xyz, residual, R, shift, scales, kscale, dim, with_stats=False):
    """(keys, tanh(keys)) of an MHCT block; R = so3_exponential_map(log_R) [H,3,3].  with_stats: also a
    non-differentiable f32[2] = (mean, unbiased variance) of the keys, reduced inside the same launch.  The variance is
    one-pass, (sum k^2 - n mean^2) / (n - 1) from float32 workgroup partials: accurate to
    3 m 2^-24 mean(k^2) n / (n - 1) with m = dim * (points per workgroup / 256) + 20, that is relative to mean(k^2), not to the
    variance (tests/test_lattice_cases_gpu.py: _check_stats)."""
    return LatticeFn.apply(xyz, residual, R, shift, scales, kscale, dim, with_stats)


class LatticeSo3Fn(torch.autograd.Function):
    """LatticeFn with the so3 exponential map of the rotation parameters inside the launches (ct_lattice_so3_fwd / _bwd): the
    forward is ONE launch (map + transform + tanh + key statistics, finished by the launch's last workgroup), the backward two
    (the tail launch also turns g_R into g_log_R) — three launches per head and step where LatticeFn + So3ExpFn are six."""

    @staticmethod
    def forward(ctx, xyz, residual, log_R, shift, scales, kscale, dim, eps, with_stats=False):
        _dev(xyz, residual, log_R, shift, scales, kscale)
        xyz, residual, log_R, shift = _f32c(xyz), _f32c(residual), _f32c(log_R), _f32c(shift)
        scales = _f32c(scales) if scales is not None else None
        ks = _f32c(kscale).reshape(1) if kscale is not None else None
        B, _, N = xyz.shape
        H = log_R.shape[0]
        assert xyz.shape[1] == 3 and residual.shape == (B, H * 3, N) and log_R.shape == (H, 3) and shift.shape == (H, 3)
        dev = xyz.device
        keys = torch.empty(B, H * dim, N, device=dev, dtype=torch.float32)
        lattice = torch.empty_like(keys)
        R = torch.empty(H, 3, 3, device=dev, dtype=torch.float32)
        lib = _lib.load()
        stats = ws = ticket = None
        ws_bytes = 0
        if with_stats:
            stats = torch.empty(2, device=dev, dtype=torch.float32)
            ws_bytes = lib.ct_lattice_fwd_workspace_bytes(B, H, N)
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            tk = raster_tickets(dev, force=True)
            ticket = tk.data_ptr() + (tk.numel() - 1) * 4          # the buffer's last word (the raster kernels use the front)
        with _on(dev):
            _lib.check(lib.ct_lattice_so3_fwd(_ptr(xyz), _ptr(residual), _ptr(log_R), float(eps), _ptr(shift), _ptr(scales), _ptr(ks),
                                              _ptr(R), _ptr(keys), _ptr(lattice), _ptr(stats), _ptr(ws), ws_bytes, ticket, B, H, N, dim,
                                              _stream()), "ct_lattice_so3_fwd")
        ctx.save_for_backward(xyz, residual, log_R, R, shift, scales, ks, lattice)
        ctx.meta = (B, H, N, dim, kscale.shape if kscale is not None else None, float(eps))
        ctx.set_materialize_grads(False)
        if with_stats:
            ctx.mark_non_differentiable(stats)
            return keys, lattice, stats
        return keys, lattice

    @staticmethod
    def backward(ctx, g_keys, g_lattice, _g_stats=None):
        xyz, residual, log_R, R, shift, scales, ks, lattice = ctx.saved_tensors
        B, H, N, dim, ks_shape, eps = ctx.meta
        if g_keys is None and g_lattice is None:
            return (None,) * 9
        g_keys = _f32c(g_keys) if g_keys is not None else None
        g_lattice = _f32c(g_lattice) if g_lattice is not None else None
        g_xyz, g_res = torch.empty_like(xyz), torch.empty_like(residual)
        g_R, g_shift, g_log_R = torch.empty_like(R), torch.empty_like(shift), torch.empty_like(log_R)
        g_scales = torch.empty_like(scales) if scales is not None else None
        g_ks = torch.empty_like(ks) if ks is not None else None
        lib = _lib.load()
        _det.push(lib)          # (the workspace is always passed: the parameter sums are ordered in either mode)
        with _on(xyz.device):
            ws_bytes = lib.ct_lattice_bwd_workspace_bytes(B, H, N)
            ws = torch.empty(ws_bytes, device=xyz.device, dtype=torch.uint8)
            _lib.check(lib.ct_lattice_so3_bwd(_ptr(xyz), _ptr(residual), _ptr(log_R), eps, _ptr(R), _ptr(shift), _ptr(scales), _ptr(ks),
                                              _ptr(lattice), _ptr(g_lattice), _ptr(g_keys), _ptr(g_xyz), _ptr(g_res), _ptr(g_log_R),
                                              _ptr(g_R), _ptr(g_shift), _ptr(g_scales), _ptr(g_ks), _ptr(ws), ws_bytes, B, H, N, dim,
                                              _stream()), "ct_lattice_so3_bwd")
        return (g_xyz, g_res, g_log_R, g_shift, g_scales, (g_ks.reshape(ks_shape) if g_ks is not None else None), None, None, None)


def lattice_so3(xyz, residual, log_R, shift, scales, kscale, dim, eps=1e-4, with_stats=False):
    """(keys, tanh(keys)[, key statistics]) of an MHCT block from the transformer's so3 parameters log_R [H,3]
    (layers/utils.py:25-34,53-61; eps: pytorch3d's so3_exponential_map default).  The reported variance is one-pass from float32
    workgroup partials, accurate to the bound that ops.lattice states: relative to mean(k^2), not to the variance."""
    return LatticeSo3Fn.apply(xyz, residual, log_R, shift, scales, kscale, dim, eps, with_stats)


class So3ExpFn(torch.autograd.Function):
    """so3 exponential map log_R [H,3] -> R [H,3,3] (pytorch3d's, layers/utils.py:6,29,56), one launch each way."""

    @staticmethod
    def forward(ctx, log_R, eps):
        _dev(log_R)
        log_R = _f32c(log_R)
        H = log_R.shape[0]
        R = torch.empty(H, 3, 3, device=log_R.device, dtype=torch.float32)
        lib = _lib.load()
        with _on(log_R.device):
            _lib.check(lib.ct_so3_exp_fwd(_ptr(log_R), _ptr(R), H, float(eps), _stream()), "ct_so3_exp_fwd")
        ctx.save_for_backward(log_R)
        ctx.eps = float(eps)
        return R

    @staticmethod
    def backward(ctx, g_R):
        (log_R,) = ctx.saved_tensors
        g_R = _f32c(g_R)
        g = torch.empty_like(log_R)
        lib = _lib.load()
        with _on(log_R.device):
            _lib.check(lib.ct_so3_exp_bwd(_ptr(log_R), _ptr(g_R), _ptr(g), log_R.shape[0], ctx.eps, _stream()), "ct_so3_exp_bwd")
        return g, None


def so3_exp(log_R, eps=1e-4):
    return So3ExpFn.apply(log_R, eps)


def _batch_stride(t, C, N):
    """Batch stride (floats) of t if it is a [B,C,N] tensor whose rows are contiguous, whose channels are N apart and
    whose batches are a multiple of 4 >= C*N apart, 16-byte aligned — a contiguous tensor or a channel slice of a wider
    one (what torch.cat's backward hands out); None otherwise."""
    if (t.dim() == 3 and t.dtype == torch.float32 and t.size(1) == C and t.size(2) == N and t.stride(2) == 1
            and (t.stride(1) == N or C == 1) and t.stride(0) >= C * N and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0):
        return t.stride(0)
    return None


def _residual_arg(residual, C, N):
    """(tensor, batch stride) of a residual the kernels read where it lies, else of its contiguous copy; (None, 0) without one."""
    if residual is None:
        return None, 0
    rbs = _batch_stride(residual, C, N)
    if rbs is None:
        residual, rbs = _f32c(residual), 0
    return residual, rbs


def _cotangent(gy, B, C, N, device):
    """(tensor, batch stride) of a cotangent the kernels can read where it lies, else of its contiguous copy (stride 0 = dense);
    None -> zeros."""
    if gy is None:
        gy = torch.zeros(B, C, N, device=device, dtype=torch.float32)
    gybs = _batch_stride(gy, C, N)
    if gybs is None:
        gy, gybs = _f32c(gy), 0
    return gy, gybs


class AdaInFn(torch.autograd.Function):
    """relu?(instance_norm(x) * (gamma + 1) + beta) [+ residual], gamma_beta [B,2,C] (layers/utils.py:88-97).  x may be a
    channel slice of a wider tensor (read where it lies), and so may the cotangent."""

    @staticmethod
    def forward(ctx, x, gamma_beta, eps, relu, residual):
        _dev(x, gamma_beta)
        if x.dtype != torch.float32:
            raise TypeError("expected float32, got %s" % x.dtype)
        B, C, N = x.shape
        xbs = _batch_stride(x, C, N)
        if xbs is None:
            x, xbs = x.contiguous(), 0
        assert gamma_beta.shape == (B, 2, C)
        gamma_beta, gbbs = _gb_arg(gamma_beta, B, C)
        residual, rbs = _residual_arg(residual, C, N)
        y = torch.empty(B, C, N, device=x.device, dtype=torch.float32)
        mean = torch.empty(B * C, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        slots = _amax_slots(B * C, x.device)
        with _on(x.device):
            _adain_group_fwd([dict(x=_ptr(x), xbs=xbs, gb=gamma_beta, gbbs=gbbs, res=_ptr(residual), rbs=rbs, y=_ptr(y), ybs=0, mean=mean,
                                   rstd=rstd, amax=_ptr(slots), abs=0, C=C, eps=eps, relu=bool(relu))], B, N)
        tag_amax(y, slots)
        ctx.save_for_backward(x, gamma_beta, mean, rstd)
        ctx.relu = int(bool(relu))
        ctx.xbs = xbs
        ctx.gbbs = gbbs
        ctx.has_residual = residual is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma_beta, mean, rstd = ctx.saved_tensors
        B, C, N = x.shape
        gy, gybs = _cotangent(gy, B, C, N, x.device)
        gx = torch.empty(B, C, N, device=x.device, dtype=torch.float32)
        g_gb = torch.empty(B, 2, C, device=x.device, dtype=torch.float32)
        slots = _amax_slots(B * C, x.device)
        with _on(x.device):
            _adain_group_bwd([dict(x=_ptr(x), xbs=ctx.xbs, gb=gamma_beta, gbbs=ctx.gbbs, mean=mean, rstd=rstd, gy=_ptr(gy), gybs=gybs,
                                   gx=_ptr(gx), gxbs=0, g_gb=g_gb, amax=_ptr(slots), abs=0, C=C, relu=ctx.relu)], B, N)
        tag_amax(gx, slots)
        return gx, g_gb, None, None, (gy if ctx.has_residual else None)


def adain(x, gamma_beta, eps=1e-5, relu=False, residual=None):
    """Adaptive instance norm of x [B,C,N] with per-(b,c) scale (+1) and bias gamma_beta [B,2,C]; `residual` is added
    to the result in the same pass."""
    return AdaInFn.apply(x, gamma_beta, eps, relu, residual)


class StyleProjFn(torch.autograd.Function):
    """The style projections of ALL adaptive instance norms of a block — `linear_i(style)` for every AdaIn1dUpd
    (layers/utils.py:90; layers/multihead_ct_adain.py: keys_bn / values_bn of each head, the heads' `after` norms, the union's `after`
    and shortcut norms) — as ONE product with the weights stacked: seven [B,L] x [L,2C_i] library GEMMs of 8-15 us, their 21
    backward products and the six accumulations of the style cotangent become 3 + 4 launches.  Arguments: style [B,L], then
    (weight [2C_i,L], bias [2C_i]) per norm.  Returns one [B,2,C_i] VIEW per norm into the stacked result (strides (sum, C_i, 1):
    the AdaIN kernels read it where it lies, `_gb_arg`)."""

    @staticmethod
    def forward(ctx, style, *wb):
        ws, bs = wb[0::2], wb[1::2]
        W = torch.cat(ws, dim=0)
        out = torch.addmm(torch.cat(bs, dim=0), style, W.t())              # [B, sum 2C_i]
        ctx.save_for_backward(style, W)
        ctx.sizes = [w.size(0) for w in ws]
        outs, o = [], 0
        for d in ctx.sizes:
            outs.append(out[:, o:o + d].unflatten(1, (2, d // 2)))
            o += d
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        style, W = ctx.saved_tensors
        B = style.size(0)
        parts = [(g.reshape(B, d) if g is not None else style.new_zeros(B, d)) for g, d in zip(gouts, ctx.sizes)]
        g = torch.cat(parts, dim=1)                                           # [B, sum 2C_i]
        g_style = g @ W if ctx.needs_input_grad[0] else None
        g_W, g_b = g.t() @ style, g.sum(0)
        grads, o = [g_style], 0
        for d in ctx.sizes:                       # row ranges of the stacked gradients: dense views, no copies
            grads += [g_W[o:o + d], g_b[o:o + d]]
            o += d
        return tuple(grads)


def _gb_arg(gb, B, C):
    """gamma_beta [B,2,C] for the AdaIN kernels without a copy: (tensor, batch stride in floats, 0 = contiguous).  A column
    range of a stacked style projection [B, sum 2*C_i] viewed as [B,2,C] has strides (sum, C, 1): the kernels take the sum."""
    if gb.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % gb.dtype)
    if gb.dim() == 3 and gb.shape == (B, 2, C) and gb.stride(2) == 1 and gb.stride(1) == C and (B == 1 or gb.stride(0) >= 2 * C):
        return gb, (0 if B == 1 or gb.stride(0) == 2 * C else gb.stride(0))
    return gb.contiguous(), 0


def _runs(n, step):
    """(first, run) of every launch over a table of n items taken `step` at a time."""
    return [(first, min(step, n - first)) for first in range(0, n, step)]


def _at(arr, first):
    """Address of item `first` of a ctypes item array."""
    return ctypes.addressof(arr) + first * ctypes.sizeof(arr._type_)


def _adain_fwd_table(items):
    """ct_adain_fwd_item array.  items: dicts with x (ptr), xbs, gb, gbbs (optional), res, rbs, y (ptr), ybs, mean, rstd, amax
    (ptr or None), abs (amax batch stride), C, eps, relu."""
    arr = (_lib.AdainFwdItem * len(items))()
    for e, it in zip(arr, items):
        e.x, e.x_batch_stride, e.gamma_beta, e.residual, e.residual_batch_stride = it["x"], it["xbs"], _ptr(it["gb"]), it["res"], it["rbs"]
        e.y, e.y_batch_stride, e.mean, e.rstd = it["y"], it["ybs"], _ptr(it["mean"]), _ptr(it["rstd"])
        e.amax_out, e.amax_batch_stride, e.C, e.eps, e.relu = it["amax"], it["abs"], it["C"], float(it["eps"]), int(it["relu"])
        e.gamma_beta_batch_stride = it.get("gbbs", 0)
    return arr


def _adain_bwd_table(items):
    """ct_adain_bwd_item array.  items: dicts with x (ptr), xbs, gb, gbbs (optional), mean, rstd, gy (ptr), gybs, gx (ptr), gxbs,
    g_gb, amax, abs, C, relu."""
    arr = (_lib.AdainBwdItem * len(items))()
    for e, it in zip(arr, items):
        e.x, e.x_batch_stride, e.gamma_beta, e.mean, e.rstd = it["x"], it["xbs"], _ptr(it["gb"]), _ptr(it["mean"]), _ptr(it["rstd"])
        e.gy, e.gy_batch_stride, e.gx, e.gx_batch_stride, e.g_gamma_beta = it["gy"], it["gybs"], it["gx"], it["gxbs"], _ptr(it["g_gb"])
        e.amax_out, e.amax_batch_stride, e.C, e.relu = it["amax"], it["abs"], it["C"], int(it["relu"])
        e.gamma_beta_batch_stride = it.get("gbbs", 0)
    return arr


def _adain_runs(n):
    """AdaIN's launch rule: runs of BN_GROUP_MAX norms, or one by one with the switch off."""
    return _runs(n, _lib.BN_GROUP_MAX if BN_GROUP_LAUNCH else 1)


def _adain_group_fwd(items, B, N):
    """The adaptive instance norms `items` (_adain_fwd_table) over the same (B, N), BN_GROUP_MAX to a launch (ct_adain_group_fwd).
    The empty shapes end here: the library takes none."""
    lib = _lib.load()
    if B == 0 or N == 0:
        return
    arr = _adain_fwd_table([it for it in items if it["C"] > 0])
    for first, run in _adain_runs(len(arr)):
        _lib.check(lib.ct_adain_group_fwd(_at(arr, first), run, B, N, _stream()), "ct_adain_group_fwd")


def _adain_group_bwd(items, B, N):
    """Backward of _adain_group_fwd (items: _adain_bwd_table).  Rows without points have zero gamma / beta gradients."""
    lib = _lib.load()
    if B == 0:
        return
    if N == 0:
        for it in items:
            it["g_gb"].zero_()
        return
    arr = _adain_bwd_table([it for it in items if it["C"] > 0])
    for first, run in _adain_runs(len(arr)):
        _lib.check(lib.ct_adain_group_bwd(_at(arr, first), run, B, N, _stream()), "ct_adain_group_bwd")


class UnionKeysValuesAdaInFn(torch.autograd.Function):
    """UnionKeysValuesFn for the AdaIN blocks (layers/multihead_ct_adain.py:104-111): one stacked GEMM for the heads'
    keys_values_pred projections, keys_bn / values_bn = adaptive instance norms on channel ranges of its output.
    Arguments: n, x, eps, then per head: weight [Co,Cin,1], gamma_beta of keys_bn [B,2,Ck], gamma_beta of values_bn
    [B,2,Cv].  Returns (keys_res_0, values_0, keys_res_1, values_1, ...)."""

    @staticmethod
    def forward(ctx, n, x, eps, *args):
        ctx.passthrough = n < 0          # x itself as the first output: see UnionKeysValuesFn
        n = abs(n)
        heads = [args[i * 3:(i + 1) * 3] for i in range(n)]
        x_in = x
        x = _f32c(x)
        _dev(x)
        B, Cin, N = x.shape
        Wc = torch.cat([h[0][:, :, 0] for h in heads], dim=0)
        Ct = Wc.size(0)
        ctx.pw_precision = _prec.code()      # the layer's three products share the forward's precision (precision.py)
        y, am_w, am_x, Wt = pw_forward(Wc, x, ctx.needs_input_grad[1])
        outs, saved, meta, items, c0 = [], [], [], [], 0
        for h in heads:
            for gb in h[1:3]:
                C = gb.size(2)
                gb, gbbs = _gb_arg(gb, B, C)
                o = torch.empty(B, C, N, device=x.device, dtype=torch.float32)
                mean = torch.empty(B * C, device=x.device, dtype=torch.float32)
                rstd = torch.empty_like(mean)
                items.append(dict(x=_ptr(y) + c0 * N * 4, xbs=Ct * N, gb=gb, gbbs=gbbs, res=None, rbs=0, y=_ptr(o), ybs=0, mean=mean,
                                  rstd=rstd, amax=None, abs=0, C=C, eps=eps, relu=0))
                outs.append(o)
                saved += [gb, mean, rstd]
                meta.append((c0, C))
                c0 += C
        with _on(x.device):
            _adain_group_fwd(items, B, N)
        assert c0 == Ct, "keys_bn + values_bn must cover the projections"
        ctx.save_for_backward(x, y, Wc, *saved)
        ctx.am = (am_w, am_x, Wt)
        ctx.meta = meta
        ctx.couts = [h[0].size(0) for h in heads]
        if ctx.passthrough:
            return (x_in,) + tuple(outs)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        g_skip = None
        if ctx.passthrough:
            g_skip, gouts = gouts[0], gouts[1:]
        x, y, Wc = ctx.saved_tensors[:3]
        saved = ctx.saved_tensors[3:]
        B, Cin, N = x.shape
        Ct = Wc.size(0)
        g_y = torch.empty_like(y)
        g_gbs, items, keep = [], [], []
        slots = _amax_slots(B * Ct, x.device)           # [B][Ct]: every norm writes its channel range of every cloud
        for i, (c0, C) in enumerate(ctx.meta):
            gb, mean, rstd = saved[i * 3:(i + 1) * 3]
            gy, gybs = _cotangent(gouts[i], B, C, N, x.device)
            keep.append(gy)
            g_gb = torch.empty(B, 2, C, device=x.device, dtype=torch.float32)
            items.append(dict(x=_ptr(y) + c0 * N * 4, xbs=Ct * N, gb=gb, gbbs=_gb_arg(gb, B, C)[1], mean=mean, rstd=rstd, gy=_ptr(gy), gybs=gybs,
                              gx=_ptr(g_y) + c0 * N * 4, gxbs=Ct * N, g_gb=g_gb,
                              amax=None if slots is None else _ptr(slots) + 4 * c0, abs=Ct, C=C, relu=0))
            g_gbs.append(g_gb)
        with _on(x.device):
            _adain_group_bwd(items, B, N)
        g_x, g_Wc = pw_backward(Wc, x, g_y, ctx.am[0], ctx.am[1], ctx.needs_input_grad[1], True,
                                am_g=None if slots is None else slots.view(-1, Ct), Wt=ctx.am[2],
                                add_gx=g_skip if ctx.needs_input_grad[1] else None, precision=ctx.pw_precision)
        grads, r0 = [None, g_x, None], 0
        for hi, Co in enumerate(ctx.couts):
            grads += [g_Wc[r0:r0 + Co].unsqueeze(-1), g_gbs[2 * hi], g_gbs[2 * hi + 1]]
            r0 += Co
        return tuple(grads)


class JoinAdaInReluFn(torch.autograd.Function):
    """cat([relu(adain_i(x_i)) for i], dim=1): the AdaIN heads' `after` stacks followed by the union's concatenation
    (layers/multihead_ct_adain.py:64-66,205-214) — JoinBnReluFn's counterpart.  Arguments: n, eps, then per head (x, gamma_beta)."""

    @staticmethod
    def forward(ctx, n, eps, *args):
        xs = [_f32c(args[2 * i]) for i in range(n)]
        gbs = [_gb_arg(args[2 * i + 1], xs[i].size(0), xs[i].size(1))[0] for i in range(n)]
        _dev(*xs)
        B, _, N = xs[0].shape
        Ct = sum(x.size(1) for x in xs)
        y = torch.empty(B, Ct, N, device=xs[0].device, dtype=torch.float32)
        slots = _amax_slots(B * Ct, y.device)
        saved, items, c0 = [], [], 0
        for x, gb in zip(xs, gbs):
            C = x.size(1)
            mean = torch.empty(B * C, device=y.device, dtype=torch.float32)
            rstd = torch.empty_like(mean)
            items.append(dict(x=_ptr(x), xbs=0, gb=gb, gbbs=_gb_arg(gb, B, C)[1], res=None, rbs=0, y=_ptr(y) + c0 * N * 4, ybs=Ct * N,
                              mean=mean, rstd=rstd, amax=None if slots is None else _ptr(slots) + 4 * c0, abs=Ct, C=C, eps=eps, relu=1))
            saved += [x, gb, mean, rstd]
            c0 += C
        with _on(y.device):
            _adain_group_fwd(items, B, N)
        tag_amax(y, slots)
        ctx.save_for_backward(*saved)
        ctx.n = n
        return y

    @staticmethod
    def backward(ctx, gy):
        n, saved = ctx.n, ctx.saved_tensors
        B, Ct, N = gy.shape
        gybs = _batch_stride(gy, Ct, N)
        if gybs is None:
            gy, gybs = _f32c(gy), Ct * N
        grads, items, c0 = [None, None], [], 0
        for i in range(n):
            x, gb, mean, rstd = saved[i * 4:(i + 1) * 4]
            C = x.size(1)
            gx, g_gb = torch.empty_like(x), torch.empty(B, 2, C, device=x.device, dtype=torch.float32)
            slots = _amax_slots(B * C, gx.device)
            items.append(dict(x=_ptr(x), xbs=0, gb=gb, gbbs=_gb_arg(gb, B, C)[1], mean=mean, rstd=rstd, gy=_ptr(gy) + c0 * N * 4, gybs=gybs,
                              gx=_ptr(gx), gxbs=0,
                              g_gb=g_gb, amax=_ptr(slots), abs=0, C=C, relu=1))
            grads += [tag_amax(gx, slots), g_gb]
            c0 += C
        with _on(gy.device):
            _adain_group_bwd(items, B, N)
        return tuple(grads)


# ---------------------------------------------------------------------------
# training-mode BatchNorm1d (+ ReLU, + skip) groups, with or without an exchange of statistics between ranks
# ---------------------------------------------------------------------------
_sync_stats_collectives = 0
BN_GROUP_LAUNCH = os.environ.get("CLOUDCT_BN_GROUP", "1") != "0"     # A/B switch: the norms of a group one by one


def sync_stats_collectives():
    """Number of statistics collectives (one all_gather per norm group in forward, one all_reduce in backward) issued
    by this process so far — bench.py reports the per-step figure."""
    return _sync_stats_collectives


SYNC_STATS_FORCE = os.environ.get("CLOUDCT_SYNCBN_FORCE", "0") == "1"


def _sync_group(bn):
    """The process group a norm module exchanges its batch statistics over, or None: a plain BatchNorm1d, no process
    group initialised, or a SyncBatchNorm whose group has a single rank (torch's own SyncBatchNorm then runs the plain
    batch norm too: nn/modules/batchnorm.py `need_sync`)."""
    if not isinstance(bn, torch.nn.SyncBatchNorm):
        return None
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    pg = bn.process_group if bn.process_group is not None else dist.group.WORLD
    # (SYNC_STATS_FORCE: keep the exchange path on in a one-rank group too — what a multi-rank step enqueues, collectives
    #  included, then runs and is timed on a single GPU: bench.py --mode ddp-step, tests/test_ddp_gpu.py)
    return pg if dist.get_world_size(pg) > 1 or SYNC_STATS_FORCE else None


def norms_share_group(bns):
    """True when the norms of a fused group are of ONE type and exchange their statistics over ONE process group: the
    group kernels take both from the first norm, so a mix (an unconverted BatchNorm1d beside SyncBatchNorms, or two
    process groups) must go through the modules one by one."""
    first, group = type(bns[0]), _sync_group(bns[0])
    return all(type(bn) is first and _sync_group(bn) is group for bn in bns[1:])


def _bn_runs(n):
    """BatchNorm's launch rule (training and eval): 2..BN_GROUP_MAX norms make ONE run; a single norm, more than BN_GROUP_MAX
    or CLOUDCT_BN_GROUP=0 go one by one."""
    return _runs(n, n if 1 < n <= _lib.BN_GROUP_MAX and BN_GROUP_LAUNCH else 1)


def _bn_fwd_table(items, stats=None):
    """ct_bn_fwd_item array.  items: dicts with x (data_ptr), xbs, C, w, b, rm, rv, eps, relu, res (ptr or None), rbs, y (ptr),
    ybs and, optionally, amax (ptr to C floats: the per-channel max |y| as written), nbt and mom (training).  stats: the
    (save_mean, save_rstd) tensors of every item (training)."""
    arr = (_lib.BnFwdItem * len(items))()
    for i, (e, it) in enumerate(zip(arr, items)):
        e.x, e.x_batch_stride, e.weight, e.bias = it["x"], it["xbs"], _ptr(it["w"]), _ptr(it["b"])
        e.running_mean, e.running_var, e.num_batches_tracked = _ptr(it["rm"]), _ptr(it["rv"]), _ptr(it.get("nbt"))
        e.residual, e.residual_batch_stride, e.y, e.y_batch_stride = it["res"], it["rbs"], it["y"], it["ybs"]
        if stats is not None:
            e.save_mean, e.save_rstd = _ptr(stats[i][0]), _ptr(stats[i][1])
        e.amax_out, e.C, e.eps, e.momentum, e.relu = it.get("amax"), it["C"], float(it["eps"]), float(it.get("mom", 0.0)), int(it["relu"])
    return arr


def _bn_bwd_table(items, grads=None):
    """ct_bn_bwd_item array.  items: dicts with x, xbs, C, w, b, mean, rstd, gy (ptr), gybs, gx (ptr), gxbs, relu and, optionally,
    amax.  grads: the (g_weight, g_bias) tensors of every item (None around an exchange: the sums buffer holds them)."""
    arr = (_lib.BnBwdItem * len(items))()
    for i, (e, it) in enumerate(zip(arr, items)):
        e.x, e.x_batch_stride, e.weight, e.bias = it["x"], it["xbs"], _ptr(it["w"]), _ptr(it["b"])
        e.save_mean, e.save_rstd, e.gy, e.gy_batch_stride = _ptr(it["mean"]), _ptr(it["rstd"]), it["gy"], it["gybs"]
        e.gx, e.gx_batch_stride, e.amax_out = it["gx"], it["gxbs"], it.get("amax")
        if grads is not None:
            e.g_weight, e.g_bias = _ptr(grads[i][0]), _ptr(grads[i][1])
        e.C, e.relu = it["C"], int(it["relu"])
    return arr


def _bn_group_fwd(items, B, N, device, group):
    """Run the norms of one group (items: _bn_fwd_table).  Returns ([(mean, rstd)] per item, count) — count is None without a
    group, else a 1-float device tensor with the job's values per channel.  With a group: local statistics of ALL items into
    one buffer, ONE all_gather, then the normalising kernels merge the ranks' statistics themselves (csrc/ct_bnorm.hip mode
    1 / 2).  Either way the launches cover the runs of _bn_runs: the whole group at once, or its norms one by one."""
    global _sync_stats_collectives
    lib = _lib.load()
    n = len(items)
    stats = [(torch.empty(it["C"], device=device, dtype=torch.float32), torch.empty(it["C"], device=device, dtype=torch.float32))
             for it in items]
    arr = _bn_fwd_table(items, stats)
    if group is None:
        for first, run in _bn_runs(n):
            _lib.check(lib.ct_bn_group_fwd(_at(arr, first), run, B, N, _stream()), "ct_bn_group_fwd")
        return stats, None
    import torch.distributed as dist
    world = dist.get_world_size(group)
    stride = 2 * sum(it["C"] for it in items) + 1           # [mean: Ct | m2: Ct | count]: the table's layout, ct_bn_group_stats_fwd
    local = torch.empty(stride, device=device, dtype=torch.float32)
    for first, run in _bn_runs(n):
        _lib.check(lib.ct_bn_group_stats_fwd(ctypes.addressof(arr), n, first, run, B, N, _ptr(local), _stream()), "ct_bn_group_stats_fwd")
    gathered = torch.empty(world * stride, device=device, dtype=torch.float32)
    # non-blocking: the collective is enqueued on RCCL's own stream (behind the statistics kernels) and the compute stream
    # waits for it only where the first normalising kernel is enqueued — the host prepares those launches meanwhile, and
    # whatever else is already queued on other streams (DDP's gradient buckets in backward) is not held up behind it
    work = dist.all_gather_into_tensor(gathered, local, group=group, async_op=True)
    _sync_stats_collectives += 1
    count = torch.empty(1, device=device, dtype=torch.float32)
    work.wait()                       # stream-level wait (no host synchronisation with the RCCL backend)
    for first, run in _bn_runs(n):
        _lib.check(lib.ct_bn_group_apply_fwd(ctypes.addressof(arr), n, first, run, B, N, _ptr(gathered), world, _ptr(count), _stream()),
                   "ct_bn_group_apply_fwd")
    # (`gathered` is read by the kernels just enqueued: torch's caching allocator keeps it alive on this stream)
    return stats, count


def _bn_group_bwd(items, B, N, device, group, count):
    """Backward of a norm group (items: _bn_bwd_table), over the same runs as the forward.  Returns [(g_weight, g_bias)] per
    item (this rank's sums: DDP averages parameter gradients itself).  With a group: the two per-channel sums of ALL items
    into one buffer, ONE all_reduce, then the input-gradient kernels."""
    global _sync_stats_collectives
    lib = _lib.load()
    n = len(items)
    if group is None:
        out = [(torch.empty(it["C"], device=device, dtype=torch.float32), torch.empty(it["C"], device=device, dtype=torch.float32))
               for it in items]
        arr = _bn_bwd_table(items, out)
        for first, run in _bn_runs(n):
            _lib.check(lib.ct_bn_group_bwd(_at(arr, first), run, B, N, _stream()), "ct_bn_group_bwd")
        return out
    import torch.distributed as dist
    Ct = sum(it["C"] for it in items)
    sums = torch.empty(2 * Ct, device=device, dtype=torch.float32)       # [sum g' | sum g' * xhat]
    arr = _bn_bwd_table(items)
    local = torch.empty_like(sums)                                        # this rank's g_bias / g_weight: written by the same launches
    for first, run in _bn_runs(n):
        _lib.check(lib.ct_bn_group_reduce_bwd(ctypes.addressof(arr), n, first, run, B, N, _ptr(sums), _ptr(local), _stream()),
                   "ct_bn_group_reduce_bwd")
    work = dist.all_reduce(sums, group=group, async_op=True)             # non-blocking, as in _bn_group_fwd
    _sync_stats_collectives += 1
    work.wait()
    for first, run in _bn_runs(n):
        _lib.check(lib.ct_bn_group_apply_bwd(ctypes.addressof(arr), n, first, run, B, N, _ptr(sums), _ptr(count), _stream()),
                   "ct_bn_group_apply_bwd")
    out, c0 = [], 0
    for it in items:
        out.append((local[Ct + c0:Ct + c0 + it["C"]], local[c0:c0 + it["C"]]))
        c0 += it["C"]
    return out


# ---------------------------------------------------------------------------
# the three modes of a fused norm, and the norms on their stored statistics (ct_bn_eval_group_fwd / ct_bn_eval_group_bwd)
# ---------------------------------------------------------------------------
# train:  batch statistics, running buffers updated in place (ct_bn_group_*, above).
# eval:   the stored statistics where autograd would record nothing — forward only, on purpose: plain functions that save
#         nothing.  "0": every eval norm through its module (A/B runs).
# frozen: the stored statistics in a forward that records gradients, only for norms marked by cloud_transformers_amd.freeze_norms
#         (an unmarked eval norm with gradients keeps its module's path).  The eval functions' launches — same items, same maxima
#         tags — which save the norm's INPUT (x, or the stacked GEMM output), never y: the backward recomputes the ReLU mask from
#         it.  "0": marked norms through their modules (A/B runs).
BN_EVAL = os.environ.get("CLOUDCT_BN_EVAL", "1") != "0"
BN_FROZEN = os.environ.get("CLOUDCT_BN_FROZEN", "1") != "0"
# nn.BatchNorm1d, and nn.SyncBatchNorm (what parallel.data_parallel / the reference's DDP recipe turns every norm into:
# train_segmentation.py:128): same parameters and buffers, statistics exchanged over its process group
_BN_TYPES = (torch.nn.BatchNorm1d, torch.nn.SyncBatchNorm)


def _bn_eval_group(items, B, N):
    """Run stored-statistics norms over the same (B, N) (ct_bn_eval_group_fwd), over the runs of _bn_runs as _bn_group_fwd.
    items: _bn_fwd_table dicts (_bn_eval_item)."""
    lib = _lib.load()
    arr = _bn_fwd_table(items)
    for first, run in _bn_runs(len(items)):
        _lib.check(lib.ct_bn_eval_group_fwd(_at(arr, first), run, B, N, _stream()), "ct_bn_eval_group_fwd")


def _bn_eval_bwd_table(items):
    """ct_bn_eval_bwd_item array.  items: dicts with x (data_ptr), xbs, C, w, b, rm, rv, eps, relu, gy (ptr), gybs, gx (ptr or
    None), gxbs and, optionally, gw / gb (tensors: both or neither) and amax (ptr)."""
    arr = (_lib.BnEvalBwdItem * len(items))()
    for e, it in zip(arr, items):
        e.x, e.x_batch_stride, e.weight, e.bias = it["x"], it["xbs"], _ptr(it["w"]), _ptr(it["b"])
        e.running_mean, e.running_var, e.gy, e.gy_batch_stride = _ptr(it["rm"]), _ptr(it["rv"]), it["gy"], it["gybs"]
        e.gx, e.gx_batch_stride, e.g_weight, e.g_bias = it["gx"], it["gxbs"], _ptr(it.get("gw")), _ptr(it.get("gb"))
        e.amax_out, e.C, e.eps, e.relu = it.get("amax"), it["C"], float(it["eps"]), int(it["relu"])
    return arr


def _bn_eval_group_bwd(items, B, N):
    """Backward of _bn_eval_group over the same runs (ct_bn_eval_group_bwd); items: _bn_eval_bwd_table dicts.  An item that
    asks for nothing (no gx, no sums) is left out."""
    items = [it for it in items if it["gx"] is not None or it.get("gw") is not None]
    if not items:
        return
    lib = _lib.load()
    arr = _bn_eval_bwd_table(items)
    for first, run in _bn_runs(len(items)):
        _lib.check(lib.ct_bn_eval_group_bwd(_at(arr, first), run, B, N, _stream()), "ct_bn_eval_group_bwd")


def _norm_args(bn, stored, detach=False):
    """A norm's run of a Function's arguments: (weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum).
    A norm on its stored statistics updates nothing, so it has neither counter nor momentum; `detach`: the parameters of an
    eval function, which records nothing."""
    w, b = (bn.weight.detach(), bn.bias.detach()) if detach else (bn.weight, bn.bias)
    if stored:
        return (w, b, bn.running_mean, bn.running_var, None, bn.eps, None)
    return (w, b, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum)


_NORM_ARGS = 7


def _stored_item(place, norm):
    """`place` (a norm's pointers, strides, C and relu) + what a stored-statistics launch reads of the norm (_norm_args)."""
    w, b, rm, rv, _, eps, _ = norm
    return dict(place, w=_f32c(w), b=_f32c(b), rm=_f32c(rm), rv=_f32c(rv), eps=float(eps))


def _bn_eval_item(bn, x_ptr, xbs, y_ptr, ybs, relu, res=None, rbs=0, amax=None):
    return _stored_item(dict(x=x_ptr, xbs=xbs, C=bn.num_features, relu=int(bool(relu)), res=res, rbs=rbs, y=y_ptr, ybs=ybs, amax=amax),
                        _norm_args(bn, True, detach=True))


def _norms_fwd(layout, norms, stored, B, N, device, group=None):
    """Launch the norms of a composition.  layout: one dict per norm with where it reads and writes (x, xbs, C, relu, res, rbs, y,
    ybs, amax: a composition's forward layout); norms: their _norm_args.  -> (per norm the four tensors its backward reads —
    weight, bias and the batch mean / rstd of a training norm or the running mean / variance of a stored one —, count: see
    _bn_group_fwd)."""
    with _on(device):
        if stored:
            items = [_stored_item(place, norm) for place, norm in zip(layout, norms)]
            _bn_eval_group(items, B, N)
            return [(it["w"], it["b"], it["rm"], it["rv"]) for it in items], None
        items = [dict(place, w=_f32c(w), b=_f32c(b), rm=rm, rv=rv, nbt=nbt, eps=eps, mom=mom)
                 for place, (w, b, rm, rv, nbt, eps, mom) in zip(layout, norms)]
        stats, count = _bn_group_fwd(items, B, N, device, group)
    return [(it["w"], it["b"], mean, rstd) for it, (mean, rstd) in zip(items, stats)], count


def _norms_bwd(ctx, layout, saved, needs, B, N, device, count):
    """Backward of _norms_fwd.  layout: one dict per norm (x, xbs, C, relu, gy, gybs, gx, gxbs, amax: a composition's backward
    layout); saved: _norms_fwd's tuples; needs: per norm whether (weight, bias) take a gradient.  -> [(g_weight, g_bias)].  A
    training norm computes both whatever `needs` says; a stored one skips the sums nobody needs, and the launch if nothing is."""
    with _on(device):
        if not ctx.stored:
            return _bn_group_bwd([dict(place, w=w, b=b, mean=mean, rstd=rstd) for place, (w, b, mean, rstd) in zip(layout, saved)],
                                 B, N, device, ctx.group, count)
        items, sums = [], []
        for place, (w, b, rm, rv), eps, (need_w, need_b) in zip(layout, saved, ctx.eps, needs):
            g_w = g_b = None
            if need_w or need_b:
                g_w, g_b = (torch.empty(place["C"], device=device, dtype=torch.float32) for _ in range(2))
            items.append(dict(place, w=w, b=b, rm=rm, rv=rv, eps=eps, gw=g_w, gb=g_b))
            sums.append((g_w if need_w else None, g_b if need_b else None))
        _bn_eval_group_bwd(items, B, N)
    return sums


def _save_norms(ctx, tensors, norms, saved, count, stored, group):
    ctx.save_for_backward(*tensors, count, *[t for s in saved for t in s])
    ctx.stored, ctx.group, ctx.eps = stored, group, [float(norm[5]) for norm in norms]


def _saved_norms(ctx, n):
    """-> (the n tensors saved in front, count, _norms_fwd's tuples, needs_input_grad — all True for a training backward, which
    computes everything)"""
    t = ctx.saved_tensors
    needs = ctx.needs_input_grad if ctx.stored else (True,) * len(ctx.needs_input_grad)
    return t[:n], t[n], [t[i:i + 4] for i in range(n + 1, len(t), 4)], needs


# -- one norm (+ ReLU, + residual) -------------------------------------------------------------------------------------------
def _single_fwd(x, norm, relu, residual, stored, group=None):
    """relu?(norm(x)) [+ residual].  -> (y with its per-channel maxima tag, x as read, *_norms_fwd's results)"""
    _dev(x, norm[0], norm[1], residual)
    x = _f32c(x)
    B, C, N = x.shape
    y = torch.empty_like(x)
    residual, rbs = _residual_arg(residual, C, N)
    slots = _amax_slots(C, x.device)
    saved, count = _norms_fwd([dict(x=_ptr(x), xbs=0, C=C, relu=int(bool(relu)), res=_ptr(residual), rbs=rbs, y=_ptr(y), ybs=0,
                                    amax=_ptr(slots))], [norm], stored, B, N, x.device, group)
    return tag_amax(y, slots), x, saved, count


class BnReluFn(torch.autograd.Function):
    """relu?(norm(x)) [+ residual]: the nn.Sequential(BatchNorm1d, ReLU) tail of the blocks' `after` stacks and the union's skip
    connection (layers/multihead_ct.py:67-68,149-153,198).  Training mode (ct_bn_group_*: batch statistics, running statistics
    and num_batches_tracked updated in place by the kernel; `group`: the process group of a SyncBatchNorm) or, `stored`, the
    running statistics with gradients (bn_eval's launch forward, ct_bn_eval_group_bwd backward; they are read, never written).
    Arguments: stored, group, x, relu, residual, then the norm (_norm_args)."""

    @staticmethod
    def forward(ctx, stored, group, x, relu, residual, *norm):
        y, x, saved, count = _single_fwd(x, norm, relu, residual, stored, group)
        _save_norms(ctx, [x], [norm], saved, count, stored, group)
        ctx.relu, ctx.has_residual = int(bool(relu)), residual is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,), count, saved, needs = _saved_norms(ctx, 1)
        B, C, N = x.shape
        gy, gybs = _cotangent(gy, B, C, N, x.device)          # a slice of the concatenation's cotangent is read where it lies
        gx = torch.empty_like(x) if needs[2] else None
        slots = _amax_slots(C, x.device) if needs[2] else None
        ((g_w, g_b),) = _norms_bwd(ctx, [dict(x=_ptr(x), xbs=0, C=C, relu=ctx.relu, gy=_ptr(gy), gybs=gybs, gx=_ptr(gx), gxbs=0,
                                              amax=_ptr(slots))], saved, [needs[5:7]], B, N, x.device, count)
        if gx is not None:
            tag_amax(gx, slots)
        return (None, None, gx, None, gy if ctx.has_residual and needs[4] else None, g_w, g_b) + (None,) * (_NORM_ARGS - 2)


def bn_relu(x, bn, relu=True, residual=None):
    """relu?(bn(x)) [+ residual] through the fused kernels; the caller checked bn_relu_eligible(bn, x).  Updates the
    module's running statistics and num_batches_tracked exactly as nn.BatchNorm1d.forward does in training mode."""
    return BnReluFn.apply(False, _sync_group(bn), x, relu, residual, *_norm_args(bn, False))


def bn_eval(x, bn, relu=True, residual=None):
    """relu?(bn(x)) [+ residual] of an eval-mode norm in one pass (ct_bn_eval_group_fwd); the caller checked
    bn_eval_eligible(bn, x, residual=residual).  Reads the running statistics, writes nothing but the result, which carries
    its per-channel maxima for the pointwise GEMM that reads it next."""
    return _single_fwd(x, _norm_args(bn, True, detach=True), relu, residual, True)[0]


def bn_frozen(x, bn, relu=True, residual=None):
    """relu?(bn(x)) [+ residual] of a frozen norm with gradients; the caller checked bn_frozen_eligible(bn, x,
    residual=residual)."""
    return BnReluFn.apply(True, None, x, relu, residual, *_norm_args(bn, True))


# -- norms on consecutive channel ranges of one tensor, each into a tensor of its own: the two norms on the halves of
#    keys_values_pred's output, and the 2n norms on the stacked projection of a union block ---------------------------------
def _ranges_fwd(src, norms, stored, group=None):
    """The norms on their channel ranges of src [B,Ct,N], read where they lie (batch stride Ct*N): neither contiguous copies of
    the slices nor maxima tags exist.  -> (the outputs, *_norms_fwd's results)"""
    B, Ct, N = src.shape
    layout, outs, c0 = [], [], 0
    for norm in norms:
        C = norm[0].numel()
        o = torch.empty(B, C, N, device=src.device, dtype=torch.float32)
        layout.append(dict(x=_ptr(src) + c0 * N * 4, xbs=Ct * N, C=C, relu=0, res=None, rbs=0, y=_ptr(o), ybs=0, amax=None))
        outs.append(o)
        c0 += C
    assert c0 == Ct, "the norms must cover the channels"
    return (outs,) + _norms_fwd(layout, norms, stored, B, N, src.device, group)


def _ranges_bwd(ctx, src, gouts, saved, needs, need_src, with_slots, count):
    """Backward of _ranges_fwd: every norm writes its input cotangent into its range of ONE [B,Ct,N] tensor (no concatenation
    of cotangents) and, `with_slots`, that range's per-channel maxima into one buffer.  -> (g_src, slots, [(g_weight, g_bias)]);
    g_src and slots are None without need_src."""
    B, Ct, N = src.shape
    g_src = torch.empty_like(src) if need_src else None
    slots = _amax_slots(Ct, src.device) if (with_slots and need_src) else None
    layout, c0 = [], 0
    for gy, (w, _, _, _) in zip(gouts, saved):
        C = w.numel()
        gy, gybs = _cotangent(gy, B, C, N, src.device)
        layout.append(dict(x=_ptr(src) + c0 * N * 4, xbs=Ct * N, C=C, relu=0, gy=_ptr(gy), gybs=gybs, keep=gy,
                           gx=None if g_src is None else _ptr(g_src) + c0 * N * 4, gxbs=Ct * N,
                           amax=None if slots is None else _ptr(slots) + 4 * c0))
        c0 += C
    return g_src, slots, _norms_bwd(ctx, layout, saved, needs, B, N, src.device, count)


def _split_fwd(x, norm_a, norm_b, stored, group=None):
    _dev(x, norm_a[0], norm_b[0])
    x = _f32c(x)
    return (x,) + _ranges_fwd(x, [norm_a, norm_b], stored, group)


class SplitBnFn(torch.autograd.Function):
    """(bn_a(x[:, :Ca]), bn_b(x[:, Ca:])) — the two BatchNorms on the halves of the keys_values_pred output
    (layers/multihead_ct.py:89-91), in training mode or, `stored`, on their running statistics with gradients (_ranges_fwd /
    _ranges_bwd).  Arguments: stored, group, x, then the two norms (_norm_args each)."""

    @staticmethod
    def forward(ctx, stored, group, x, *args):
        norms = [args[:_NORM_ARGS], args[_NORM_ARGS:]]
        x, outs, saved, count = _split_fwd(x, norms[0], norms[1], stored, group)
        _save_norms(ctx, [x], norms, saved, count, stored, group)
        return outs[0], outs[1]

    @staticmethod
    def backward(ctx, *gouts):
        (x,), count, saved, needs = _saved_norms(ctx, 1)
        at = [3 + _NORM_ARGS * i for i in range(2)]                       # each norm's weight among the inputs
        gx, _, sums = _ranges_bwd(ctx, x, gouts, saved, [needs[a:a + 2] for a in at], needs[2], False, count)
        grads = [None, None, gx]
        for g_w, g_b in sums:
            grads += [g_w, g_b] + [None] * (_NORM_ARGS - 2)
        return tuple(grads)


def split_bn(x, bn_a, bn_b):
    """(bn_a(x[:, :Ca]), bn_b(x[:, Ca:])) through SplitBnFn; the caller checked bn_relu_eligible for both modules (each
    against its own slice's shape) and that x is contiguous."""
    return SplitBnFn.apply(False, _sync_group(bn_a), x, *_norm_args(bn_a, False), *_norm_args(bn_b, False))


def split_bn_eval(x, bn_a, bn_b):
    """(bn_a(x[:, :Ca]), bn_b(x[:, Ca:])) of two eval-mode norms in one launch, the halves of x read where they lie; the
    caller checked bn_eval_eligible for both (each against its own slice's channels)."""
    outs = _split_fwd(x, _norm_args(bn_a, True, detach=True), _norm_args(bn_b, True, detach=True), True)[1]
    return outs[0], outs[1]


def split_bn_frozen(x, bn_a, bn_b):
    """(bn_a(x[:, :Ca]), bn_b(x[:, Ca:])) of two frozen norms with gradients; the caller checked bn_frozen_eligible for both
    (each against its own slice's channels)."""
    return SplitBnFn.apply(True, None, x, *_norm_args(bn_a, True), *_norm_args(bn_b, True))


# -- n norms + ReLU written into one concatenation -----------------------------------------------------------------------------
def _join_layout(xs, c0s, y, slots):
    """relu(norm_i(x_i)) into the channels from c0_i on of y [B,Ct,N], every norm's maxima into the same range of `slots`."""
    Ct, N = y.size(1), y.size(2)
    return [dict(x=_ptr(x), xbs=0, C=x.size(1), relu=1, res=None, rbs=0, y=_ptr(y) + c0 * N * 4, ybs=Ct * N,
                 amax=None if slots is None else _ptr(slots) + 4 * c0) for x, c0 in zip(xs, c0s)]


def _join_fwd(xs, norms, stored, group=None):
    """cat([relu(norm_i(x_i)) for i], dim=1): every norm writes its channel range of the result where it belongs; the separate
    outputs and their copy never exist.  -> (y with one maxima tag over all its channels, the x_i as read, *_norms_fwd's results)"""
    xs = [_f32c(x) for x in xs]
    _dev(*xs)
    B, _, N = xs[0].shape
    sizes = [x.size(1) for x in xs]
    y = torch.empty(B, sum(sizes), N, device=xs[0].device, dtype=torch.float32)
    slots = _amax_slots(sum(sizes), y.device)
    c0s = [sum(sizes[:i]) for i in range(len(xs))]
    saved, count = _norms_fwd(_join_layout(xs, c0s, y, slots), norms, stored, B, N, y.device, group)
    return tag_amax(y, slots), xs, saved, count


class JoinBnReluFn(torch.autograd.Function):
    """cat([relu(bn_i(x_i)) for i], dim=1) — the heads' `after` stacks of a union block followed by its concatenation
    (layers/multihead_ct.py:67-68,187-196), in training mode or, `stored`, on the running statistics with gradients; in backward
    every norm reads its range of the cotangent where it lies.  Arguments: stored, group, then per head x and its norm
    (_norm_args)."""

    PER_HEAD = 1 + _NORM_ARGS

    @staticmethod
    def forward(ctx, stored, group, *args):
        P = JoinBnReluFn.PER_HEAD
        heads = [args[i:i + P] for i in range(0, len(args), P)]
        norms = [h[1:] for h in heads]
        y, xs, saved, count = _join_fwd([h[0] for h in heads], norms, stored, group)
        _save_norms(ctx, xs, norms, saved, count, stored, group)
        return y

    @staticmethod
    def backward(ctx, gy):
        P = JoinBnReluFn.PER_HEAD
        n = (len(ctx.needs_input_grad) - 2) // P
        xs, count, saved, needs = _saved_norms(ctx, n)
        B, Ct, N = gy.shape
        gy, gybs = _cotangent(gy, B, Ct, N, gy.device)
        layout, gxs, c0 = [], [], 0
        for i, x in enumerate(xs):
            C = x.size(1)
            gx = torch.empty_like(x) if needs[2 + P * i] else None
            slots = _amax_slots(C, x.device) if gx is not None else None
            layout.append(dict(x=_ptr(x), xbs=0, C=C, relu=1, gy=_ptr(gy) + c0 * N * 4, gybs=gybs or Ct * N, gx=_ptr(gx), gxbs=0,
                               amax=_ptr(slots)))
            gxs.append((gx, slots))
            c0 += C
        sums = _norms_bwd(ctx, layout, saved, [needs[3 + P * i:5 + P * i] for i in range(n)], B, N, gy.device, count)
        grads = [None, None]
        for (gx, slots), (g_w, g_b) in zip(gxs, sums):
            grads += [gx if gx is None else tag_amax(gx, slots), g_w, g_b] + [None] * (_NORM_ARGS - 2)
        return tuple(grads)


def _join_args(xs, bns, stored):
    return [a for x, bn in zip(xs, bns) for a in (x,) + _norm_args(bn, stored)]


def join_bn_relu(xs, bns):
    """cat([relu(bn(x)) for x, bn in zip(xs, bns)], dim=1) through JoinBnReluFn; the caller checked bn_relu_eligible for
    every pair."""
    return JoinBnReluFn.apply(False, _sync_group(bns[0]), *_join_args(xs, bns, False))


def join_bn_relu_eval(xs, bns):
    """cat([relu(bn(x)) for x, bn in zip(xs, bns)], dim=1) of eval-mode norms; the result carries one maxima tag over all its
    channels; the caller checked bn_eval_eligible for every pair."""
    return _join_fwd(xs, [_norm_args(bn, True, detach=True) for bn in bns], True)[0]


def join_bn_relu_frozen(xs, bns):
    """cat([relu(bn(x)) for x, bn in zip(xs, bns)], dim=1) of frozen norms with gradients; the caller checked
    bn_frozen_eligible for every pair."""
    return JoinBnReluFn.apply(True, None, *_join_args(xs, bns, True))


def bn_relu_eval_into(joined, parts):
    """relu(bn(x)) of eval-mode norms into the channels from c0 on of an existing concatenation `joined` [B,Ct,N], for every
    (bn, x, c0) of `parts`, in one launch; no maxima are written and `joined` gets no tag.  The caller checked
    bn_eval_eligible(bn, x) for every pair."""
    B, _, N = joined.shape
    _norms_fwd(_join_layout([x for _, x, _ in parts], [c0 for _, _, c0 in parts], joined, None),
               [_norm_args(bn, True, detach=True) for bn, _, _ in parts], True, B, N, joined.device)


# -- stacked projection + 2n norms ------------------------------------------------------------------------------------------
def _union_fwd(x, weights, norms, stored, group=None, need_dgrad=False):
    """The heads' projections as ONE [sum Co, Cin] x [Cin, N] product per cloud and the norms on the channel ranges of its output
    (_ranges_fwd).  -> ((x as read, the product, the stacked weight), pw_forward's (am_w, am_x, Wt), outs, *_norms_fwd's results)"""
    x = _f32c(x)
    _dev(x)
    Wc = torch.cat([w[:, :, 0] for w in weights], dim=0)                # [sum Co, Cin]
    y, am_w, am_x, Wt = pw_forward(Wc, x, need_dgrad)                   # [B, sum Co, N]
    return ((x, y, Wc), (am_w, am_x, Wt)) + _ranges_fwd(y, norms, stored, group)


def _kv_pairs(outs, n, passthrough=False):
    """(key, values) per head from a union Function's flat outputs; passthrough: (x', that list)."""
    first = 1 if passthrough else 0
    pairs = [(outs[first + 2 * i], outs[first + 2 * i + 1]) for i in range(n)]
    return (outs[0], pairs) if passthrough else pairs


class UnionKeysValuesFn(torch.autograd.Function):
    """The `keys_values_pred` projections of all heads of a union block and the key_bn / values_bn norms on their
    outputs (layers/multihead_ct.py:31-33,89-91), as ONE GEMM with the heads' weights stacked: the heads share the input,
    so forward is one [sum Co, Cin] x [Cin, N] product per cloud instead of one per head, the data gradient one product
    with K = sum Co instead of one per head plus autograd's accumulation of their results, the weight gradient one
    product.  The norms read their channel ranges of the GEMM output where they lie and write their input cotangents
    into the ranges of ONE tensor with its maxima slots, which is the data / weight gradient GEMMs' operand.  In training mode
    the 2n norms share ONE statistics all_gather in forward and ONE all_reduce in backward under SyncBatchNorm; `stored`: on the
    running statistics with gradients — no statistics, so no collective.
    Arguments: stored, group, passthrough, x, then per head: weight [Co,Cin,1], key_bn, values_bn (_norm_args each).
    Returns (keys_res_0, values_0, keys_res_1, values_1, ...)."""

    PER_HEAD = 1 + 2 * _NORM_ARGS

    @staticmethod
    def forward(ctx, stored, group, passthrough, x, *args):
        # passthrough: x itself as the first output too (the block's identity shortcut, layers/multihead_ct.py:170-176:
        # its cotangent comes back here and rides the data gradient's epilogue instead of a separate add over three tensors)
        ctx.passthrough = passthrough
        P = UnionKeysValuesFn.PER_HEAD
        heads = [args[i:i + P] for i in range(0, len(args), P)]
        norms = [h[1 + _NORM_ARGS * j:1 + _NORM_ARGS * (j + 1)] for h in heads for j in range(2)]
        ctx.pw_precision = _prec.code()      # the layer's three products share the forward's precision (precision.py)
        tensors, ctx.am, outs, saved, count = _union_fwd(x, [h[0] for h in heads], norms, stored, group, ctx.needs_input_grad[3])
        _save_norms(ctx, tensors, norms, saved, count, stored, group)
        ctx.couts = [h[0].size(0) for h in heads]
        return ((x,) if ctx.passthrough else ()) + tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        P = UnionKeysValuesFn.PER_HEAD
        g_skip = None
        if ctx.passthrough:
            g_skip, gouts = gouts[0], gouts[1:]
        (x, y, Wc), count, saved, needs = _saved_norms(ctx, 3)
        need_x = ctx.needs_input_grad[3]
        need_W = any(needs[4 + P * h] for h in range(len(ctx.couts)))
        at = [4 + P * (i // 2) + 1 + _NORM_ARGS * (i % 2) for i in range(len(saved))]      # each norm's weight among the inputs
        g_y, slots, sums = _ranges_bwd(ctx, y, gouts, saved, [needs[a:a + 2] for a in at], need_x or need_W, True, count)
        g_x = g_Wc = None
        if g_y is not None:
            g_x, g_Wc = pw_backward(Wc, x, g_y, ctx.am[0], ctx.am[1], need_x, need_W,
                                    am_g=None if slots is None else slots.view(-1, g_y.shape[1]), Wt=ctx.am[2],
                                    add_gx=g_skip if need_x else None, precision=ctx.pw_precision)      # g_Wc [sum Co, Cin]
        elif need_x:
            g_x = g_skip
        grads, r0 = [None, None, None, g_x], 0
        for hi, Co in enumerate(ctx.couts):
            grads.append(g_Wc[r0:r0 + Co].unsqueeze(-1) if (g_Wc is not None and needs[4 + P * hi]) else None)
            for g_w, g_b in sums[2 * hi:2 * hi + 2]:
                grads += [g_w, g_b] + [None] * (_NORM_ARGS - 2)
            r0 += Co
        return tuple(grads)


def _union_args(convs, key_bns, values_bns, stored):
    args = []
    for conv, kb, vb in zip(convs, key_bns, values_bns):
        args += (conv.weight,) + _norm_args(kb, stored) + _norm_args(vb, stored)
    return args


def union_keys_values(x, convs, key_bns, values_bns, passthrough=False):
    """[(key_bn_i(y_i[:, :Ck]), values_bn_i(y_i[:, Ck:])) with y_i = conv_i(x)] for the heads of a union block through
    UnionKeysValuesFn; the caller checked union_keys_values_eligible.  passthrough: -> (x', that list) with x' = x as an output
    of the same node — the block's identity shortcut takes x' so that its cotangent is summed inside the data gradient."""
    return _kv_pairs(UnionKeysValuesFn.apply(False, _sync_group(key_bns[0]), passthrough, x,
                                             *_union_args(convs, key_bns, values_bns, False)), len(convs), passthrough)


def union_keys_values_frozen(x, convs, key_bns, values_bns, passthrough=False):
    """union_keys_values for frozen norms with gradients; the caller checked union_keys_values_frozen_eligible."""
    return _kv_pairs(UnionKeysValuesFn.apply(True, None, passthrough, x,
                                             *_union_args(convs, key_bns, values_bns, True)), len(convs), passthrough)


def union_keys_values_eval(x, convs, key_bns, values_bns):
    """[(key_bn_i(y_i[:, :Ck]), values_bn_i(y_i[:, Ck:])) with y_i = conv_i(x)] for the heads of a union block in eval mode:
    ONE stacked projection GEMM with the 2n norms in its epilogue (PW_NORM, 2n <= BN_GROUP_MAX and a product the forward
    kernel takes), else that GEMM and then the norms on its channel ranges in one launch; the caller checked
    union_keys_values_eval_eligible."""
    bns = [bn for kb, vb in zip(key_bns, values_bns) for bn in (kb, vb)]
    weights = [conv.weight.detach() for conv in convs]
    B, _, N = x.shape
    if _pw_norm_takes(sum(w.size(0) for w in weights), weights[0].size(1), N, len(bns), PW_FWD):
        # the 2n norms in the stacked GEMM's epilogue: the [B, sum Co, N] tensor is never written
        x = _f32c(x)
        _dev(x)
        outs = [torch.empty(B, bn.num_features, N, device=x.device, dtype=torch.float32) for bn in bns]
        pw_gemm_norm(torch.cat([w[:, :, 0] for w in weights], dim=0), x,
                     [_bn_eval_item(bn, None, 0, _ptr(o), 0, False) for bn, o in zip(bns, outs)])
    else:
        outs = _union_fwd(x, weights, [_norm_args(bn, True, detach=True) for bn in bns], True)[2]
    return _kv_pairs(outs, len(convs))


# ---------------------------------------------------------------------------
# which norms take the fused kernels, and in which mode
# ---------------------------------------------------------------------------
_bn_supported = {}
_bn_eval_supported = {}


def _shape_ok(cache, supported, key):
    """The library's answer to `supported`(B, C, N), asked once per shape."""
    ok = cache.get(key)
    if ok is None:
        ok = cache[key] = bool(getattr(_lib.load(), supported)(*key))
    return ok


def _input_ok(x, aligned=True):
    """x CUDA fp32 [B,C,N] contiguous and, with `aligned`, 16-byte aligned."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()
            and (not aligned or x.data_ptr() % 16 == 0))


def _residual_ok(residual):
    """No residual, or a CUDA fp32 3-D one (_residual_arg reads it where it lies or copies it)."""
    return residual is None or (residual.is_cuda and residual.dtype == torch.float32 and residual.dim() == 3)


def _conv1x1_ok(conv, x, Co, weight_like_x=True):
    """A plain bias-free 1x1 nn.Conv1d from x's channels to Co and, with `weight_like_x`, an fp32 weight on x's device."""
    return (isinstance(conv, torch.nn.Conv1d) and conv.kernel_size == (1,) and conv.stride == (1,) and conv.padding == (0,)
            and conv.dilation == (1,) and conv.groups == 1 and conv.bias is None and conv.in_channels == x.size(1)
            and conv.out_channels == Co
            and (not weight_like_x or (conv.weight.dtype == torch.float32 and conv.weight.device == x.device)))


def _bn_train_norm_ok(bn, B, C, N):
    """A training-mode affine norm of C channels with running statistics and a fixed momentum whose shape the register-resident
    ct_bn_group_* kernels take."""
    return (type(bn) in _BN_TYPES and bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None
            and C == bn.num_features and _shape_ok(_bn_supported, "ct_bn_relu_supported", (B, C, N)))


def _bn_eval_norm_ok(bn, B, C, N):
    """An eval-mode affine norm of C channels with running statistics whose shape ct_bn_eval_* takes."""
    return (type(bn) in _BN_TYPES and not bn.training and bn.affine and bn.track_running_stats
            and bn.running_mean is not None and bn.running_var is not None and C == bn.num_features
            and bn.weight.dtype == torch.float32 and bn.running_mean.dtype == torch.float32
            and _shape_ok(_bn_eval_supported, "ct_bn_eval_supported", (B, C, N)))


def _bn_train_ok(bn, x, C):
    return _bn_train_norm_ok(bn, x.size(0), C, x.size(2))


def _bn_stored_ok(bn, x, C):
    return _bn_eval_norm_ok(bn, x.size(0), C, x.size(2)) and bn.weight.device == x.device


def _channels(x, channels):
    return x.size(1) if channels is None and x.dim() == 3 else channels


def _records_nothing(*tensors):
    """True when autograd would record nothing for an op on `tensors` (None entries skipped)."""
    return not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in tensors)


def records_gradients(*tensors):
    """True when autograd would record an op on `tensors` (None entries skipped): the other half of a frozen norm's routing
    rule — where nothing is recorded the eval functions take the norm, marked or not."""
    return not _records_nothing(*tensors)


def norm_frozen(bn):
    """True for a norm marked by freeze_norms (norms.py)."""
    return bool(getattr(bn, "_ct_frozen", False))


def _affine(bns):
    return [p for bn in bns for p in (bn.weight, bn.bias)]


def bn_relu_eligible(bn, x, channels=None):
    """True when `bn` (an nn.BatchNorm1d / nn.SyncBatchNorm, exactly) applied to x (or, with `channels`, to a slice of that many
    of its channels) can run as ct_bn_group_*: training mode with running statistics and a fixed momentum, affine, CUDA fp32
    [B,C,N] contiguous and 16-byte aligned, and a shape the register-resident kernels take (ct_bn_relu_supported)."""
    return _input_ok(x) and _bn_train_ok(bn, x, _channels(x, channels))


def bn_eval_eligible(bn, x, channels=None, residual=None):
    """True when `bn` applied to x (or, with `channels`, to a slice of that many of its channels) can run as
    ct_bn_eval_group_fwd: an nn.BatchNorm1d / nn.SyncBatchNorm (exactly) in eval mode, affine, with running statistics; x CUDA
    fp32 [B,C,N] contiguous and 16-byte aligned; a shape ct_bn_eval_supported takes; and nothing for autograd to record
    (grad mode off, or none of x, the affine parameters and `residual` requires grad)."""
    return (BN_EVAL and _input_ok(x) and _residual_ok(residual) and _bn_stored_ok(bn, x, _channels(x, channels))
            and _records_nothing(x, bn.weight, bn.bias, residual))


def bn_frozen_eligible(bn, x, channels=None, residual=None):
    """bn_eval_eligible without its "nothing to record" clause, for a norm that freeze_norms marked."""
    return (BN_FROZEN and norm_frozen(bn) and _input_ok(x) and _residual_ok(residual)
            and _bn_stored_ok(bn, x, _channels(x, channels)))


def _union_ok(x, convs, key_bns, values_bns, norm_ok, strict=True):
    """More than one plain bias-free 1x1 Conv1d projection of x, each covered by its two norms, every norm passing
    norm_ok(bn, x, C).  The training form is not `strict`: it asks neither for x's alignment nor for the weights' dtype and
    device."""
    return (_input_ok(x, aligned=strict) and len(convs) > 1
            and all(_conv1x1_ok(conv, x, kb.num_features + vb.num_features, weight_like_x=strict)
                    and norm_ok(kb, x, kb.num_features) and norm_ok(vb, x, vb.num_features)
                    for conv, kb, vb in zip(convs, key_bns, values_bns)))


def union_keys_values_eligible(x, convs, key_bns, values_bns):
    """Plain bias-free 1x1 Conv1d projections of the same input and training-mode norms the fused kernels take, of one type and
    one process group."""
    return _union_ok(x, convs, key_bns, values_bns, _bn_train_ok, strict=False) and norms_share_group(list(key_bns) + list(values_bns))


def union_keys_values_eval_eligible(x, convs, key_bns, values_bns):
    """Plain bias-free 1x1 Conv1d projections of the same input, eval-mode norms ct_bn_eval_* takes, and nothing for
    autograd to record."""
    return (BN_EVAL and _union_ok(x, convs, key_bns, values_bns, _bn_stored_ok)
            and _records_nothing(x, *[conv.weight for conv in convs], *_affine(list(key_bns) + list(values_bns))))


def union_keys_values_frozen_eligible(x, convs, key_bns, values_bns):
    """union_keys_values_eval_eligible without its "nothing to record" clause, every norm marked by freeze_norms."""
    return BN_FROZEN and _union_ok(x, convs, key_bns, values_bns, lambda bn, x, C: norm_frozen(bn) and _bn_stored_ok(bn, x, C))


def norm_route(norms, residual=None, watch=(), convs=None):
    """Which fused path takes a group of norms: "train", "eval", "frozen" or None (the modules).  norms: [(bn, x, channels)] —
    one x per norm for a join, one shared x whose channel ranges the norms read for a split (channels None: all of x's); with
    `convs` the union form: the norms are (key_bn, values_bn) per projection of the shared x.  `residual`: added by a single
    norm's launch; `watch`: further tensors whose gradients the forward would have to record (the union's conv weights).
    Train needs training-mode norms, eval and frozen eval-mode ones; eval needs nothing recorded, frozen the mark and something
    recorded: at most one of the three holds, whatever the order they are asked in."""
    bns = [bn for bn, _, _ in norms]
    if convs is not None:
        union = (norms[0][1], convs, bns[0::2], bns[1::2])
        if union_keys_values_eligible(*union):
            return "train"
        if union_keys_values_eval_eligible(*union):
            return "eval"
        stored = union_keys_values_frozen_eligible(*union)
    else:
        if all(bn_relu_eligible(bn, x, C) for bn, x, C in norms) and norms_share_group(bns):
            return "train"
        if all(bn_eval_eligible(bn, x, C, residual) for bn, x, C in norms):
            return "eval"
        stored = all(bn_frozen_eligible(bn, x, C, residual) for bn, x, C in norms)
    if stored and records_gradients(*[x for _, x, _ in norms], *_affine(bns), residual, *watch):
        return "frozen"
    return None


# ---------------------------------------------------------------------------
# eval-mode norms in the epilogue of the pointwise GEMM that produces their input (ct_pw_gemm_rs_norm)
# ---------------------------------------------------------------------------
# Consulted only where BN_EVAL already routes to the eval kernels; the results carry the bits of the GEMM followed by
# ct_bn_eval_group_fwd.  "0": the two launches (A/B runs).
PW_NORM = os.environ.get("CLOUDCT_PW_NORM", "1") != "0"


def _pw_norm_takes(Co, Ci, N, n, mode=None):
    """The switches, a table of 1..BN_GROUP_MAX norms and a product ct_pw_gemm takes (`mode` as pw_eligible: PW_FWD where
    the unfused path would otherwise run the library GEMM, so that the switch never changes which GEMM computes a value)."""
    return PW_NORM and BN_EVAL and 1 <= n <= _lib.BN_GROUP_MAX and pw_eligible(Co, Ci, N, mode)


def pw_norm_eligible(conv, bns, x, residual=None, mode=PW_FWD):
    """True when `conv` (a bias-free 1x1 nn.Conv1d) followed by the eval-mode norms `bns` on consecutive channel ranges of its
    output can run as ONE ct_pw_gemm_rs_norm call: x CUDA fp32 [B,Ci,N] contiguous and 16-byte aligned, at most BN_GROUP_MAX
    norms that cover the output channels, each one ct_bn_eval_* takes, a product ct_pw_gemm takes, and nothing for autograd
    to record (bn_eval_eligible's rule)."""
    return (PW_NORM and BN_EVAL and _input_ok(x) and all(type(bn) in _BN_TYPES for bn in bns)
            and _conv1x1_ok(conv, x, sum(bn.num_features for bn in bns)) and _residual_ok(residual)
            and _pw_norm_takes(conv.out_channels, x.size(1), x.size(2), len(bns), mode)
            and all(_bn_stored_ok(bn, x, bn.num_features) for bn in bns)
            and _records_nothing(x, conv.weight, residual, *_affine(bns)))


def pw_gemm_norm(W, x, items, want_amax=False):
    """ct_pw_gemm_rs_norm: W [Co,Ci] x[b] with the eval norms `items` (_bn_eval_item dicts without an input, in the order of
    the output rows they cover) applied in the epilogue; the operand maxima exactly as pw_forward takes them.  want_amax:
    -> the partial maxima of everything stored (1-D: partials of one maximum, as ops.amax), or None where a GEMM could not
    fold that many."""
    lib = _lib.load()
    W, x = _f32c(W), _f32c(x)
    _dev(W, x)
    Co, Ci = W.shape
    B, _, N = x.shape
    am_w = prep_weight(W, False)[0][0]
    am_x = amax_of(x)
    n_out = lib.ct_pw_gemm_norm_amax_len(B, Co, N) if want_amax else 0
    slots = torch.empty(n_out, device=x.device, dtype=torch.float32) if n_out else None
    arr = _bn_fwd_table(items)
    _prec.push(lib)          # the product's precision (precision.py), read by the entry point where it plans its launch
    with _on(x.device):
        _lib.check(lib.ct_pw_gemm_rs_norm(_ptr(W), _ptr(x), _at(arr, 0), len(items), _ptr(slots), _ptr(am_w), am_w.numel(),
                                          _rows_of(am_w, Co), _ptr(am_x), am_x.numel(), None, 0, B, Co, Ci, N, _stream()),
                   "ct_pw_gemm_rs_norm")
    return slots


def pw_bn_eval(x, conv, bn, relu=True, residual=None):
    """relu?(bn(conv(x))) [+ residual] in one launch; the caller checked pw_norm_eligible(conv, [bn], x, residual).  The
    result carries the partial maxima of its values for the pointwise GEMM that reads it next."""
    B, _, N = x.shape
    C = bn.num_features
    y = torch.empty(B, C, N, device=x.device, dtype=torch.float32)
    residual, rbs = _residual_arg(residual, C, N)
    slots = pw_gemm_norm(conv.weight.detach()[:, :, 0], x, [_bn_eval_item(bn, None, 0, _ptr(y), 0, relu, _ptr(residual), rbs)],
                         want_amax=True)
    if slots is not None:
        y._ct_amax = (slots, y._version)        # (1-D on purpose: tag_amax would read [n / C, C] as per-channel maxima)
    return y


def split_pw_bn_eval(x, conv, bn_a, bn_b):
    """(bn_a(y[:, :Ca]), bn_b(y[:, Ca:])) with y = conv(x), in one launch; the caller checked
    pw_norm_eligible(conv, [bn_a, bn_b], x)."""
    B, _, N = x.shape
    outs = [torch.empty(B, bn.num_features, N, device=x.device, dtype=torch.float32) for bn in (bn_a, bn_b)]
    pw_gemm_norm(conv.weight.detach()[:, :, 0], x, [_bn_eval_item(bn, None, 0, _ptr(o), 0, False) for bn, o in zip((bn_a, bn_b), outs)])
    return outs[0], outs[1]


# ---------------------------------------------------------------------------
# functional entry points
# ---------------------------------------------------------------------------
def positions(keys, tensor_size, heads, dim):
    if keys.numel() == 0:
        _dev(keys)
        B, _, N = keys.shape
        V = 1 << dim
        lc = torch.zeros(B, heads, V, N, device=keys.device, dtype=torch.float32)
        e = _empty(keys)
        return (lc if e is None else lc + e), torch.zeros(B, heads, V, N, device=keys.device, dtype=torch.int64)
    return PositionsFn.apply(keys, sizes_of(tensor_size, dim), heads)


def _empty(*tensors):
    """Empty batches / empty clouds never reach the kernels (the ABI rejects zero sizes): their result is
    defined by the op itself — an empty cloud rasterises to the zero floor, slices to an empty tensor —
    and stays connected to the autograd graph with zero cotangents."""
    z = None
    for t in tensors:
        if t is not None and t.requires_grad:
            z = t.sum() * 0 if z is None else z + t.sum() * 0
    return z


def splat_keys(keys, features, pts_padding, tensor_size, heads, dim, reduce="max"):
    W = sizes_of(tensor_size, dim)
    if features.numel() == 0:
        _dev(keys, features)
        out = torch.zeros(features.shape[0], features.shape[1], *W, device=features.device, dtype=torch.float32)
        e = _empty(keys, features)
        return out if e is None else out + e
    return SplatKeysFn.apply(keys, features, pts_padding, W, heads, reduce)


def slice_keys(keys, grid, pts_padding, tensor_size, heads, dim):
    W = sizes_of(tensor_size, dim)
    if keys.numel() == 0 or grid.numel() == 0:
        _dev(keys, grid)
        out = torch.zeros(grid.shape[0], grid.shape[1], keys.shape[-1], device=grid.device, dtype=torch.float32)
        e = _empty(keys, grid)
        return out if e is None else out + e
    return SliceKeysFn.apply(keys, grid, pts_padding, W, heads)


def splat_lc(lc, idx, features, pts_padding, tensor_size, heads, dim, reduce="max"):
    W = sizes_of(tensor_size, dim)
    if features.numel() == 0:
        _dev(lc, features)
        out = torch.zeros(features.shape[0], features.shape[1], *W, device=features.device, dtype=torch.float32)
        e = _empty(lc, features)
        return out if e is None else out + e
    return SplatLcFn.apply(lc, idx, features, pts_padding, W, heads, reduce)


def slice_lc(lc, idx, grid, pts_padding, tensor_size, heads, dim):
    W = sizes_of(tensor_size, dim)
    if lc.numel() == 0 or grid.numel() == 0:
        _dev(lc, grid)
        out = torch.zeros(grid.shape[0], grid.shape[1], lc.shape[-1], device=grid.device, dtype=torch.float32)
        e = _empty(lc, grid)
        return out if e is None else out + e
    return SliceLcFn.apply(lc, idx, grid, pts_padding, W, heads)


def grid_occupancy_count(grid):
    """Number of elements with |z| > 1e-9 as a 0-dim int64 device tensor
    (layers/multihead_ct.py:104-105 divides it by B*C*H)."""
    _dev(grid)
    grid = _f32c(grid)
    count = torch.empty((), device=grid.device, dtype=torch.int64)
    lib = _lib.load()
    with _on(grid.device):
        _lib.check(lib.ct_grid_occupancy(_ptr(grid), grid.numel(), _ptr(count), _stream()), "ct_grid_occupancy")
    return count


_occ_ws = {}


def occupancy_scale(denominator):
    """float32(1) / float32(K) as a Python float: the scalar torch multiplies by when a float tensor is divided by the number K."""
    import numpy as np
    return float(np.float32(1.0) / np.float32(denominator))



def grid_occupancy_ratio(grid, denominator):
    """count(|z| > 1e-9) / denominator as a 0-dim float32 device tensor — the `occ` statistic of a block
    (layers/multihead_ct.py:104-105) — in ONE launch (ct_grid_occupancy_ratio): `grid_occupancy_count(z).float() / K` is a
    memset node, a kernel and two elementwise launches per head and forward.  Same arithmetic as torch's: float(count) * (1 / K)."""
    _dev(grid)
    grid = _f32c(grid)
    key = (grid.device.index, _stream(grid.device))
    ws = _occ_ws.get(key)
    if ws is None:          # zeroed once; the kernel hands its ticket back as zero; one workspace per stream (ordered launches)
        ws = torch.zeros(_lib.OCC_WORKSPACE_BYTES // 8, device=grid.device, dtype=torch.int64)
        if not _capturing(grid.device):          # (made during a capture: this launch's alone, raster_tickets)
            _occ_ws[key] = ws
    out = torch.empty((), device=grid.device, dtype=torch.float32)
    inv = occupancy_scale(denominator)
    lib = _lib.load()
    with _on(grid.device):
        _lib.check(lib.ct_grid_occupancy_ratio(_ptr(grid), grid.numel(), inv, _ptr(out), _ptr(ws), _stream()),
                   "ct_grid_occupancy_ratio")
    return out


# ---------------------------------------------------------------------------
# plane-resident MHCT core: Splat -> grouped conv -> Slice in one kernel
# ---------------------------------------------------------------------------
# The blocks route their Splat -> conv -> Slice core through the plane-resident kernel where it is built (the shapes of
# ct_mhct_core_supported); CLOUDCT_FUSED_CORE=0 (or ops.FUSED_CORE = False) keeps the three-kernel chain, for A/B runs.
import os as _os
FUSED_CORE = _os.environ.get("CLOUDCT_FUSED_CORE", "1") != "0"
# the LDS-resident backward (16^2 C16 planes: ct_mhct_core_bwd_fused).  Built, parity-tested and MEASURED SLOWER than the backward
# from saved grids (114 vs 82 us at B8 H16 N4096, 74 vs 79 at N2048, tools/core_bwd_bench.py: one workgroup per plane moves
# 5 x 256 KiB through one CU) — so it is off unless CLOUDCT_FUSED_CORE_BWD=1
FUSED_CORE_BWD = _os.environ.get("CLOUDCT_FUSED_CORE_BWD", "0") == "1"
_core_supported = {}


def mhct_core_supported(B, H, C, N, W):
    key = (B, H, C, N, tuple(W))
    ok = _core_supported.get(key)
    if ok is None:
        ok = _core_supported[key] = bool(_lib.load().ct_mhct_core_supported(B, H, C, N, len(W), _lib.int_array(W)))
    return ok


_core_ws = {}


def mhct_core_workspace(device, B, H, C, N, W):
    """The forward's exchange workspace for a shape, allocated and initialised (counters zeroed) ONCE per device, STREAM and
    shape: every launch leaves the counters zeroed, and launches on one stream are ordered, so the buffer is reused — two
    blocks of one shape running side by side on two streams (the heads of a union block, user code) get a buffer each.
    On a capturing stream that has none yet the launch gets a workspace of its own, zeroed by a node of the graph and
    not cached (raster_tickets): the graph is then complete by itself, and its replays re-initialise nobody else's counters
    or status word."""
    key = (device.index, _stream(device), B, H, C, N, tuple(W))
    ws = _core_ws.get(key)
    if ws is None:
        lib = _lib.load()
        Wa = _lib.int_array(W)
        n = lib.ct_mhct_core_workspace_bytes(B, H, C, N, len(W), Wa)
        if _capturing(device):
            # this launch's alone, zeroed as a whole by a fill kernel of the graph (what ct_mhct_core_workspace_init sets is
            # all zeros).  Not the init call's memset: with it the occupancy count of a replay on fresh data came out as a
            # mix of that replay's workgroups and the one's before it (the launch-wide done counter behind the planes'
            # counters did not start at zero once the buffer's memory had been reused inside the graph) —
            # tests/test_graph_replay_gpu.py::test_mhct_core_clusters
            return torch.zeros(n, device=device, dtype=torch.uint8)
        ws = torch.empty(n, device=device, dtype=torch.uint8)
        with _on(device):
            _lib.check(lib.ct_mhct_core_workspace_init(_ptr(ws), n, B, H, C, N, len(W), Wa, _stream()), "ct_mhct_core_workspace_init")
        _core_ws[key] = ws
    return ws


def mhct_core_check(raise_on_fault=True):
    """Did a cluster of any ct_mhct_core_fwd launch so far give up waiting for its partners (include/cloudct.h: status word of
    the workspace)?  Reads the status of every cached workspace — one small copy each, AFTER synchronising: call it at points
    that wait for the device anyway (harness.fit's logging flush).  A workspace whose word is set is re-initialised; with
    `raise_on_fault` the first such workspace raises (the affected launch wrote NaN where its results would have gone).
    It sees the CACHED workspaces only, the ones created by eager launches: a graph captured on a stream without one owns
    the workspaces of its launches (mhct_core_workspace) and re-initialises them at every replay, so a give-up inside such a
    graph shows only as the NaNs the kernel writes."""
    lib = _lib.load()
    bad = []
    for key, ws in list(_core_ws.items()):
        dev_index, _stream_id, B, H, C, N, W = key
        Wa = _lib.int_array(W)
        st = ctypes.c_int(0)
        with torch.cuda.device(dev_index):
            _lib.check(lib.ct_mhct_core_status(_ptr(ws), ws.numel(), B, H, C, N, len(W), Wa, ctypes.byref(st),
                                               _stream()), "ct_mhct_core_status")
            if st.value != 0:
                bad.append(key)
                _lib.check(lib.ct_mhct_core_workspace_init(_ptr(ws), ws.numel(), B, H, C, N, len(W), Wa,
                                                           _stream()), "ct_mhct_core_workspace_init")
    if bad and raise_on_fault:
        raise RuntimeError("ct_mhct_core_fwd: a cluster timed out waiting for its partners on %d workspace(s) %r; the affected "
                           "outputs hold NaN.  The workspaces were re-initialised." % (len(bad), bad[:2]))
    return bad


class MhctCoreFn(torch.autograd.Function):
    """out = Slice(keys, conv(Splat(keys, feat))) and the occupancy count of the rasterised grid
    (layers/multihead_ct.py:99-107).  Forward: ct_mhct_core_fwd — z and conv(z) stay in LDS; when a gradient is needed
    the kernel also writes them out once for the backward (ct_mhct_core_bwd: Slice backward, the two conv gradients,
    Splat backward with the key cotangents summed)."""

    @staticmethod
    def forward(ctx, keys, feat, pad, weight, bias, W, H):
        _dev(keys, feat, pad, weight, bias)
        keys, feat, weight = _f32c(keys), _f32c(feat), _f32c(weight)
        bias = _f32c(bias) if bias is not None else None
        dim = len(W)
        B, HC, N = feat.shape
        C = HC // H
        assert keys.shape == (B, H * dim, N) and weight.shape[0] == HC and weight.shape[1] == C
        padt, pad_code = _pad_args(pad, B, N)
        dev = feat.device
        need_grad = any(ctx.needs_input_grad[i] for i in (0, 1, 3, 4))
        lib = _lib.load()
        Wa = _lib.int_array(W)
        # one workgroup per plane recomputes z and conv(z) in the backward where all five tiles fit a CU: nothing to save
        # (off in deterministic mode: its Splat step keeps the first-claim tie rule)
        recompute = bool(need_grad and FUSED_CORE_BWD and not _det.is_deterministic() and B * H >= 64
                         and lib.ct_mhct_core_bwd_fused_supported(B, H, C, N, dim, Wa))
        out = torch.empty(B, HC, N, device=dev, dtype=torch.float32)
        z = torch.empty(B, HC, *W, device=dev, dtype=torch.float32) if need_grad and not recompute else None
        y = torch.empty(B, HC, *W, device=dev, dtype=torch.float32) if need_grad and not recompute else None
        occ = torch.empty((), device=dev, dtype=torch.int64)
        ws = mhct_core_workspace(dev, B, H, C, N, W)
        nws = ws.numel()
        with _on(dev):
            _lib.check(lib.ct_mhct_core_fwd(_ptr(keys), _ptr(feat), _ptr(padt), pad_code, _ptr(weight), _ptr(bias), _ptr(out),
                                            _ptr(z), _ptr(y), _ptr(occ), _ptr(ws), nws, B, H, C, N, dim, Wa, _stream()),
                       "ct_mhct_core_fwd")
        ctx.save_for_backward(keys, feat, padt, weight, z, y, bias if recompute else None)
        ctx.meta = (W, H, C, pad_code, bias is not None)
        ctx.mark_non_differentiable(occ)
        return out, occ

    @staticmethod
    def backward(ctx, g_out, _g_occ):
        keys, feat, padt, weight, z, y, bias = ctx.saved_tensors
        W, H, C, pad_code, has_bias = ctx.meta
        dim = len(W)
        B, HC, N = feat.shape
        dev = feat.device
        g_out = _f32c(g_out)
        g_feat = torch.empty_like(feat)
        g_keys = torch.empty_like(keys)
        g_w = torch.empty_like(weight)
        g_b = torch.empty(HC, device=dev, dtype=torch.float32) if has_bias else None
        lib = _lib.load()
        Wa = _lib.int_array(W)
        if _det.push(lib) and z is None:
            _det.refuse("ct_mhct_core_bwd_fused")      # (the forward ran outside the mode and saved no grids)
        if z is None:                 # LDS-resident backward: recomputes the grids from the points
            nws = lib.ct_mhct_core_bwd_fused_workspace_bytes(B, H, C, N, dim, Wa)
            ws = torch.empty(nws, device=dev, dtype=torch.uint8)
            with _on(dev):
                _lib.check(lib.ct_mhct_core_bwd_fused(_ptr(keys), _ptr(feat), _ptr(padt), pad_code, _ptr(weight), _ptr(bias), _ptr(g_out),
                                                      _ptr(g_feat), _ptr(g_keys), _ptr(g_w), _ptr(g_b), _ptr(ws), nws,
                                                      B, H, C, N, dim, Wa, _stream()), "ct_mhct_core_bwd_fused")
            return g_keys, g_feat, None, g_w, g_b, None, None
        nws = lib.ct_mhct_core_bwd_workspace_bytes(B, H, C, N, dim, Wa)
        ws = torch.empty(nws, device=dev, dtype=torch.uint8)
        tk = raster_tickets(dev)
        with _on(dev):
            _lib.check(lib.ct_mhct_core_bwd_tk(_ptr(keys), _ptr(feat), _ptr(padt), pad_code, _ptr(weight), _ptr(z), _ptr(y),
                                               _ptr(g_out), _ptr(g_feat), _ptr(g_keys), _ptr(g_w), _ptr(g_b), _ptr(ws), nws,
                                               _ptr(tk), B, H, C, N, dim, Wa, _stream()), "ct_mhct_core_bwd_tk")
        return g_keys, g_feat, None, g_w, g_b, None, None


def mhct_core(keys, features, pts_padding, weight, bias, tensor_size, heads, dim):
    """(sliced features, occupancy count) of one MHCT core; raises unless mhct_core_supported(...)."""
    W = sizes_of(tensor_size, dim)
    return MhctCoreFn.apply(keys, features, pts_padding, weight, bias, W, heads)


# ---------------------------------------------------------------------------
# eval-mode head norms in the Slice write-out (ct_slice_fwd_norm / ct_mhct_core_fwd_norm)
# ---------------------------------------------------------------------------
# The heads' `after` pair (BatchNorm1d -> ReLU on the Slice output) applied in the store of the kernel that produces the value:
# the sliced features are never written un-normed, and a union block in eval mode launches no norm kernel at all.  The results
# carry the bits of Slice (or the core) followed by ct_bn_eval_group_fwd.  Opt-in — "1" turns it on — and consulted only where
# BN_EVAL already routes to the eval kernels: forward only, nothing for autograd to record.
SLICE_NORM = os.environ.get("CLOUDCT_SLICE_NORM", "0") == "1"


class NormTarget:
    """Where the normed Slice output of one head goes: relu?(bn(.)) into channels [c0, c0 + bn.num_features) of `y` [B, Ct, N]
    (None: a dense tensor of its own) and its partial maxima into the 1-D buffer `amax` from slot a0 on (None with a `y`: no
    maxima; without a `y` the op allocates them and tags the result).  The op that takes the target sets `out` to the result."""
    __slots__ = ("bn", "relu", "y", "c0", "amax", "a0", "out")

    def __init__(self, bn, relu=True, y=None, c0=0, amax=None, a0=0):
        self.bn, self.relu, self.y, self.c0, self.amax, self.a0, self.out = bn, relu, y, c0, amax, a0, None


def slice_norm_plannable(bn, x, N):
    """The part of slice_norm_eligible a block can check before its heads run (the union block sizes one maxima buffer for all
    of them first): the switches, an eval-mode norm ct_bn_eval_* takes on clouds of N % 4 == 0 points, a CUDA fp32 input."""
    return bool(SLICE_NORM and BN_EVAL and x.is_cuda and x.dtype == torch.float32 and N % 4 == 0 and not bn.training
                and _bn_eval_norm_ok(bn, x.size(0), bn.num_features, N) and bn.weight.device == x.device)


def slice_norm_eligible(bn, keys, grid, *more):
    """True when relu?(bn(Slice(keys, grid))) can run as ONE ct_slice_fwd_norm (grid: the convolved grid [B, H*C, *W]) or
    ct_mhct_core_fwd_norm (grid: the values [B, H*C, N]; `more`: the filter bank and its bias) call: ops.SLICE_NORM, and
    bn_eval_eligible's rule — an nn.BatchNorm1d / nn.SyncBatchNorm (exactly) in eval mode, affine, with running statistics over the
    H*C channels, fp32, and nothing for autograd to record — on CUDA fp32 contiguous tensors that are 16-byte aligned, N % 4 == 0."""
    if not (SLICE_NORM and BN_EVAL and keys.dim() == 3 and keys.size(2) % 4 == 0 and grid.dim() >= 3):
        return False
    for t in (keys, grid) + more:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0):
            return False
    return (not bn.training and _bn_eval_norm_ok(bn, keys.size(0), grid.size(1), keys.size(2)) and bn.weight.device == keys.device
            and _records_nothing(keys, grid, bn.weight, bn.bias, *more))


def slice_norm_amax_len(B, H, C, N, W):
    """Partial maxima ct_slice_fwd_norm writes for the shape (under the current debug flags); 0: none can be asked for."""
    if PW_GEMM != "split16":
        return 0
    return int(_lib.load().ct_slice_fwd_norm_amax_len(B, H, C, N, len(W), _lib.int_array(W)))


def mhct_core_norm_amax_len(B, H, C, N, W):
    """The same for ct_mhct_core_fwd_norm."""
    if PW_GEMM != "split16":
        return 0
    return int(_lib.load().ct_mhct_core_fwd_norm_amax_len(B, H, C, N, len(W), _lib.int_array(W)))


def _norm_target_args(target, B, HC, N, n_len, device):
    """(the [B, HC, N] result view, its ct_bn_fwd_item, the maxima pointer, the op's own maxima buffer or None)."""
    bn = target.bn
    assert bn.num_features == HC
    if target.y is None:
        y = view = torch.empty(B, HC, N, device=device, dtype=torch.float32)
        ybs, y_ptr = 0, _ptr(y)
        own = torch.empty(n_len, device=device, dtype=torch.float32) if n_len else None
        am_ptr = _ptr(own)
    else:
        y, own = target.y, None
        assert y.dim() == 3 and y.is_contiguous() and y.size(0) == B and y.size(2) == N and target.c0 + HC <= y.size(1)
        view = y[:, target.c0:target.c0 + HC]
        ybs, y_ptr = y.size(1) * N, _ptr(y) + target.c0 * N * 4
        am_ptr = None
        if target.amax is not None and n_len:
            assert target.a0 + n_len <= target.amax.numel()
            am_ptr = _ptr(target.amax) + 4 * target.a0
    item = _bn_eval_item(bn, None, 0, y_ptr, ybs, target.relu)
    return view, item, am_ptr, own


def _norm_target_done(target, view, own):
    if own is not None:
        view._ct_amax = (own, view._version)        # (1-D on purpose: partials of ONE maximum, as pw_bn_eval's)
    target.out = view
    return view


def slice_keys_norm(keys, grid, pts_padding, tensor_size, heads, dim, target):
    """relu?(bn(Slice(keys, grid))) in one launch (ct_slice_fwd_norm) into `target` (a NormTarget); the caller checked
    slice_norm_eligible(target.bn, keys, grid).  Returns the result (a channel range of target.y, or a dense tensor that carries
    the partial maxima of its values for the pointwise GEMM that reads it next)."""
    W = sizes_of(tensor_size, dim)
    _dev(keys, grid, pts_padding)
    keys, grid = _f32c(keys), _f32c(grid)
    B, HC = grid.shape[:2]
    N = keys.shape[-1]
    assert HC % heads == 0 and keys.shape == (B, heads * dim, N) and list(grid.shape[2:]) == list(W)
    C = HC // heads
    padt, pad_code = _pad_args(pts_padding, B, N)
    view, item, am_ptr, own = _norm_target_args(target, B, HC, N, slice_norm_amax_len(B, heads, C, N, W), grid.device)
    arr = _bn_fwd_table([item])
    lib = _lib.load()
    with _on(grid.device):
        _lib.check(lib.ct_slice_fwd_norm(_ptr(keys), _ptr(grid), _ptr(padt), pad_code, _at(arr, 0), am_ptr,
                                         B, heads, C, N, dim, _lib.int_array(W), _stream()), "ct_slice_fwd_norm")
    return _norm_target_done(target, view, own)


def mhct_core_norm(keys, features, pts_padding, weight, bias, tensor_size, heads, dim, target):
    """(relu?(bn(sliced features)), occupancy count) of one MHCT core in one launch (ct_mhct_core_fwd_norm) into `target`; the
    caller checked mhct_core_supported(...) and slice_norm_eligible(target.bn, keys, features, weight, bias).  Forward only:
    nothing is saved.  The launch runs on the workspace mhct_core's launches of this shape and stream use, so a cluster that
    gave up waiting shows where theirs do: mhct_core_check reads (and re-initialises) that workspace's status word."""
    W = sizes_of(tensor_size, dim)
    _dev(keys, features, pts_padding, weight, bias)
    keys, features, weight = _f32c(keys), _f32c(features), _f32c(weight)
    bias = _f32c(bias) if bias is not None else None
    B, HC, N = features.shape
    C = HC // heads
    assert keys.shape == (B, heads * dim, N) and weight.shape[0] == HC and weight.shape[1] == C
    padt, pad_code = _pad_args(pts_padding, B, N)
    dev = features.device
    view, item, am_ptr, own = _norm_target_args(target, B, HC, N, mhct_core_norm_amax_len(B, heads, C, N, W), dev)
    arr = _bn_fwd_table([item])
    occ = torch.empty((), device=dev, dtype=torch.int64)
    ws = mhct_core_workspace(dev, B, heads, C, N, W)
    lib = _lib.load()
    with _on(dev):
        _lib.check(lib.ct_mhct_core_fwd_norm(_ptr(keys), _ptr(features), _ptr(padt), pad_code, _ptr(weight), _ptr(bias), _at(arr, 0),
                                             am_ptr, None, None, _ptr(occ), _ptr(ws), ws.numel(), B, heads, C, N, dim,
                                             _lib.int_array(W), _stream()), "ct_mhct_core_fwd_norm")
    return _norm_target_done(target, view, own), occ


# ---------------------------------------------------------------------------
# eval-mode norms of the grouped-conv Res blocks in the convolution's write-out (ct_gconv_fwd_norm)
# ---------------------------------------------------------------------------
# Res2DBlock / Res3DBlock / Basic2DBlock / Basic3DBlock (layers/grouped_conv.py) in eval mode: relu?(bn(conv(x)) + bn'?(skip)) in
# the stores of the convolution kernel that holds the value, so a Res block costs two convolution launches and the skip GEMM and
# no norm, add or ReLU pass.  The results carry the bits of ct_gconv_fwd, ct_bn_eval_group_fwd, torch.add and torch.relu in a row;
# where the shape runs on a kernel without the write-out (four-channel groups, the one-position form) exactly that sequence is
# composed instead, so those shapes leave the torch norms too.  Forward only, consulted only where BN_EVAL already routes to
# the eval kernels.  "0": the modules' own path (A/B runs).
GCONV_NORM = os.environ.get("CLOUDCT_GCONV_NORM", "1") != "0"
_GCONV_BN_TYPES = (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d, torch.nn.SyncBatchNorm)
_gconv_norm_supported = {}


def _gconv_bn_ok(bn, C, device):
    return (type(bn) in _GCONV_BN_TYPES and not bn.training and bn.affine and bn.track_running_stats
            and bn.running_mean is not None and bn.running_var is not None and bn.num_features == C
            and bn.weight.dtype == torch.float32 and bn.running_mean.dtype == torch.float32
            and bn.weight.device == device and bn.running_mean.device == device)


def gconv_norm_eligible(conv, bn, x, skip=None, skip_bn=None):
    """True when relu?(bn(conv(x)) + skip_bn?(skip)) can run as gconv_bn_eval: ops.BN_EVAL and ops.GCONV_NORM; `conv` a grouped 3^d
    convolution the MFMA kernels take for x (layers.gconv._eligible: CUDA fp32, kernel 3, stride 1, padding 1); every norm an
    nn.BatchNorm2d / nn.BatchNorm3d / nn.SyncBatchNorm (exactly) in eval mode, affine, with running statistics over the
    convolution's output channels, fp32, on x's device; `skip` a CUDA fp32 tensor of the output's shape; and nothing for autograd
    to record."""
    if not (BN_EVAL and GCONV_NORM and isinstance(conv, torch.nn.modules.conv._ConvNd) and x.is_cuda and x.dim() in (4, 5)
            and x.dim() - 2 == len(conv.kernel_size) and x.size(1) == conv.in_channels):
        return False
    from .layers.gconv import _eligible
    if not _eligible(conv, x):
        return False
    C = conv.out_channels
    if not _gconv_bn_ok(bn, C, x.device) or (skip_bn is not None and (skip is None or not _gconv_bn_ok(skip_bn, C, x.device))):
        return False
    if skip is not None and not (skip.is_cuda and skip.dtype == torch.float32 and skip.device == x.device
                                 and tuple(skip.shape) == (x.size(0), C) + tuple(x.shape[2:])):
        return False
    N = 1
    for w in x.shape[2:]:
        N *= int(w)
    key = (x.size(0), C, N)
    ok = _bn_eval_supported.get(key)
    if ok is None:
        ok = _bn_eval_supported[key] = bool(_lib.load().ct_bn_eval_supported(*key))
    watched = [x, conv.weight, conv.bias, bn.weight, bn.bias, skip]
    if skip_bn is not None:
        watched += [skip_bn.weight, skip_bn.bias]
    return ok and _records_nothing(*watched)


def _gconv_norm_struct(bn):
    """(ct_gconv_norm, the tensors it points to)"""
    keep = (_f32c(bn.weight.detach()), _f32c(bn.bias.detach()), _f32c(bn.running_mean), _f32c(bn.running_var))
    return _lib.GconvNorm(_ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]), float(bn.eps)), keep


def gconv_bn_eval(x, conv, bn, relu, skip=None, skip_bn=None):
    """relu?(bn(conv(x)) + skip_bn?(skip)) of a grouped 3^d convolution and eval-mode norms; the caller checked
    gconv_norm_eligible(conv, bn, x, skip, skip_bn).  One ct_gconv_fwd_norm launch where ct_gconv_fwd_norm_supported takes the
    shape and the tensors lie on the 16-byte grid; else the sequence whose bits that launch carries: ct_gconv_fwd, one
    ct_bn_eval_group_fwd (both norms), torch add and ReLU."""
    _dev(x, skip)
    x, w = _f32c(x), _f32c(conv.weight.detach())
    b = _f32c(conv.bias.detach()) if conv.bias is not None else None
    skip = _f32c(skip) if skip is not None else None
    B, G = x.size(0), conv.groups
    Cin, Cout = conv.in_channels // G, conv.out_channels // G
    W = list(x.shape[2:])
    nd = len(W)
    lib = _lib.load()
    _prec.conv_push(lib)     # the convolution's precision (precision.py): an eval Res block is in one mode throughout
    key = (B, G, Cin, Cout, tuple(W))
    fused = _gconv_norm_supported.get(key)
    if fused is None:
        fused = _gconv_norm_supported[key] = bool(lib.ct_gconv_fwd_norm_supported(B, G, Cin, Cout, nd, _lib.int_array(W)))
    y = torch.empty(B, G * Cout, *W, device=x.device, dtype=torch.float32)
    if fused and all(t is None or t.data_ptr() % 16 == 0 for t in (x, w, y, skip)):
        norm, keep = _gconv_norm_struct(bn)
        snorm, skeep = _gconv_norm_struct(skip_bn) if skip_bn is not None else (None, None)
        with _on(x.device):
            _lib.check(lib.ct_gconv_fwd_norm(_ptr(x), _ptr(w), _ptr(b), ctypes.addressof(norm), _ptr(skip),
                                             ctypes.addressof(snorm) if snorm is not None else None, int(bool(relu)), _ptr(y),
                                             B, G, Cin, Cout, nd, _lib.int_array(W), _stream()), "ct_gconv_fwd_norm")
        return y
    # the composed sequence: four-channel groups, the one-position form, tensors off the 16-byte grid
    N = y[0, 0].numel()
    C = G * Cout
    with _on(x.device):
        _lib.check(lib.ct_gconv_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), B, G, Cin, Cout, nd, _lib.int_array(W), _stream()),
                   "ct_gconv_fwd")
        out = torch.empty_like(y)
        items = [_bn_eval_item(bn, _ptr(y), 0, _ptr(out), 0, relu and skip is None)]
        t = skip
        if skip_bn is not None:
            t = torch.empty_like(skip)
            items.append(_bn_eval_item(skip_bn, _ptr(skip), 0, _ptr(t), 0, False))
        _bn_eval_group(items, B, N)
    if t is not None:
        out.add_(t)
        if relu:
            torch.relu_(out)
    return out
