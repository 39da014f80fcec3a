"""What tests/test_gconv_precision_cpu.py and tests/test_gconv_precision_gpu.py share: the shapes, every pass written as a
forward convolution, and the documented error bound of CT_GCONV_PRECISION_HIGH (include/cloudct.h), term by term in float64.
Plain helpers, importable without a GPU.  Inputs and the fp32-accumulation allowance are those of
tests/test_gconv_families_gpu.py (imported, never changed)."""
import torch
import torch.nn.functional as Fn

from tests.test_gconv_families_gpu import bound as fp32_bound, inputs

# (B, G, Cin, Cout, W): the smallest shapes of the families table that reach each branch of the two kernels
QUAD = [
    (2, 3, 16, 16, (32, 32)),        # plain quad
    (1, 3, 16, 48, (8, 8)),          # msplit, three 16-row blocks
    (1, 2, 16, 16, (8, 256)),        # 1024 threads
    (1, 1, 16, 16, (101, 32)),       # ragged tile height
    (1, 2, 16, 16, (16, 16, 16)),    # 3D depth tiles with halo
    (1, 2, 20, 24, (8, 8)),          # Cin, Cout not multiples of 16: zero operands in the k slots past Cin, a ragged row block
]
KSPLIT = [
    (1, 2, 64, 64, (8, 8, 8)),       # one tile, DMA
    (1, 2, 64, 64, (16, 16, 16)),    # tiled
    (3, 2, 48, 40, (4, 8, 8)),       # element staging, ragged channels
    (1, 2, 32, 16, (40, 32)),        # items 2
    (1, 1, 64, 64, (64, 64)),        # items 4, tiled
]
FWD_SHAPES = QUAD + KSPLIT
BWD_SHAPES = [(2, 3, 16, 16, (32, 32)), (1, 3, 48, 16, (8, 8)), (3, 2, 48, 40, (4, 8, 8)), (1, 2, 64, 64, (16, 16, 16)),
              (1, 2, 16, 32, (40, 32))]
# forward shapes whose backward-data is NOT covered: as a convolution of g_y it has 48 input channels per group, so it is a K-split
# call, and its 8 x 8 tile is one span of 16 quads — measured slower than fp32 (8^2 and 4^3 tiles), fp32 kept
BWD_FP32 = [(1, 3, 16, 48, (8, 8))]
# what stays fp32 in every mode (rows of the families table): four-channel groups, the one-position form, dense 2^d
UNCOVERED = [(2, 4, 4, 4, (16, 16)), (1, 3, 4, 4, (5, 7, 16)), (1, 1, 5, 7, (9, 11)), (1, 2, 8, 8, (9, 18)), (3, 2, 5, 7, (2, 2)),
             (2, 3, 40, 24, (2, 2, 2))]


def shape_id(s):
    return "B%d_G%d_%dto%d_%s" % (s[0], s[1], s[2], s[3], "x".join(map(str, s[4])))


def as_forward(shape, ops, bwd, scale=1.0):
    """(x, w, bias | None, channels in, channels out) of the pass written as a forward convolution, float64: backward-data is
    the convolution of g_y with the bank transposed within each group and flipped along the taps, without a bias"""
    B, G, Cin, Cout, W = shape
    d = len(W)
    w = ops["w"].double() * scale
    if not bwd:
        return ops["x"].double() * scale, w, ops["b"].double(), Cin, Cout
    wt = w.reshape(G, Cout, Cin, 3 ** d).transpose(1, 2).flip(-1).reshape(G * Cin, Cout, *([3] * d))
    return ops["g_y"].double() * scale, wt.contiguous(), None, Cout, Cin


def conv(x, w, b, G):
    return (Fn.conv3d if x.dim() == 5 else Fn.conv2d)(x, w, b, padding=1, groups=G)


def high_bound(shape, x, w, b, cin, cout):
    """(float64 reference, the bound of include/cloudct.h) for the forward-form operands of as_forward:
    (2^-10 + 2^-22) sum|w x| + 2^-37 (M_w sum|x| + M_x sum|w|) + the fp32 accumulation term of the families table, with
    M_w the maximum of the output channel's weight row and M_x the maximum of x over the output's (batch, group) slab; the sums
    run over the taps inside the volume (a padded zero has no error)."""
    B, G = shape[0], shape[1]
    sp = x.shape[2:]
    ones = [1] * len(sp)
    ref = conv(x, w, b, G)
    ax, aw = x.abs(), w.abs()
    s_wx = conv(ax, aw, None, G)
    m_w = aw.reshape(G * cout, -1).amax(1).reshape(1, G * cout, *ones)
    m_x = ax.reshape(B, G, -1).amax(2).reshape(B, G, 1, *ones).expand(B, G, cin, *sp).reshape(B, G * cin, *sp)
    s_x = conv(ax, torch.ones_like(aw), None, G)                      # sum |x| over the output's receptive field
    mx_sw = conv(m_x.contiguous(), aw, None, G)                       # M_x sum |w|
    K = cin * 3 ** len(sp) + (1 if b is not None else 0)
    mag = s_wx + (b.abs().reshape(1, -1, *ones) if b is not None else 0)
    return ref, (2.0 ** -10 + 2.0 ** -22) * s_wx + 2.0 ** -37 * (m_w * s_x + mx_sw) + fp32_bound(mag, K)


def quantise(v, amax, bits):
    """v rounded as the one-term kernels round it, in float64: a `bits`-bit significand with f16's exponent range under the
    power-of-two scale s with s * amax in [2^13, 2^14) (amax broadcastable to v; s = 1 where amax is 0)"""
    e = torch.floor(torch.log2(torch.where(amax > 0, amax, torch.ones_like(amax))))
    s = torch.where(amax > 0, 2.0 ** (13 - e), torch.ones_like(amax))
    t = v * s
    ex = torch.floor(torch.log2(torch.where(t != 0, t.abs(), torch.ones_like(t))))
    q = 2.0 ** torch.clamp(ex - (bits - 1), min=-24.0)                # f16: subnormals below 2^-14 keep the spacing 2^-24
    return torch.round(t / q) * q / s


def emulate(shape, x, w, b, cin, cout, bits):
    """the convolution of the operands rounded to `bits` bits under per-slab / per-row scales, summed in float64"""
    B, G = shape[0], shape[1]
    sp = x.shape[2:]
    ones = [1] * len(sp)
    m_x = x.abs().reshape(B, G, -1).amax(2).reshape(B, G, 1, *ones).expand(B, G, cin, *sp).reshape(B, G * cin, *sp)
    m_w = w.abs().reshape(G * cout, -1).amax(1).reshape(G * cout, 1, *ones)
    return conv(quantise(x, m_x, bits), quantise(w, m_w.expand_as(w), bits), b, G)


def scaled_ops(shape):
    return inputs(shape, "scaled")
