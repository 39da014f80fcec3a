"""Precision of the pointwise-convolution GEMMs (include/cloudct.h: ct_set_pw_precision).

    set_matmul_precision("highest" | "high" | "medium" | None)
    get_matmul_precision()                    the effective name, now
    with matmul_precision("high"): ...        a scope; the previous mode comes back on exit

"highest" (the default): three f16 MFMA terms per product, 22-bit operands — fp32 accuracy.  "high": ONE f16 term per
operand, 11-bit significands with fp32 accumulation — the precision of TF32, which gfx950 has no matrix instruction for, so
torch.set_float32_matmul_precision changes nothing about an fp32 GEMM on this machine.  "medium" is served by the "high"
kernels (a request for less may be answered with more).  None follows torch.get_float32_matmul_precision() at call time.

CLOUDCT_PW_PRECISION=highest|high|medium in the environment sets the initial mode; unset, or anything else, means "highest"
— not None: a process that never asks stays exactly as it is, even if it sets torch's flag.  The mode is a permission, not an
order: under CLOUDCT_PW_GEMM=lib, for the shapes ops.pw_eligible sends to torch.bmm and for the products the library keeps on
three terms it changes nothing.

The mode is process-wide like the library's switch, and the ops push the effective mode into the library before their
workspace query and launch (`push`).  A layer's three products share the FORWARD's precision: the autograd Functions remember
the forward's mode and run their backward products under the library's per-thread override (`forced`), on whichever thread
autograd runs them — a `with` scope around the forward alone still gives a consistent layer.

HIP graphs: the mode is read when a launch is RECORDED.  A replay runs the kernels that were captured, whatever the mode is
by then; capture again to change it.

Precision of the grouped 3^d convolutions (include/cloudct.h: ct_set_gconv_precision), the same pattern and an
INDEPENDENT mode, like torch's two flags:

    set_conv_precision("highest" | "high" | "medium" | None)
    get_conv_precision()
    with conv_precision("high"): ...

"highest" (the default): fp32 MFMA.  "high": the quad and K-split kernels of ct_gconv_fwd / ct_gconv_bwd_data / ct_gconv_fwd_norm
multiply one f16 term per operand (11-bit significands, fp32 accumulation); "medium" is served by the same kernels.  None follows
torch.backends.cudnn.allow_tf32 at call time.  CLOUDCT_GCONV_PRECISION=highest|high|medium sets the initial mode; unset, or anything
else, means "highest" — not None: torch's flag defaults to True, and a process that never asks stays exactly as it is.  A layer's
backward-data runs in its forward's mode (`conv_forced`); the weight gradient is fp32 in every mode.
"""
import contextlib
import os

import torch

from . import _lib

HIGHEST, HIGH = 0, 1          # CT_PW_PRECISION_HIGHEST / _HIGH
_NAMES = ("highest", "high", "medium")


def _from_env():
    v = os.environ.get("CLOUDCT_PW_PRECISION")
    return v if v in _NAMES else "highest"


_mode = _from_env()


def set_matmul_precision(mode):
    """"highest" / "high" / "medium": that mode whatever torch says; None: follow torch.get_float32_matmul_precision() at call time."""
    global _mode
    if mode is not None and not isinstance(mode, str):
        raise TypeError("set_matmul_precision expects 'highest', 'high', 'medium' or None, got %r" % (mode,))
    if mode is not None and mode not in _NAMES:
        raise ValueError("set_matmul_precision expects 'highest', 'high', 'medium' or None, got %r" % (mode,))
    _mode = mode
    if _lib._lib is not None:          # keep a loaded library in step (direct ABI callers; a scope that just ended)
        push(_lib._lib)


def get_mode():
    """What set_matmul_precision was given (a name or None)."""
    return _mode


def get_matmul_precision():
    return torch.get_float32_matmul_precision() if _mode is None else _mode


def code():
    """The effective mode as the library's constant."""
    return HIGHEST if get_matmul_precision() == "highest" else HIGH


@contextlib.contextmanager
def matmul_precision(mode="high"):
    prev = _mode
    set_matmul_precision(mode)
    try:
        yield
    finally:
        set_matmul_precision(prev)


def push(lib=None):
    """Set the library's switch to the effective mode; returns its constant.  Called by the ops ahead of their workspace queries and launches."""
    p = code()
    (lib or _lib.load()).ct_set_pw_precision(p)
    return p


@contextlib.contextmanager
def forced(p, lib=None):
    """Mode `p` (a library constant) for the entry points THIS thread calls inside the scope, whatever the process-wide switch
    says: how a backward runs its products in its forward's precision."""
    lib = lib or _lib.load()
    lib.ct_pw_precision_override(p)
    try:
        yield
    finally:
        lib.ct_pw_precision_override(-1)


# ---- the grouped convolutions' mode ----

def _conv_from_env():
    v = os.environ.get("CLOUDCT_GCONV_PRECISION")
    return v if v in _NAMES else "highest"


_conv_mode = _conv_from_env()


def set_conv_precision(mode):
    """"highest" / "high" / "medium": that mode whatever torch says; None: follow torch.backends.cudnn.allow_tf32 at call time."""
    global _conv_mode
    if mode is not None and not isinstance(mode, str):
        raise TypeError("set_conv_precision expects 'highest', 'high', 'medium' or None, got %r" % (mode,))
    if mode is not None and mode not in _NAMES:
        raise ValueError("set_conv_precision expects 'highest', 'high', 'medium' or None, got %r" % (mode,))
    _conv_mode = mode
    if _lib._lib is not None:          # keep a loaded library in step (direct ABI callers; a scope that just ended)
        conv_push(_lib._lib)


def get_conv_mode():
    """What set_conv_precision was given (a name or None)."""
    return _conv_mode


def get_conv_precision():
    if _conv_mode is None:
        return "high" if torch.backends.cudnn.allow_tf32 else "highest"
    return _conv_mode


def conv_code():
    """The effective mode as the library's constant (CT_GCONV_PRECISION_HIGHEST / _HIGH)."""
    return HIGHEST if get_conv_precision() == "highest" else HIGH


@contextlib.contextmanager
def conv_precision(mode="high"):
    prev = _conv_mode
    set_conv_precision(mode)
    try:
        yield
    finally:
        set_conv_precision(prev)


def conv_push(lib=None):
    """Set the library's switch to the effective mode; returns its constant.  Called by the ops ahead of their launches."""
    p = conv_code()
    (lib or _lib.load()).ct_set_gconv_precision(p)
    return p


@contextlib.contextmanager
def conv_forced(p, lib=None):
    """Mode `p` (a library constant) for the entry points THIS thread calls inside the scope, whatever the process-wide switch
    says: how a backward-data runs in its forward's precision."""
    lib = lib or _lib.load()
    lib.ct_gconv_precision_override(p)
    try:
        yield
    finally:
        lib.ct_gconv_precision_override(-1)
