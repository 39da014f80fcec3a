"""MI355X-native Multi-Headed Cloud Transform (Splat / Slice / multihead_ct*).

Python + PyTorch-ROCm host code over hand-written HIP kernels (libcloudct.so,
C ABI in include/cloudct.h).  No CPU fallback: ops raise on non-HIP tensors.
"""
from . import _lib  # noqa: F401
from .determinism import set_deterministic, is_deterministic, deterministic  # noqa: F401
from .graphs import GraphedForward  # noqa: F401
from .norms import freeze_norms, unfreeze_norms, norms_frozen  # noqa: F401
from .precision import set_matmul_precision, get_matmul_precision, matmul_precision  # noqa: F401
from .precision import set_conv_precision, get_conv_precision, conv_precision  # noqa: F401

__all__ = ["_lib", "set_deterministic", "is_deterministic", "deterministic", "freeze_norms", "unfreeze_norms", "norms_frozen",
           "set_matmul_precision", "get_matmul_precision", "matmul_precision",
           "set_conv_precision", "get_conv_precision", "conv_precision", "GraphedForward"]
