"""Deterministic mode: run-to-run bit-equal gradients (include/cloudct.h: ct_set_deterministic).

    set_deterministic(True | False | None)    None (the default): follow torch.are_deterministic_algorithms_enabled()
    is_deterministic()                        the effective mode, now
    with deterministic(on=True): ...          a scope; the previous mode comes back on exit

CLOUDCT_DETERMINISTIC=1|0 in the environment sets the initial mode (anything else, or unset: None), so that bench.py and the
tools can be compared with and without it unedited.  The mode is process-wide like the library's switch — autograd calls the
backward entry points from threads of its own — and the ops push the effective mode into the library before they launch
(`push`).  An op that has no reproducible form raises a RuntimeError in the wording torch uses, or warns under torch's
warn_only (`refuse`); nothing stays non-deterministic silently.
"""
import contextlib
import os
import warnings

import torch

from . import _lib


def _from_env():
    v = os.environ.get("CLOUDCT_DETERMINISTIC")
    return True if v == "1" else False if v == "0" else None


_mode = _from_env()


def set_deterministic(mode):
    """True / False: on / off whatever torch says; None: follow torch.use_deterministic_algorithms at call time."""
    global _mode
    if mode is not None and not isinstance(mode, bool):
        raise TypeError("set_deterministic expects True, False or None, got %r" % (mode,))
    _mode = mode
    if _lib._lib is not None:          # keep a loaded library in step (direct ABI callers; a scope that just ended)
        push(_lib._lib)


def get_mode():
    """What set_deterministic was given (True, False or None)."""
    return _mode


def is_deterministic():
    return torch.are_deterministic_algorithms_enabled() if _mode is None else _mode


@contextlib.contextmanager
def deterministic(on=True):
    prev = _mode
    set_deterministic(on)
    try:
        yield
    finally:
        set_deterministic(prev)


def push(lib=None):
    """Set the library's switch to the effective mode; returns it.  Called by the ops ahead of their workspace queries and launches."""
    on = is_deterministic()
    (lib or _lib.load()).ct_set_deterministic(1 if on else 0)
    return on


def refuse(op):
    """`op` has no deterministic implementation: raise, or warn when torch's warn_only is set (the caller then runs its
    ordinary form under the library's per-thread override: `relaxed`, `call`)."""
    msg = ("%s does not have a deterministic implementation, but you set 'cloud_transformers_amd.set_deterministic(True)' or "
           "'torch.use_deterministic_algorithms(True)'. You can turn off determinism just for this operation, or you can use the "
           "'warn_only=True' option of torch.use_deterministic_algorithms, if that's acceptable for your application." % op)
    if torch.is_deterministic_algorithms_warn_only_enabled():
        warnings.warn(msg, UserWarning, stacklevel=3)
        return
    raise RuntimeError(msg)


@contextlib.contextmanager
def relaxed(lib=None):
    """The mode off for the entry points THIS thread calls inside the scope (after `refuse` only warned): the library's
    per-thread override, so a backward running on another thread keeps the mode between its workspace query and its launch."""
    lib = lib or _lib.load()
    lib.ct_deterministic_override(0)
    try:
        yield
    finally:
        lib.ct_deterministic_override(-1)


def call(lib, name, what, *args):
    """status of lib.<name>(*args); a CT_EPRECOND that is the mode's refusal raises or warns through `refuse(what)` and, after
    a warning, the call is made again in its ordinary form"""
    fn = getattr(lib, name)
    rc = fn(*args)
    if rc == _lib.CT_EPRECOND and lib.ct_get_deterministic():
        refuse(what)
        with relaxed(lib):
            rc = fn(*args)
    return rc
