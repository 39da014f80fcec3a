"""Precision mode of the grouped convolutions, the host side: the four ABI symbols, the Python switch and its three sources
(explicit, torch's cudnn flag, the environment), its independence of the matmul mode, the planner's answer
ct_gconv_precision_covers, the scope around Trainer.fit — and that the documented bound (include/cloudct.h) means something: an
11-bit emulation stays inside it, an 8-bit one does not.  No GPU: the switch is host state that no kernel reads."""
import os
import re
import subprocess
import sys
import threading

import pytest
import torch

from tests import gconv_precision_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def clean_mode():
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import _lib, precision
    prev, prev_mm, prev_torch = precision.get_conv_mode(), precision.get_mode(), torch.backends.cudnn.allow_tf32
    lib = _lib.load()
    before, before_pw = lib.ct_get_gconv_precision(), lib.ct_get_pw_precision()
    yield ct
    precision.set_conv_precision(prev)
    precision.set_matmul_precision(prev_mm)
    torch.backends.cudnn.allow_tf32 = prev_torch
    lib.ct_gconv_precision_override(-1)
    lib.ct_set_gconv_precision(before)
    lib.ct_set_pw_precision(before_pw)


def test_symbols_are_declared_and_exported():
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import _lib
    text = open(os.path.join(ROOT, "include", "cloudct.h")).read()
    assert re.search(r"void\s+ct_set_gconv_precision\(int p\);", text) and re.search(r"int\s+ct_get_gconv_precision\(void\);", text)
    assert re.search(r"void\s+ct_gconv_precision_override\(int p\);", text)
    assert re.search(r"int\s+ct_gconv_precision_covers\(int pass, int B, int groups, int Cin, int Cout, int dim, const int\* W\);", text)
    assert re.search(r"#define CT_GCONV_PRECISION_HIGHEST\s+0\b", text) and re.search(r"#define CT_GCONV_PRECISION_HIGH\s+1\b", text)
    assert int(re.search(r"#define CT_ABI_VERSION\s+(\d+)", text).group(1)) == 3 and _lib.ABI_VERSION == 3
    lib = _lib.load()
    assert lib.ct_abi_version() == 3
    for name in ("ct_set_gconv_precision", "ct_get_gconv_precision", "ct_gconv_precision_override", "ct_gconv_precision_covers"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    for name in ("set_conv_precision", "get_conv_precision", "conv_precision"):
        assert name in ct.__all__ and hasattr(ct, name)


def test_default_is_highest_and_other_values_map_to_it(clean_mode):
    from cloud_transformers_amd import _lib
    code = ("from cloud_transformers_amd import _lib; print(_lib.load().ct_get_gconv_precision())")
    env = {k: v for k, v in os.environ.items() if k != "CLOUDCT_GCONV_PRECISION"}
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == "0"
    lib = _lib.load()
    lib.ct_set_gconv_precision(1)
    assert lib.ct_get_gconv_precision() == 1
    lib.ct_set_gconv_precision(0)
    assert lib.ct_get_gconv_precision() == 0
    for other in (2, 7, -3):
        lib.ct_set_gconv_precision(1)
        lib.ct_set_gconv_precision(other)
        assert lib.ct_get_gconv_precision() == 0


def test_override_belongs_to_the_calling_thread(clean_mode):
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    seen = []

    def other_thread():
        t = threading.Thread(target=lambda: seen.append(lib.ct_get_gconv_precision()))
        t.start()
        t.join()

    lib.ct_set_gconv_precision(0)
    lib.ct_gconv_precision_override(1)
    assert lib.ct_get_gconv_precision() == 1
    other_thread()
    assert seen == [0]                                   # the other thread keeps the process-wide switch
    lib.ct_gconv_precision_override(7)                   # another value overrides with HIGHEST
    lib.ct_set_gconv_precision(1)
    assert lib.ct_get_gconv_precision() == 0
    other_thread()
    assert seen == [0, 1]
    lib.ct_gconv_precision_override(-1)
    assert lib.ct_get_gconv_precision() == 1


def test_the_four_values_and_the_refusals(clean_mode):
    ct = clean_mode
    torch.backends.cudnn.allow_tf32 = False
    for name in ("highest", "high", "medium"):
        ct.set_conv_precision(name)
        assert ct.get_conv_precision() == name
    ct.set_conv_precision(None)
    assert ct.get_conv_precision() == "highest"
    for bad in ("low", "HIGH", "", "tf32"):
        with pytest.raises(ValueError):
            ct.set_conv_precision(bad)
    for bad in (1, True, 0.5, b"high", ["high"]):
        with pytest.raises(TypeError):
            ct.set_conv_precision(bad)
    assert ct.get_conv_precision() == "highest"          # a refused value changes nothing


def test_none_follows_the_cudnn_flag(clean_mode):
    ct = clean_mode
    from cloud_transformers_amd import precision
    ct.set_conv_precision(None)
    torch.backends.cudnn.allow_tf32 = True
    assert ct.get_conv_precision() == "high" and precision.conv_code() == 1
    torch.backends.cudnn.allow_tf32 = False
    assert ct.get_conv_precision() == "highest" and precision.conv_code() == 0
    torch.backends.cudnn.allow_tf32 = True
    ct.set_conv_precision("highest")                     # explicit beats torch's flag
    assert ct.get_conv_precision() == "highest"


def test_push_forced_and_medium_is_served_by_high(clean_mode):
    ct = clean_mode
    from cloud_transformers_amd import _lib, precision
    lib = _lib.load()
    for name, want in (("highest", 0), ("high", 1), ("medium", 1)):
        ct.set_conv_precision(name)
        assert precision.conv_code() == want and precision.conv_push() == want and lib.ct_get_gconv_precision() == want
    ct.set_conv_precision("highest")
    with precision.conv_forced(precision.HIGH):
        assert lib.ct_get_gconv_precision() == 1
    assert lib.ct_get_gconv_precision() == 0
    with ct.conv_precision("high"):
        assert ct.get_conv_precision() == "high" and lib.ct_get_gconv_precision() == 1
        with pytest.raises(KeyError):
            with ct.conv_precision("highest"):
                raise KeyError("leaves the scope by an exception")
        assert ct.get_conv_precision() == "high"
    assert ct.get_conv_precision() == "highest" and lib.ct_get_gconv_precision() == 0


def test_matmul_and_conv_modes_do_not_touch_each_other(clean_mode):
    ct = clean_mode
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    ct.set_matmul_precision("highest")
    ct.set_conv_precision("highest")
    with ct.conv_precision("high"):
        assert ct.get_matmul_precision() == "highest" and lib.ct_get_pw_precision() == 0 and lib.ct_get_gconv_precision() == 1
    with ct.matmul_precision("high"):
        assert ct.get_conv_precision() == "highest" and lib.ct_get_gconv_precision() == 0 and lib.ct_get_pw_precision() == 1
    assert (lib.ct_get_pw_precision(), lib.ct_get_gconv_precision()) == (0, 0)


@pytest.mark.parametrize("value,expect", [("high", "high high"), ("medium", "medium medium"), (None, "highest highest"),
                                          ("garbage", "highest highest")])
def test_environment_sets_the_initial_mode(value, expect):
    env = {k: v for k, v in os.environ.items() if k not in ("CLOUDCT_GCONV_PRECISION", "CLOUDCT_PW_PRECISION")}
    if value is not None:
        env["CLOUDCT_GCONV_PRECISION"] = value
    # torch's flag is True by default: a process that never asks this package stays on "highest"
    code = ("import torch; assert torch.backends.cudnn.allow_tf32; import cloud_transformers_amd as ct; "
            "from cloud_transformers_amd import precision as p; print(p.get_conv_mode(), ct.get_conv_precision()); "
            "assert ct.get_matmul_precision() == 'highest'")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == expect


def test_covers_is_the_planners_answer(clean_mode):
    from cloud_transformers_amd import _lib
    lib = _lib.load()

    def covers(p, s):
        return lib.ct_gconv_precision_covers(p, s[0], s[1], s[2], s[3], len(s[4]), _lib.int_array(list(s[4])))

    for mode in (0, 1):                                  # independent of the current mode
        lib.ct_set_gconv_precision(mode)
        for s in C.FWD_SHAPES:
            assert covers(0, s) == 1 and covers(1, s) == (0 if s in C.BWD_FP32 else 1), s
        for s in C.BWD_SHAPES:
            assert covers(1, s) == 1, s
        for s in C.UNCOVERED:
            assert covers(0, s) == 0 and covers(1, s) == 0, s
    assert covers(2, C.FWD_SHAPES[0]) == 0 and covers(0, (0, 1, 16, 16, (8, 8))) == 0


@pytest.fixture(scope="module")
def emulated():
    """shape, pass -> (worst |err| / bound of the 11-bit emulation, of the 8-bit one), on the `scaled` inputs"""
    out = {}
    for bwd, shapes in ((False, C.FWD_SHAPES), (True, C.BWD_SHAPES)):
        for s in shapes:
            x, w, b, cin, cout = C.as_forward(s, C.scaled_ops(s), bwd)
            ref, bnd = C.high_bound(s, x, w, b, cin, cout)
            out[(s, bwd)] = tuple(float(((C.emulate(s, x, w, b, cin, cout, bits) - ref).abs() / bnd).max()) for bits in (11, 8))
    return out


def test_eleven_bits_stay_inside_the_bound(emulated):
    for key, (r11, _) in emulated.items():
        print(C.shape_id(key[0]), "bwd" if key[1] else "fwd", "11-bit err/bound %.3f" % r11)
        assert r11 <= 1.0, key


def test_eight_bits_do_not(emulated):
    worst = max(r8 for _, r8 in emulated.values())
    print("8-bit worst err/bound %.3f" % worst)
    assert worst > 1.0


def test_trainer_config_switch_scopes_the_fit(clean_mode):
    """`train.conv_precision: high` sets the mode for Trainer.fit and gives the previous mode back afterwards; a bad value raises
    before _fit runs."""
    ct = clean_mode
    from cloud_transformers_amd import harness as H
    seen = []

    class Stub:
        cfg = {"train": {"conv_precision": "high"}}

        def _fit(self, max_iters, hip_graph, log_each):
            seen.append((ct.get_conv_precision(), ct.get_matmul_precision()))
            return [0.0]

    ct.set_conv_precision("highest")
    ct.set_matmul_precision("highest")
    assert H.Trainer.fit(Stub(), max_iters=1) == [0.0] and seen == [("high", "highest")]
    assert ct.get_conv_precision() == "highest"
    Stub.cfg = {"train": {}}
    H.Trainer.fit(Stub(), max_iters=1)
    assert seen[-1] == ("highest", "highest")
    Stub.cfg = {"train": {"conv_precision": "medium", "matmul_precision": "high", "deterministic": True}}
    H.Trainer.fit(Stub(), max_iters=1)
    assert seen[-1] == ("medium", "high") and ct.get_conv_precision() == "highest" and ct.get_matmul_precision() == "highest"
    for bad in ("tf32", "HIGH", 1, True):
        Stub.cfg = {"train": {"conv_precision": bad}}
        n = len(seen)
        with pytest.raises(ValueError):
            H.Trainer.fit(Stub(), max_iters=1)
        assert len(seen) == n and ct.get_conv_precision() == "highest"
