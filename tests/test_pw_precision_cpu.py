"""Precision mode of the pointwise GEMMs, the host side: the three ABI symbols, the Python switch and its three sources
(explicit, torch's flag, the environment), the scope around Trainer.fit.  No GPU: the switch is host state that no kernel reads."""
import os
import re
import subprocess
import sys
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def clean_mode():
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import _lib, precision
    prev, prev_torch = precision.get_mode(), torch.get_float32_matmul_precision()
    lib = _lib.load()
    before = lib.ct_get_pw_precision()
    yield ct
    precision.set_matmul_precision(prev)
    torch.set_float32_matmul_precision(prev_torch)
    lib.ct_pw_precision_override(-1)
    lib.ct_set_pw_precision(before)


def test_symbols_are_declared_and_exported():
    from cloud_transformers_amd import _lib
    text = open(os.path.join(ROOT, "include", "cloudct.h")).read()
    assert "void ct_set_pw_precision(int p);" in text and re.search(r"int\s+ct_get_pw_precision\(void\);", text)
    assert "void ct_pw_precision_override(int p);" in text
    assert re.search(r"#define CT_PW_PRECISION_HIGHEST\s+0\b", text) and re.search(r"#define CT_PW_PRECISION_HIGH\s+1\b", text)
    assert int(re.search(r"#define CT_ABI_VERSION\s+(\d+)", text).group(1)) == 3
    head = text[:text.index("#ifndef CLOUDCT_H")]
    assert "ct_set_pw_precision" in head                 # named among the library's process-wide state
    lib = _lib.load()
    for name in ("ct_set_pw_precision", "ct_get_pw_precision", "ct_pw_precision_override"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_abi_symbols_round_trip(clean_mode):
    from cloud_transformers_amd import _lib, precision
    lib = _lib.load()
    assert (precision.HIGHEST, precision.HIGH) == (0, 1)
    lib.ct_set_pw_precision(1)
    assert lib.ct_get_pw_precision() == 1
    lib.ct_set_pw_precision(0)
    assert lib.ct_get_pw_precision() == 0
    for other in (2, 7, -3):                             # anything else is the default
        lib.ct_set_pw_precision(1)
        lib.ct_set_pw_precision(other)
        assert lib.ct_get_pw_precision() == 0


def test_override_belongs_to_the_calling_thread(clean_mode):
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    seen = []
    lib.ct_set_pw_precision(0)
    lib.ct_pw_precision_override(1)
    assert lib.ct_get_pw_precision() == 1
    t = threading.Thread(target=lambda: seen.append(lib.ct_get_pw_precision()))
    t.start()
    t.join()
    assert seen == [0]                                   # the other thread keeps the process-wide switch
    lib.ct_pw_precision_override(-1)
    assert lib.ct_get_pw_precision() == 0
    lib.ct_set_pw_precision(1)
    lib.ct_pw_precision_override(0)
    assert lib.ct_get_pw_precision() == 0
    t = threading.Thread(target=lambda: seen.append(lib.ct_get_pw_precision()))
    t.start()
    t.join()
    assert seen == [0, 1]
    lib.ct_pw_precision_override(-1)
    assert lib.ct_get_pw_precision() == 1


def test_the_four_values_and_the_refusals(clean_mode):
    ct = clean_mode
    torch.set_float32_matmul_precision("highest")
    for name in ("highest", "high", "medium"):
        ct.set_matmul_precision(name)
        assert ct.get_matmul_precision() == name
    ct.set_matmul_precision(None)
    assert ct.get_matmul_precision() == "highest"
    for bad in ("low", "HIGH", "", "tf32"):
        with pytest.raises(ValueError):
            ct.set_matmul_precision(bad)
    for bad in (1, True, 0.5, b"high", ["high"]):
        with pytest.raises(TypeError):
            ct.set_matmul_precision(bad)
    assert ct.get_matmul_precision() == "highest"        # a refused value changes nothing


def test_none_follows_torch(clean_mode):
    ct = clean_mode
    ct.set_matmul_precision(None)
    for name in ("high", "medium", "highest"):
        torch.set_float32_matmul_precision(name)
        assert ct.get_matmul_precision() == name
    torch.set_float32_matmul_precision("high")
    ct.set_matmul_precision("highest")                   # explicit beats torch's flag
    assert ct.get_matmul_precision() == "highest"


def test_push_and_medium_is_served_by_high(clean_mode):
    ct = clean_mode
    from cloud_transformers_amd import _lib, precision
    lib = _lib.load()
    for name, want in (("highest", 0), ("high", 1), ("medium", 1)):
        ct.set_matmul_precision(name)
        assert precision.code() == want and precision.push() == want and lib.ct_get_pw_precision() == want
    ct.set_matmul_precision("highest")
    with precision.forced(precision.HIGH):
        assert lib.ct_get_pw_precision() == 1
    assert lib.ct_get_pw_precision() == 0


def test_context_manager_restores_the_previous_mode(clean_mode):
    ct = clean_mode
    from cloud_transformers_amd import precision
    torch.set_float32_matmul_precision("highest")
    for prev in (None, "highest", "high", "medium"):
        ct.set_matmul_precision(prev)
        with ct.matmul_precision("high"):
            assert ct.get_matmul_precision() == "high"
            with ct.matmul_precision("highest"):
                assert ct.get_matmul_precision() == "highest"
            assert ct.get_matmul_precision() == "high"
        assert precision.get_mode() == prev
        with pytest.raises(KeyError):
            with ct.matmul_precision("high"):
                raise KeyError("leaves the scope by an exception")
        assert precision.get_mode() == prev


@pytest.mark.parametrize("value,expect", [("high", "high high"), ("medium", "medium medium"), (None, "highest highest"),
                                          ("garbage", "highest highest")])
def test_environment_sets_the_initial_mode(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "CLOUDCT_PW_PRECISION"}
    if value is not None:
        env["CLOUDCT_PW_PRECISION"] = value
    # torch's flag set to "high" as well: a process that never asks this package stays on "highest"
    code = ("import torch; torch.set_float32_matmul_precision('high'); import cloud_transformers_amd as ct; "
            "from cloud_transformers_amd import precision as p; print(p.get_mode(), ct.get_matmul_precision())")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == expect


def test_trainer_config_switch_scopes_the_fit(clean_mode):
    """`train.matmul_precision: high` sets the mode for Trainer.fit and gives the previous mode back afterwards."""
    ct = clean_mode
    from cloud_transformers_amd import harness as H
    seen = []

    class Stub:
        cfg = {"train": {"matmul_precision": "high"}}

        def _fit(self, max_iters, hip_graph, log_each):
            seen.append(ct.get_matmul_precision())
            return [0.0]

    ct.set_matmul_precision("highest")
    assert H.Trainer.fit(Stub(), max_iters=1) == [0.0] and seen == ["high"]
    assert ct.get_matmul_precision() == "highest"
    Stub.cfg = {"train": {}}
    H.Trainer.fit(Stub(), max_iters=1)
    assert seen == ["high", "highest"]
    Stub.cfg = {"train": {"matmul_precision": "high", "deterministic": True}}
    H.Trainer.fit(Stub(), max_iters=1)
    assert seen[-1] == "high" and ct.get_matmul_precision() == "highest"
