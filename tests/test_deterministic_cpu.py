"""Deterministic mode, the host side: the two ABI symbols, the Python switch and its three sources (explicit, torch's flag, the
environment).  No GPU: the switch is host state that no kernel reads."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def clean_mode():
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import determinism
    prev, prev_torch, prev_warn = determinism.get_mode(), torch.are_deterministic_algorithms_enabled(), \
        torch.is_deterministic_algorithms_warn_only_enabled()
    yield ct
    determinism.set_deterministic(prev)
    torch.use_deterministic_algorithms(prev_torch, warn_only=prev_warn)


def test_abi_symbols_round_trip():
    from cloud_transformers_amd import _lib
    assert "ct_set_deterministic" in _lib.SIGNATURES and "ct_get_deterministic" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.ct_abi_version() == 3                     # additive symbols: no version bump
    before = lib.ct_get_deterministic()
    try:
        lib.ct_set_deterministic(1)
        assert lib.ct_get_deterministic() == 1
        lib.ct_set_deterministic(0)
        assert lib.ct_get_deterministic() == 0
        lib.ct_set_deterministic(7)                      # any non-zero value is "on"
        assert lib.ct_get_deterministic() == 1
    finally:
        lib.ct_set_deterministic(before)


def test_override_is_the_calling_threads_alone():
    """ct_deterministic_override: the mode for the entry points the calling thread invokes; other threads keep the switch"""
    import threading
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    before = lib.ct_get_deterministic()
    seen = []
    try:
        lib.ct_set_deterministic(1)
        lib.ct_deterministic_override(0)
        assert lib.ct_get_deterministic() == 0
        t = threading.Thread(target=lambda: seen.append(lib.ct_get_deterministic()))
        t.start()
        t.join()
        assert seen == [1]
        Wa = _lib.int_array([8, 8, 8])
        off = lib.ct_splat_bwd_workspace_bytes(8, 16, 32, 4096, 3, Wa, 0)
        lib.ct_deterministic_override(-1)
        assert lib.ct_get_deterministic() == 1
        lib.ct_set_deterministic(0)
        assert off == lib.ct_splat_bwd_workspace_bytes(8, 16, 32, 4096, 3, Wa, 0)      # the queries follow the override too
        lib.ct_deterministic_override(1)
        assert lib.ct_get_deterministic() == 1
    finally:
        lib.ct_deterministic_override(-1)
        lib.ct_set_deterministic(before)


def test_header_declares_the_switch_and_names_it_among_the_global_state():
    text = open(os.path.join(ROOT, "include", "cloudct.h")).read()
    assert "void ct_set_deterministic(int on);" in text and "int ct_get_deterministic(void);" in text
    assert "void ct_deterministic_override(int on);" in text
    head = text[:text.index("#ifndef CLOUDCT_H")]
    assert "ct_set_deterministic" in head                # the remark on global state
    version_comment = text[text.index("2 (round 6)"):text.index("#define CT_ABI_VERSION")]
    assert "ct_set_deterministic" in version_comment and "ct_get_deterministic" in version_comment


def test_workspace_query_is_sized_by_the_mode():
    """The Splat(max) backward queries read the switch: in the mode they cover the deterministic kernel's needs — the claim
    words of a grid whose single-channel tile exceeds a CU's LDS (256^2), the chunk groups' partial g_keys — and never ask for
    less than the default query; CT_BWD_ACCUMULATE_KEYS adds its tail in either mode."""
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    before = lib.ct_get_deterministic()
    try:
        for B, H, C, N, W in [(1, 2, 1, 1024, [256, 256]), (2, 16, 8, 1024, [32, 32]), (8, 16, 32, 4096, [8, 8, 8]), (1, 2, 2, 1024, [160, 160])]:
            dim, Wa = len(W), _lib.int_array(W)
            lib.ct_set_deterministic(0)
            off = lib.ct_splat_bwd_workspace_bytes(B, H, C, N, dim, Wa, 0)
            lib.ct_set_deterministic(1)
            on = lib.ct_splat_bwd_workspace_bytes(B, H, C, N, dim, Wa, 0)
            on_ex = lib.ct_splat_bwd_ex_workspace_bytes(B, H, C, N, dim, Wa, 0, 1)
            assert on >= off, (W, on, off)
            assert on_ex == on + B * H * dim * N * 4
            if W == [256, 256]:
                assert on >= B * H * C * 256 * 256 * 4
            if W == [8, 8, 8]:                           # 128 planes, four chunks: four groups' partials of (B, H, V, N) floats
                assert on >= 4 * B * H * 8 * N * 4
    finally:
        lib.ct_set_deterministic(before)


def test_none_follows_torch(clean_mode):
    ct = clean_mode
    ct.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    assert ct.is_deterministic() is False
    torch.use_deterministic_algorithms(True)
    assert ct.is_deterministic() is True
    ct.set_deterministic(False)                          # explicit beats torch's flag
    assert ct.is_deterministic() is False
    torch.use_deterministic_algorithms(False)
    ct.set_deterministic(True)
    assert ct.is_deterministic() is True
    with pytest.raises(TypeError):
        ct.set_deterministic(1)


def test_context_manager_restores_the_previous_mode(clean_mode):
    ct = clean_mode
    from cloud_transformers_amd import determinism
    torch.use_deterministic_algorithms(False)
    for prev in (None, False, True):
        ct.set_deterministic(prev)
        with ct.deterministic():
            assert ct.is_deterministic() is True
            with ct.deterministic(False):
                assert ct.is_deterministic() is False
            assert ct.is_deterministic() is True
        assert determinism.get_mode() is prev
        with pytest.raises(ValueError):
            with ct.deterministic(True):
                raise ValueError("leaves the scope by an exception")
        assert determinism.get_mode() is prev


def test_push_sets_the_library_switch(clean_mode):
    ct = clean_mode
    from cloud_transformers_amd import _lib, determinism
    lib = _lib.load()
    before = lib.ct_get_deterministic()
    try:
        with ct.deterministic(True):
            assert determinism.push() is True and lib.ct_get_deterministic() == 1
            with determinism.relaxed():
                assert lib.ct_get_deterministic() == 0
            assert lib.ct_get_deterministic() == 1
        ct.set_deterministic(False)
        assert determinism.push() is False and lib.ct_get_deterministic() == 0
    finally:
        lib.ct_set_deterministic(before)


def test_refuse_raises_in_torchs_wording_or_warns(clean_mode):
    from cloud_transformers_amd import determinism
    torch.use_deterministic_algorithms(False)
    with pytest.raises(RuntimeError, match="some_op does not have a deterministic implementation"):
        determinism.refuse("some_op")
    torch.use_deterministic_algorithms(True, warn_only=True)
    with pytest.warns(UserWarning, match="some_op does not have a deterministic implementation"):
        determinism.refuse("some_op")


@pytest.mark.parametrize("value,expect", [("1", "True True"), ("0", "False False"), (None, "None False")])
def test_environment_sets_the_initial_mode(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "CLOUDCT_DETERMINISTIC"}
    if value is not None:
        env["CLOUDCT_DETERMINISTIC"] = value
    code = ("import cloud_transformers_amd as ct; from cloud_transformers_amd import determinism as d; "
            "print(d.get_mode(), ct.is_deterministic())")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == expect


def test_trainer_config_switch_scopes_the_fit(clean_mode, monkeypatch):
    """`train.deterministic: true` turns the mode on for Trainer.fit and gives the previous mode back afterwards."""
    ct = clean_mode
    from cloud_transformers_amd import harness as H
    seen = []

    class Stub:
        cfg = {"train": {"deterministic": True}}

        def _fit(self, max_iters, hip_graph, log_each):
            seen.append(ct.is_deterministic())
            return [0.0]

    ct.set_deterministic(False)
    assert H.Trainer.fit(Stub(), max_iters=1) == [0.0] and seen == [True]
    assert ct.is_deterministic() is False
    Stub.cfg = {"train": {}}
    H.Trainer.fit(Stub(), max_iters=1)
    assert seen == [True, False]
