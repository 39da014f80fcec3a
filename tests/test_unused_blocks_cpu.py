"""The blocks of the reference's import surface that none of its model_zoo files use — unet2d.unet_parts.{DoubleConv, Down,
Up, OutConv, GroupCat}, unet2d.unet_model.UNet, layers.v2v_groups.{EncoderDecorder, V2VModel}
(unet2d/unet_parts.py:49-150, unet2d/unet_model.py:8-41, layers/v2v_groups.py:73-171) — exist under the same import
paths, draw the reference's initial weights at the same seed and compute the same function (CPU: the torch fall-back of the
conv modules; the reference side is tests/golden/unused_blocks_reference.npz, written by tests/golden/gen_unused_blocks_golden.py)."""
import hashlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_import_surface():
    sys.path.insert(0, ROOT)
    import unet2d.unet_parts as P
    import unet2d.unet_model as M
    import layers.v2v_groups as V
    for name in ("Res2DBlock", "Basic2DBlock", "DoubleConv", "Down", "Up", "OutConv", "GroupCat", "nn", "F", "torch"):
        assert hasattr(P, name), name
    assert hasattr(M, "UNet")
    for name in ("Basic3DBlock", "Res3DBlock", "Pool3DBlock", "Upsample3DBlock", "EncoderDecorder", "V2VModel"):
        assert hasattr(V, name), name
    gc = P.GroupCat(2)
    a, b = torch.arange(8.).reshape(1, 4, 1, 2), -torch.arange(4.).reshape(1, 2, 1, 2)
    out = gc(a, b)
    assert out.shape == (1, 6, 1, 2)
    assert torch.equal(out[0, :, 0, 0], torch.tensor([0., 2., -0., 4., 6., -2.]))


def build(kind):
    """UNet(2, 3, 16) / V2VModel(2, 3, groups=2) after torch.manual_seed(0), from whichever unet2d / layers is first on sys.path"""
    if kind == "unet":
        from unet2d.unet_model import UNet
        torch.manual_seed(0)
        return UNet(2, 3, 16)
    from layers.v2v_groups import V2VModel
    torch.manual_seed(0)
    return V2VModel(2, 3, groups=2)


def forward(model, kind):
    torch.manual_seed(1)
    x = torch.randn(2, 32, 32, 32) if kind == "unet" else torch.randn(1, 4, 16, 16, 16)
    model.eval()
    with torch.no_grad():
        return model(x)


def tensor_digest(t):
    t = t.detach().contiguous()
    return hashlib.sha256(("%s %s " % (t.dtype, tuple(t.shape))).encode() + t.numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("kind", ["unet", "v2v"])
def test_matches_reference_module(kind, golden):
    ref = golden("unused_blocks_reference")[kind]
    sys.path.insert(0, ROOT)
    ours = build(kind)
    assert ROOT in sys.modules[ours.__class__.__module__].__file__ or "cloud_transformers_amd" in ours.__class__.__module__
    sd = ours.state_dict()
    names = [str(n) for n in ref["sd_names"]]
    assert list(sd) == names or set(sd) == set(names)
    # same seed -> same initial weights (module creation order matches): the reference's tensors by digest
    differ = [n for n, d in zip(names, ref["sd_sha256"]) if tensor_digest(sd[n]) != str(d)]
    assert not differ, ("initial weights differ from the reference's at the same seed", differ[:5])
    a, b = torch.from_numpy(ref["out"]), forward(ours, kind)
    assert a.shape == b.shape
    assert float((a - b).abs().max() / a.abs().max()) <= 1e-5
