"""The MHCT blocks in eval mode without gradients: every BatchNorm1d of a block runs on the eval kernels (ct_bn_eval_*: the
stacked projection with its 2n norms in one launch, the heads' `after` norms written into the concatenation, the block's
`after` norm with the skip connection) and agrees with the modules' own path (ops.BN_EVAL = False); an eval forward WITH
gradients keeps the module path; the forward can be captured in a HIP graph; and the whole S3DIS segmenter stays inside
the routing-noise bounds of tests/test_zoo_gpu.py against its golden."""
import os

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu


def _randomise_norms(module, seed):
    """Running statistics and affine parameters of every norm off their initial values — except key_bn.weight, which stays
    at its zero init: the keys are then key_bn.bias on both paths, the lattice is bit-identical, and no cell or arg-max
    flip can enter a comparison of the two paths."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in module.named_modules():
            if isinstance(m, nn.BatchNorm1d):
                C, dev = m.num_features, m.weight.device
                m.running_mean.copy_((torch.rand(C, generator=g) * 2 - 1).to(dev) * 0.5)
                m.running_var.copy_((torch.rand(C, generator=g) * 1.5 + 0.5).to(dev))
                m.bias.copy_((torch.rand(C, generator=g) - 0.5).to(dev))
                if not name.endswith("key_bn"):
                    m.weight.copy_((torch.rand(C, generator=g) + 0.5).to(dev))
    return module


class _CountNorms:
    """Counts the calls of nn.BatchNorm1d.forward (the module path of a norm) while active."""

    def __enter__(self):
        self.calls = 0
        self.real = nn.BatchNorm1d.forward
        outer = self

        def forward(module, x):
            outer.calls += 1
            return outer.real(module, x)

        nn.BatchNorm1d.forward = forward
        return self

    def __exit__(self, *exc):
        nn.BatchNorm1d.forward = self.real
        return False


def _both_paths(run):
    """(result on the eval kernels, module-norm calls there, result with ops.BN_EVAL = False, calls there)."""
    from cloud_transformers_amd import ops
    assert ops.BN_EVAL
    with torch.no_grad():
        with _CountNorms() as new:
            got = run()
        ops.BN_EVAL = False
        try:
            with _CountNorms() as old:
                want = run()
        finally:
            ops.BN_EVAL = True
    return got, new.calls, want, old.calls


def _agree(got, want):
    tol = 1e-4 * max(1.0, float(want.abs().max()))        # the fused-versus-plain bound of tests/test_blocks_gpu.py
    err = float((got - want).abs().max())
    print("max |new - module path| %.3e (bound %.3e)" % (err, tol))
    assert got.shape == want.shape and err <= tol, (err, tol)


def _union(model_dim_out=None, seed=12):
    from cloud_transformers_amd.layers.multihead_ct import MultiHeadUnion
    torch.manual_seed(seed)
    blk = MultiHeadUnion(128, [8, 8], [16, 8], [2, 3], [16, 16], model_dim_out=model_dim_out).cuda().eval()
    return _randomise_norms(blk, seed + 1)


def _inputs(B, D, N, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, N, generator=g).cuda(), (torch.rand(B, 3, N, generator=g) * 2 - 1).cuda()


def test_union_block_in_eval_runs_no_module_norm():
    blk = _union()
    x, pcd = _inputs(2, 128, 1024)
    got, calls, want, old_calls = _both_paths(lambda: blk(x, pcd)[0])
    assert calls == 0, calls                               # 2 key + 2 values + 2 heads' after + the block's after: all fused
    assert old_calls == 7, old_calls
    _agree(got, want)


def test_union_block_with_projected_shortcut_runs_one_module_norm():
    blk = _union(model_dim_out=64)
    x, pcd = _inputs(2, 128, 1024)
    got, calls, want, _ = _both_paths(lambda: blk(x, pcd)[0])
    assert calls == 1, calls                               # shortcut_bn: out of this path's scope
    _agree(got, want)


@pytest.mark.parametrize("kind", ["head", "pool"])
def test_single_heads_in_eval_run_no_module_norm(kind):
    from cloud_transformers_amd.layers.multihead_ct import MultiHead, MultiHeadPool
    torch.manual_seed(3)
    blk = MultiHead(16, 4, 16, 8, 2, 2) if kind == "head" else MultiHeadPool(16, 4, 8, 2, 2)
    blk = _randomise_norms(blk.cuda().eval(), 4)
    x, pcd = _inputs(2, 16, 1024)
    got, calls, want, old_calls = _both_paths(lambda: blk(x, pcd)[0])
    assert calls == 0 and old_calls == (3 if kind == "head" else 2), (calls, old_calls)
    _agree(got, want)


def test_eval_with_gradients_keeps_the_module_path():
    blk = _union()
    x, pcd = _inputs(2, 128, 1024)
    x.requires_grad_(True)
    with _CountNorms() as n:
        out, _ = blk(x, pcd)
    assert n.calls == 7, n.calls
    out.sum().backward()
    assert torch.isfinite(x.grad).all()
    grads = [p.grad for p in blk.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)


def test_eval_forward_replays_from_a_captured_graph():
    blk = _union()
    x, pcd = _inputs(2, 128, 1024)
    with torch.no_grad():
        want = blk(x, pcd)[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                blk(x, pcd)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = blk(x, pcd)[0]
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        g.replay()                                         # nothing of the forward depends on state it changed
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_segmenter_smoke_whole_model_eval_without_gradients():
    """The statistical routing-noise bounds tests/test_zoo_gpu.py uses for this network (twelve blocks of arg-max routing
    turn a 1e-7 difference into another winner now and then), relative to the logits' magnitude."""
    from tests.test_zoo_gpu import _model
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zoo_segmenter_forward.npz"))
    net = _model(int(gold["seed"])).eval()
    with torch.no_grad(), _CountNorms() as n:
        out = net(torch.from_numpy(gold["cloud"]).cuda())
    assert n.calls == 2, n.calls                           # the model's own stem and head norms; none inside the 12 blocks
    ref = gold["out_eval"].astype(np.float64)
    assert tuple(out.shape) == ref.shape
    err = np.abs(out.cpu().double().numpy() - ref)
    scale = max(1.0, float(np.abs(ref).max()))
    print("segmenter eval/no-grad: median %.3e, within 1e-4 %.4f, max %.3e, scale %.3f"
          % (np.median(err), np.mean(err <= 1e-4 * scale), err.max(), scale))
    assert np.median(err) <= 3e-6 * scale and np.mean(err <= 1e-4 * scale) >= 0.97 and err.max() <= 2e-2 * scale, \
        (np.median(err), np.mean(err <= 1e-4 * scale), err.max(), scale)
