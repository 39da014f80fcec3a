"""The MHCT blocks with frozen norms in a forward that records gradients: after freeze_norms every BatchNorm1d of a block
runs on the eval kernels forward and on ct_bn_eval_group_bwd backward — the stacked projection with its 2n norms, the heads'
`after` norms written into the concatenation, the block's `after` norm with the skip connection and, in a block that projects
its shortcut, the shortcut's norm too (that stack IS routed: 0 module-norm calls there as well) — and agrees, output and every
gradient, with the same block unmarked in eval mode, which is the modules' own path.  The step is deterministic in
deterministic mode, captures in a HIP graph, and trains the segmenter through harness.Trainer without moving a statistic."""
import copy

import pytest
import torch
import torch.distributed as dist
from torch import nn

from tests.test_eval_blocks_gpu import _agree, _CountNorms, _inputs, _randomise_norms, _union

pytestmark = pytest.mark.gpu


def _step(blk, x, pcd, cot=None):
    """(output, input gradient, {name: parameter gradient}, module-norm calls) of one forward + backward."""
    blk.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    with _CountNorms() as n:
        out = blk(x, pcd)[0]
    if cot is None:
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(out.device)
    out.backward(cot)
    return out.detach(), x.grad, {k: p.grad for k, p in blk.named_parameters()}, n.calls


def _frozen_and_module_paths(blk, x, pcd, module_calls):
    """The block marked and put in training mode against its unmarked eval twin; returns the frozen step's results."""
    from cloud_transformers_amd import freeze_norms, norms_frozen
    twin = copy.deepcopy(blk).eval()
    freeze_norms(blk)
    blk.train()
    assert norms_frozen(blk) is True and norms_frozen(twin) is False
    stats = [b.clone() for b in blk.buffers()]
    out, gx, grads, calls = _step(blk, x, pcd)
    want, want_gx, want_grads, twin_calls = _step(twin, x, pcd)
    assert calls == 0, calls
    assert twin_calls == module_calls, twin_calls
    _agree(out, want)
    _agree(gx, want_gx)
    assert set(grads) == set(want_grads)
    for name in grads:
        assert (grads[name] is None) == (want_grads[name] is None), name
        if grads[name] is not None:
            print(name, end=": ")
            _agree(grads[name], want_grads[name])
    assert all(torch.equal(a, b) for a, b in zip(stats, blk.buffers()))           # statistics and num_batches_tracked
    return out, gx, grads


def test_union_block_with_frozen_norms_runs_no_module_norm():
    blk = _union()
    x, pcd = _inputs(2, 128, 1024)
    _, _, grads = _frozen_and_module_paths(blk, x, pcd, 7)
    assert all(g is not None for g in grads.values())                              # affine=False: the norms' parameters train


def test_union_block_with_projected_shortcut_runs_no_module_norm_either():
    """model_dim_out=64: the shortcut is PointwiseConv1d -> BatchNorm1d, and MultiHeadUnion._shortcut routes that norm through
    ops.bn_frozen (no ReLU): 0 module-norm calls, where the eval path without gradients leaves it to the module (1)."""
    blk = _union(model_dim_out=64)
    x, pcd = _inputs(2, 128, 1024)
    _frozen_and_module_paths(blk, x, pcd, 8)


@pytest.mark.parametrize("kind", ["head", "pool"])
def test_single_heads_with_frozen_norms_run_no_module_norm(kind):
    from cloud_transformers_amd.layers.multihead_ct import MultiHead, MultiHeadPool
    torch.manual_seed(3)
    blk = MultiHead(16, 4, 16, 8, 2, 2) if kind == "head" else MultiHeadPool(16, 4, 8, 2, 2)
    blk = _randomise_norms(blk.cuda().eval(), 4)
    x, pcd = _inputs(2, 16, 1024)
    _frozen_and_module_paths(blk, x, pcd, 3 if kind == "head" else 2)


def test_frozen_affine_gives_no_parameter_gradient_and_the_same_input_gradient():
    """affine=True against affine=False, both in deterministic mode (the raster kernels' float atomics would otherwise differ
    from run to run): the norms' parameters get no .grad, everything else carries the same bits."""
    from cloud_transformers_amd import deterministic, freeze_norms
    blk = _union()
    twin = copy.deepcopy(blk)
    x, pcd = _inputs(2, 128, 1024)
    freeze_norms(blk).train()
    freeze_norms(twin, affine=True).train()
    with deterministic():
        out, gx, grads, _ = _step(blk, x, pcd)
        out_a, gx_a, grads_a, calls = _step(twin, x, pcd)
    assert calls == 0
    norm_params = {"%s.%s" % (n, k) for n, m in twin.named_modules() if isinstance(m, nn.BatchNorm1d) for k in ("weight", "bias")}
    assert len(norm_params) == 14
    assert torch.equal(out, out_a) and torch.equal(gx, gx_a)
    for name, g in grads_a.items():
        if name in norm_params:
            assert g is None and grads[name] is not None, name
        else:
            assert torch.equal(g, grads[name]), name


def test_two_fresh_runs_in_deterministic_mode_give_equal_gradients():
    from cloud_transformers_amd import deterministic, freeze_norms
    x, pcd = _inputs(2, 128, 1024)
    runs = []
    for _ in range(2):
        blk = freeze_norms(_union()).train()
        with deterministic():
            runs.append(_step(blk, x, pcd))
    (out, gx, grads, _), (out2, gx2, grads2, _) = runs
    assert torch.equal(out, out2) and torch.equal(gx, gx2)
    assert all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_frozen_step_replays_from_a_captured_graph():
    """Forward + backward in ONE graph after a side-stream warm-up (tests/test_graph_replay_gpu.py's pattern), replayed twice with
    fresh inputs copied into the static tensors: the gradients are the eager ones bit for bit (deterministic mode: the heads'
    and the GEMMs' stream forks inside a capture must not show either)."""
    from cloud_transformers_amd import deterministic, freeze_norms
    blk = freeze_norms(_union()).train()
    eager_blk = copy.deepcopy(blk)
    x, pcd = _inputs(2, 128, 1024, seed=5)
    sx = x.clone().requires_grad_(True)
    spcd = pcd.clone()
    cot = torch.randn(2, 128, 1024, generator=torch.Generator().manual_seed(9)).cuda()
    stats = [b.clone() for b in blk.buffers()]
    with deterministic():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                blk.zero_grad(set_to_none=True)
                sx.grad = None
                blk(sx, spcd)[0].backward(cot)
        torch.cuda.current_stream().wait_stream(side)
        blk.zero_grad(set_to_none=True)
        sx.grad = None
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = blk(sx, spcd)[0]
            out.backward(cot)
        static = {k: p.grad for k, p in blk.named_parameters()}
        assert sx.grad is not None and all(v is not None for v in static.values())
        for seed in (21, 22):
            nx, npcd = _inputs(2, 128, 1024, seed=seed)
            with torch.no_grad():
                sx.copy_(nx)
                spcd.copy_(npcd)
            g.replay()
            torch.cuda.synchronize()
            want, want_gx, want_grads, calls = _step(eager_blk, nx, npcd, cot)
            assert calls == 0
            assert torch.equal(out.detach(), want) and torch.equal(sx.grad, want_gx), seed
            for k in static:
                assert torch.equal(static[k], want_grads[k]), (seed, k)
    assert all(torch.equal(a, b) for a, b in zip(stats, blk.buffers()))


def test_the_switch_restores_the_module_path():
    from cloud_transformers_amd import freeze_norms, ops
    blk = freeze_norms(_union()).train()
    x, pcd = _inputs(2, 128, 1024)
    switch = ops.BN_FROZEN
    ops.BN_FROZEN = False
    try:
        _, gx, grads, calls = _step(blk, x, pcd)
    finally:
        ops.BN_FROZEN = switch
    assert calls == 7, calls
    assert torch.isfinite(gx).all() and all(g is not None and torch.isfinite(g).all() for g in grads.values())
    assert _step(blk, x, pcd)[3] == 0


def test_unmarked_training_and_eval_routes_are_untouched():
    """What the mark must not change: a training-mode block calls no module norm (the training kernels), an unmarked eval block
    with gradients calls all seven."""
    blk = _union()
    x, pcd = _inputs(2, 128, 1024)
    assert _step(blk, x, pcd)[3] == 7
    before = [b.clone() for b in blk.buffers()]
    blk.train()
    assert _step(blk, x, pcd)[3] == 0
    assert not all(torch.equal(a, b) for a, b in zip(before, blk.buffers()))       # training mode: the statistics move


def _config(tmp_path):
    from tests.test_harness_gpu import CONFIG, MODEL
    (tmp_path / "segmenter.py").write_text(MODEL)
    text = CONFIG.format(root=str(tmp_path)).replace("save_each: 3", "save_each: 100000").replace("num_points: 512", "num_points: 1024")
    assert "num_points: 1024" in text
    cfg_path = tmp_path / "s3dis.yaml"
    cfg_path.write_text(text.replace("train:\n", "train:\n    freeze_norms: true\n"))
    return cfg_path


def _norm_state(model):
    return {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches_tracked" in k}


@pytest.mark.parametrize("graph", [False, True])
def test_segmenter_trains_on_frozen_norms_through_the_harness(tmp_path, graph):
    from cloud_transformers_amd import harness as H
    from cloud_transformers_amd import norms_frozen
    torch.manual_seed(0)
    tr = H.Trainer(H.load_config(_config(tmp_path)), "segmentation", n_classes=13, device=torch.device("cuda", 0), dataset_length=8,
                   channels=6, make_dirs=False)
    assert norms_frozen(tr.model) is True
    stats = _norm_state(tr.model)
    assert len(stats) == 3 * (2 + 12 * 7)                                          # stem, head and seven norms per block
    start = {k: p.detach().clone() for k, p in tr.model.named_parameters()}
    hist = tr.fit(max_iters=3, hip_graph=graph, log_each=3)
    assert len(hist) == 3 and all(v == v and abs(v) != float("inf") for v in hist), hist
    now = _norm_state(tr.model)
    assert all(torch.equal(v, now[k]) for k, v in stats.items())                   # bit-unchanged, num_batches_tracked too
    # the parameters moved: every projection and — affine=False — every norm's weight and bias, frozen statistics or not
    norm_params = ["%s.%s" % (n, k) for n, m in tr.model.named_modules() if isinstance(m, nn.BatchNorm1d) for k in ("weight", "bias")]
    watched = norm_params + [k for k in start if k.endswith("keys_values_pred.0.weight")]
    assert len(watched) == 2 * (2 + 12 * 7) + 24
    still = [k for k, p in tr.model.named_parameters() if k in watched and torch.equal(start[k], p.detach())]
    assert not still, still
    if graph:                                                                      # really captured: no eager fallback
        assert len(tr._graphs) == 1 and all(rec not in (None, False) for rec in tr._graphs.values())
    assert tr.model.training and not any(m.training for m in tr.model.modules() if isinstance(m, nn.BatchNorm1d))
    batch = next(iter(tr.loader))
    with _CountNorms() as n:
        tr._loss(batch).backward()
    assert n.calls == 2, n.calls                                                   # the model file's own stem and head norms


def test_frozen_ddp_step_exchanges_no_statistics(tmp_path):
    """One RCCL rank with the statistics exchange forced on (tests/test_ddp_gpu.py): an unfrozen step would count 72 collectives;
    with every SyncBatchNorm frozen the counter does not move."""
    from cloud_transformers_amd import harness as H
    from cloud_transformers_amd import norms_frozen, ops
    from tests.test_ddp_gpu import _free_port
    cfg = H.load_config(_config(tmp_path))
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    forced = ops.SYNC_STATS_FORCE
    ops.SYNC_STATS_FORCE = True
    try:
        torch.manual_seed(0)
        tr = H.Trainer(cfg, "segmentation", n_classes=13, device=torch.device("cuda", 0), dist=dist, dataset_length=8, channels=6,
                       make_dirs=False)
        assert isinstance(tr.model, torch.nn.parallel.DistributedDataParallel) and norms_frozen(tr.model) is True
        assert any(isinstance(m, nn.SyncBatchNorm) for m in tr.model.modules())
        stats = _norm_state(tr.model)
        c0 = ops.sync_stats_collectives()
        hist = tr.fit(max_iters=2, hip_graph=False, log_each=2)
        assert ops.sync_stats_collectives() == c0
        assert len(hist) == 2 and all(v == v for v in hist)
        now = _norm_state(tr.model)
        assert all(torch.equal(v, now[k]) for k, v in stats.items())
    finally:
        ops.SYNC_STATS_FORCE = forced
        dist.destroy_process_group()
