"""cloud_transformers_amd.GraphedForward: an eval-mode forward by HIP-graph replay, keyed by the inputs' shapes and dtypes, the
model's parameter addresses and the precision / deterministic modes.  The blocks: one MultiHeadUnion with the zoo's six head
shapes (128^2 C4, 32^3 C4, 64^2 C16, 16^3 C16, 16^2 C16, 8^3 C32) at four heads each, B 2, N 256; one MultiHeadUnionAdaIn (two
heads, a style input, a tuple output).  An eval forward has no order-dependent sum, so a replay equals the eager forward bit
for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _stream_pool():
    """Every capture here creates a side stream; the pool's round robin is left where the suite before this module had it."""
    from tests.stream_pool import neutral_stream_pool
    with neutral_stream_pool():
        yield


DEV = torch.device("cuda", 0)
B, N, D, LATENT = 2, 256, 64, 24


def _settle(model, seed):
    """Eval mode on running statistics that are not the identity."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def union():
    from cloud_transformers_amd.layers.multihead_ct import MultiHeadUnion
    torch.manual_seed(0)
    return _settle(MultiHeadUnion(D, [4, 4, 16, 16, 16, 32], [128, 32, 64, 16, 16, 8], [2, 3, 2, 3, 2, 3], [4] * 6), 1)


@pytest.fixture(scope="module")
def adain():
    from cloud_transformers_amd.layers.multihead_ct import MultiHeadUnionAdaIn
    torch.manual_seed(0)
    return _settle(MultiHeadUnionAdaIn(D, [4, 4], [16, 8], [2, 3], [4, 4], n_latent=LATENT), 2)


def _inputs(seed, n=N, style=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, D, n, device=DEV, generator=g)
    pcd = torch.tanh(torch.randn(B, 3, n, device=DEV, generator=g))
    if style:
        return x, torch.randn(B, LATENT, device=DEV, generator=g), pcd
    return x, pcd


def _eager(model, args):
    with torch.no_grad():
        return model(*args)


def _tensors(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _tensors(o)]
    return []


def _same(got, want):
    got, want = _tensors(got), _tensors(want)
    assert len(got) == len(want) and len(got) >= 1
    return all(torch.equal(a, b) for a, b in zip(got, want))


def test_the_package_exports_it():
    import cloud_transformers_amd as ct
    from cloud_transformers_amd.graphs import GraphedForward
    assert ct.GraphedForward is GraphedForward and "GraphedForward" in ct.__all__


def test_union_replays_equal_the_eager_forward(union):
    from cloud_transformers_amd import GraphedForward
    gf = GraphedForward(union)
    for seed in (11, 12, 13):
        args = _inputs(seed)
        want = _eager(union, args)
        got = gf(*args)
        assert isinstance(got, tuple) and _same(got, want), seed
    assert gf.graphs_captured == 1


def test_adain_two_inputs_and_a_tuple_output(adain):
    from cloud_transformers_amd import GraphedForward
    gf = GraphedForward(adain)
    for seed in (21, 22, 23):
        args = _inputs(seed, style=True)
        want = _eager(adain, args)
        got = gf(*args)
        assert type(got) is type(want) and len(got) == len(want) and _same(got, want), seed
    assert gf.graphs_captured == 1


def test_two_shapes_give_two_independent_graphs(union):
    from cloud_transformers_amd import GraphedForward
    gf = GraphedForward(union)
    a, b = _inputs(31), _inputs(32, n=192)
    out_a = gf(*a)[0]
    out_b = gf(*b)[0]
    assert gf.graphs_captured == 2 and out_a.shape[-1] == N and out_b.shape[-1] == 192
    assert torch.equal(out_a, _eager(union, a)[0])             # the other shape's replay did not touch it
    assert torch.equal(out_b, _eager(union, b)[0])
    a2 = _inputs(33)
    out_a2 = gf(*a2)[0]
    assert out_a2.data_ptr() == out_a.data_ptr()               # static: the same key's next call overwrites the output
    assert torch.equal(out_a2, _eager(union, a2)[0]) and torch.equal(out_b, _eager(union, b)[0])
    assert gf.graphs_captured == 2


def test_clone_outputs(union):
    from cloud_transformers_amd import GraphedForward
    gf = GraphedForward(union, clone_outputs=True)
    a, a2 = _inputs(41), _inputs(42)
    first = gf(*a)[0]
    second = gf(*a2)[0]
    assert first.data_ptr() != second.data_ptr()
    assert torch.equal(first, _eager(union, a)[0]) and torch.equal(second, _eager(union, a2)[0])


def test_new_values_in_place_are_seen_without_a_capture(union):
    from cloud_transformers_amd import GraphedForward
    gf = GraphedForward(union)
    args = _inputs(51)
    before = gf(*args)[0].clone()
    saved = {k: v.clone() for k, v in union.state_dict().items()}
    try:
        with torch.no_grad():
            for p in union.parameters():
                p.mul_(1.25)
        after = gf(*args)[0]
        assert gf.graphs_captured == 1
        assert torch.equal(after, _eager(union, args)[0]) and not torch.equal(after, before)
    finally:
        union.load_state_dict(saved)
    assert torch.equal(gf(*args)[0], before) and gf.graphs_captured == 1


def test_a_replaced_tensor_and_a_mode_change_capture_anew(union):
    import cloud_transformers_amd as ct
    gf = ct.GraphedForward(union)
    args = _inputs(61)
    gf(*args)
    p = next(union.parameters())
    old = p.data
    try:
        p.data = (old * 0.5).clone()                           # another tensor behind the same Parameter
        got = gf(*args)[0]
        assert gf.graphs_captured == 2 and torch.equal(got, _eager(union, args)[0])
    finally:
        p.data = old
    prev = ct.precision.get_mode()
    try:
        ct.set_matmul_precision("high")
        n = gf.graphs_captured
        got = gf(*args)[0]
        assert gf.graphs_captured == n + 1 and torch.equal(got, _eager(union, args)[0])
    finally:
        ct.set_matmul_precision(prev)


def test_refuses_training_mode(union):
    from cloud_transformers_amd import GraphedForward
    gf = GraphedForward(union)
    union.train()
    try:
        with pytest.raises(RuntimeError, match=r"Trainer\.fit\(hip_graph=True\)"):
            gf(*_inputs(71))
    finally:
        union.eval()
    assert gf.graphs_captured == 0


def test_refuses_cpu_tensors(union):
    from cloud_transformers_amd import GraphedForward
    gf = GraphedForward(union)
    x, pcd = _inputs(81)
    with pytest.raises(RuntimeError, match="HIP device"):
        gf(x.cpu(), pcd)
    assert gf.graphs_captured == 0


def test_reset_drops_the_graphs(union):
    from cloud_transformers_amd import GraphedForward
    gf = GraphedForward(union)
    args = _inputs(91)
    gf(*args)
    gf(*args)
    assert gf.graphs_captured == 1
    gf.reset()
    assert torch.equal(gf(*args)[0], _eager(union, args)[0]) and gf.graphs_captured == 2
