"""HIP-graph replays of the ops that keep device-side state between launches, and of the code that runs only while a stream
is capturing.  Every number the project reports is a graph replay, and harness.Trainer.fit(hip_graph=True) trains by replay.

State: three "zeroed once, the kernel leaves it zero" buffers cached per (device, stream) in ops.py — the arrival tickets
(ops._tickets: ticketed Slice / Splat backward, the key statistics of lattice_so3), the occupancy workspace (ops._occ_ws)
and the cluster exchange workspace of the fused core (ops._core_ws).  Capture-only code: the two-stream fork of
ops.pw_backward and the heads' fork of layers.multihead_ct._run_heads ("auto").

torch.cuda.graph(g) without stream= captures on a stream no eager work runs on, so a stateful launch captured there finds no
cached buffer.  It must then own one (allocated in the graph's pool, zeroed by a node of the graph, never cached): a graph is
complete by itself, replays in any order, and re-zeroes nobody else's state.  `replay_protocol` below holds every case to
that: fresh data per replay, the same data twice, two graphs on one capture stream with the SECOND replayed first and the
first dropped while the second lives on, and an eager launch after all of it.  The references and tolerances are those of
the eager tests of each op (named per case); nothing here is looser."""
import copy
import gc
import itertools

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.test_mhct_core_gpu import SHAPES as CORE_SHAPES, core_flags, make_inputs, oracle_core, relerr  # noqa: F401 (fixture)
from tests.test_pw_gemm_gpu import BOUND, _ref as pw_ref
from tests.test_raster_gpu import close

pytestmark = pytest.mark.gpu

STATE = ("_tickets", "_occ_ws", "_core_ws")


def _fill(static, fresh):
    with torch.no_grad():
        for dst, src in zip(static, fresh):
            if dst is not None:
                dst.copy_(src)


def _capture(step, static):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):           # no stream=: torch's own capture stream, which never ran anything eagerly
        outs = step(static)
    return g, outs


def _capture_stream_has_no_cached_state():
    """Nothing made during a capture may end up in the process-wide caches (it lives in one graph's pool)."""
    from cloud_transformers_amd import ops
    handle = torch.cuda.graph.default_capture_stream.cuda_stream
    for name in STATE:
        assert all(key[1] != handle for key in getattr(ops, name)), (name, list(getattr(ops, name)))


def _tickets_are_zero():
    from cloud_transformers_amd import ops
    for key, t in ops._tickets.items():
        assert int(t.abs().sum()) == 0, key


def replay_protocol(monkeypatch, new_inputs, step, check, deterministic, on_phase=None, reset=None, two_graphs=True,
                    eager_after=True):
    """new_inputs(seed) -> list of device tensors (None allowed); step(static) -> dict of static outputs;
    check(static, outs, seed, where) compares every output with its references for the data of `seed` (exactly one call per
    replay); `deterministic`: the outputs that must repeat bit for bit on unchanged inputs; on_phase(name) after the eager
    warm-up ("warmed"), after the first capture ("captured") and after the final eager launch ("eager"); reset() before the
    first replay (module state back to its start)."""
    from cloud_transformers_amd import ops
    seeds = itertools.count(1000)
    phase = on_phase or (lambda name: None)

    def fresh_state():
        for name in STATE:
            monkeypatch.setattr(ops, name, {})

    def replay(g, static, outs, seed, where, refill=True):
        if refill:
            _fill(static, new_inputs(seed))
        g.replay()
        torch.cuda.synchronize()
        check(static, outs, seed, where)

    # set-up: where the state is created does not depend on what ran earlier in the session
    fresh_state()
    static = new_inputs(next(seeds))
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(2):              # lazy attributes, library choices, allocator
            step(static)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    phase("warmed")
    g1, outs1 = _capture(step, static)
    phase("captured")
    _capture_stream_has_no_cached_state()
    if reset is not None:
        reset()

    # A: fresh data per replay
    for i in range(3):
        seed = next(seeds)
        replay(g1, static, outs1, seed, "A%d" % i)
    # B: the same data twice more
    for i in range(2):
        before = {n: outs1[n].clone() for n in deterministic}
        replay(g1, static, outs1, seed, "B%d" % i, refill=False)
        for n in deterministic:
            assert torch.equal(outs1[n], before[n]), ("B%d" % i, n, float((outs1[n] - before[n]).abs().max()))

    if two_graphs:
        # C: two graphs on one capture stream, from empty caches; the second is replayed first
        del g1, outs1
        fresh_state()
        s1, s2 = next(seeds), next(seeds)
        static1, static2 = new_inputs(s1), new_inputs(s2)
        g1, outs1 = _capture(step, static1)
        g2, outs2 = _capture(step, static2)
        _capture_stream_has_no_cached_state()
        replay(g2, static2, outs2, s2, "C:G2 first", refill=False)
        replay(g1, static1, outs1, s1, "C:G1 second", refill=False)
        replay(g2, static2, outs2, next(seeds), "C:G2")
        replay(g1, static1, outs1, next(seeds), "C:G1")
        replay(g2, static2, outs2, next(seeds), "C:G2 again")
        del g1, outs1, static1
        gc.collect()
        replay(g2, static2, outs2, next(seeds), "C:G2 without G1")
        static = static2
        _capture_stream_has_no_cached_state()

    if eager_after:
        # D: an eager launch on the ordinary stream after all the replays
        seed = next(seeds)
        _fill(static, new_inputs(seed))
        outs = step(static)
        torch.cuda.synchronize()
        phase("eager")
        check(static, outs, seed, "D:eager")
        _tickets_are_zero()


def _raster_oracle(static, Wl, H, C, dim):
    """positions -> Splat(max) -> Slice and its autograd on the CPU (oracle/ref_cpu.py, as tests/test_raster_gpu.py), plus where
    the oracle itself saw an EXACT tie in a cell's maximum.  There the two disagree by design: scatter_reduce("amax") shares the
    cell's cotangent evenly among the tied contributions, the kernels award it to one of them (torch_scatter's rule, which of them
    is unspecified: ct_raster_hot.h).  Independent random products tie in fp32 about once in ten clouds of these sizes, and the
    protocol draws a dozen clouds per case, so the comparison has to know the rule instead of hoping for tie-free seeds."""
    keys, feat, cot = (t.detach().cpu().clone() for t in static)
    B, _, N = keys.shape
    k, f = keys.requires_grad_(True), feat.requires_grad_(True)
    lc, idx = R.positions(k, Wl, H, dim)
    z = R.splat(lc, idx, f, None, Wl, H, dim, "max")
    z.retain_grad()
    o = R.slice_(lc, idx, z, None, Wl, H, dim)
    o.backward(cot)
    V = 1 << dim
    zf = z.detach().reshape(B, H, C, -1)
    index = idx[:, :, None].reshape(B, H, 1, V * N).expand(B, H, C, V * N)
    pre = (feat.detach().reshape(B, H, C, N)[:, :, :, None] * lc.detach()[:, :, None]).reshape(B, H, C, V * N)
    hit = pre == torch.gather(zf, 3, index)                       # the contributions equal to their cell's maximum ...
    sharers = (zf == 0).float().scatter_add(3, index, hit.float())         # ... and the zero floor, which takes part in the maximum
    tied = hit & (torch.gather(sharers, 3, index) > 1)
    tied_feat = tied.reshape(B, H, C, V, N).any(dim=3)             # [B, H, C, N]: candidates of a tied (cell, channel)
    tied_keys = tied_feat.any(dim=2)[:, :, None].expand(B, H, dim, N).reshape(B, H * dim, N)
    cells = [(b, h, c, int(index[b, h, c, j])) for b, h, c, j in tied.nonzero().tolist()]
    return dict(z=z.detach(), out=o.detach(), g_keys=k.grad, g_feat=f.grad, g_z=z.grad.reshape(B, H, C, -1), lc=lc.detach(), idx=idx,
                sharers=sharers, hit=hit, tied_feat=tied_feat.reshape(B, H * C, N), tied_keys=tied_keys, tied_cells=sorted(set(cells)))


def _single_winners(g_feat, orc, where):
    """At every exactly tied (cell, channel) of the oracle: one of the tied contributions holds the cell's whole cotangent and the
    others none of it (a cell tied with the zero floor: nobody does), to the tolerance of the element-wise comparison."""
    assert len(orc["tied_cells"]) <= 2, (where, "exact ties are rare in random clouds", orc["tied_cells"])
    B, H, V, N = orc["lc"].shape
    C = orc["g_feat"].shape[1] // H
    tol = 1e-4 * max(1.0, float(orc["g_feat"].abs().max()))
    for b, h, c, cell in orc["tied_cells"]:
        share = float(orc["g_z"][b, h, c, cell]) / float(orc["sharers"][b, h, c, cell])
        at_floor = float(orc["z"].reshape(B, H, C, -1)[b, h, c, cell]) == 0.0
        winners = 0
        for j in (orc["hit"][b, h, c] & (orc["idx"][b, h].reshape(-1) == cell)).nonzero().flatten().tolist():
            v, n = divmod(j, N)
            w = float(orc["lc"][b, h, v, n])
            d = float(g_feat[b, h * C + c, n] - orc["g_feat"][b, h * C + c, n])
            won = abs(d - (float(orc["g_z"][b, h, c, cell]) - share) * w) <= tol
            lost = abs(d + share * w) <= tol
            assert won or lost, (where, (b, h, c, cell, n), d, share * w)
            winners += int(won and not lost)
        assert winners == (0 if at_floor else 1), (where, (b, h, c, cell), winners)


# ---------------------------------------------------------------------------------------------------------------------
# ticketed raster backward through autograd (references: tests/test_tickets_gpu.py and tests/test_raster_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 1024, 12, 16, 16, 2), (5, 2048, 7, 32, 8, 3)], ids=lambda s: "B%dN%dH%dC%dW%dD%d" % s)
def test_ticketed_raster_backward(shape, monkeypatch):
    from cloud_transformers_amd import _lib, ops
    lib = _lib.load()
    B, N, H, C, W, dim = shape
    Wl = [W] * dim
    monkeypatch.setattr(ops, "RASTER_TICKETS", True)

    def new_inputs(seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        return [torch.tanh(torch.randn(B, H * dim, N, device="cuda", generator=g)),
                torch.randn(B, H * C, N, device="cuda", generator=g), torch.randn(B, H * C, N, device="cuda", generator=g)]

    def step(static):
        keys, feat, cot = static
        k, f = keys.detach().requires_grad_(True), feat.detach().requires_grad_(True)
        z = ops.splat_keys(k, f, None, W, H, dim, "max")
        out = ops.slice_keys(k, z, None, W, H, dim)
        out.backward(cot)
        return dict(z=z.detach(), out=out.detach(), g_keys=k.grad, g_feat=f.grad)

    refs = {}

    def references(static, seed):
        if seed not in refs:
            with monkeypatch.context() as m:        # the two-launch form on the same data
                m.setattr(ops, "RASTER_TICKETS", False)
                two = {n: t.clone() for n, t in step(static).items()}
                tag = lib.ct_debug_last_launch().decode()
            assert "folded" not in tag and "segments" not in tag, tag
            refs.clear()
            refs[seed] = (two, _raster_oracle(static, Wl, H, C, dim))
        return refs[seed]

    def check(static, outs, seed, where):
        two, orc = references(static, seed)
        for n in ("z", "out", "g_feat"):
            assert torch.equal(outs[n], two[n]), (where, n, float((outs[n] - two[n]).abs().max()))
        err, top = float((outs["g_keys"] - two["g_keys"]).abs().max()), float(two["g_keys"].abs().max())
        assert err <= 2e-6 * top, (where, err, top)
        assert torch.equal(outs["z"].cpu(), orc["z"]), where
        close(outs["out"], orc["out"], 1e-5)
        g_feat, g_keys = outs["g_feat"].cpu(), outs["g_keys"].cpu()
        _single_winners(g_feat, orc, where)
        # outside the candidates of an exactly tied cell (none at all in most clouds) the oracle is the reference element by element
        close(torch.where(orc["tied_feat"], orc["g_feat"], g_feat), orc["g_feat"])
        close(torch.where(orc["tied_keys"], orc["g_keys"], g_keys), orc["g_keys"])

    def on_phase(name):
        if name == "eager":             # the launch that just ran eagerly took the ticketed kernels
            tag = lib.ct_debug_last_launch().decode()
            assert "folded" in tag or "segments" in tag, tag
            assert ops._tickets, "the eager launch caches its stream's tickets"

    replay_protocol(monkeypatch, new_inputs, step, check, ("z", "out", "g_feat"), on_phase)


# ---------------------------------------------------------------------------------------------------------------------
# lattice_so3 with the key statistics (reference: tests/test_lattice_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,use_scales,use_kscale", [(2, True, True), (3, True, False)], ids=["dim2", "dim3"])
def test_lattice_so3_with_statistics(dim, use_scales, use_kscale, monkeypatch):
    """B2 H5 N333: the forward deals every (b, h) row to two workgroups (lattice_fwd_nbx), so the statistics' ticket is shared
    by 20 workgroups."""
    from cloud_transformers_amd import ops
    B, H, N = 2, 5, 333

    def new_inputs(seed):
        g = torch.Generator().manual_seed(seed)
        t = [torch.rand(B, 3, N, generator=g) * 2 - 1, torch.randn(B, H * 3, N, generator=g) * 0.3, torch.randn(H, 3, generator=g),
             torch.randn(H, 3, generator=g) * 0.1, (1 + 0.2 * torch.randn(H, dim, generator=g)) if use_scales else None,
             (0.5 + 0.4 * torch.rand((), generator=g)) if use_kscale else None,
             torch.randn(B, H * dim, N, generator=g), torch.randn(B, H * dim, N, generator=g) * 0.1]
        return [None if x is None else x.cuda() for x in t]

    names = ("xyz", "residual", "log_R", "shift", "scales", "kscale")

    def step(static):
        leaves = [None if t is None else t.detach().requires_grad_(True) for t in static[:6]]
        keys, lat, stats = ops.lattice_so3(*leaves, dim, with_stats=True)
        ((lat * static[6]).sum() + (keys * static[7]).sum()).backward()
        outs = dict(keys=keys.detach(), lattice=lat.detach(), stats=stats)
        outs.update({"g_" + n: t.grad for n, t in zip(names, leaves) if t is not None})
        return outs

    refs = {}

    def references(static, seed):
        if seed not in refs:
            cpu = [None if t is None else t.cpu() for t in static]
            xyz, res, log_R, shift, sc, ks = [None if t is None else t.clone().requires_grad_(True) for t in cpu[:6]]
            p = xyz[:, None] + (res if ks is None else ks * res).reshape(B, H, 3, N)
            keys = R.rigid_transform(p, log_R, torch.zeros(H, 3) + shift, sc, dim).reshape(B, H * dim, N)
            lat = torch.tanh(keys)
            ((lat * cpu[6]).sum() + (keys * cpu[7]).sum()).backward()
            ref = dict(keys=keys.detach(), lattice=lat.detach())
            ref.update({"g_" + n: t.grad for n, t in zip(names, (xyz, res, log_R, shift, sc, ks)) if t is not None})
            refs.clear()
            refs[seed] = ref
        return refs[seed]

    def check(static, outs, seed, where):
        ref = references(static, seed)
        assert set(outs) == set(ref) | {"stats"}
        for n, b in ref.items():
            tol = 2e-5 if n in ("keys", "lattice") else 1e-4
            err = float((outs[n].cpu() - b).abs().max())
            assert err <= tol * max(1.0, float(b.abs().max())), (where, n, err)
        kd = outs["keys"].double()
        mean, var = float(kd.mean()), float(kd.var())
        assert abs(float(outs["stats"][0]) - mean) <= 1e-5, (where, float(outs["stats"][0]), mean)
        assert abs(float(outs["stats"][1]) - var) <= 1e-4 * var, (where, float(outs["stats"][1]), var)

    def on_phase(name):
        if name == "eager":
            assert ops._tickets, "the statistics take a word of the stream's ticket buffer"

    replay_protocol(monkeypatch, new_inputs, step, check, ("keys", "lattice"), on_phase)


# ---------------------------------------------------------------------------------------------------------------------
# grid_occupancy_ratio (reference: tests/test_occupancy_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 32, 32, 32), (1, 3, 5, 7)], ids=str)
def test_grid_occupancy_ratio(shape, monkeypatch):
    from cloud_transformers_amd import ops
    K = shape[0] * shape[1] * 3

    def new_inputs(seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        z = torch.relu(torch.randn(*shape, device="cuda", generator=g) - 0.5 + 0.1 * (seed % 7))      # a changing share of zeros
        z.view(-1)[:3] = torch.tensor([1e-10, -1e-10, 2e-9], device="cuda")                          # around the 1e-9 threshold
        return [z]

    def step(static):
        return dict(occ=ops.grid_occupancy_ratio(static[0], K))

    def check(static, outs, seed, where):
        want = (static[0].abs() > 1e-9).sum().float() / K
        assert outs["occ"].dtype == torch.float32 and outs["occ"].dim() == 0
        assert torch.equal(outs["occ"], want), (where, float(outs["occ"]), float(want))

    def on_phase(name):
        if name == "eager":
            assert ops._occ_ws

    replay_protocol(monkeypatch, new_inputs, step, check, ("occ",), on_phase)


# ---------------------------------------------------------------------------------------------------------------------
# fused MHCT core with clusters (reference: tests/test_mhct_core_gpu.py::test_core_matches_oracle_every_cluster_size)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,W,C", CORE_SHAPES)
@pytest.mark.parametrize("S", [2, 8])
def test_mhct_core_clusters(core_flags, dim, W, C, S, monkeypatch):
    from cloud_transformers_amd import _lib, ops
    lib = _lib.load()
    B, H, N = 2, 4, 2048
    Wa = _lib.int_array([W] * dim)
    core_flags(1 << 8)
    alone = lib.ct_mhct_core_workspace_bytes(B, H, C, N, dim, Wa)
    core_flags(S << 8)
    assert lib.ct_mhct_core_workspace_bytes(B, H, C, N, dim, Wa) > alone, "no exchange between workgroups: nothing stateful to test"
    assert ops.mhct_core_supported(B, H, C, N, [W] * dim)

    def new_inputs(seed):
        keys, feat, w, bias, cot, _ = make_inputs(B, H, C, N, dim, seed)
        return [t.cuda() for t in (keys, feat, w, bias, cot)]

    def step(static):
        k, f, wt, bt = (t.detach().requires_grad_(True) for t in static[:4])
        out, occ = ops.mhct_core(k, f, None, wt, bt, W, H, dim)
        out.backward(static[4])
        return dict(out=out.detach(), occ=occ, g_keys=k.grad, g_feat=f.grad, g_w=wt.grad, g_b=bt.grad)

    refs = {}

    def check(static, outs, seed, where):
        if seed not in refs:
            refs.clear()
            refs[seed] = oracle_core(*(t.cpu() for t in static), None, W, H, dim)
        ref = refs[seed]
        print(where, "occ", int(outs["occ"]), "oracle", ref["occ"],
              {n: "%.1e" % relerr(outs[n], ref[n]) for n in ("out", "g_keys", "g_feat", "g_w", "g_b")})
        for n, t in outs.items():
            assert not torch.isnan(t).any(), (where, n)
        assert int(outs["occ"]) == ref["occ"], where
        for n in ("out", "g_keys", "g_feat", "g_w", "g_b"):
            assert relerr(outs[n], ref[n]) <= 1e-4, (where, n, relerr(outs[n], ref[n]))

    def on_phase(name):
        if name == "eager":
            assert ops._core_ws and ops.mhct_core_check() == []

    # (g_w, g_b: summed in batch order, "bitwise reproducible" in the kernel's own words; out: conv of the exact max grid)
    replay_protocol(monkeypatch, new_inputs, step, check, ("out", "occ", "g_w", "g_b"), on_phase)


# ---------------------------------------------------------------------------------------------------------------------
# pw_backward's two-stream fork (reference: tests/test_pw_gemm_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.fn(*a, **k)


@pytest.mark.parametrize("shape", [(2, 132, 128, 260), (3, 256, 192, 1024)], ids=lambda s: "B%dCo%dCi%dN%d" % s)
def test_pw_backward_fork(shape, monkeypatch):
    from cloud_transformers_amd import ops
    B, Co, Ci, N = shape
    monkeypatch.setattr(ops, "PW_GEMM", "split16")
    monkeypatch.setattr(ops, "PW_BWD_STREAMS", True)
    assert ops.pw_eligible(Co, Ci, N, ops.PW_DGRAD) and ops.pw_eligible(Co, Ci, N, ops.PW_WGRAD)
    spy = _Spy(ops._pw_side_stream)
    monkeypatch.setattr(ops, "_pw_side_stream", spy)

    def new_inputs(seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        x = torch.randn(B, Ci, N, device="cuda", generator=g)
        gy = torch.randn(B, Co, N, device="cuda", generator=g)
        gy[:, 64:96] *= 2.0 ** -26             # a nearly-dead channel group: the per-row maxima must reach the weight gradient
        return [torch.randn(Co, Ci, device="cuda", generator=g) / Ci ** 0.5, x, gy]

    def step(static):
        W, x, gy = static
        # as a producer would: per-channel maxima in a slots buffer, tagged on the tensors
        sx, sg = torch.empty(Ci, device="cuda"), torch.empty(Co, device="cuda")
        sx.copy_(x.abs().amax(dim=(0, 2)))
        sg.copy_(gy.abs().amax(dim=(0, 2)))
        ops.tag_amax(x, sx)
        ops.tag_amax(gy, sg)
        assert ops.amax_of(x).shape == (1, Ci) and ops.amax_of(gy).shape == (1, Co)
        y, am_w, am_x, Wt = ops.pw_forward(W, x, True)
        g_x, g_w = ops.pw_backward(W, x, gy, am_w, am_x, True, True, Wt=Wt)
        return dict(y=y, g_x=g_x, g_w=g_w)

    def check(static, outs, seed, where):
        W, x, gy = static
        if where != "D:eager":
            calls = spy.calls
            eager = step(static)                # same kernels on one stream: bit for bit
            assert spy.calls == calls, "the eager reference must not fork"
            for n in ("y", "g_x", "g_w"):
                assert torch.equal(outs[n], eager[n]), (where, n, float((outs[n] - eager[n]).abs().max()))
        for n, mode in (("y", 0), ("g_x", 1), ("g_w", 2)):
            ref, mag = pw_ref(mode, W, x, gy)
            err = (outs[n].double() - ref).abs()
            assert bool((err <= BOUND * mag + 1e-44).all()), (where, n, float((err / (mag + 1e-44)).max()))

    def on_phase(name):
        if name == "warmed":
            assert spy.calls == 0, "eager launches stay on one stream"
        elif name == "captured":
            assert spy.calls == 1, "the capture forks the data gradient to the side stream"

    replay_protocol(monkeypatch, new_inputs, step, check, ("y", "g_x", "g_w"), on_phase)


# ---------------------------------------------------------------------------------------------------------------------
# a whole union block in train() mode: forked heads, forked output projection, every parameter gradient
# (reference: tests/test_blocks_gpu.py::test_heads_on_side_streams_equal_the_serial_block)
# ---------------------------------------------------------------------------------------------------------------------
def test_union_block_training_step(monkeypatch):
    """The serial eager block on the same data, step for step from the same state dict: output, input cotangent, EVERY parameter
    gradient, and the running statistics after the same number of steps."""
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers import multihead_ct as M
    monkeypatch.setattr(M, "HEAD_STREAMS", "auto")
    monkeypatch.setattr(ops, "PW_BWD_STREAMS", True)
    torch.manual_seed(23)
    B, D, N = 2, 128, 1024
    blk = M.MultiHeadUnion(D, [8, 8], [16, 8], [2, 3], [16, 16]).cuda().train()
    serial = copy.deepcopy(blk)
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    pw_spy, heads_spy = _Spy(ops._pw_side_stream), _Spy(M._record)
    monkeypatch.setattr(ops, "_pw_side_stream", pw_spy)
    monkeypatch.setattr(M, "_record", heads_spy)

    def new_inputs(seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        return [torch.randn(B, D, N, device="cuda", generator=g), torch.rand(B, 3, N, device="cuda", generator=g) * 2 - 1,
                torch.randn(B, D, N, device="cuda", generator=g)]

    def run(block, static):
        x0, pcd, cot = static
        block.zero_grad(set_to_none=True)
        x = x0.detach().requires_grad_(True)
        out, _ = block(x, pcd)
        (out * cot).sum().backward()
        grads = {n: p.grad for n, p in block.named_parameters()}
        assert all(g is not None for g in grads.values())
        return dict(out=out.detach(), g_x=x.grad, grads=grads)

    def reset():
        blk.load_state_dict(state)
        serial.load_state_dict(state)

    def check(static, outs, seed, where):
        calls = pw_spy.calls, heads_spy.calls
        want = run(serial, static)              # one serial eager step per replay: the running statistics stay in step
        torch.cuda.synchronize()
        assert (pw_spy.calls, heads_spy.calls) == calls, "the eager reference must not fork"
        np.testing.assert_allclose(outs["out"].cpu().numpy(), want["out"].cpu().numpy(), rtol=1e-5, atol=1e-5, err_msg=where)
        np.testing.assert_allclose(outs["g_x"].cpu().numpy(), want["g_x"].cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg=where)
        assert outs["grads"].keys() == want["grads"].keys()
        for n, b in want["grads"].items():
            np.testing.assert_allclose(outs["grads"][n].cpu().numpy(), b.cpu().numpy(), rtol=1e-3, atol=1e-4, err_msg=where + " " + n)
        for (n, a), (_, b) in zip(blk.named_buffers(), serial.named_buffers()):
            assert torch.equal(a, b), (where, n, float((a.double() - b.double()).abs().max()))

    def on_phase(name):
        if name == "warmed":
            assert pw_spy.calls == 0 and heads_spy.calls == 0, "eager launches stay on one stream"
        elif name == "captured":
            assert heads_spy.calls > 0, "_run_heads did not fork under capture"
            assert pw_spy.calls > 0, "the output projection's backward did not fork under capture"

    replay_protocol(monkeypatch, new_inputs, lambda static: run(blk, static), check, ("out",), on_phase, reset=reset,
                    two_graphs=False, eager_after=False)
