"""SphereSampler.plan as one ct_kp_plan call (csrc/ct_kpplan.hip) against the torch loop it replaced (`_plan_torch`), bit for
bit and draw for draw, on twin samplers built from one seed: clouds of 1, 1 500 and ~20 000 points (one below a reduction
workgroup's span, the largest no multiple of the reduction's stride), a radius at which d2 / r^2 and d2 * (1 / r^2) differ;
carried state across plans with legacy picks in between; ties; the numpy restatement of the header's contract
(tests/kp_plan_ref.py); `items` / `sample` over mixed clouds against the per-cloud procedure they replaced; and no
device-to-host synchronisation in `plan` or `items`."""
import numpy as np
import pytest
import torch

from tests import kp_plan_ref
from tests.test_s3dis_kpconv_gpu import _areas

pytestmark = pytest.mark.gpu


def _tiny_area(name, m, seed, size):
    from cloud_transformers_amd.data.s3dis_kpconv import Area
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(0.0, 1.0, (m, 3)) * np.asarray(size)).astype(np.float32) + np.float32([3.0, -2.0, 0.1])
    cols = rng.uniform(0.0, 1.0, (m, 3)).astype(np.float32)
    labs = rng.integers(0, 13, m).astype(np.int32)
    return Area(name, pts, cols * 255, labs, pts, cols, labs)


@pytest.fixture(scope="module")
def areas():
    big = _areas(seeds=(0,), n=20000)[0]
    out = [_tiny_area("one", 1, 1, (1.0, 1.0, 1.0)), _tiny_area("small", 1500, 2, (3.0, 2.0, 1.0)), big]
    sizes = [a.sub_points.shape[0] for a in out]
    blocks = -(-sizes[2] // 4096)                                               # the reduction's grid: 256 work-items each
    assert sizes[:2] == [1, 1500] and 4096 < sizes[2] <= 20000 and sizes[2] % (256 * blocks) != 0
    return out


def _sampler(areas, r, N, seed=0, F=4):
    from cloud_transformers_amd.data.s3dis_kpconv import SphereSampler
    smp = SphereSampler(areas, N, in_radius=r, input_features_dim=F, generator=torch.Generator(device="cuda").manual_seed(seed))
    # Uniform potentials in [0, 1e-3) leave a cloud's k-th smallest near k * 1e-3 / M: the big cloud alone would be picked for
    # hundreds of picks.  Scaled by M / M_max, every cloud's smallest potentials lie on one scale and a few picks mix them.
    biggest = max(p.shape[0] for p in smp.potentials)
    for k, p in enumerate(smp.potentials):
        p.mul_(p.shape[0] / biggest)
        smp.min_potentials[k] = p.min()
    return smp


def _bits(t):
    t = t.cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b)), what


def _compare_plans(new, old, n, what):
    """plan(n) on `new` (the device plan) against _plan_torch(n) on `old`: outputs, last_picks, every potential."""
    cloud, picks = new.plan(n)
    want_cloud, want_picks = old._plan_torch(n)
    _same(cloud, want_cloud, (what, "cloud"))
    _same(picks, want_picks, (what, "picks"))
    got_last, want_last = new.last_picks, old.last_picks
    assert len(got_last) == len(want_last) == n
    for i, ((c, p, x), (wc, wp, wx)) in enumerate(zip(got_last, want_last)):
        assert isinstance(c, int) and c == wc, (what, i)
        assert p.dtype == torch.int64 and p.dim() == 0 and x.dtype == torch.float32 and tuple(x.shape) == (3,)
        assert int(p) == int(wp), (what, i, "point")
        _same(x, wx, (what, i, "pick"))
    for k, (a, b) in enumerate(zip(new.potentials, old.potentials)):
        _same(a, b, (what, "potentials", k))
    _same(new.min_potentials, old.min_potentials, (what, "min_potentials"))
    return cloud, picks


def _same_generator_state(new, old):
    assert torch.equal(torch.rand(4, generator=new.gen, device="cuda"), torch.rand(4, generator=old.gen, device="cuda"))


@pytest.mark.parametrize("N", [64, 2048])
@pytest.mark.parametrize("r", [0.3, 2.0])
def test_device_plan_equals_the_torch_loop(areas, r, N):
    new, old = _sampler(areas, r, N), _sampler(areas, r, N)
    for k, p in enumerate(new.potentials):                                     # views of the one buffer ct_kp_plan updates
        assert p.data_ptr() == new._all_potentials.data_ptr() + 4 * new.table.offsets[k]
    cloud, _ = _compare_plans(new, old, 24, (r, N))
    assert len(set(cloud.tolist())) == 3                                       # every cloud was picked
    _same_generator_state(new, old)


def test_carried_state_across_plans_and_legacy_picks(areas):
    new, old = _sampler(areas, 0.3, 64, seed=3), _sampler(areas, 0.3, 64, seed=3)
    _compare_plans(new, old, 9, "first")
    for n_legacy, n_plan in ((3, 7), (2, 5)):
        for smp in (new, old):                                                  # legacy picks move potentials and minima
            for _ in range(n_legacy):
                smp._pick()
        assert len(new.last_picks) == len(old.last_picks)
        _compare_plans(new, old, n_plan, ("after", n_legacy, n_plan))
    _same_generator_state(new, old)


def _noise_of_next_plan(smp, n):
    """The n scaled noise draws the next plan(n) will make, from a copy of the sampler's generator."""
    gen = torch.Generator(device="cuda")
    gen.set_state(smp.gen.get_state())
    return torch.stack([torch.randn(3, generator=gen, device="cuda") * (smp.in_radius / 10) for _ in range(n)]).cpu().numpy()


def _check_against_restatement(smp, areas, n):
    before = [p.cpu().numpy().copy() for p in smp.potentials]
    noise = _noise_of_next_plan(smp, n)
    cloud, picks = smp.plan(n)
    w_cloud, w_point, w_picks, w_pots, w_mins = kp_plan_ref.plan([a.sub_points for a in areas], before, noise, smp.in_radius,
                                                                 smp.num_points)
    np.testing.assert_array_equal(cloud.cpu().numpy(), w_cloud)
    np.testing.assert_array_equal(np.array([int(p) for _, p, _ in smp.last_picks]), w_point)
    assert np.array_equal(picks.cpu().numpy().view(np.uint32), w_picks.view(np.uint32))
    for k, (a, b) in enumerate(zip(smp.potentials, w_pots)):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32)), k
    assert np.array_equal(smp.min_potentials.cpu().numpy().view(np.uint32), w_mins.view(np.uint32))
    return w_cloud, w_point


@pytest.mark.parametrize("r,N", [(0.3, 64), (2.0, 2048)])
def test_ties_go_to_the_lowest_index(areas, r, N):
    new, old = _sampler(areas, r, N, seed=5), _sampler(areas, r, N, seed=5)
    for smp in (new, old):
        for p in smp.potentials:
            p.fill_(0.5)
        smp.min_potentials.fill_(0.5)
    ref = _sampler(areas, r, N, seed=5)
    for p in ref.potentials:
        p.fill_(0.5)
    ref.min_potentials.fill_(-1.0)                                             # stale on purpose: plan recomputes the minima
    cloud, _ = _compare_plans(new, old, 24, ("ties", r))
    w_cloud, w_point = _check_against_restatement(ref, areas, 24)
    np.testing.assert_array_equal(cloud.cpu().numpy(), w_cloud)
    # all clouds tie: cloud 0 and its only point; then clouds 1 and 2 tie: cloud 1, point 0; while untouched points keep
    # cloud 1 at 0.5 it is picked again, at its lowest untouched index
    assert (w_cloud[0], w_point[0]) == (0, 0) and (w_cloud[1], w_point[1]) == (1, 0)
    run = []
    for c, p in zip(w_cloud[1:], w_point[1:]):
        if c != 1:
            break
        run.append(int(p))
    assert run == sorted(run) and (r != 0.3 or len(set(run)) >= 2)
    _same_generator_state(new, old)


def test_plan_equals_the_numpy_restatement(areas):
    smp = _sampler(areas, 0.3, 64, seed=11)
    w_cloud, _ = _check_against_restatement(smp, areas, 24)
    assert len(set(w_cloud.tolist())) == 3
    _check_against_restatement(smp, areas, 5)                                  # and from the state the first plan left


def _parent_items(smp, cloud, picks, gen):
    """SphereSampler.items of the parent revision: the cloud ids read back, one radius query per distinct cloud, the rows
    scattered together; then the same draws and ct_kp_items."""
    from cloud_transformers_amd.data.s3dis_kpconv import COLOR_MEAN, COLOR_STD, kp_items
    dev, N = smp.device, smp.num_points
    B = picks.shape[0]
    idx = torch.empty(B, N, dtype=torch.int64, device=dev)
    count = torch.empty(B, dtype=torch.int64, device=dev)
    host_cloud = cloud.tolist()
    for ci in sorted(set(host_cloud)):
        rows = [b for b, c in enumerate(host_cloud) if c == ci]
        sel = torch.tensor(rows, dtype=torch.int64, device=dev)
        q_idx, _, q_count = smp.indices[ci].query_radius(picks[sel], smp.in_radius, N)
        idx[sel], count[sel] = q_idx, q_count
    nvalid = torch.clamp(count, max=N)
    live = torch.arange(N, device=dev)[None, :] < nvalid[:, None]
    keys = torch.where(live, torch.rand(B, N, generator=gen, device=dev), torch.full((B, N), 2.0, device=dev))
    perm = torch.argsort(keys, dim=1)
    u_pad = torch.rand(B, N, generator=gen, device=dev)
    drop = (torch.rand(B, generator=gen, device=dev) > smp.color_drop).float()
    points, mask, features, labels, input_inds = kp_items(idx, count, perm, u_pad, smp.offsets[cloud], picks, drop,
                                                          smp._all_points, smp._all_colors, smp._all_labels, COLOR_MEAN,
                                                          COLOR_STD, smp.input_features_dim)
    return points, mask, features, labels, cloud, input_inds


@pytest.mark.parametrize("r,N", [(0.3, 64), (2.0, 2048)])
def test_items_and_sample_on_mixed_clouds(areas, r, N):
    new, old = _sampler(areas, r, N, seed=7, F=7), _sampler(areas, r, N, seed=7, F=7)
    cloud, picks = new.plan(12)
    old._plan_torch(12)
    assert len(set(cloud.tolist())) == 3
    got, want = new.items(cloud, picks), _parent_items(old, cloud, picks, old.gen)
    for k, (a, b) in enumerate(zip(got, want)):
        _same(a, b, ("items", k))
    got = new.sample(6)
    want = _parent_items(old, *old._plan_torch(6), old.gen)
    for k, (a, b) in enumerate(zip(got, want)):
        _same(a, b, ("sample", k))
    _same_generator_state(new, old)


def test_plan_and_items_do_not_synchronise(areas):
    """No device-to-host synchronisation in plan or items with several clouds: under torch's sync debug mode set to "error" a
    synchronising call raises — checked first on `.item()`, so that the mode is known to be live."""
    smp = _sampler(areas, 2.0, 2048, seed=9)
    probe = smp.min_potentials.sum()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        cloud, picks = smp.plan(8)
        out = smp.items(cloud, picks)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(set(cloud.tolist())) == 3 and tuple(out[0].shape) == (8, 2048, 3)
    assert [c for c, _, _ in smp.last_picks] == cloud.tolist()                  # read back now, on request


def test_plan_switch_selects_the_torch_loop(areas, monkeypatch):
    new, old = _sampler(areas, 0.3, 64, seed=13), _sampler(areas, 0.3, 64, seed=13)
    monkeypatch.setenv("CLOUDCT_KP_PLAN", "0")
    cloud, picks = new.plan(4)
    assert new._device_plan is None                                            # the loop ran: nothing came from ct_kp_plan
    monkeypatch.delenv("CLOUDCT_KP_PLAN")
    want_cloud, want_picks = old.plan(4)
    assert old._device_plan is not None
    _same(cloud, want_cloud, "cloud")
    _same(picks, want_picks, "picks")
