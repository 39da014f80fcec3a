"""Cost of the S3DIS KPConv protocol's neighbour work on the device (cloud_transformers_amd.neighbors,
cloud_transformers_amd.data.s3dis_kpconv) on synthetic Area-like clouds (floor, ceiling, walls and clutter, grid-subsampled
at 0.04 on the host), beside sklearn's CPU KDTree where it is importable.

    python tools/kpconv_data_bench.py [--points 1000000] [--queries 10000000] [--iters 20] [--cloud area|clustered]

Rows: the raw cloud's grid subsampling through both paths (`subsample_rows`: the host call, the whole device call, and its
bounds, key, sort and reduce parts alone; --cloud clustered times these rows alone, on blobs of thousands of points per
voxel, where summing a voxel in input order costs most); the GridIndex build of the subsampled cloud, with the default
cell choice (what SphereSampler / VoteEvaluator run) and with the cell given; one radius query (one workgroup per centre) and six in one launch;
SphereSampler.sample(6) at N = 8192, r = 2 (pick, query, Tukey update per item, then the batch assembly); nearest() of
--queries raw-like points (the full-resolution reprojection of VoteEvaluator.full_ious); the host KD-tree's build,
six sorted radius queries and nearest of 10^6 queries (that time scaled to --queries is reported as such, not measured)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def area_like(n_raw, seed, size):
    rng = np.random.default_rng(seed)
    X, Y, Z = size
    k = n_raw // 8
    u = lambda m, lo, hi: rng.uniform(lo, hi, m)       # noqa: E731
    parts = [np.stack([u(k, 0, X), u(k, 0, Y), np.zeros(k)], 1), np.stack([u(k, 0, X), u(k, 0, Y), np.full(k, Z)], 1),
             np.stack([np.zeros(k), u(k, 0, Y), u(k, 0, Z)], 1), np.stack([np.full(k, X), u(k, 0, Y), u(k, 0, Z)], 1),
             np.stack([u(k, 0, X), np.zeros(k), u(k, 0, Z)], 1), np.stack([u(k, 0, X), np.full(k, Y), u(k, 0, Z)], 1)]
    rest = n_raw - 6 * k
    centres = rng.uniform([1, 1, 0.3], [X - 1, Y - 1, 1.5], (max(rest // 2000, 1), 3))
    parts.append(centres[rng.integers(0, centres.shape[0], rest)] + rng.normal(0, 0.25, (rest, 3)))
    return np.concatenate(parts).astype(np.float32)


def clustered(n_raw, seed):
    """Dense blobs a voxel or two wide: thousands of points per 0.04 voxel."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform([0, 0, 0], [20, 20, 3], (300, 3))
    return (centres[rng.integers(0, centres.shape[0], n_raw)] + rng.normal(0, 0.006, (n_raw, 3))).astype(np.float32)


def windows_ms(fn, iters, windows=5, warmup=2):
    """[median, lowest, highest] of `windows` timed windows of `iters` calls each, after a warm-up"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3 / iters)
    return [round(v, 3) for v in (float(np.median(t)), min(t), max(t))]


def subsample_rows(raw, cols, labs, dl, iters):
    """The same raw cloud through data.subsampling.grid_subsampling (host) and grid_subsampling_device: rows of seconds /
    milliseconds as [median, lowest, highest] over windows; the device call whole (inputs resident), with its copies (what
    load_areas pays), and its parts alone: ct_voxel_bounds (beside torch.aminmax), ct_voxel_keys, the stable sort, ct_voxel_reduce."""
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.data.subsampling import compute_device, grid_subsampling, grid_subsampling_device
    res, host_s = {}, []
    for _ in range(3):
        t0 = time.perf_counter()
        hp, hf, hl = grid_subsampling(raw, features=cols, labels=labs[:, None], sampleDl=dl)
        host_s.append(time.perf_counter() - t0)
    res["subsample_host_s"] = [round(v, 3) for v in (float(np.median(host_s)), min(host_s), max(host_s))]
    N = raw.shape[0]
    res["subsample_raw_points"], res["subsample_rows"] = int(N), int(hp.shape[0])
    P, F, L = torch.from_numpy(raw).cuda(), torch.from_numpy(cols).cuda(), torch.from_numpy(labs[:, None].copy()).cuda()
    dp, df, dlab, counts = compute_device(P, features=F, classes=L, sampleDl=dl, return_counts=True)
    res["subsample_equal"] = bool(np.array_equal(dp.cpu().numpy(), hp) and np.array_equal(df.cpu().numpy(), hf)
                                  and np.array_equal(dlab.cpu().numpy(), hl))
    res["subsample_points_per_voxel_mean_max"] = [round(N / hp.shape[0], 1), int(counts.max())]
    res["subsample_device_ms"] = windows_ms(lambda: grid_subsampling_device(P, F, L, sampleDl=dl), iters)

    def with_copies():
        up = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
        return [t.cpu() for t in grid_subsampling_device(up(raw), up(cols), up(labs[:, None].copy()), sampleDl=dl)]

    res["subsample_device_with_copies_ms"] = windows_ms(with_copies, max(1, iters // 4), windows=3, warmup=1)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    i64 = dict(dtype=torch.int64, device="cuda")
    bounds = torch.empty(6, device="cuda")
    bws = torch.empty(lib.ct_voxel_bounds_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    bounds_call = lambda: _lib.check(lib.ct_voxel_bounds(P.data_ptr(), N, bounds.data_ptr(), bws.data_ptr(), bws.numel(), stream),   # noqa: E731
                                     "ct_voxel_bounds")
    bounds_call()
    record, keys = torch.zeros(_lib.VOXEL_GRID_BYTES // 8 + 1, **i64), torch.empty(N, **i64)
    keys_call = lambda: _lib.check(lib.ct_voxel_keys(P.data_ptr(), N, dl, bounds.data_ptr(), record.data_ptr(), keys.data_ptr(),   # noqa: E731
                                                     stream), "ct_voxel_keys")
    keys_call()
    ks, order = torch.sort(keys, stable=True)
    ws = torch.empty(lib.ct_voxel_reduce_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    op, of, oc = torch.empty(N, 3, device="cuda"), torch.empty(N, 3, device="cuda"), torch.empty(N, 1, dtype=torch.int32, device="cuda")
    inv, cnt = torch.empty(N, **i64), torch.empty(N, **i64)
    reduce_call = lambda inverse: _lib.check(lib.ct_voxel_reduce(                                   # noqa: E731
        ks.data_ptr(), order.data_ptr(), P.data_ptr(), F.data_ptr(), L.data_ptr(), N, 3, 1, op.data_ptr(), of.data_ptr(), oc.data_ptr(),
        inv.data_ptr() if inverse else None, cnt.data_ptr() if inverse else None, record.data_ptr() + _lib.VOXEL_GRID_BYTES,
        ws.data_ptr(), ws.numel(), stream), "ct_voxel_reduce")
    res["subsample_bounds_call_ms"] = windows_ms(bounds_call, iters)
    res["subsample_bounds_torch_aminmax_ms"] = windows_ms(lambda: torch.aminmax(P, dim=0), iters)      # torch's reduction of the same bounds, for comparison
    res["subsample_keys_call_ms"] = windows_ms(keys_call, iters)
    res["subsample_sort_ms"] = windows_ms(lambda: torch.sort(keys, stable=True), iters)
    res["subsample_reduce_call_ms"] = windows_ms(lambda: reduce_call(False), iters)
    res["subsample_reduce_call_inverse_counts_ms"] = windows_ms(lambda: reduce_call(True), iters)
    return res


def gpu_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000, help="target size of the subsampled cloud")
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cloud", choices=("area", "clustered"), default="area", help="clustered: the subsampling rows alone")
    args = ap.parse_args()
    if args.cloud == "clustered":
        raw = clustered(int(args.points * 2.5), 0)
        rng = np.random.default_rng(1)
        res = {"cloud": "clustered"}
        res.update(subsample_rows(raw, rng.integers(0, 256, (raw.shape[0], 3)).astype(np.float32),
                                  rng.integers(0, 13, raw.shape[0]).astype(np.int32), 0.04, max(2, args.iters // 4)))
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))
        return
    from cloud_transformers_amd.data.s3dis_kpconv import Area, SphereSampler
    from cloud_transformers_amd.data.subsampling import grid_subsampling
    from cloud_transformers_amd.neighbors import GridIndex

    # surfaces subsampled at 0.04 keep ~625 points per m^2: size the room so that the subsampled cloud is ~--points
    side = float(np.sqrt(args.points / 625.0 / 2.6))
    size = (1.6 * side, side, 3.5)
    t0 = time.perf_counter()
    raw = area_like(int(args.points * 2.5), 0, size)
    rng = np.random.default_rng(1)
    cols = rng.integers(0, 256, (raw.shape[0], 3)).astype(np.float32)
    labs = rng.integers(0, 13, raw.shape[0]).astype(np.int32)
    sp, sc, sl = grid_subsampling(raw, features=cols, labels=labs[:, None], sampleDl=0.04)
    host_prep_s = time.perf_counter() - t0
    res = {"room_m": [round(v, 2) for v in size], "raw_points": int(raw.shape[0]), "sub_points": int(sp.shape[0]),
           "host_generate_and_subsample_s": round(host_prep_s, 2)}
    res.update(subsample_rows(raw, cols, labs, 0.04, max(2, args.iters // 4)))

    P = torch.from_numpy(sp).cuda()
    index = GridIndex(P)
    res["cell_m"] = index.h
    res["dims"] = index.dims
    res["points_per_occupied_cell"] = round(sp.shape[0] / int((torch.diff(index.cell_start) > 0).sum()), 2)
    cell = index.h
    # the sampler's and the evaluator's construction (cell=None) also picks the cell: occupancy of a ladder of edges,
    # one device sort each, and a second device-to-host read
    res["index_build_default_cell_ms"] = round(gpu_ms(lambda: GridIndex(P), args.iters), 3)
    res["index_build_given_cell_ms"] = round(gpu_ms(lambda: GridIndex(P, cell), args.iters), 3)

    c6 = P[torch.randint(0, P.shape[0], (6,), generator=torch.Generator().manual_seed(2))].contiguous()
    res["radius_counts_r2"] = index.query_radius(c6, 2.0, 8192)[2].tolist()
    res["radius_1_query_K8192_ms"] = round(gpu_ms(lambda: index.query_radius(c6[:1], 2.0, 8192), args.iters), 3)
    res["radius_6_queries_one_launch_K8192_ms"] = round(gpu_ms(lambda: index.query_radius(c6, 2.0, 8192), args.iters), 3)

    area = Area("Area_bench", raw, cols, labs, sp, sc / np.float32(255), sl[:, 0])
    smp = SphereSampler([area], 8192, in_radius=2.0, input_features_dim=4, generator=torch.Generator(device="cuda").manual_seed(0))
    smp.indices[0] = index
    res["sample6_N8192_ms"] = round(gpu_ms(lambda: smp.sample(6), args.iters), 3)

    q = torch.from_numpy(raw[rng.integers(0, raw.shape[0], args.queries)]).cuda()
    q += torch.randn(q.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 0.01
    res["nearest_queries"] = args.queries
    res["nearest_ms"] = round(gpu_ms(lambda: index.nearest(q), max(2, args.iters // 5), warmup=1), 2)
    del q

    try:
        from sklearn.neighbors import KDTree
    except ImportError:
        res["sklearn"] = "not importable"
    else:
        t0 = time.perf_counter()
        tree = KDTree(sp, leaf_size=50)
        res["sklearn_kdtree_build_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        c6h = c6.cpu().numpy()
        t0 = time.perf_counter()
        for i in range(6):
            tree.query_radius(c6h[i:i + 1], r=2.0, return_distance=True, sort_results=True)
        res["sklearn_6_radius_queries_sorted_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        nq = min(1_000_000, args.queries)
        qh = raw[rng.integers(0, raw.shape[0], nq)]
        t0 = time.perf_counter()
        tree.query(qh, k=1, return_distance=False)
        dt = time.perf_counter() - t0
        res["sklearn_nearest_%d_queries_ms" % nq] = round(dt * 1e3, 1)
        res["sklearn_nearest_scaled_to_queries_ms"] = round(dt * 1e3 * args.queries / nq, 1)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
