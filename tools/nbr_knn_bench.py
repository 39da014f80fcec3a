"""Cost of GridIndex.query_knn and GridIndex.interpolate (csrc/ct_nbr_knn.h: one wavefront per query) on the synthetic
Area-like cloud of tools/kpconv_data_bench.py, grid-subsampled at 0.04 on the host, with raw-like queries; beside
GridIndex.nearest (one work-item per query) on the same queries and sklearn's KDTree.query on the host.

    python tools/nbr_knn_bench.py [--points 1000000] [--queries 1000000] [--host-queries 100000] [--rounds 7]
                                  [--out profiles/nbr_knn_bench.txt]

Method: every device variant is warmed up, then the variants are run in turn, `--rounds` times round robin in one process,
each run timed by a pair of device events; a row is the median, the lowest and the highest of its runs.  The host rows are
wall-clock times of one call after a warm-up call, with the thread count sklearn used stated.  Needs a GPU: no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed_round_robin(variants, rounds, warmup=2):
    """{name: [ms per run]} of the callables in `variants`, run in turn `rounds` times, each between two device events."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return times


def row(ms):
    return [round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000, help="target size of the subsampled cloud")
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--host-queries", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbr_knn_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nbr_knn_bench needs a HIP device")
    from kpconv_data_bench import area_like
    from cloud_transformers_amd.data.subsampling import grid_subsampling
    from cloud_transformers_amd.neighbors import GridIndex

    side = float(np.sqrt(args.points / 625.0 / 2.6))            # kpconv_data_bench's room for ~--points subsampled points
    size = (1.6 * side, side, 3.5)
    raw = area_like(int(args.points * 2.5), 0, size)
    sp, _, _ = grid_subsampling(raw, features=np.zeros((raw.shape[0], 3), np.float32),
                                labels=np.zeros((raw.shape[0], 1), np.int32), sampleDl=0.04)
    rng = np.random.default_rng(1)
    qh = raw[rng.integers(0, raw.shape[0], args.queries)] + rng.normal(0, 0.01, (args.queries, 3)).astype(np.float32)
    qh = np.ascontiguousarray(qh, np.float32)

    index = GridIndex(torch.from_numpy(sp).cuda())
    q = torch.from_numpy(qh).cuda()
    values = torch.randn(sp.shape[0], 13, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    variants = {"nearest": lambda: index.nearest(q)}
    for k in (1, 3, 16, 64):
        variants["query_knn_k%d" % k] = lambda k=k: index.query_knn(q, k)
    variants["interpolate_k3_C13"] = lambda: index.interpolate(values, q, 3)
    times = timed_round_robin(variants, args.rounds)

    res = {"device": torch.cuda.get_device_name(0), "room_m": [round(v, 2) for v in size], "sub_points": int(sp.shape[0]),
           "cell_m": index.h, "dims": index.dims, "queries": args.queries, "rounds": args.rounds,
           "points_per_occupied_cell": round(sp.shape[0] / int((torch.diff(index.cell_start) > 0).sum()), 2),
           "device_ms_median_min_max": {name: row(ms) for name, ms in times.items()}}
    med = {name: float(np.median(ms)) for name, ms in times.items()}
    res["query_knn_k1_over_nearest"] = round(med["query_knn_k1"] / med["nearest"], 2)
    res["k1_equals_nearest"] = bool(torch.equal(index.query_knn(q, 1)[0][:, 0], index.nearest(q)[0]))

    try:
        from sklearn.neighbors import KDTree
    except ImportError:
        res["sklearn"] = "not importable"
    else:
        nq = min(args.host_queries, args.queries)
        tree = KDTree(sp, leaf_size=50)
        tree.query(qh[:1000], k=3)
        t0 = time.perf_counter()
        dist, ind = tree.query(qh[:nq], k=3)
        dt = (time.perf_counter() - t0) * 1e3
        res["sklearn_query_k3_%d_queries_ms" % nq] = round(dt, 1)
        res["sklearn_threads"] = 1                              # KDTree.query runs on the calling thread
        res["sklearn_query_k3_scaled_to_queries_ms"] = round(dt * args.queries / nq, 1)
        res["host_over_device_k3"] = round(dt * args.queries / nq / med["query_knn_k3"], 1)
        res["k3_indices_equal_sklearn_fraction"] = round(float((index.query_knn(q[:nq], 3)[0].cpu().numpy() == ind).mean()), 6)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/nbr_knn_bench.py --points %d --queries %d --host-queries %d --rounds %d\n" %
                (args.points, args.queries, args.host_queries, args.rounds))
        f.write("device rows: ms per call as [median, lowest, highest] of %d runs, variants alternating, device events\n" % args.rounds)
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
