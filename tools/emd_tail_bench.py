"""What finishing a long auction in one launch per cloud buys (ct_emd_fwd_tail), recorded in
profiles/emd_tail_bench.txt.  Device events; the parent build (libcloudct.so of the parent commit, named by CLOUDCT_LIB or
--parent-lib) is loaded beside this build in ONE process and the two alternate after a warm-up of both.

(a) forward at (eps, iters) = (0.004, 3000): B4 n8192 and B2 n16384 uniform, B2 n10000 with counts, a collapsed pair (thousands
    of bidders for hundreds of iterations) — the parent's ct_emd_fwd / ct_emd_fwd_counts against ct_emd_fwd_tail;
(b) forward at (0.005, 50) through the unchanged entry (tail=False) against the parent: the same device code;
(c) crossover: per-iteration time of the tail kernel and of the ordinary launches against the bidder count;
(d) empty launches: what an iteration costs after every cloud has finished.

    python tools/emd_tail_bench.py [--parent-lib PATH] [--out profiles/emd_tail_bench.txt] [--quick]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.environ.get("CLOUDCT_LIB"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emd_tail_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    args = ap.parse_args()
    os.environ.pop("CLOUDCT_LIB", None)                    # the package loads THIS build; the parent is loaded by hand below
    import numpy as np
    import torch
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.ops import _ptr, _stream
    assert torch.cuda.is_available(), "emd_tail_bench needs an MI355X"
    lib = _lib.load()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("ct_emd_workspace_bytes", "ct_emd_fwd", "ct_emd_fwd_counts"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    reps = 3 if args.quick else 5

    def uniform(B, n, seed):
        rng = np.random.default_rng(seed)
        a, b = rng.random((B, n, 3), dtype=np.float32), rng.random((B, n, 3), dtype=np.float32)
        return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()

    def collapsed(B, n, seed):
        rng = np.random.default_rng(seed)
        a = (rng.standard_normal((B, n, 3)) * 0.02).astype(np.float32)
        a[:, n // 2:] = a[:, :n // 2]
        g = rng.standard_normal((B, n, 3))
        b = (0.4 * g / np.linalg.norm(g, axis=2, keepdims=True)).astype(np.float32)
        return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()

    class Call:
        """One forward with its buffers allocated once: old(L) -> ct_emd_fwd / ct_emd_fwd_counts of library L, new() -> ct_emd_fwd_tail."""
        def __init__(self, a, b, count=None):
            self.a, self.b, self.count = a, b, count
            self.B, self.n = a.shape[0], a.shape[1]
            self.dist = torch.empty(self.B, self.n, device="cuda")
            self.ass = torch.empty(self.B, self.n, device="cuda", dtype=torch.int32)
            self.info = torch.empty(self.B, 2, device="cuda", dtype=torch.int32)
            self.nws = lib.ct_emd_tail_workspace_bytes(self.B, self.n)
            self.ws = torch.empty(self.nws, device="cuda", dtype=torch.uint8)

        def old(self, L, eps, iters):
            if self.count is None and self.n % 1024 == 0:
                st = L.ct_emd_fwd(_ptr(self.a), _ptr(self.b), _ptr(self.dist), _ptr(self.ass), _ptr(self.ws), self.nws, self.B, self.n,
                                  eps, iters, _stream())
            else:
                st = L.ct_emd_fwd_counts(_ptr(self.a), _ptr(self.b), _ptr(self.count), _ptr(self.dist), _ptr(self.ass), _ptr(self.ws),
                                         self.nws, self.B, self.n, eps, iters, _stream())
            assert st == 0, st

        def new(self, eps, iters, tail_from=-1):
            st = lib.ct_emd_fwd_tail(_ptr(self.a), _ptr(self.b), _ptr(self.count), _ptr(self.dist), _ptr(self.ass), _ptr(self.info),
                                     _ptr(self.ws), self.nws, self.B, self.n, eps, iters, tail_from, _stream())
            assert st == 0, st

    def ms(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def alternate(fs, n=reps):
        """fs: list of callables -> per callable (median, min, max) over n alternating single calls after one warm-up of each."""
        for f in fs:
            f()
        t = [[] for _ in fs]
        for _ in range(n):
            for k, f in enumerate(fs):
                t[k].append(ms(f))
        return [(statistics.median(x), min(x), max(x)) for x in t]

    def fmt(r):
        return "%8.2f ms (%.2f .. %.2f)" % r

    say("emd_tail_bench: %s, schedule defaults unless a row says otherwise" % torch.cuda.get_device_name(0))
    say("parent library: %s" % (args.parent_lib or "none given: this build's unchanged entries stand in for it"))
    P = parent or lib

    # (a)
    say()
    say("(a) forward, eps 0.004, iters 3000; median (lowest .. highest) of %d alternating calls" % reps)
    rows = [("B4 n8192 uniform", Call(*uniform(4, 8192, 0))), ("B2 n16384 uniform", Call(*uniform(2, 16384, 1))),
            ("B2 n10000 counts [10000, 7500]", Call(*uniform(2, 10000, 2), count=torch.tensor([10000, 7500], dtype=torch.int32, device="cuda"))),
            ("B2 n8192 collapsed", Call(*collapsed(2, 8192, 3)))]
    for name, c in rows:
        c.old(P, 0.004, 3000)
        d0, a0 = c.dist.clone(), c.ass.clone()
        c.new(0.004, 3000)
        torch.cuda.synchronize()
        same = torch.equal(a0, c.ass) and torch.equal(d0.view(torch.int32), c.dist.view(torch.int32))
        info = c.info.cpu().tolist()
        r_old, r_new = alternate([lambda: c.old(P, 0.004, 3000), lambda: c.new(0.004, 3000)])
        spread = r_old[2] - r_old[1]
        gain = r_old[0] - r_new[0]
        say("  %-32s parent %s   tail %s   ratio %.2fx   gain %.2f ms = %.1f x the parent's spread (%.2f ms)   same bits: %s   info %s"
            % (name, fmt(r_old), fmt(r_new), r_old[0] / r_new[0], gain, gain / max(spread, 1e-3), spread, same, info))

    # (b)
    say()
    say("(b) forward, eps 0.005, iters 50, the unchanged entries (tail=False): this build against the parent, %d alternating windows of 10 calls" % reps)
    for name, c in rows[:3]:
        def win(L):
            def f():
                for _ in range(10):
                    c.old(L, 0.005, 50)
            return f
        r_p, r_t = alternate([win(P), win(lib)])
        say("  %-32s parent %s   this build %s   (per 10 calls)" % (name, fmt(r_p), fmt(r_t)))

    # (c)
    say()
    say("(c) crossover: per-iteration time against the bidder count, from calls of T + 2 and T + D iterations entered alike")
    say("    (tail: one tail launch after iteration T - 1 takes every cloud; ordinary: no tail launch); D = 40")
    D = 40
    for B, n, seed in ((4, 8192, 0), (2, 16384, 1), (4, 2048, 4)):
        c = Call(*uniform(B, n, seed))
        for T in (6, 12, 24, 48, 100, 250, 500, 1000):
            if args.quick and T > 250:
                continue
            lib.ct_debug_set_emd_tail(2048, 1 << 30)
            try:
                c.new(0.004, T + 1, T + 1)                # never: info[:, 1] = the bidders of iteration T
                torch.cuda.synchronize()
                u = c.info[:, 1].cpu().tolist()
                if max(u) > 2048:
                    say("  B%d n%-6d T %-5d bidders %s: above the tail kernel's capacity" % (B, n, T, u))
                    continue
                r = alternate([lambda: c.new(0.004, T + 2, T - 1), lambda: c.new(0.004, T + D, T - 1),
                               lambda: c.new(0.004, T + 2, T + D), lambda: c.new(0.004, T + D, T + D)], n=reps)
            finally:
                lib.ct_debug_set_emd_tail(-1, 0)
            tail_us = (r[1][0] - r[0][0]) / (D - 2) * 1e3
            ord_us = (r[3][0] - r[2][0]) / (D - 2) * 1e3
            say("  B%d n%-6d T %-5d bidders %-28s tail %7.1f us/iteration   ordinary %7.1f us/iteration" % (B, n, T, u, tail_us, ord_us))

    # (d)
    say()
    say("(d) empty launches: iterations after every cloud has finished (eps 0.05, clouds that finish within a few hundred iterations)")
    for B, n, seed in ((4, 1024, 2), (4, 8192, 5)):
        c = Call(*uniform(B, n, seed))
        c.new(0.05, 4000)
        torch.cuda.synchronize()
        info = c.info.cpu().tolist()
        r = alternate([lambda: c.new(0.05, 4000), lambda: c.new(0.05, 6000), lambda: c.old(P, 0.05, 4000), lambda: c.old(P, 0.05, 6000)], n=reps)
        say("  B%d n%-6d info %s: tail entry %.2f us per iteration beyond 4000, parent %.2f us"
            % (B, n, info, (r[1][0] - r[0][0]) / 2000 * 1e3, (r[3][0] - r[2][0]) / 2000 * 1e3))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
