"""What the EMD for any cloud size and per-cloud counts costs, recorded in profiles/emd_counts_bench.txt.

(a) The ragged path against the dense one.  At B2 n=16384 and B4 n=8192 with (eps, iters) = (0.005, 50): `ct_emd_fwd` (4096-target
    tiles in the late iterations, the update on several workgroups), `ct_emd_fwd_counts` with count = n on the same clouds (1024-target
    tiles and the single-workgroup update throughout: the same bits, checked here) and with count = 3n/4; then n = 10000 without
    a count, the size the dense entry refuses.  Device events around 20 calls after 2 warm-up calls, 3 such windows each.
(b) The dense path against another build of the library (`--parent-lib`: libcloudct.so of the parent commit — its csrc with stubs
    for the symbols it lacks — selected through CLOUDCT_LIB): the `emd` rows of tools/loss_bench.py, each library in `--runs` fresh
    processes, alternating; medians and the parent's own spread.

    python tools/emd_counts_bench.py [--parent-lib PATH] [--runs 3] [--out profiles/emd_counts_bench.txt]"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPS, ITERS = 0.005, 50


def window(f, calls=20, warmup=2):
    import torch
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def timed(f):
    t = sorted(window(f) for _ in range(3))
    return "%.2f ms (min %.2f, max %.2f)" % (t[1], t[0], t[2]), t[1]


def ragged_cost(say):
    import torch
    from cloud_transformers_amd.emd import emd_with_counts, emdModule
    assert torch.cuda.is_available(), "emd_counts_bench needs an MI355X"
    say("(a) ragged path against the dense path, forward, (eps, iters) = (%g, %d); median of 3 windows of 20 calls" % (EPS, ITERS))
    for B, n in [(2, 16384), (4, 8192)]:
        torch.manual_seed(0)
        a, b = torch.rand(B, n, 3, device="cuda"), torch.rand(B, n, 3, device="cuda")
        full = torch.full((B,), n, dtype=torch.int32, device="cuda")
        part = torch.full((B,), 3 * n // 4, dtype=torch.int32, device="cuda")
        d0, a0 = emdModule()(a, b, EPS, ITERS)
        d1, a1 = emd_with_counts(a, b, EPS, ITERS, full)
        same = torch.equal(a0, a1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32))
        s_dense, t_dense = timed(lambda: emdModule()(a, b, EPS, ITERS))
        s_full, t_full = timed(lambda: emd_with_counts(a, b, EPS, ITERS, full))
        s_part, _ = timed(lambda: emd_with_counts(a, b, EPS, ITERS, part))
        say("  B%d n=%d  ct_emd_fwd                     %s" % (B, n, s_dense))
        say("  B%d n=%d  ct_emd_fwd_counts count = n     %s   x%.2f of the dense path; same bits: %s" % (B, n, s_full, t_full / t_dense, same))
        say("  B%d n=%d  ct_emd_fwd_counts count = 3n/4  %s" % (B, n, s_part))
    for B in (2, 4):
        torch.manual_seed(1)
        a, b = torch.rand(B, 10000, 3, device="cuda"), torch.rand(B, 10000, 3, device="cuda")
        s, _ = timed(lambda: emd_with_counts(a, b, EPS, ITERS))
        say("  B%d n=10000 ct_emd_fwd_counts no count      %s" % (B, s))


def dense_unchanged(say, parent_lib, runs):
    say("(b) dense path, the `emd` rows of tools/loss_bench.py: parent commit's library against this one, %d fresh processes each, "
        "alternating" % runs)
    rows = {}
    for r in range(runs):
        for tag, lib in (("parent", parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("CLOUDCT_LIB", None)
            if lib:
                env["CLOUDCT_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loss_bench.py")], env=env, check=True,
                                 stdout=subprocess.PIPE, universal_newlines=True).stdout
            for line in out.splitlines():
                m = re.match(r"emd\s+(B\d+ n=\d+).*fwd ([\d.]+) ms, fwd\+bwd ([\d.]+) ms", line)
                if m:
                    rows.setdefault((m.group(1), "fwd"), {}).setdefault(tag, []).append(float(m.group(2)))
                    rows.setdefault((m.group(1), "fwd+bwd"), {}).setdefault(tag, []).append(float(m.group(3)))
    for (shape, what), v in sorted(rows.items()):
        p, t = v["parent"], v["this"]
        mp, mt = statistics.median(p), statistics.median(t)
        say("  emd %s %-7s  parent %s median %.2f ms (spread %.2f)   this %s median %.2f ms   difference %+.2f ms"
            % (shape, what, ["%.2f" % x for x in p], mp, max(p) - min(p), ["%.2f" % x for x in t], mt, mt - mp))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", default=None, help="libcloudct.so of the parent commit, for part (b)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emd_counts_bench.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ragged_cost(say)
    if args.parent_lib:
        dense_unchanged(say, args.parent_lib, args.runs)
    else:
        say("(b) not run: no --parent-lib")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
