"""Per-kernel cost of the grouped convolution's precision modes, straight through the C ABI.

    python tools/gconv_precision_bench.py --precision both            HIGHEST and HIGH alternating in one process
    python tools/gconv_precision_bench.py --precision highest --lib PATH/libcloudct.so    another build's default path (A/B)

Rows: the zoo's convolution shapes at batch 8 (and the shapes around the planner's thresholds), forward and backward-data.  Method: device events around windows of `--launches`
launches, both modes warmed up first, then `--windows` windows per mode alternating; the median per mode, the range of the
HIGHEST windows (the spread a gain has to beat), and the worst error over each mode's own bound against a float64 convolution of
the first cloud (HIGHEST: the fp32 bound of tests/test_gconv_families_gpu.py; HIGH: the bound of include/cloudct.h).
`covers` is ct_gconv_precision_covers; `verdict` says whether HIGH beats HIGHEST by more than that range."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPES = [("2D 32^2 C16 H64", 8, 64, 16, 16, (32, 32)), ("2D 64^2 C16 H16", 8, 16, 16, 16, (64, 64)),
          ("3D 16^3 C16 H16", 8, 16, 16, 16, (16, 16, 16)), ("3D 8^3 C32 H16", 8, 16, 32, 32, (8, 8, 8)),
          ("3D 8^3 C64 G16", 8, 16, 64, 64, (8, 8, 8)), ("3D 4^3 C64 G16", 8, 16, 64, 64, (4, 4, 4)),
          ("3D 4x8x8 C64 G16", 8, 16, 64, 64, (4, 8, 8)), ("2D 16^2 C64 G16", 8, 16, 64, 64, (16, 16)),
          ("2D 8^2 C64 G16", 8, 16, 64, 64, (8, 8)),
          # the K-split variants that keep 2 and 4 items per wave (rows of tests/gconv_families.py, batch 8 and 32 groups)
          ("2D 40x32 C32>16 G32", 8, 32, 32, 16, (40, 32)), ("2D 64^2 C64 G32", 8, 32, 64, 64, (64, 64))]


def load(path):
    lib = ctypes.CDLL(path)
    ip, vp, i = ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int
    lib.ct_gconv_fwd.argtypes = [vp, vp, vp, vp, i, i, i, i, i, ip, vp]
    lib.ct_gconv_bwd_data.argtypes = [vp, vp, vp, i, i, i, i, i, ip, vp]
    lib.ct_debug_last_launch.restype = ctypes.c_char_p
    return lib


def errors(shape, x, w, b, g_y, y, g_x):
    """worst |err| / bound of the first cloud, forward and backward-data, for both bounds: {(pass, mode): ratio}"""
    from tests import gconv_precision_common as C
    from tests.test_gconv_families_gpu import bound
    one = (1,) + tuple(shape[1:])
    ops = {"x": x[:1].cpu(), "w": w.cpu(), "b": b.cpu(), "g_y": g_y[:1].cpu()}
    out = {}
    for bwd, got in ((False, y), (True, g_x)):
        xs, ws, bs, cin, cout = C.as_forward(one, ops, bwd)
        ref, high = C.high_bound(one, xs, ws, bs, cin, cout)
        mag = C.conv(xs.abs(), ws.abs(), bs.abs() if bs is not None else None, shape[1])
        fp32 = bound(mag, cin * 3 ** len(shape[4]) + (0 if bwd else 1))
        for mode in (0, 1):
            if got[mode] is not None:
                err = (got[mode][:1].double().cpu() - ref).abs()
                out[(bwd, mode)] = float((err / (high if mode else fp32)).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("both", "highest", "high"), default="both")
    ap.add_argument("--lib", default=None, help="another build of libcloudct.so (default: this tree's)")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--no-errors", action="store_true")
    args = ap.parse_args()
    if args.lib is None:
        from cloud_transformers_amd import _lib
        args.lib = _lib.build()
    lib = load(args.lib)
    has_mode = hasattr(lib, "ct_set_gconv_precision")
    modes = {"both": (0, 1), "highest": (0,), "high": (1,)}[args.precision]
    if 1 in modes and not has_mode:
        sys.exit("%s has no ct_set_gconv_precision" % args.lib)
    st = torch.cuda.current_stream().cuda_stream
    print("lib %s  windows %d x %d launches  modes %s" % (os.path.relpath(args.lib, ROOT), args.windows, args.launches, args.precision))
    print("%-18s %-4s %-44s %9s %9s %7s %9s %8s %8s %6s %s" % ("shape", "pass", "tag", "highest", "high", "ratio", "spread", "err/b hi",
                                                              "err/b h", "covers", "verdict"))
    for name, B, G, Cin, Cout, W in SHAPES:
        shape = (B, G, Cin, Cout, W)
        gen = torch.Generator(device="cuda").manual_seed(7)
        d = len(W)
        x = torch.randn(B, G * Cin, *W, device="cuda", generator=gen)
        w = torch.randn(G * Cout, Cin, *([3] * d), device="cuda", generator=gen) * (Cin * 3 ** d) ** -0.5
        b = torch.randn(G * Cout, device="cuda", generator=gen)
        g_y = torch.randn(B, G * Cout, *W, device="cuda", generator=gen)
        Wa = (ctypes.c_int * d)(*W)
        y = {m: None for m in (0, 1)}
        g_x = {m: None for m in (0, 1)}

        def launch(bwd, out):
            if bwd:
                rc = lib.ct_gconv_bwd_data(g_y.data_ptr(), w.data_ptr(), out.data_ptr(), B, G, Cin, Cout, d, Wa, st)
            else:
                rc = lib.ct_gconv_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), B, G, Cin, Cout, d, Wa, st)
            assert rc == 0, rc

        rows = []
        for bwd in (False, True):
            times = {m: [] for m in modes}
            outs = g_x if bwd else y
            for m in modes:                                   # warm-up of both modes
                outs[m] = torch.empty_like(x if bwd else g_y)
                if has_mode:
                    lib.ct_set_gconv_precision(m)
                for _ in range(args.launches):
                    launch(bwd, outs[m])
            tag = lib.ct_debug_last_launch().decode()
            torch.cuda.synchronize()
            for _ in range(args.windows):
                for m in modes:
                    if has_mode:
                        lib.ct_set_gconv_precision(m)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.launches):
                        launch(bwd, outs[m])
                    e1.record()
                    torch.cuda.synchronize()
                    times[m].append(e0.elapsed_time(e1) * 1e3 / args.launches)
            rows.append((bwd, tag, times))
        if has_mode:
            lib.ct_set_gconv_precision(0)
        err = {} if args.no_errors else errors(shape, x, w, b, g_y, y, g_x)
        for bwd, tag, times in rows:
            med = {m: statistics.median(t) for m, t in times.items()}
            spread = max(times[0]) - min(times[0]) if 0 in times else float("nan")
            covers = lib.ct_gconv_precision_covers(int(bwd), B, G, Cin, Cout, d, Wa) if has_mode else -1
            verdict = ""
            if len(modes) == 2:
                verdict = "one-term wins" if med[1] < med[0] - spread else "no gain beyond the spread"
            f = lambda v: "%9.1f" % v if v is not None else "%9s" % "-"          # noqa: E731
            e = lambda k: "%8.3f" % err[k] if k in err else "%8s" % "-"            # noqa: E731
            print("%-18s %-4s %-44s %s %s %7s %9.1f %s %s %6d %s" % (
                name, "bwd" if bwd else "fwd", tag, f(med.get(0)), f(med.get(1)),
                "%.2f" % (med[0] / med[1]) if len(modes) == 2 else "-", spread, e((bwd, 0)), e((bwd, 1)), covers, verdict), flush=True)


if __name__ == "__main__":
    main()
