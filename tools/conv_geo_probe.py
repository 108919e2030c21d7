"""Run-time-geometry convolution (t4k_conv2d_geo_fwd / _bwd): time per call of forward, dX and dF | dB at five layers, beside
the specialised entries of the same library on the same device in the same run.

    python tools/conv_geo_probe.py [--reps R] [--runs K] [--batch N] [--torch] [--json profiles/conv_geo_probe.json]

Each timing is the wall time of R back-to-back calls on the library's default stream, bracketed by t4k_sync, divided by R; it is repeated K
times, the sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported, with the
dispatches of one call from t4k_launch_count.

  cases (N = 256): 3x3 / 2 P 1, 32x32x64 -> 16x16x128;  3x3 D 2 P 2, 16x16x128 -> 16x16x128;  7x7 / 2 P 3, 64x64x3 -> 32x32x64;
                   2x2 / 2, 32x32x64 -> 16x16x64;  3x3 / 2 P 1, 28x28x1 -> 14x14x8
  (a) t4k_conv2d_fwd / _bwd at (4,2,1) on the SAME tensors as the first case (32x32x64 -> 16x16x128): the (3,2,1,1) layer does 9/16 of that
      work; the bar is that it takes no longer, beyond the two spreads
  (b) both families at (3,1,1) on 16x16x64 -> 128: a ratio, no bar
  --torch adds torch.nn.functional.conv2d on the GPU per case (informative only)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = ctypes.c_void_p
I8 = ctypes.c_int * 8

CASES = [("3x3/2 P1 32x32x64->16x16x128", 32, 64, 128, 3, 2, 1, 1),
         ("3x3 D2 P2 16x16x128->16x16x128", 16, 128, 128, 3, 1, 2, 2),
         ("7x7/2 P3 64x64x3->32x32x64", 64, 3, 64, 7, 2, 3, 1),
         ("2x2/2 32x32x64->16x16x64", 32, 64, 64, 2, 2, 0, 1),
         ("3x3/2 P1 28x28x1->14x14x8", 28, 1, 8, 3, 2, 1, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(os.environ.get("T4K_LIB") or None); h.init(0)                # T4K_LIB: another build of the library, for A/B runs
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    h.lib.t4k_conv_last_plan.restype = ctypes.c_char_p
    N = args.batch
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g) - 0.5

    def timed(fn):
        h.call("t4k_sync", None)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        h.call("t4k_sync", None)
        return (time.perf_counter() - t0) / args.reps * 1e6

    def measure(row, sides):
        """sides: [(name, fn)]; alternating within every repeat"""
        times = {k: [] for k, _ in sides}
        for k, fn in sides:
            fn(); h.call("t4k_sync", None)                              # warm: code objects loaded
            l0 = int(h.lib.t4k_launch_count()); fn(); row["launches_" + k] = int(h.lib.t4k_launch_count()) - l0
            row["plan_" + k] = h.lib.t4k_conv_last_plan().decode()
        for _ in range(args.runs):
            for k, fn in sides:
                times[k].append(timed(fn))
        for k, _ in sides:
            row[k + "_us"] = round(statistics.median(times[k]), 2)
            row[k + "_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]

    def tensors(H1, C1, C0, K, S, P, D):
        H0 = (H1 + 2 * P - D * (K - 1) - 1) // S + 1
        t = dict(I=rnd(N, H1, H1, C1), F=rnd(C1, K, K, C0), B=rnd(C0), O=torch.zeros(N, H0, H0, C0, device="cuda"), G=rnd(N, H0, H0, C0),
                 DX=torch.zeros(N, H1, H1, C1, device="cuda"), DFB=torch.zeros(C1 * K * K * C0 + C0, device="cuda"))
        return H0, t

    def geo_sides(t, geo, ndf):
        p = {k: V(v.data_ptr()) for k, v in t.items()}
        pdb = V(t["DFB"].data_ptr() + 4 * ndf)
        return [("fwd", lambda: h.call("t4k_conv2d_geo_fwd", p["I"], None, p["O"], p["F"], p["B"], *geo, None)),
                ("dx", lambda: h.call("t4k_conv2d_geo_bwd", p["I"], p["G"], p["DX"], None, p["F"], None, None, *geo, 0, None)),
                ("dfdb", lambda: h.call("t4k_conv2d_geo_bwd", p["I"], p["G"], None, None, p["F"], p["DFB"], pdb, *geo, 1, None))]

    def old_sides(t, geo, ndf):
        p = {k: V(v.data_ptr()) for k, v in t.items()}
        pdb = V(t["DFB"].data_ptr() + 4 * ndf)
        return [("fwd", lambda: h.call("t4k_conv2d_fwd", p["I"], p["O"], p["F"], p["B"], *geo, None)),
                ("dx", lambda: h.call("t4k_conv2d_bwd", p["I"], p["G"], p["DX"], p["F"], None, None, *geo, 0, None)),
                ("dfdb", lambda: h.call("t4k_conv2d_bwd", p["I"], p["G"], None, p["F"], p["DFB"], pdb, *geo, 1, None))]

    rows = []
    for name, H1, C1, C0, K, S, P, D in CASES:
        H0, t = tensors(H1, C1, C0, K, S, P, D)
        geo = (N, H1, H1, C1, H0, H0, C0, K, S, P, D)
        out = I8(); h.call("t4k_conv2d_geo_plan", N, H1, H1, C1, C0, K, S, P, D, 1, out)
        row = {"case": name, "N": N, "plan": list(out)}
        sides = [("geo_" + k, fn) for k, fn in geo_sides(t, geo, C1 * K * K * C0)]
        if args.torch:
            x = t["I"].permute(0, 3, 1, 2).contiguous(); w = t["F"].permute(3, 0, 1, 2).contiguous()
            tfwd = lambda: torch.nn.functional.conv2d(x, w, t["B"], stride=S, padding=P, dilation=D)

            def torch_timed(fn=tfwd):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.reps * 1e6
            tfwd(); ts = [torch_timed() for _ in range(args.runs)]
            row["torch_fwd_us"] = round(statistics.median(ts), 2); row["torch_fwd_min_max_us"] = [round(min(ts), 2), round(max(ts), 2)]
        measure(row, sides)
        print(json.dumps(row), flush=True); rows.append(row)
        del t

    # (a) the parent's only strided geometry on the tensors of the first case
    name, H1, C1, C0 = "(a) (3,2,1,1) beside t4k_conv2d_* at (4,2,1), 32x32x64->16x16x128", 32, 64, 128
    H0, tn = tensors(H1, C1, C0, 3, 2, 1, 1)
    _, to = tensors(H1, C1, C0, 4, 2, 1, 1)
    to["I"], to["G"] = tn["I"], tn["G"]                                 # the same activations; the 4x4 filter is the parent's own
    row = {"case": name, "N": N}
    sides = []
    for (k, fn), (_, fo) in zip(geo_sides(tn, (N, H1, H1, C1, H0, H0, C0, 3, 2, 1, 1), C1 * 9 * C0), old_sides(to, (N, H1, H1, C1, H0, H0, C0, 4, 2, 1), C1 * 16 * C0)):
        sides += [("geo321_" + k, fn), ("old421_" + k, fo)]
    measure(row, sides)
    for k in ("fwd", "dx", "dfdb"):
        row["ratio_" + k] = round(row["geo321_%s_us" % k] / row["old421_%s_us" % k], 3)
        row["no_longer_" + k] = row["geo321_%s_min_max_us" % k][0] <= row["old421_%s_min_max_us" % k][1]
    print(json.dumps(row), flush=True); rows.append(row)

    # (b) both families at (3,1,1)
    H1, C1, C0 = 16, 64, 128
    H0, t = tensors(H1, C1, C0, 3, 1, 1, 1)
    row = {"case": "(b) both families at (3,1,1), 16x16x64->128", "N": N}
    sides = []
    for (k, fn), (_, fo) in zip(geo_sides(t, (N, H1, H1, C1, H0, H0, C0, 3, 1, 1, 1), C1 * 9 * C0), old_sides(t, (N, H1, H1, C1, H0, H0, C0, 3, 1, 1), C1 * 9 * C0)):
        sides += [("geo_" + k, fn), ("old_" + k, fo)]
    measure(row, sides)
    for k in ("fwd", "dx", "dfdb"):
        row["geo_over_old_" + k] = round(row["geo_%s_us" % k] / row["old_%s_us" % k], 2)
    print(json.dumps(row), flush=True); rows.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
