"""Grouped / depthwise convolution (t4k_conv2d_grp_fwd / _bwd): time per call of forward, dX and dF | dB at six layers, beside the only way
the library had to compute such a layer - t4k_conv2d_geo_fwd / _bwd on the SAME tensors with the block-diagonal dense filter, G times the arithmetic.

    python tools/conv_grp_probe.py [--reps R] [--runs K] [--json profiles/conv_grp_probe.json]

The method of tools/conv_geo_probe.py: each timing is the wall time of R back-to-back calls on the library's default stream, bracketed by t4k_sync, divided
by R; it is repeated K times, the two sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are
reported, with the dispatches of one call from t4k_launch_count.

  rows: 1 depthwise 3x3 / 1 P 1, 32x32x64, N 256;  2 depthwise 3x3 / 2 P 1, 112x112x32 -> 56x56x32, N 64;  3 depthwise 5x5 / 1 P 2, 16x16x128, N 256;
        4 multiplier 2, 3x3 / 1, 32x32x32 -> 64, N 256;  5 G = 32, 3x3 / 1, 16x16x128 -> 128 (Cg 4), N 256;  6 G = 2, 3x3 / 1, 16x16x128 -> 128 (Cg 64), N 256
  bar (rows 1-4): forward, dX and dF | dB each take no longer than the dense call, beyond the two spreads ("no_longer_*": the grouped side's fastest repeat
  against the dense side's slowest).  Rows 5 and 6 report the same comparison without a bar.
  bytes by the rule - I + F + O forward; dO + F + dX for dX; I + dO + the slabs for dF | dB - and their rate as a fraction of the 8 TB/s of SURVEY.md."""
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

#        name, N, H1, C1, C0, K, S, P, D, G
CASES = [("1 depthwise 3x3/1 P1 32x32x64", 256, 32, 64, 64, 3, 1, 1, 1, 64),
         ("2 depthwise 3x3/2 P1 112x112x32->56x56x32", 64, 112, 32, 32, 3, 2, 1, 1, 32),
         ("3 depthwise 5x5/1 P2 16x16x128", 256, 16, 128, 128, 5, 1, 2, 1, 128),
         ("4 multiplier 2 3x3/1 32x32x32->64", 256, 32, 32, 64, 3, 1, 1, 1, 32),
         ("5 G=32 3x3/1 16x16x128->128 (Cg 4)", 256, 16, 128, 128, 3, 1, 1, 1, 32),
         ("6 G=2 3x3/1 16x16x128->128 (Cg 64)", 256, 16, 128, 128, 3, 1, 1, 1, 2)]
HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rows", default="123456")
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(); h.init(0)
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    h.lib.t4k_conv_last_plan.restype = ctypes.c_char_p
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

    rows = []
    for name, N, H1, C1, C0, K, S, P, D, G in CASES:
        if name[0] not in args.rows:
            continue
        H0 = (H1 + 2 * P - D * (K - 1) - 1) // S + 1
        Cg1, Cg0 = C1 // G, C0 // G
        I, B, O, Gr, DX = rnd(N, H1, H1, C1), rnd(C0), torch.zeros(N, H0, H0, C0, device="cuda"), rnd(N, H0, H0, C0), torch.zeros(N, H1, H1, C1, device="cuda")
        F = rnd(Cg1, K, K, C0)
        dense = torch.zeros(C1, K, K, C0, device="cuda")
        for q in range(G):
            dense[q * Cg1:(q + 1) * Cg1, :, :, q * Cg0:(q + 1) * Cg0] = F[:, :, :, q * Cg0:(q + 1) * Cg0]
        ndf, ndd = Cg1 * K * K * C0, C1 * K * K * C0
        DFB, DDB = torch.zeros(ndf + C0, device="cuda"), torch.zeros(ndd + C0, device="cuda")
        p = lambda t: V(t.data_ptr())
        geo = (N, H1, H1, C1, H0, H0, C0, K, S, P, D)
        out = I8(); h.call("t4k_conv2d_grp_plan", N, H1, H1, C1, C0, K, S, P, D, G, 1, out)
        row = {"case": name, "N": N, "plan": list(out)}
        sides = [("grp_fwd", lambda: h.call("t4k_conv2d_grp_fwd", p(I), None, p(O), p(F), p(B), *geo, G, None)),
                 ("dense_fwd", lambda: h.call("t4k_conv2d_geo_fwd", p(I), None, p(O), p(dense), p(B), *geo, None)),
                 ("grp_dx", lambda: h.call("t4k_conv2d_grp_bwd", p(I), p(Gr), p(DX), None, p(F), None, None, *geo, G, 0, None)),
                 ("dense_dx", lambda: h.call("t4k_conv2d_geo_bwd", p(I), p(Gr), p(DX), None, p(dense), None, None, *geo, 0, None)),
                 ("grp_dfdb", lambda: h.call("t4k_conv2d_grp_bwd", p(I), p(Gr), None, None, p(F), p(DFB), V(DFB.data_ptr() + 4 * ndf), *geo, G, 1, None)),
                 ("dense_dfdb", lambda: h.call("t4k_conv2d_geo_bwd", p(I), p(Gr), None, None, p(dense), p(DDB), V(DDB.data_ptr() + 4 * ndd), *geo, 1, None))]
        measure(row, sides)
        nbytes = {"fwd": 4 * (I.numel() + F.numel() + O.numel()), "dx": 4 * (Gr.numel() + F.numel() + DX.numel()),
                  "dfdb": 4 * (I.numel() + Gr.numel() + out[5] * (ndf + C0))}
        for k in ("fwd", "dx", "dfdb"):
            row["ratio_" + k] = round(row["grp_%s_us" % k] / row["dense_%s_us" % k], 3)
            row["no_longer_" + k] = row["grp_%s_min_max_us" % k][0] <= row["dense_%s_min_max_us" % k][1]
            row["bytes_" + k] = nbytes[k]
            row["hbm_fraction_" + k] = round(nbytes[k] / (row["grp_%s_us" % k] * 1e-6) / HBM, 3)
        print(json.dumps(row), flush=True); rows.append(row)
        del I, O, Gr, DX, dense, DFB, DDB
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
