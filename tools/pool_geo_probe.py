"""Run-time-geometry pooling (t4k_pool_geo_fwd / _bwd): time per call of forward and backward for max and avg at six layers, the
bytes each call moves by the rule and the achieved GB/s, and - on the two layers both families admit - the old entries t4k_pool / t4k_dpool of the
same library on the same tensors in the same run.

    python tools/pool_geo_probe.py [--reps R] [--runs K] [--json profiles/pool_geo_probe.json]

Each timing is the wall time of R back-to-back calls on the library's default stream, bracketed by t4k_sync, divided by R; it is repeated K times, the
sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported.

  rows: 3x3 / 2 P 1, 112x112x64 -> 56x56x64, N = 64;  3x3 / 1 P 1, 32x32x64, N = 256;  global 7x7 on 7x7x512, N = 256;  global 16x16 on 16x16x64, N = 256;
        2x2 / 2, 32x32x64 -> 16x16x64, N = 256;  3x3 / 3, 48x48x64 -> 16x16x64, N = 256
  bytes by the rule: forward I + O + codes (one byte per max / min output element, none for avg), backward codes + dY + dX; GB/s against SURVEY's 8 TB/s
  the bar, on the last two rows against t4k_pool / t4k_dpool: the avg forward and every backward take no longer than the old entry, the max / min
  forward no longer than the old entry's time x (I + O + codes) / (I + O) - "no longer" beyond the two spreads: new min <= allowed old max."""
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
AVG, MAXP, MINP = 13, 14, 15                                              # T4K_L_* of include/t4k.h
PEAK_GBS = 8000.0

# name, N, H1, W1, C, K, S, P, beside the old entries
CASES = [("3x3/2 P1 112x112x64->56x56x64", 64, 112, 112, 64, 3, 2, 1, False),
         ("3x3/1 P1 32x32x64", 256, 32, 32, 64, 3, 1, 1, False),
         ("global 7x7 on 7x7x512", 256, 7, 7, 512, 7, 7, 0, False),
         ("global 16x16 on 16x16x64", 256, 16, 16, 64, 16, 16, 0, False),
         ("2x2/2 32x32x64->16x16x64", 256, 32, 32, 64, 2, 2, 0, True),
         ("3x3/3 48x48x64->16x16x64", 256, 48, 48, 64, 3, 3, 0, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(); h.init(0)
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
        for _ in range(args.runs):
            for k, fn in sides:
                times[k].append(timed(fn))
        for k, _ in sides:
            row[k + "_us"] = round(statistics.median(times[k]), 2)
            row[k + "_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]

    rows = []
    for name, N, H1, W1, C, K, S, P, beside in CASES:
        H0, W0 = (H1 + 2 * P - K) // S + 1, (W1 + 2 * P - K) // S + 1
        I, O, G, DX = rnd(N, H1, W1, C), torch.zeros(N, H0, W0, C, device="cuda"), rnd(N, H0, W0, C), torch.zeros(N, H1, W1, C, device="cuda")
        CODE = torch.zeros(N * H0 * W0 * ((C + 3) // 4), device="cuda")
        X = I.clone() if beside else None                                # t4k_dpool works in place on the forward input: a copy of its own
        p = {k: V(t.data_ptr()) for k, t in dict(I=I, O=O, G=G, DX=DX, CODE=CODE).items()}
        geo = (N, H1, W1, C, H0, W0, K, S, P)
        nI, nO = 4 * I.numel(), 4 * O.numel()
        ncode = N * H0 * W0 * 4 * ((C + 3) // 4)
        row = {"case": name, "N": N, "out": [H0, W0]}
        sides = []
        layers = [("max", MAXP), ("avg", AVG)] + ([("min", MINP)] if beside else [])
        for ln, L in layers:
            pc = None if L == AVG else p["CODE"]
            sides.append(("geo_%s_fwd" % ln, lambda L=L, pc=pc: h.call("t4k_pool_geo_fwd", L, p["I"], p["O"], pc, *geo, None)))
            if beside:
                sides.append(("old_%s_fwd" % ln, lambda L=L: h.call("t4k_pool", L, p["I"], p["O"], N, H1, W1, H0, W0, C, K, None)))
            sides.append(("geo_%s_bwd" % ln, lambda L=L, pc=pc: h.call("t4k_pool_geo_bwd", L, pc, p["G"], p["DX"], *geo, None)))
            if beside:
                sides.append(("old_%s_bwd" % ln, lambda L=L: h.call("t4k_dpool", L, V(X.data_ptr()), p["G"], N, H1, W1, H0, W0, C, K, None)))
        measure(row, sides)
        for ln, L in layers:
            codes = 0 if L == AVG else ncode
            for d, nbytes in (("fwd", nI + nO + codes), ("bwd", codes + nO + nI)):
                k = "geo_%s_%s" % (ln, d)
                row[k + "_bytes"] = nbytes
                row[k + "_gbs"] = round(nbytes / row[k + "_us"] / 1e3, 1)
                row[k + "_of_peak"] = round(nbytes / row[k + "_us"] / 1e3 / PEAK_GBS, 3)
                if beside:
                    allow = (nI + nO + codes) / (nI + nO) if d == "fwd" else 1.0
                    o = "old_%s_%s" % (ln, d)
                    row["ratio_%s_%s" % (ln, d)] = round(row[k + "_us"] / row[o + "_us"], 3)
                    row["allowed_%s_%s" % (ln, d)] = round(allow, 4)
                    row["met_%s_%s" % (ln, d)] = row[k + "_min_max_us"][0] <= row[o + "_min_max_us"][1] * allow
        print(json.dumps(row), flush=True); rows.append(row)
        del I, O, G, DX, CODE, X
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
