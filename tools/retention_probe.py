"""Retention (t4k_retention_fwd / _bwd): time per call of forward and backward at four sequence lengths, beside the one causal mixer the
product had before it, t4k_attention_fwd / _bwd with causal = 1 on the same N, heads and d - a yardstick, not the code under test.

    python tools/retention_probe.py [--reps R] [--runs K] [--json profiles/retention_probe.json]

The protocol of tools/attention_probe.py: each timing is the wall time of R back-to-back calls, bracketed by a device synchronisation, divided by R; it is
repeated K times, the sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported, with the
dispatches of one call from t4k_launch_count.

  rows: L = 256, 1024, 4096, 16384 at 8 heads of 64, N = 16384 / L
  bar, from L = 4096 up: retention's slowest repeat takes no longer than attention's fastest, forward and backward ("bar_fwd", "bar_bwd": met | MISSED)
  FLOP by the chunkwise count per token and head, the in-chunk products at their causal half: forward 2 B d + 4 d^2 (scores, output; cross term, state),
  backward 6 B d + 8 d^2; their rate as a fraction of the 157.3 TFLOP/s of SURVEY.md."""
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
PEAK = 157.3e12
HEADS, D, TOKENS = 8, 64, 16384


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(); h.init(0)
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: (torch.rand(*s, device="cuda", generator=g) - 0.5) * 2.0
    zeros = lambda *s: torch.zeros(*s, device="cuda")
    p = lambda t: V(t.data_ptr())

    def timed(fn):
        h.call("t4k_sync", None); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        h.call("t4k_sync", None); torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e6

    def one(L):
        N, E = TOKENS // L, HEADS * D
        out = I8(); h.call("t4k_retention_plan", N, L, HEADS, D, 1, 32 << 20, out)
        B, chunks = out[2], out[3]
        QKV, DY = rnd(N, L, 3 * E), rnd(N, L, E)
        O, OK, LSE, G, ST = zeros(N, L, E), zeros(N, L, E), zeros(N, HEADS, L), zeros(N, L, 3 * E), zeros(N, HEADS, chunks, D, D)
        row = {"case": "L=%d h=%d d=%d N=%d" % (L, HEADS, D, N), "N": N, "L": L, "heads": HEADS, "d": D, "plan": list(out)}
        sides = [("retn_fwd", lambda: h.call("t4k_retention_fwd", p(QKV), p(O), p(ST), N, L, HEADS, D, None)),
                 ("attn_fwd", lambda: h.call("t4k_attention_fwd", p(QKV), p(O), p(OK), p(LSE), N, L, HEADS, D, 1, None)),
                 ("retn_bwd", lambda: h.call("t4k_retention_bwd", p(QKV), p(DY), p(ST), p(G), N, L, HEADS, D, None)),
                 ("attn_bwd", lambda: h.call("t4k_attention_bwd", p(QKV), p(OK), p(DY), p(LSE), p(G), N, L, HEADS, D, 1, None))]
        times = {k: [] for k, _ in sides}
        for k, fn in sides:
            fn(); h.call("t4k_sync", None); torch.cuda.synchronize()    # warm: code objects loaded (and ST, OK, LSE hold a forward's results)
            l0 = int(h.lib.t4k_launch_count()); fn(); row["launches_" + k] = int(h.lib.t4k_launch_count()) - l0
        for _ in range(args.runs):
            for k, fn in sides:
                times[k].append(timed(fn))
        for k, _ in sides:
            row[k + "_us"] = round(statistics.median(times[k]), 2)
            row[k + "_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
        per = {"fwd": 2.0 * B * D + 4.0 * D * D, "bwd": 6.0 * B * D + 8.0 * D * D}
        for kk in ("fwd", "bwd"):
            row["flop_" + kk] = per[kk] * TOKENS * HEADS
            row["peak_fraction_" + kk] = round(row["flop_" + kk] / (row["retn_%s_us" % kk] * 1e-6) / PEAK, 4)
            row["ratio_attn_" + kk] = round(row["retn_%s_us" % kk] / row["attn_%s_us" % kk], 3)
            if L >= 4096:
                row["bar_" + kk] = "met" if row["retn_%s_min_max_us" % kk][1] <= row["attn_%s_min_max_us" % kk][0] else "MISSED"
        print(json.dumps(row), flush=True)
        return row

    rows = [one(L) for L in (256, 1024, 4096, 16384)]
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "devices": 1, "reps": args.reps, "runs": args.runs, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
