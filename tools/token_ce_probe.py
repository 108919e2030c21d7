"""The per-token softmax / cross-entropy head (t4k_token_softmax_fwd, t4k_token_ce_bwd, t4k_token_ce_score): time per call at five shapes
beside two yardsticks, neither of them the code under test.  Yardstick 1 is the route the library has without the unit, on the same buffers: forward - the
faster of t4k_softmax(x, p, T, V) and t4k_softmax_axes with mask 1; backward - t4k_tt_op(SUB) against a prebuilt one-hot [T, V], whose construction is not
charged; loss - Tensor::loss's sequence (copy, LN map, MUL by the one-hot, sum, read-back of the scalar).  Yardstick 2, a ratio only, is torch's
cross_entropy(reduction="sum") forward and its autograd on the same device.

    python tools/token_ce_probe.py [--reps R] [--runs K] [--json profiles/token_ce_probe.json]

The protocol of tools/embed_probe.py: each timing is the wall time of R back-to-back calls ending in a device synchronisation, divided by R; it is repeated K
times after a warm-up of every side, the sides of a row alternating within every repeat; the MEDIAN and the spread (min .. max) are reported, with the
launches of one call from t4k_launch_count.

  rows: 1 a character model V=65 T=16384;  2 V=4096 T=8192;  3 a BPE-sized V=32768 T=4096;  4 the first two-pass shape V=8196 T=4096;  5 tiny V=11 T=32
  bars: forward - the unit's median no slower than yardstick 1's beyond the sum of the two spreads; CE backward and score - the unit's slowest repeat
        faster than the composed route's fastest ("met" | "MISSED"; the tiny row's backward is reported, not barred).
  hbm_fraction: SURVEY's byte rule (forward 8 T V + 8 T bytes, CE backward 8 T V + 4 T, score 16 T + a 64-byte sector per gathered P) over the time, as a
        fraction of 8 TB/s.  A row whose tensors fit the 256 MiB last-level cache is served from it between back-to-back calls: no HBM figure there."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VP = ctypes.c_void_p
HBM = 8.0e12
LN, SUB, MUL, RED_SUM = 3, 17, 18, 0
CASES = [("1 char V=65 T=16384", 16384, 65), ("2 V=4096 T=8192", 8192, 4096), ("3 BPE V=32768 T=4096", 4096, 32768),
         ("4 first two-pass V=8196 T=4096", 4096, 8196), ("5 tiny V=11 T=32", 32, 11)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rows", default="12345")
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(); h.init(0)
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    g = torch.Generator(device="cuda").manual_seed(1)
    p = lambda t: VP(t.data_ptr())

    def timed(fn):
        h.call("t4k_sync", None); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        h.call("t4k_sync", None); torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e6

    def measure(row, sides):
        times = {k: [] for k, _ in sides}
        for k, fn in sides:
            fn(); h.call("t4k_sync", None); torch.cuda.synchronize()    # warm: code objects loaded
            l0 = int(h.lib.t4k_launch_count()); fn(); row["launches_" + k] = int(h.lib.t4k_launch_count()) - l0
        for _ in range(args.runs):
            for k, fn in sides:
                times[k].append(timed(fn))
        for k, _ in sides:
            row[k + "_us"] = round(statistics.median(times[k]), 2)
            row[k + "_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]

    def one(name, T, V):
        row = {"case": name, "T": T, "V": V}
        out = (ctypes.c_int * 8)(); h.call("t4k_token_ce_plan", T, V, 1, 32 << 20, out); row["plan"] = list(out)
        X = (torch.rand(T, V, device="cuda", generator=g) - 0.5) * 8.0
        idx = torch.randint(0, V, (T,), device="cuda", generator=g)
        IDS, OH = idx.float(), torch.nn.functional.one_hot(idx, V).float().contiguous()
        P, P2, DX, TMP = (torch.zeros(T, V, device="cuda") for _ in range(4))
        STAT, REC, SC = torch.zeros(T, 2, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
        host = ctypes.c_float()
        dim = (ctypes.c_int * 4)(1, 1, T, V)

        def composed_loss():                                               # Tensor::loss(CE): a copy of the output, ln, times the target, the sum read back
            h.call("t4k_copy", p(P), p(TMP), T * V, None)
            h.call("t4k_math", LN, p(TMP), 0.0, T * V, None)
            h.call("t4k_tt_op", MUL, p(TMP), p(OH), p(TMP), T * V, None)
            h.call("t4k_reduce", RED_SUM, p(TMP), T * V, 0.0, p(SC), None)
            h.call("t4k_memcpy_d2h", ctypes.byref(host), p(SC), 4, None); h.call("t4k_sync", None)

        def score():
            h.call("t4k_token_ce_score", p(P), p(STAT), p(IDS), p(REC), T, V, None)
            h.call("t4k_memcpy_d2h", ctypes.byref(host), p(REC), 4, None); h.call("t4k_sync", None)
        tx = X.clone().requires_grad_(True)
        tl = torch.nn.functional.cross_entropy(tx, idx, reduction="sum")
        sides = [("tc_fwd", lambda: h.call("t4k_token_softmax_fwd", p(X), p(P), p(STAT), T, V, None)),
                 ("softmax_fwd", lambda: h.call("t4k_softmax", p(X), p(P2), T, V, None)),
                 ("axes_fwd", lambda: h.call("t4k_softmax_axes", p(X), p(P2), dim, 1, None)),
                 ("tc_bwd", lambda: h.call("t4k_token_ce_bwd", p(P), p(IDS), p(DX), T, V, None)),
                 ("composed_bwd", lambda: h.call("t4k_tt_op", SUB, p(P), p(OH), p(DX), T * V, None)),
                 ("tc_score", score), ("composed_loss", composed_loss),
                 ("torch_fwd", lambda: torch.nn.functional.cross_entropy(tx, idx, reduction="sum")),
                 ("torch_bwd", lambda: torch.autograd.grad(tl, (tx,), retain_graph=True))]
        measure(row, sides)
        spread = lambda k: row[k + "_min_max_us"][1] - row[k + "_min_max_us"][0]
        y1 = min(("softmax_fwd", "axes_fwd"), key=lambda k: row[k + "_us"])
        row["yardstick_fwd"] = y1
        row["bar_fwd"] = "met" if row["tc_fwd_us"] <= row[y1 + "_us"] + spread("tc_fwd") + spread(y1) else "MISSED"
        for k, y in (("tc_bwd", "composed_bwd"), ("tc_score", "composed_loss")):
            row["bar_" + k[3:]] = "met" if row[k + "_min_max_us"][1] < row[y + "_min_max_us"][0] else "MISSED"
        row["ratio_fwd"], row["ratio_bwd"] = round(row["tc_fwd_us"] / row[y1 + "_us"], 3), round(row["tc_bwd_us"] / row["composed_bwd_us"], 3)
        row["ratio_score"] = round(row["tc_score_us"] / row["composed_loss_us"], 3)
        row["ratio_torch_fwd"] = round((row["tc_fwd_us"] + row["tc_score_us"]) / row["torch_fwd_us"], 3)
        row["ratio_torch_bwd"] = round(row["tc_bwd_us"] / row["torch_bwd_us"], 3)
        fb, bb, sb = 8.0 * T * V + 8.0 * T, 8.0 * T * V + 4.0 * T, 16.0 * T + 64.0 * T
        row["bytes"] = [fb, bb, sb]
        row["hbm_fraction"] = [round(b / (row[k + "_us"] * 1e-6) / HBM, 3) for b, k in ((fb, "tc_fwd"), (bb, "tc_bwd"), (sb, "tc_score"))]
        row["fits_llc"] = bool(3 * 4.0 * T * V < 256 * 2 ** 20)
        print(json.dumps(row), flush=True)
        return row

    rows = [one(*c) for c in CASES if c[0][0] in args.rows]
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "devices": 1, "reps": args.reps, "runs": args.runs, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
