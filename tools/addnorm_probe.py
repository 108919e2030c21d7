"""Add & norm (t4k_addnorm_fwd / _bwd): time per call of forward and backward at six shapes, in mode 1 and mode 2 with a skip, the backward with
and without a dy2, beside two yardsticks, neither of them the code under test: the route the library already has - t4k_tt_op(T4K_ADD) then
t4k_groupnorm_fwd(rows, 1, C, 1), two launches, and t4k_tt_op(T4K_ADD) on the two gradients then t4k_groupnorm_bwd - and torch's layer_norm(x + s) and its autograd
of the installed torch-ROCm on the same device.  Mode 0 is timed against t4k_tt_op(T4K_ADD) alone (both move 12 bytes per element: reported, no bar).

    python tools/addnorm_probe.py [--reps R] [--runs K] [--json profiles/addnorm_probe.json]

The protocol of tools/attention_probe.py: each timing is the wall time of R back-to-back calls, bracketed by a device synchronisation, divided by R; it is repeated
K times, the sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported, with the dispatches of one
call from t4k_launch_count.

  rows: 1 ViT-tiny 128 x 196 tokens of 192;  2 256 x 64 of 128;  3 8 x 1024 of 512;  4 256 x 32 x 32 of 16;  5 4096 of 4096 (rung 2);  6 256 x 8 x 8 of 256
  bar: the fused launch's slowest repeat takes no longer than the composed route's fastest ("bar_fwd_m1" ...: met | MISSED), forward and backward, where the
       composed route is admitted: its dW | dB slab is one row per token, and the library refuses it above the workspace, forward and backward alike (the
       refusal is recorded and the fused side reported alone).  By bytes the fused forward moves 16 per element
       (x, s in; o, xhat out) against the composed route's 24.
  torch: the ratio, no bar.
  hbm_fraction: the bytes the rule needs (forward 16 per element, backward 12 and 16 with a dy2; the per-token and per-channel vectors beside them) over the time,
       as a fraction of the 8 TB/s of SURVEY.md."""
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
HBM = 8.0e12
T4K_ADD = 16
EPS = 1.0e-5

#        name, rows, C
CASES = [("1 ViT-tiny 128x196 C=192", 128 * 196, 192),
         ("2 256x64 C=128", 256 * 64, 128),
         ("3 8x1024 C=512", 8 * 1024, 512),
         ("4 256x32x32 C=16", 256 * 32 * 32, 16),
         ("5 4096 C=4096 (rung 2)", 4096, 4096),
         ("6 256x8x8 C=256", 256 * 8 * 8, 256)]


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

    def one(name, rows, C):
        n = rows * C
        row = {"case": name, "rows": rows, "C": C}
        for m in (0, 1, 2):
            out = I8(); h.call("t4k_addnorm_plan", rows, C, m, 1, 32 << 20, out); row["plan_m%d" % m] = list(out)
        X, S, DY, DY2 = rnd(rows, C), rnd(rows, C), rnd(rows, C), rnd(rows, C)
        O, XH, DX, Z, T = zeros(rows, C), zeros(rows, C), zeros(rows, C), zeros(rows, C), zeros(rows, C)
        R, STAT = zeros(rows), zeros(4 * rows)
        Wg, B, DW, DB = rnd(C) + 1.5, rnd(C), zeros(C), zeros(C)
        h.call("t4k_addnorm_fwd", p(X), p(S), p(O), p(XH), p(R), p(Wg), p(B), rows, C, 1, EPS, None)       # XH, RSTD for the backward sides
        # the composed route, where the library admits it: t4k_groupnorm_* plan one dW | dB slab row per "sample" - here per token - and refuse, forward and
        # backward alike, a call whose slab is above the workspace
        h.call("t4k_tt_op", T4K_ADD, p(X), p(S), p(Z), n, None)
        rcf = h.lib.t4k_groupnorm_fwd(p(Z), p(O), p(XH), p(Wg), p(B), p(STAT), rows, 1, C, 1, EPS, None)
        row["composed_fwd_admitted"] = rcf == 0
        if rcf != 0:
            row["composed_fwd_refusal"] = h.lib.t4k_last_error().decode()
            h.call("t4k_addnorm_fwd", p(X), p(S), p(O), p(XH), p(R), p(Wg), p(B), rows, C, 1, EPS, None)

        def composed_fwd():
            h.call("t4k_tt_op", T4K_ADD, p(X), p(S), p(Z), n, None)
            h.call("t4k_groupnorm_fwd", p(Z), p(O), p(XH), p(Wg), p(B), p(STAT), rows, 1, C, 1, EPS, None)

        def composed_bwd():
            h.call("t4k_tt_op", T4K_ADD, p(DY), p(DY2), p(T), n, None)
            h.call("t4k_groupnorm_bwd", p(Wg), p(T), p(XH), p(STAT), p(DX), p(DW), p(DB), rows, 1, C, 1, 1, None)

        rc = h.lib.t4k_groupnorm_bwd(p(Wg), p(T), p(XH), p(STAT), p(DX), p(DW), p(DB), rows, 1, C, 1, 1, None)
        row["composed_bwd_admitted"] = rc == 0
        if rc != 0:
            row["composed_bwd_refusal"] = h.lib.t4k_last_error().decode()
        tx, ts = rnd(rows, C).requires_grad_(True), rnd(rows, C).requires_grad_(True)
        tw, tb = (rnd(C) + 1.5).requires_grad_(True), rnd(C).requires_grad_(True)
        tfwd = lambda: torch.nn.functional.layer_norm(tx + ts, (C,), tw, tb, EPS)
        ty = tfwd()
        fwd = lambda m: (lambda: h.call("t4k_addnorm_fwd", p(X), p(S), p(O), p(XH), p(R), p(Wg), p(B), rows, C, m, EPS, None))
        bwd = lambda m, d2: (lambda: h.call("t4k_addnorm_bwd", p(Wg), p(DY), p(DY2) if d2 else None, p(XH), p(R), p(DX), p(DW), p(DB), rows, C, m, 1, None))
        sides = [("an_fwd_m1", fwd(1)), ("an_fwd_m2", fwd(2)), ("an_bwd_m1", bwd(1, 0)), ("an_bwd_m2", bwd(2, 0)), ("an_bwd_dy2_m1", bwd(1, 1)), ("an_bwd_dy2_m2", bwd(2, 1)),
                 ("an_fwd_m0", fwd(0)), ("tt_add", lambda: h.call("t4k_tt_op", T4K_ADD, p(X), p(S), p(Z), n, None)),
                 ] + ([("composed_fwd", composed_fwd)] if rcf == 0 else []) + ([("composed_bwd", composed_bwd)] if rc == 0 else []) + \
                [("torch_fwd", tfwd), ("torch_bwd", lambda: torch.autograd.grad(ty, (tx, ts, tw, tb), DY, retain_graph=True))]
        measure(row, sides)
        nbytes = {"an_fwd": 16.0 * n + 4.0 * rows + 8.0 * C, "an_bwd": 12.0 * n + 4.0 * rows + 12.0 * C, "an_bwd_dy2": 16.0 * n + 4.0 * rows + 12.0 * C}
        for m in (1, 2):
            for k in ("an_fwd", "an_bwd", "an_bwd_dy2"):
                row["hbm_fraction_%s_m%d" % (k, m)] = round(nbytes[k] / (row["%s_m%d_us" % (k, m)] * 1e-6) / HBM, 3)
            if rcf == 0:
                row["ratio_composed_fwd_m%d" % m] = round(row["an_fwd_m%d_us" % m] / row["composed_fwd_us"], 3)
                row["bar_fwd_m%d" % m] = "met" if row["an_fwd_m%d_min_max_us" % m][1] <= row["composed_fwd_min_max_us"][0] else "MISSED"
            if rc == 0:
                row["ratio_composed_bwd_m%d" % m] = round(row["an_bwd_dy2_m%d_us" % m] / row["composed_bwd_us"], 3)
                row["bar_bwd_m%d" % m] = "met" if row["an_bwd_dy2_m%d_min_max_us" % m][1] <= row["composed_bwd_min_max_us"][0] else "MISSED"
        row["ratio_torch_fwd"] = round(row["an_fwd_m1_us"] / row["torch_fwd_us"], 3)
        row["ratio_torch_bwd"] = round(row["an_bwd_dy2_m1_us"] / row["torch_bwd_us"], 3)
        row["ratio_m0_tt_add"] = round(row["an_fwd_m0_us"] / row["tt_add_us"], 3)
        row["hbm_fraction_an_fwd_m0"] = round(12.0 * n / (row["an_fwd_m0_us"] * 1e-6) / HBM, 3)
        print(json.dumps(row), flush=True)
        return row

    rows = [one(*c) for c in CASES if c[0][0] in args.rows]
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "devices": 1, "reps": args.reps, "runs": args.runs, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
