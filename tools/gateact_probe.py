"""The smooth and gated feed-forward activations (t4k_gateact_fwd / _bwd): time per call at four shapes beside two yardsticks, neither of them
the code under test.  Yardstick 1 is the route the library has for a comparable activation on the same extents: t4k_activate(T4K_L_ELU), which stores a
derivative mask beside the output, and its backward t4k_tt_op(MUL) of dY with that mask - one more T C tensor each way.  For a gated row the extents are the
input's [T, C].  Yardstick 2, a ratio only, is torch's gelu / silu / mish (and silu(a) * b) with autograd on the same device.

    python tools/gateact_probe.py [--reps R] [--runs K] [--json profiles/gateact_probe.json] [--lib PATH]

The protocol of tools/token_ce_probe.py: each timing is the wall time of R back-to-back calls ending in a device synchronisation, divided by R; it is
repeated K times after a warm-up of every side, the sides of a row alternating within every repeat; the MEDIAN and the spread (min .. max) are reported,
with the launches of one call from t4k_launch_count.

  rows: 1 ViT-tiny FFN 25088 x 768 GELU;  2 GPT-2-small 8192 x 3072 tanh-GELU;  3 SwiGLU 8192 x 2 x 2048;  4 tiny 256 x 64 SiLU
  bars: the unit's slowest repeat no slower than yardstick 1's fastest, forward and backward ("met" | "MISSED"; the tiny row is launch-bound: "reported")
  hbm_fraction: SURVEY's byte rule (plain: forward 8, backward 12 bytes an element; gated: 12 and 20 an output element) over the median time, as a
        fraction of 8 TB/s.  A row whose tensors fit the 256 MiB last-level cache is served from it between back-to-back calls: no HBM figure there."""
import argparse
import ctypes
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VP = ctypes.c_void_p
HBM = 8.0e12
L_ELU, MUL = 9, 18
CASES = [("1 ViT-tiny 25088x768 gelu", 25088, 768, 0, 0), ("2 GPT-2-small 8192x3072 tanh-gelu", 8192, 3072, 1, 0),
         ("3 SwiGLU 8192x2x2048", 8192, 4096, 2, 1), ("4 tiny 256x64 silu", 256, 64, 2, 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rows", default="1234")
    ap.add_argument("--json")
    ap.add_argument("--lib")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(args.lib); h.init(0)
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    g = torch.Generator(device="cuda").manual_seed(1)
    p = lambda t: VP(t.data_ptr())
    fn = torch.nn.functional

    def timed(f):
        h.call("t4k_sync", None); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            f()
        h.call("t4k_sync", None); torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e6

    def measure(row, sides):
        times = {k: [] for k, _ in sides}
        for k, f in sides:
            f(); h.call("t4k_sync", None); torch.cuda.synchronize()    # warm: code objects loaded
            l0 = int(h.lib.t4k_launch_count()); f(); row["launches_" + k] = int(h.lib.t4k_launch_count()) - l0
        for _ in range(args.runs):
            for k, f in sides:
                times[k].append(timed(f))
        for k, _ in sides:
            row[k + "_us"] = round(statistics.median(times[k]), 2)
            row[k + "_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]

    def one(name, T, C, kind, gate):
        row = {"case": name, "T": T, "C": C, "kind": kind, "gate": gate}
        out = (ctypes.c_int * 8)(); h.call("t4k_gateact_plan", T, C, kind, gate, 1, out); row["plan"] = list(out)
        Hc = C // 2 if gate else C
        X = (torch.rand(T, C, device="cuda", generator=g) - 0.5) * 8.0
        DY = torch.randn(T, Hc, device="cuda", generator=g)
        Y, DX = torch.zeros(T, Hc, device="cuda"), torch.zeros(T, C, device="cuda")
        EY, EM, EDY, EDX = (torch.zeros(T, C, device="cuda") for _ in range(4))
        tx = X.clone().requires_grad_(True)
        tf = lambda a: (fn.silu(a[:, :Hc]) * a[:, Hc:]) if gate else (fn.gelu(a), fn.gelu(a, approximate="tanh"), fn.silu(a), fn.mish(a))[kind]
        ty, tdy = tf(tx), DY.clone()
        sides = [("ga_fwd", lambda: h.call("t4k_gateact_fwd", p(X), p(Y), T, C, kind, gate, None)),
                 ("elu_fwd", lambda: h.call("t4k_activate", L_ELU, p(X), p(EY), p(EM), 1.0, T * C, None)),
                 ("ga_bwd", lambda: h.call("t4k_gateact_bwd", p(X), p(DY), p(DX), T, C, kind, gate, None)),
                 ("elu_bwd", lambda: h.call("t4k_tt_op", MUL, p(EDY), p(EM), p(EDX), T * C, None)),
                 ("torch_fwd", lambda: tf(tx)),
                 ("torch_bwd", lambda: torch.autograd.grad(ty, (tx,), tdy, retain_graph=True))]
        measure(row, sides)
        for k, y in (("fwd", "elu_fwd"), ("bwd", "elu_bwd")):
            met = row["ga_" + k + "_min_max_us"][1] <= row[y + "_min_max_us"][0]
            row["bar_" + k] = "reported" if T * C < (1 << 20) else ("met" if met else "MISSED")
            row["ratio_" + k] = round(row["ga_" + k + "_us"] / row[y + "_us"], 3)
            row["ratio_torch_" + k] = round(row["ga_" + k + "_us"] / row["torch_" + k + "_us"], 3)
        fb, bb = (12.0 if gate else 8.0) * T * Hc, (20.0 if gate else 12.0) * T * Hc
        row["bytes"] = [fb, bb]
        row["hbm_fraction"] = [round(b / (row[k + "_us"] * 1e-6) / HBM, 3) for b, k in ((fb, "ga_fwd"), (bb, "ga_bwd"))]
        row["fits_llc"] = bool(bb < 256 * 2 ** 20)
        print(json.dumps(row), flush=True)
        return row

    rows = [one(*c) for c in CASES if c[0][0] in args.rows]
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "devices": 1, "date": datetime.date.today().isoformat(), "reps": args.reps, "runs": args.runs,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
