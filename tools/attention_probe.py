"""Attention (t4k_attention_fwd / _bwd): time per call of forward and backward at seven shapes, beside two yardsticks, neither of them the code
under test: the composed route the product already has - t4k_gemm_batched for Q K^T, a t4k_math scale, t4k_softmax_axes, t4k_gemm_batched for P V - on operands
already laid out as [N heads, L, d], so no permute is charged to it (it has no mask: the causal rows are held against the same unmasked route, and no backward), and
torch's scaled_dot_product_attention and its autograd of the installed torch-ROCm on the same device.

    python tools/attention_probe.py [--reps R] [--runs K] [--json profiles/attention_probe.json]

The protocol of tools/groupnorm_probe.py: each timing is the wall time of R back-to-back calls, bracketed by a device synchronisation, divided by R; it is repeated
K times, the sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported, with the dispatches of one
call from t4k_launch_count.

  rows: 1 ViT-tiny-like L 196, 3 heads of 64, N 128;  2 L 64, 4 heads of 32, N 256;  3 L 1024, 8 heads of 64, N 8;  4-6 the same three causal;
        7 L 16, 2 heads of 16, N 256
  bar: the fused forward's slowest repeat takes no longer than the composed route's fastest ("bar_fwd": met | MISSED).  The backward is reported, not barred.
  torch: the ratio, no bar.
  FLOP by the rule 4 L^2 d heads N forward (half of it causal), 2.5 times that backward, and their rate as a fraction of the 157.3 TFLOP/s of SURVEY.md."""
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
I4 = ctypes.c_int * 4
PEAK = 157.3e12
T4K_SCALE = 14

#        name, N, L, heads, d, causal
CASES = [("1 ViT-tiny-like L=196 h=3 d=64 N=128", 128, 196, 3, 64, 0),
         ("2 L=64 h=4 d=32 N=256", 256, 64, 4, 32, 0),
         ("3 L=1024 h=8 d=64 N=8", 8, 1024, 8, 64, 0),
         ("4 causal L=196 h=3 d=64 N=128", 128, 196, 3, 64, 1),
         ("5 causal L=64 h=4 d=32 N=256", 256, 64, 4, 32, 1),
         ("6 causal L=1024 h=8 d=64 N=8", 8, 1024, 8, 64, 1),
         ("7 L=16 h=2 d=16 N=256", 256, 16, 2, 16, 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rows", default="1234567")
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

    def one(name, N, L, heads, d, causal):
        out = I8(); h.call("t4k_attention_plan", N, L, heads, d, causal, 1, 32 << 20, out)
        E, B = heads * d, N * heads
        QKV, DY = rnd(N, L, 3 * E), rnd(N, L, E)
        O, OK, LSE, G = zeros(N, L, E), zeros(N, L, E), zeros(N, heads, L), zeros(N, L, 3 * E)
        row = {"case": name, "N": N, "L": L, "heads": heads, "d": d, "causal": causal, "plan": list(out)}
        scale = float(d) ** -0.5
        # the composed route on [N heads, L, d] operands
        q, k, v = rnd(B, L, d), rnd(B, L, d), rnd(B, L, d)
        S, Y = zeros(B, L, L), zeros(B, L, d)
        dim = I4(B, L, L, 1)

        def composed():
            h.call("t4k_gemm_batched", p(q), p(k), p(S), 1.0, 0.0, 0, 1, L, L, d, 1, 1, 1, B, L * d, L * d, L * L, None)
            h.call("t4k_math", T4K_SCALE, p(S), scale, B * L * L, None)
            h.call("t4k_softmax_axes", p(S), p(S), dim, 2, None)
            h.call("t4k_gemm_batched", p(S), p(v), p(Y), 1.0, 0.0, 0, 0, L, d, L, 1, 1, 1, B, L * L, L * d, L * d, None)

        tq, tk, tv = (rnd(N, heads, L, d).requires_grad_(True) for _ in range(3))
        tgy = rnd(N, heads, L, d)
        sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(tq, tk, tv, is_causal=bool(causal))
        ty = sdpa()
        sides = [("attn_fwd", lambda: h.call("t4k_attention_fwd", p(QKV), p(O), p(OK), p(LSE), N, L, heads, d, causal, None)),
                 ("attn_bwd", lambda: h.call("t4k_attention_bwd", p(QKV), p(OK), p(DY), p(LSE), p(G), N, L, heads, d, causal, None)),
                 ("composed_fwd", composed),
                 ("torch_fwd", sdpa),
                 ("torch_bwd", lambda: torch.autograd.grad(ty, (tq, tk, tv), tgy, retain_graph=True))]
        measure(row, sides)
        flop = 4.0 * L * L * d * heads * N * (0.5 if causal else 1.0)
        row["flop_fwd"] = flop; row["flop_bwd"] = 2.5 * flop
        for kk in ("fwd", "bwd"):
            row["peak_fraction_" + kk] = round(row["flop_" + kk] / (row["attn_%s_us" % kk] * 1e-6) / PEAK, 4)
            row["ratio_torch_" + kk] = round(row["attn_%s_us" % kk] / row["torch_%s_us" % kk], 3)
        row["ratio_composed_fwd"] = round(row["attn_fwd_us"] / row["composed_fwd_us"], 3)
        row["bar_fwd"] = "met" if row["attn_fwd_min_max_us"][1] <= row["composed_fwd_min_max_us"][0] else "MISSED"
        print(json.dumps(row), flush=True)
        return row

    rows = [one(*c) for c in CASES if c[0][0] in args.rows]
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "devices": 1, "reps": args.reps, "runs": args.runs, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
