"""The embedding layer (t4k_embed_fwd / _bwd): time per call of forward and backward at five shapes beside two yardsticks, neither of them the
code under test: the route the library has without the layer - t4k_gemm of a prebuilt one-hot [T, V] matrix with the table forward, one-hot^T dY accumulated
onto the table gradient backward (for the position row a one-hot [T, L] of the positions, with the t4k_copy of x and of dY the route needs beside it);
building the one-hot rows is not charged to it - and torch's F.embedding (+ the position add) and its autograd of the installed torch-ROCm on the same device.

    python tools/embed_probe.py [--reps R] [--runs K] [--json profiles/embed_probe.json]

The protocol of tools/attention_probe.py / addnorm_probe.py: each timing is the wall time of R back-to-back calls, bracketed by a device synchronisation, divided
by R; it is repeated K times, the sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported, with
the dispatches of one call from t4k_launch_count.

  rows: 1 a character model V=65 E=128 L=256 N=64;  2 a BPE-sized table V=32768 E=512 L=512 N=16;  3 ViT-tiny positions (position mode) L=196 E=192 N=128;
        4 tiny, launch-bound V=16 E=8 L=16 N=2;  5 a mid vocabulary V=4096 E=256 L=128 N=64
  bar: the fused pass's slowest repeat takes no longer than the composed route's fastest ("bar_fwd", "bar_bwd": met | MISSED).
  torch: the ratio, no bar.
  hbm_fraction: the bytes the rule needs by SURVEY's byte rule (forward: ids + rows read + output written; backward: dY read once + the table rows touched,
       read and written, + the position table read and written) over the time, as a fraction of the 8 TB/s of SURVEY.md."""
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
I8 = ctypes.c_int * 8
HBM = 8.0e12

#        name, N, L, V, E, pos
CASES = [("1 char V=65 E=128 L=256 N=64", 64, 256, 65, 128, 1),
         ("2 BPE V=32768 E=512 L=512 N=16", 16, 512, 32768, 512, 1),
         ("3 ViT-tiny positions L=196 E=192 N=128", 128, 196, 0, 192, 1),
         ("4 tiny V=16 E=8 L=16 N=2", 2, 16, 16, 8, 1),
         ("5 mid V=4096 E=256 L=128 N=64", 64, 128, 4096, 256, 0)]


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
    rnd = lambda *s: (torch.rand(*s, device="cuda", generator=g) - 0.5) * 2.0
    zeros = lambda *s: torch.zeros(*s, device="cuda")
    p = lambda t: VP(t.data_ptr()) if t is not None else None

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

    def one(name, N, L, V, E, pos):
        T = N * L
        row = {"case": name, "N": N, "L": L, "V": V, "E": E, "pos": pos, "T": T}
        out = I8(); h.call("t4k_embed_plan", T, L, V, E, pos, 1, 32 << 20, out); row["plan"] = list(out)
        K = V if V else L                                                  # rows of the table the one-hot matrix selects from
        idx = torch.randint(0, V, (T,), device="cuda", generator=g) if V else (torch.arange(T, device="cuda") % L)
        IDS = idx.float() if V else None
        X = None if V else rnd(T, E)
        TAB = rnd(V, E) if V else None
        POS = rnd(L, E) * 0.02 if pos else None
        DY, O, DX = rnd(T, E), zeros(T, E), (None if V else zeros(T, E))
        DTAB, DPOS = (zeros(V, E) if V else None), (zeros(L, E) if pos else None)
        OH = torch.nn.functional.one_hot(idx, K).float().contiguous()
        W, DW = (TAB if V else POS), (DTAB if V else DPOS)

        def composed_fwd():                                                # O = onehot @ table (position row: O = x, then += onehot @ POS)
            if V:
                h.call("t4k_gemm", p(OH), p(W), p(O), 1.0, 0.0, 0, 0, T, E, K, 1, None)
            else:
                h.call("t4k_copy", p(X), p(O), T * E, None)
                h.call("t4k_gemm", p(OH), p(W), p(O), 1.0, 1.0, 0, 0, T, E, K, 1, None)

        def composed_bwd():                                                # dW += onehot^T @ dY (position row: and dX = dY)
            h.call("t4k_gemm", p(OH), p(DY), p(DW), 1.0, 1.0, 1, 0, K, E, T, 1, None)
            if not V:
                h.call("t4k_copy", p(DY), p(DX), T * E, None)

        tt = (rnd(V, E) if V else rnd(T, E)).requires_grad_(True)
        tp = (rnd(L, E) * 0.02).requires_grad_(True) if pos else None

        def tfwd():
            y = torch.nn.functional.embedding(idx, tt) if V else tt
            return (y.view(N, L, E) + tp).view(T, E) if pos else y
        ty = tfwd()
        sides = [("em_fwd", lambda: h.call("t4k_embed_fwd", p(IDS), p(X), p(TAB), p(POS), p(O), T, L, V, E, None)),
                 ("em_bwd", lambda: h.call("t4k_embed_bwd", p(IDS), p(DY), p(DTAB), p(DPOS), p(DX), T, L, V, E, 1, None)),
                 ("composed_fwd", composed_fwd), ("composed_bwd", composed_bwd),
                 ("torch_fwd", tfwd), ("torch_bwd", lambda: torch.autograd.grad(ty, (tt, tp) if pos else (tt,), DY, retain_graph=True))]
        measure(row, sides)
        touched = min(V, T) if V else 0
        fb = 4.0 * ((T if V else T * E) + T * E + T * E + (L * E if pos and V else 0) + (L * E if not V else 0))
        bb = 4.0 * (T * E + 2.0 * touched * E + (2.0 * L * E if pos else 0) + (T if V else T * E))
        row["bytes_fwd"], row["bytes_bwd"] = fb, bb
        row["hbm_fraction_fwd"] = round(fb / (row["em_fwd_us"] * 1e-6) / HBM, 3)
        row["hbm_fraction_bwd"] = round(bb / (row["em_bwd_us"] * 1e-6) / HBM, 3)
        for d in ("fwd", "bwd"):
            row["ratio_composed_" + d] = round(row["em_%s_us" % d] / row["composed_%s_us" % d], 4)
            row["bar_" + d] = "met" if row["em_%s_min_max_us" % d][1] <= row["composed_%s_min_max_us" % d][0] else "MISSED"
            row["ratio_torch_" + d] = round(row["em_%s_us" % d] / row["torch_%s_us" % d], 3)
        print(json.dumps(row), flush=True)
        return row

    rows = [one(*c) for c in CASES if c[0][0] in args.rows]
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "devices": 1, "reps": args.reps, "runs": args.runs, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
