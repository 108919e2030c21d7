"""Batched products: t4k_gemm_batched (one launch) against the per-matrix t4k_gemm loop on the same device.

    python tools/bmm_probe.py [--reps R] [--once] [--json out.json]

Cases: 128 x 28^3, 128 x 64^3 with C = 3, 64 x 256^3, 8 x 1024^3 (fp32, NHWC, A[b] @ B[b]).  Each timing is the wall time of R back-to-back
calls on the library's default stream, bracketed by t4k_sync, divided by R (so it includes the dispatches the loop pays for); TF/s and the
fraction of the 157.3 TF fp32 MFMA peak are computed from 2 M N K C batch.  --once: one call of each path per case and nothing else
(the run to put under `rocprofv3 --kernel-trace --stats -- python tools/bmm_probe.py --once`: dispatch counts per call)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 157.3
CASES = [(128, 28, 28, 28, 1), (128, 64, 64, 64, 3), (64, 256, 256, 256, 1), (8, 1024, 1024, 1024, 1)]   # batch, M, N, K, C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(); h.init(0)
    rows = []
    for batch, M, N, K, C in CASES:
        g = torch.Generator(device="cuda").manual_seed(1)
        A = torch.randn(batch * M * K * C, device="cuda", generator=g)
        B = torch.randn(batch * K * N * C, device="cuda", generator=g)
        O1 = torch.zeros(batch * M * N * C, device="cuda"); O2 = torch.zeros_like(O1)
        torch.cuda.synchronize()
        pa, pb, p1, p2 = (t.data_ptr() for t in (A, B, O1, O2))
        sA, sB, sO = M * K * C, K * N * C, M * N * C

        def batched():
            h.call("t4k_gemm_batched", ctypes.c_void_p(pa), ctypes.c_void_p(pb), ctypes.c_void_p(p1), 1.0, 0.0, 0, 0,
                   M, N, K, C, C, C, batch, sA, sB, sO, None)

        def loop():
            for b in range(batch):
                h.call("t4k_gemm", ctypes.c_void_p(pa + 4 * b * sA), ctypes.c_void_p(pb + 4 * b * sB), ctypes.c_void_p(p2 + 4 * b * sO),
                       1.0, 0.0, 0, 0, M, N, K, C, None)

        def timed(fn, reps):
            fn(); h.call("t4k_sync", None)                              # warm: code objects loaded, LDS attributes set
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            h.call("t4k_sync", None)
            return (time.perf_counter() - t0) / reps

        if args.once:
            l0 = h.lib.t4k_launch_count(); batched(); l1 = h.lib.t4k_launch_count(); loop(); l2 = h.lib.t4k_launch_count()
            h.call("t4k_sync", None)
            rows.append({"case": "%d x %dx%dx%d C=%d" % (batch, M, N, K, C), "launches_batched": l1 - l0, "launches_loop": l2 - l1})
        else:
            reps = max(3, args.reps if M < 1024 else args.reps // 5)
            tb, tl = timed(batched, reps), timed(loop, reps)
            diff = float((O1 - O2).abs().max())
            flop = 2.0 * batch * M * N * K * C
            rows.append({"case": "%d x %dx%dx%d C=%d" % (batch, M, N, K, C), "batched_us": round(tb * 1e6, 2), "loop_us": round(tl * 1e6, 2),
                         "speedup": round(tl / tb, 2), "batched_tflops": round(flop / tb / 1e12, 2),
                         "batched_frac_peak": round(flop / tb / 1e12 / PEAK_TF, 3), "max_abs_diff_vs_loop": diff})
        print(json.dumps(rows[-1]), flush=True)
        del A, B, O1, O2
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
