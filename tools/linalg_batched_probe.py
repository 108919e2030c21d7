"""Batched linear algebra: each t4k_*_batched entry (one launch per call) against the loop of the per-matrix entry on the same device.

    python tools/linalg_batched_probe.py [--reps R] [--once] [--json out.json]

Cases: 128 x 4^2, 128 x 16^2, 1024 x 16^2, 128 x 64^2, 32 x 128^2, 8 x 512^2 (fp32, diagonally dominant entries).  Per case and entry three wall
times per call on the library's default stream, bracketed by t4k_sync and divided by the repetitions:
  batched       one t4k_*_batched call and ONE read-back of the int[batch] status array (what a word pays now);
  loop+readback the per-matrix entry once per matrix, each followed by the 4-byte status read-back and the sync the words paid per entry;
  loop          the same without the read-backs.
The factorisations work in place, so every repetition of every path first restores the inputs with one device copy of the whole batch (and, for
the per-matrix inverse / lu_inverse, one more of the identity those entries expect); det's loop is t4k_plu + t4k_logdet per matrix and, with
read-back, the three read-backs Tensor::det makes.  --once: one call of each path per case and nothing else (the run to put under
`rocprofv3 --kernel-trace --stats -- python tools/linalg_batched_probe.py --once`: dispatch counts per call)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(128, 4), (128, 16), (1024, 16), (128, 64), (32, 128), (8, 512)]      # batch, K
ENTRIES = ("inverse", "plu", "lu_inverse", "lu_extract", "det")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    import numpy as np
    import torch
    from tensorforth_amd.lib import load
    h = load(); h.init(0)
    h.call("t4k_set_default_stream", None)                       # the null stream: torch's restoring copies are ordered with the library's launches
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    V = ctypes.c_void_p
    rows = []
    for batch, K in CASES:
        rng = np.random.default_rng(K * 1000 + batch)
        A0 = torch.from_numpy((rng.standard_normal((batch, K, K)) + np.eye(K) * (2.0 + 3.0 * np.sqrt(K))).astype(np.float32)).cuda()
        I0 = torch.eye(K, device="cuda").repeat(batch, 1, 1).contiguous()
        A, X = torch.empty_like(A0), torch.empty_like(A0)
        piv = torch.zeros(batch * K, dtype=torch.int32, device="cuda"); st = torch.zeros(batch, dtype=torch.int32, device="cuda")
        ld = torch.zeros(batch, device="cuda"); sg = torch.zeros(batch, dtype=torch.int32, device="cuda"); det = torch.zeros(batch, device="cuda")
        hst = (ctypes.c_int * batch)(); hpiv = (ctypes.c_int * K)(); one = ctypes.c_int(0); fone = ctypes.c_float(0)
        pa, px, pp, ps, pl, pg, pd = (t.data_ptr() for t in (A, X, piv, st, ld, sg, det))
        kk = 4 * K * K

        def read(dst, src, n):
            h.call("t4k_memcpy_d2h", ctypes.byref(dst), V(src), n, None); h.call("t4k_sync", None)

        def batched(e):
            A.copy_(A0)
            if e == "inverse": h.call("t4k_inverse_batched", V(pa), V(px), K, batch, V(ps), None)
            elif e == "plu": h.call("t4k_plu_batched", V(pa), V(px), V(pp), K, batch, V(ps), None)
            elif e == "lu_inverse": h.call("t4k_lu_inverse_batched", V(pa), V(px), V(pp), K, batch, V(ps), None)
            elif e == "lu_extract": h.call("t4k_lu_extract_batched", V(pa), 1, K, batch, None); return
            else: h.call("t4k_det_batched", V(pa), V(pp), K, batch, V(pd), V(ps), None)
            read(hst, ps, 4 * batch)

        def loop(e, readback):
            A.copy_(A0)
            if e in ("inverse", "lu_inverse", "plu"): X.copy_(I0)
            for b in range(batch):
                a, x, pv, s = V(pa + b * kk), V(px + b * kk), V(pp + 4 * b * K), V(ps + 4 * b)
                if e == "inverse": h.call("t4k_inverse", a, x, K, s, None)
                elif e == "plu": h.call("t4k_plu", a, x, pv, K, s, None)
                elif e == "lu_inverse": h.call("t4k_lu_inverse", a, x, pv, K, s, None)
                elif e == "lu_extract": h.call("t4k_lu_extract", a, 1, K, None); continue
                else:
                    h.call("t4k_plu", a, None, pv, K, s, None)
                    if readback: read(one, ps + 4 * b, 4); read(hpiv, pp + 4 * b * K, 4 * K)      # status, then the pivots (Tensor::det reads K ints)
                    h.call("t4k_logdet", a, K, V(pl + 4 * b), V(pg + 4 * b), None)
                    if readback: read(fone, pl + 4 * b, 4)
                if readback: read(one, ps + 4 * b, 4)

        def timed(fn, reps):
            fn(); h.call("t4k_sync", None)                              # warm: code objects loaded, LDS attributes set
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            h.call("t4k_sync", None)
            return (time.perf_counter() - t0) / reps

        for e in ENTRIES:
            case = "%d x %dx%d" % (batch, K, K)
            if args.once:
                l0 = h.lib.t4k_launch_count(); batched(e); l1 = h.lib.t4k_launch_count(); loop(e, False); l2 = h.lib.t4k_launch_count()
                h.call("t4k_sync", None)
                rows.append({"case": case, "entry": e, "launches_batched": l1 - l0, "launches_loop": l2 - l1})
            else:
                reps = max(2, args.reps if K <= 64 else args.reps // 5 if K <= 128 else 2)
                tb = timed(lambda: batched(e), reps)
                ref = (X if e in ("inverse", "lu_inverse") else det if e == "det" else A).clone()
                tr, tl = timed(lambda: loop(e, True), reps), timed(lambda: loop(e, False), reps)
                row = {"case": case, "entry": e, "batched_us": round(tb * 1e6, 1), "loop_readback_us": round(tr * 1e6, 1), "loop_us": round(tl * 1e6, 1),
                       "speedup_vs_loop_readback": round(tr / tb, 1), "speedup_vs_loop": round(tl / tb, 1)}
                if e != "det":
                    row["max_abs_diff_vs_loop"] = float(((X if e in ("inverse", "lu_inverse") else A) - ref).abs().max())
                rows.append(row)
            print(json.dumps(rows[-1]), flush=True)
        del A0, I0, A, X
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
