"""Axis permutation: t4k_permute beside the entry it doubles (t4k_transpose_batched) and beside the floor of any data movement (t4k_copy of
the same byte count), on the same device in the same run.

    python tools/permute_probe.py [--reps R] [--runs K] [--json profiles/permute_probe.json]

Each timing is the wall time of R back-to-back calls on the library's default stream, bracketed by t4k_sync, divided by R; it is repeated K
times, the paths alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported, with the
dispatches of one call from t4k_launch_count.  GB/s = 8 bytes per element (one read, one write) over the median.

  (a) 8241 on (128,64,64,1) and (64,128,128,3) beside t4k_transpose_batched on the same buffers: the bar is "no slower beyond the two spreads"
  (b) 8142 (NHWC -> channel-first) on (256,32,32,64) and (128,224,224,3) beside t4k_copy
  (c) 8412 ([N,L,heads,D] -> [N,L,D,heads]) on (128,256,16,64) beside t4k_copy
For (b) and (c) the ratio to the copy is reported, no bar is set."""
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
I4 = ctypes.c_int * 4
I7 = ctypes.c_int * 7
AXIS = {"8": 0, "4": 1, "2": 2, "1": 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(); h.init(0)
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong

    def timed(fn, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        h.call("t4k_sync", None)
        return (time.perf_counter() - t0) / reps * 1e6

    def compare(case, new, old, old_name, nelem, equal, plan):
        paths = [("permute", new), (old_name, old)]
        counts, times = {}, {k: [] for k, _ in paths}
        for k, fn in paths:
            fn(); h.call("t4k_sync", None)                              # warm: code objects loaded
            l0 = int(h.lib.t4k_launch_count()); fn(); counts[k] = int(h.lib.t4k_launch_count()) - l0
        h.call("t4k_sync", None)
        ok = bool(equal())
        for _ in range(args.runs):
            for k, fn in paths:
                times[k].append(timed(fn, args.reps))
        row = {"case": case, "plan": plan, "bit_equal": ok}
        for k, _ in paths:
            med = statistics.median(times[k])
            row.update({k + "_us": round(med, 2), k + "_min_max_us": [round(min(times[k]), 2), round(max(times[k]), 2)],
                        "launches_" + k: counts[k], k + "_GBps": round(8 * nelem / med / 1e3, 1)})
        row["permute_over_" + old_name] = round(row["permute_us"] / row[old_name + "_us"], 2)
        print(json.dumps(row), flush=True)
        return row

    rows = []
    g = torch.Generator(device="cuda").manual_seed(1)
    for p, dim, rival in (("8241", (128, 64, 64, 1), "transpose_batched"), ("8241", (64, 128, 128, 3), "transpose_batched"),
                          ("8142", (256, 32, 32, 64), "copy"), ("8142", (128, 224, 224, 3), "copy"), ("8412", (128, 256, 16, 64), "copy")):
        perm = [AXIS[c] for c in p]
        n = dim[0] * dim[1] * dim[2] * dim[3]
        X = torch.rand(n, device="cuda", generator=g)
        o1, o2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        px, p1, p2 = X.data_ptr(), o1.data_ptr(), o2.data_ptr()
        out = I7()
        h.call("t4k_permute_plan", I4(*dim), I4(*perm), 1, out)
        new = lambda: h.call("t4k_permute", V(px), V(p1), I4(*dim), I4(*perm), None)
        want = X.view(*dim).permute(*perm).contiguous().view(-1)
        if rival == "copy":
            old = lambda: h.call("t4k_copy", V(px), V(p2), n, None)
            equal = lambda: torch.equal(o1, want) and torch.equal(o2, X)
        else:
            old = lambda: h.call("t4k_transpose_batched", V(px), V(p2), dim[1], dim[2], dim[3], dim[0], None)
            equal = lambda: torch.equal(o1, want) and torch.equal(o2, o1)
        rows.append(compare("%s on (%d,%d,%d,%d)" % ((p,) + dim), new, old, rival, n, equal, list(out)))
        del X, o1, o2, want
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
