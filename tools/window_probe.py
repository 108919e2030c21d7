"""Box windows: the four-scalar `slice` through the VM beside the same word of another build of this repository (the parent commit, built
in a directory of its own), and t4k_window beside the floor of any data movement (t4k_copy of the box's element count), on the same
device in the same run.

    python tools/window_probe.py [--parent DIR] [--reps R] [--runs K] [--json profiles/window_probe.json]

Each timing is the wall time of R back-to-back calls on the library's default stream, bracketed by t4k_sync, divided by R; it is repeated K
times, the two sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported,
with the dispatches of one call from t4k_launch_count.  GB/s = 8 bytes per element of the box (one read, one write) over the median.

  (a) `4 24 4 24 slice drop` on (128,28,28,1) through the VM, R of them in one eval.  --parent names the root of a built checkout of the
      parent commit: a second process imports ITS tensorforth_amd (two builds of the libraries cannot share a process) and times the same
      source when asked, so the two sides still alternate.  The bar: faster outside both spreads.  Without --parent the row has one side.
  (b) a C-third of (128,256,1,192)            (c) a [16,208)^2 crop of (128,224,224,3)
  (d) (128,1,1,64) stored into (128,256,1,64) at h0 = 100            (e) an N-half of (256,32,32,64)
For (b) - (e) the ratio to the copy is reported, no bar is set.  Every result is checked bit-equal to torch slicing."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V = ctypes.c_void_p
I4 = ctypes.c_int * 4
I6 = ctypes.c_int * 6
SLICE_DIM, SLICE_WORD = (128, 28, 28, 1), "4 24 4 24 slice"


class VmSide:
    """the four-scalar slice through the VM of the checkout at `root`"""

    def __init__(self, root):
        sys.path.insert(0, root)
        import numpy as np
        from tensorforth_amd.lib import load
        from tensorforth_amd.vm import VM
        self.h = load(); self.h.init(0)
        self.h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
        self.vm = VM(device=0, seed=1)
        self.x = np.random.default_rng(1).random(SLICE_DIM).astype(np.float32)
        self.vm.store(self.x, "%d %d %d %d tensor" % SLICE_DIM)

    def check(self):
        """[bit-equal to slicing, launches of one word]"""
        import numpy as np
        l0 = int(self.h.lib.t4k_launch_count())
        got = self.vm.fetch(SLICE_WORD)
        n = int(self.h.lib.t4k_launch_count()) - l0
        self.vm.eval("drop")
        return [bool(np.array_equal(got, self.x[:, 4:24, 4:24, :])), n]

    def timed(self, reps):
        src = (SLICE_WORD + " drop\n") * reps
        self.h.call("t4k_sync", None)
        t0 = time.perf_counter()
        self.vm.eval(src)
        self.h.call("t4k_sync", None)
        return (time.perf_counter() - t0) / reps * 1e6


def worker(root):
    """serve `check` / `timed R` / `quit` on stdin, one JSON line each"""
    side = VmSide(root)
    print(json.dumps("ready"), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        print(json.dumps(side.check() if cmd[0] == "check" else side.timed(int(cmd[1]))), flush=True)


class Remote:
    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root)
        assert json.loads(self.p.stdout.readline()) == "ready"

    def ask(self, cmd):
        self.p.stdin.write(cmd + "\n"); self.p.stdin.flush()
        return json.loads(self.p.stdout.readline())

    def check(self):
        return self.ask("check")

    def timed(self, reps):
        return self.ask("timed %d" % reps)

    def close(self):
        self.p.stdin.write("quit\n"); self.p.stdin.close(); self.p.wait(timeout=60)


def summary(row, name, times, nelem):
    med = statistics.median(times)
    row.update({name + "_us": round(med, 2), name + "_min_max_us": [round(min(times), 2), round(max(times), 2)], name + "_GBps": round(8 * nelem / med / 1e3, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--parent")
    ap.add_argument("--worker")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    rows = []

    # (a) the word, this build beside the parent's
    own = VmSide(ROOT)
    sides = [("window", own)] + ([("parent", Remote(os.path.abspath(args.parent)))] if args.parent else [])
    box = 128 * 20 * 20
    row = {"case": "(a) `%s` on (%d,%d,%d,%d) through the VM" % ((SLICE_WORD,) + SLICE_DIM)}
    times = {k: [] for k, _ in sides}
    for k, s in sides:
        s.timed(args.reps)                                              # warm: code objects loaded, the arena grown
        row["bit_equal_" + k], row["launches_" + k] = s.check()
    for _ in range(args.runs):
        for k, s in sides:
            times[k].append(s.timed(args.reps))
    for k, _ in sides:
        summary(row, k, times[k], box)
    if args.parent:
        row["window_over_parent"] = round(row["window_us"] / row["parent_us"], 3)
        row["outside_both_spreads"] = row["window_min_max_us"][1] < row["parent_min_max_us"][0]
        sides[1][1].close()
    own.vm.eval("drop")
    print(json.dumps(row), flush=True)
    rows.append(row)

    # (b) - (e) the entry beside t4k_copy of the box's element count
    import torch
    h = own.h

    def timed(fn, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        h.call("t4k_sync", None)
        return (time.perf_counter() - t0) / reps * 1e6

    g = torch.Generator(device="cuda").manual_seed(1)
    for case, sdim, soff, ddim, doff, ext in (
            ("(b) a C-third of (128,256,1,192)", (128, 256, 1, 192), (0, 0, 0, 64), (128, 256, 1, 64), (0, 0, 0, 0), (128, 256, 1, 64)),
            ("(c) a [16,208)^2 crop of (128,224,224,3)", (128, 224, 224, 3), (0, 16, 16, 0), (128, 192, 192, 3), (0, 0, 0, 0), (128, 192, 192, 3)),
            ("(d) (128,1,1,64) stored into (128,256,1,64) at h0 = 100", (128, 1, 1, 64), (0, 0, 0, 0), (128, 256, 1, 64), (0, 100, 0, 0), (128, 1, 1, 64)),
            ("(e) an N-half of (256,32,32,64)", (256, 32, 32, 64), (128, 0, 0, 0), (128, 32, 32, 64), (0, 0, 0, 0), (128, 32, 32, 64))):
        ns, nd, nbox = (sdim[0] * sdim[1] * sdim[2] * sdim[3], ddim[0] * ddim[1] * ddim[2] * ddim[3], ext[0] * ext[1] * ext[2] * ext[3])
        X = torch.rand(ns, device="cuda", generator=g)
        D0 = torch.rand(nd, device="cuda", generator=g)
        o1 = D0.clone()
        c1, c2 = torch.rand(nbox, device="cuda", generator=g), torch.zeros(nbox, device="cuda")
        out = I6()
        h.call("t4k_window_plan", I4(*sdim), I4(*soff), I4(*ddim), I4(*doff), I4(*ext), 1, out)
        px, p1, pc1, pc2 = X.data_ptr(), o1.data_ptr(), c1.data_ptr(), c2.data_ptr()
        new = lambda: h.call("t4k_window", V(px), I4(*sdim), I4(*soff), V(p1), I4(*ddim), I4(*doff), I4(*ext), None)
        old = lambda: h.call("t4k_copy", V(pc1), V(pc2), nbox, None)
        sl = lambda off: tuple(slice(o, o + e) for o, e in zip(off, ext))
        want = D0.view(*ddim).clone(); want[sl(doff)] = X.view(*sdim)[sl(soff)]
        paths = [("window", new), ("copy", old)]
        counts, times = {}, {k: [] for k, _ in paths}
        for k, fn in paths:
            fn(); h.call("t4k_sync", None)                              # warm: code objects loaded
            l0 = int(h.lib.t4k_launch_count()); fn(); counts[k] = int(h.lib.t4k_launch_count()) - l0
        h.call("t4k_sync", None)
        row = {"case": case, "plan": list(out), "bit_equal": bool(torch.equal(o1.view(*ddim), want) and torch.equal(c2, c1))}
        for _ in range(args.runs):
            for k, fn in paths:
                times[k].append(timed(fn, args.reps))
        for k, _ in paths:
            summary(row, k, times[k], nbox)
            row["launches_" + k] = counts[k]
        row["window_over_copy"] = round(row["window_us"] / row["copy_us"], 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del X, D0, o1, c1, c2, want
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
