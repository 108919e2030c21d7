"""Group / layer / instance norm (t4k_groupnorm_fwd / _bwd): time per call of forward and backward at six layers, beside two yardsticks, neither
of them the code under test: t4k_batchnorm_fwd / _bwd on the SAME tensor (the same bytes over more launches) and torch's native_group_norm / _backward of the
installed torch-ROCm on the same device in its native contiguous NCHW layout.

    python tools/groupnorm_probe.py [--reps R] [--runs K] [--json profiles/groupnorm_probe.json]

The protocol of tools/conv_grp_probe.py: each timing is the wall time of R back-to-back calls, bracketed by a device synchronisation, divided by R; it is repeated
K times, the sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported, with the dispatches of one
call from t4k_launch_count.

  rows: 1 instance norm 32x32x64, N 256;  2 G = 32 on 16x16x128, N 256;  3 G = 32 on 56x56x64, N 64;  4 layer norm 14x14x384, N 256;
        5 layer norm 56x56x64, N 8 (the split rung);  6 G = 8 on 8x8x32, N 128
  bar: where the groups fill the device (N G >= 256) forward and backward take no longer than batchnorm's, beyond the two spreads ("no_longer_*": the new
  side's fastest repeat against batchnorm's slowest); the other rows report the same comparison without a bar.  torch: the ratio, no bar.
  bytes by the rule - I + O + XH forward; DY + XH + DX backward, DY and XH twice where the group is not resident (rungs 3 and 4) - and their rate as a fraction
  of the 8 TB/s of SURVEY.md.
  sweep: E from 256 to 65536 floats per group at 2^24 elements in all (C = 64, G = 16, Cg = 4, 16-byte path), one row per E on either side of each threshold
  of the plan, the rung the plan chose beside it.  With --lib tensorforth_amd/libt4hip_lab.so (make -C tensorforth_amd/csrc LAB=1) and T4K_GN_RUNG=2 | 3 in
  the environment the same rows run one or two rungs higher: that comparison sets the thresholds."""
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
EPS = 1.0e-5
HBM = 8.0e12

#        name, N, H, C, G
CASES = [("1 instance norm 32x32x64", 256, 32, 64, 64),
         ("2 G=32 16x16x128", 256, 16, 128, 32),
         ("3 G=32 56x56x64", 64, 56, 64, 32),
         ("4 layer norm 14x14x384", 256, 14, 384, 1),
         ("5 layer norm 56x56x64 N=8 (split)", 8, 56, 64, 1),
         ("6 G=8 8x8x32", 128, 8, 32, 8)]
SWEEP_HW = [64, 256, 512, 528, 1024, 2048, 4096, 4112, 8192, 16384]     # x Cg = 4: E = 4 HW


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rows", default="123456s")
    ap.add_argument("--json")
    ap.add_argument("--lib", help="another build of the library (the LAB build, whose T4K_GN_RUNG moves a group to a higher rung)")
    ap.add_argument("--tag", default="", help="a suffix for the case names of this run")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(args.lib); h.init(0)
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g) - 0.5
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

    def one(name, N, HW, C, G, yardsticks):
        out = I8(); h.call("t4k_groupnorm_plan", N, HW, C, G, 1, 32 << 20, out)
        I, DY, O, XH, DX = rnd(N, HW, C), rnd(N, HW, C), torch.zeros(N, HW, C, device="cuda"), torch.zeros(N, HW, C, device="cuda"), torch.zeros(N, HW, C, device="cuda")
        W, B, DWB, ST = rnd(C) + 1.0, rnd(C), torch.zeros(2 * C, device="cuda"), torch.zeros(4 * N * G, device="cuda")
        row = {"case": name + args.tag, "N": N, "HW": HW, "C": C, "G": G, "E": HW * C // G, "groups": N * G, "plan": list(out)}
        sides = [("gn_fwd", lambda: h.call("t4k_groupnorm_fwd", p(I), p(O), p(XH), p(W), p(B), p(ST), N, HW, C, G, EPS, None)),
                 ("gn_bwd", lambda: h.call("t4k_groupnorm_bwd", p(W), p(DY), p(XH), p(ST), p(DX), p(DWB), V(DWB.data_ptr() + 4 * C), N, HW, C, G, 1, None))]
        if yardsticks:
            BST = torch.zeros(3 * C, device="cuda")
            sides += [("bn_fwd", lambda: h.call("t4k_batchnorm_fwd", p(I), p(O), p(XH), p(W), p(B), p(BST), N, HW, C, None)),
                      ("bn_bwd", lambda: h.call("t4k_batchnorm_bwd", p(W), p(DY), p(XH), p(DX), p(DWB), V(DWB.data_ptr() + 4 * C), p(BST), N, HW, C, 1, None))]
            x = I.reshape(N, HW, C).permute(0, 2, 1).contiguous(); gy = DY.reshape(N, HW, C).permute(0, 2, 1).contiguous()
            y, mean, rstd = torch.ops.aten.native_group_norm(x, W, B, N, C, HW, G, EPS)
            sides += [("torch_fwd", lambda: torch.ops.aten.native_group_norm(x, W, B, N, C, HW, G, EPS)),
                      ("torch_bwd", lambda: torch.ops.aten.native_group_norm_backward(gy, x, mean, rstd, W, N, C, HW, G, [True, True, True]))]
        measure(row, sides)
        n = I.numel()
        nbytes = {"fwd": 4 * 3 * n, "bwd": 4 * (3 + (2 if out[0] >= 3 else 0)) * n}
        for k in ("fwd", "bwd"):
            row["bytes_" + k] = nbytes[k]
            row["hbm_fraction_" + k] = round(nbytes[k] / (row["gn_%s_us" % k] * 1e-6) / HBM, 3)
            if yardsticks:
                row["ratio_bn_" + k] = round(row["gn_%s_us" % k] / row["bn_%s_us" % k], 3)
                row["no_longer_" + k] = row["gn_%s_min_max_us" % k][0] <= row["bn_%s_min_max_us" % k][1]
                row["ratio_torch_" + k] = round(row["gn_%s_us" % k] / row["torch_%s_us" % k], 3)
        row["barred"] = bool(yardsticks and N * G >= 256)
        print(json.dumps(row), flush=True)
        return row

    rows = []
    for name, N, H, C, G in CASES:
        if name[0] in args.rows:
            rows.append(one(name, N, H * H, C, G, True))
    if "s" in args.rows:
        for HW in SWEEP_HW:
            rows.append(one("sweep E=%d" % (4 * HW), (1 << 24) // (HW * 64), HW, 64, 16, False))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "devices": 1, "reps": args.reps, "runs": args.runs, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
