#!/usr/bin/env python3
"""Time t4k_mlp_head_bwd (k_head_bwd_l32) alone, with the LAB build's ablation bits (T4K_HB_LAB, wrong results - timing only):
   T4K_LIB=tensorforth_amd/libt4hip_lab.so T4K_HB_LAB=1 python tools/experiments/head_bwd_lab.py [N E1 EA EB]
   bits: 1 no column riders, 2 no tiles, 4 no target-store counter, 8 tiles skip P/T/W2 loads, 64 tiles skip mask loads, 16 tiles stop behind the prologue, 32 no in-place gate,
         128 the OTHER order of the roles over blockIdx.x (right results: riders between the tile kinds where the library puts them last, and the reverse)
and print the stamped timeline of one launch of a back-to-back train (LAB build; csrc/gemm_head_bwd.h, HB_STAMP):
   T4K_LIB=tensorforth_amd/libt4hip_lab.so python tools/experiments/head_bwd_lab.py --stamps [--r09] [N E1 EA EB]
(--r09: the record layout of the round-9 kernel with the stamps added - its riders stored dX2 / dY1 before they accumulated DW2)
per role (dW1 tiles, dX1 tiles, store rider, column riders, rider 0) the average and maximum of every link in shader cycles, where on the launch's
own clock (100 MHz, one for all XCDs) each role starts and ends, which workgroup ends last, and how the workgroups that share a CU fare."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from tensorforth_amd import lib as t4lib

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
stamps, r09 = "--stamps" in sys.argv[1:], "--r09" in sys.argv[1:]
N, E1, EA, EB = [int(x) for x in (argv[:4] if len(argv) >= 4 else (128, 980, 100, 10))]
WORDS = 32                                                   # HB_PROF_WORDS
t32 = lambda m, n: ((m + 31) // 32) * ((n + 31) // 32)
a1, a2, nr = t32(EA, E1), t32(N, E1), 1 + (EA + 3) // 4
nwg = a1 + a2 + nr
if stamps:                                                   # the library reads the address at every launch
    prof = torch.zeros(nwg * WORDS, dtype=torch.int64, device="cuda")
    os.environ["T4K_HB_PROF_PTR"] = "%x" % prof.data_ptr()
k = t4lib.load(os.environ.get("T4K_LIB") or None); k.init(0)
k.call("t4k_set_default_stream", None)
p = lambda t: t.data_ptr()
g = lambda *s: torch.rand(*s, device="cuda") - 0.5
X1, W1, X2, W2, P, T, M = g(N, E1), g(EA, E1), g(N, EA), g(EB, EA), g(N, EB), g(N, EB), (torch.rand(N, EA, device="cuda") > 0.5).float()
Y1, Y2, DW1, DB1, DW2, DB2 = g(N, EA), g(N, EB), g(EA, E1), g(EA), g(EB, EA), g(EB)
def once():
    k.call("t4k_mlp_head_bwd", p(X2), p(W2), p(P), p(T), p(Y2), p(M), p(Y1), p(DW2), p(DB2), p(X1), p(W1), p(DW1), p(DB1), N, E1, EA, EB, None)

if not stamps:
    best = 1e9
    for rep in range(4):
        for _ in range(300): once()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(2000): once()
        torch.cuda.synchronize(); best = min(best, (time.perf_counter() - t0) / 2000 * 1e6)
    print("T4K_HB_LAB=%s  N=%d E1=%d EA=%d EB=%d: %.2f us per launch (back to back)" % (os.environ.get("T4K_HB_LAB", "0"), N, E1, EA, EB, best), flush=True)
    sys.exit(0)

# ---- the stamped timeline: the record of the LAST launch of a back-to-back train (every launch overwrites the records)
LINKS = {
    "tile": ["start", "DMA + operand loads issued", "first dY1 MFMA (operands landed)", "dY1 blocks in LDS", "DMA landed (vmcnt 0)", "past barrier 1",
             "K loop issued", "meeting written", "gate passed", "past barrier 2", "stores issued", "stores drained"],
    "store rider": ["start", "P - T in LDS", "poll passed", "stored", "stores drained"],
    "column rider": ["start", "staged (past barrier 1)", "dW2 loop done", "DW2 accumulated", "dX2 / dY1 stored", "DB1 accumulated", "DB2 accumulated (rider 0)", "stores drained"],
}
if r09: LINKS["column rider"][3:5] = ["dX2 / dY1 stored", "DW2 accumulated"]
for _ in range(500): once()
torch.cuda.synchronize()
rec = prof.cpu().numpy().reshape(nwg, WORDS)
assert rec[:, 0].all(), "no stamps: is T4K_LIB the LAB build?"
role = rec[:, 17]
w0, w1 = rec[:, 14].astype(float), rec[:, 15].astype(float)
t0 = w0.min()
start_us, end_us = (w0 - t0) / 100.0, (w1 - t0) / 100.0
cu_key = [(int(rec[i, 19]) & 15, (int(rec[i, 18]) >> 8) & 0xff) for i in range(nwg)]          # (XCC, SE | SH | CU of HW_ID)
share = {}
for i, c in enumerate(cu_key): share.setdefault(c, []).append(i)
shared = {i for v in share.values() if len(v) > 1 for i in v}
# a workgroup's role is word 17 of its record (0 dW1 tile, 1 dX1 tile, 2 store rider, 3 column rider), its number within the role the order of
# blockIdx.x: the tables read either order of the roles
by_role = {r: [i for i in range(nwg) if role[i] == r] for r in range(4)}
rank = {i: n for idx in by_role.values() for n, i in enumerate(idx)}
def name_of(i):
    return ("dW1 tile %d", "dX1 tile %d", "store rider", "column rider %d")[int(role[i])].replace("%d", str(rank[i]))
def table(title, idx, links):
    idx = list(idx)
    if not idx: return
    print("\n%s: %d workgroups; starts at %.2f .. %.2f us of the launch, ends at %.2f .. %.2f us (avg %.2f)" % (
        title, len(idx), start_us[idx].min(), start_us[idx].max(), end_us[idx].min(), end_us[idx].max(), end_us[idx].mean()))
    r = rec[idx].astype(float)
    print("  %-36s %9s %9s %9s" % ("link (shader cycles)", "avg", "max", "avg cum"))
    for j in range(1, len(links)):
        prev = j - 1
        while prev > 0 and not r[:, prev].all(): prev -= 1                                    # a stamp the role skips (DB2 of riders other than 0)
        if not r[:, j].all(): continue
        d = r[:, j] - r[:, prev]
        print("  %-36s %9.0f %9.0f %9.0f" % ("-> " + links[j], d.mean(), d.max(), (r[:, j] - r[:, 0]).mean()))
    sp = rec[idx, 16]
    if sp.any() or title.startswith(("dX1", "store")): print("  failed looks of the wait: avg %.2f, max %d, workgroups with any %d" % (sp.mean(), sp.max(), (sp > 0).sum()))
# the order of the roles, from where the store rider's record sits (no such record, as under an ablation that drops it: not known)
riders_last = None if not by_role[2] else by_role[2][0] == nwg - nr
counts = "%d dW1 tiles, %d dX1 tiles, %d riders" % (a1, a2, nr) if riders_last else "%d dW1 tiles, %d riders, %d dX1 tiles" % (a1, nr, a2)
print("k_head_bwd_l32 stamped: N=%d E1=%d EA=%d EB=%d, %d workgroups (%s) on %d CUs, %d of them on a CU that holds two or more" % (
    N, E1, EA, EB, nwg, counts, len(share), len(shared)))
print("launch, first start to last end on the 100 MHz clock: %.2f us; roles over blockIdx.x: %s" % (
    end_us.max(), "not known (no store rider's record)" if riders_last is None else "riders last" if riders_last else "riders between the tile kinds"))
table("dW1 tiles", by_role[0], LINKS["tile"]); table("dX1 tiles", by_role[1], LINKS["tile"])
table("store rider", by_role[2], LINKS["store rider"])
table("column riders 1 ..", by_role[3][1:], LINKS["column rider"]); table("column rider 0 (carries dB2)", by_role[3][:1], LINKS["column rider"])
order = sorted(range(nwg), key=lambda i: -end_us[i])
print("\nlast to end:")
for i in order[:8]:
    print("  %-18s starts %.2f us, ends %.2f us, XCC %d CU %#04x%s" % (name_of(i), start_us[i], end_us[i], cu_key[i][0], cu_key[i][1], ", shares its CU" if i in shared else ""))
if shared:
    s, a = sorted(shared), sorted(set(range(nwg)) - shared)
    print("workgroups that share a CU: end avg %.2f us, max %.2f us | alone on a CU: end avg %.2f us, max %.2f us" % (end_us[s].mean(), end_us[s].max(), end_us[a].mean(), end_us[a].max()))
