"""Cases of the linear-layer sweep and a Python mirror of the host-side dispatch they are chosen against - shared by the GPU sweep
(tests/test_gpu_linear_sweep.py) and its CPU self-test (tests/test_linear_cases.py), the arrangement of small_kernel_cases.py.

The mirror restates, inequality by inequality, tensorforth_amd/csrc/linear.hip (the entry points, linear_bwd_dual, head_bwd_ok),
linear_small.hip (linear_small_ok, linear_small_fwd, linear_small_bwd) and what gemm_launch (gemm.hip) does with a linear layer's three
products in the release build (every LAB switch at its default).  A change there must be followed here: the GPU sweep asserts the label AND
the launch count of every case, so a heuristic that moves a case to another kernel fails the sweep instead of leaving it green on the wrong
kernel.  Everything is sized for the MI355X's 256 CUs; plan_of takes the CU count, the sweep passes the device's.

Orientation (Model::_flinear / _blinear): Y[N, E0] = X[N, E1] W[E0, E1]^T + B; dW[E0, E1] += dY^T X, dB[E0] += sum_n dY, dX[N, E1] = dY W."""
import numpy as np

import f64_witness as wt
import gemm_cases

CU = 256                                    # the MI355X
LS_MAX_FLOATS = 12288                       # linear_small.hip: 48 KiB of dynamic LDS
LSC_CW = 4                                  # ... columns per workgroup of k_linsmall_bwd_cols
THIN_RA = 8                                 # ... rows per workgroup of k_linthin_bwd
HB_CW, HB_AP = 4, 33                        # gemm_head_bwd.h
S32_MAXK = 832                              # gemm_types.h GemmLab::s32_maxk: deepest K one sliver workgroup walks
DUAL_MAXK = 1024                            # ... dual_maxk
WS_BYTES = 64 << 20                         # runtime.hip: the stream's workspace
KG = 64                                     # gemm.hip: split-K granularity
# k_head_bwd_l32 as compiled for gfx950: 144 VGPRs -> 3 waves per SIMD, one wave of a 256-thread workgroup per SIMD; 160 KiB of LDS per CU
HB_WAVES, LDS_PER_CU = 3, 160 << 10


def cdiv(a, b):
    return -(-a // b)


def t32(m, n):
    return cdiv(m, 32) * cdiv(n, 32)


def t64(m, n):
    return cdiv(m, 64) * cdiv(n, 64)


def small_ok(E0, E1):
    """linear_small_ok: the vector-ALU kernels' LDS holds W (pitch E1 + 1) and 16 rows of X forward, W and 64 rows of dY backward"""
    return 1 <= E0 <= 64 and 1 <= E1 <= 512 and E0 * (E1 + 1) + 16 * E1 <= LS_MAX_FLOATS and E0 * E1 + 64 * E0 <= LS_MAX_FLOATS


# ----------------------------------------------------------------------------- gemm_launch for one product of a linear layer
def gemm_plan(M, N, K, tA, tB, cu=CU, defer=False, cs_rows=0, plain=False):
    """(label, launches, riders ride, column sums ride, slabs deferred) of gemm_launch on 16-byte aligned operands, C = 1.
    cs_rows > 0: a ColSum request over that many rows; plain: no epilogue, rider or column sum requested (the two-workgroup lean kernel asks
    for that); defer: the caller folds split slabs itself (t4k_mlp_head_fwd)"""
    r = gemm_cases.ladder(M, N, K, tA, tB, 1, cu, defer=defer, cs_rows=cs_rows, riders=not plain, bias=True)
    if r["base"].startswith("l32"):
        return ("sliver" if r["nsplit"] == 1 else "sliver_deferred"), 1, r["riders_ride"], r["cs_ride"], r["deferred"]
    if r["base"] == "pair":
        return "pair", 1, False, False, False
    if r["nsplit"] > 1:
        return ("splitk_deferred" if r["deferred"] else "splitk"), r["launches"], r["riders_ride"], False, r["deferred"]   # the fold launch carries every rider
    return "unsplit", 1, False, r["cs_ride"], False


def colsum_add_launches(rows):
    """colsum.hip colsum_add: one chunk accumulates in place up to 1024 rows, partial slabs + a fold above"""
    return 1 if rows <= 1024 else 2


# ----------------------------------------------------------------------------- linear_small.hip
def small_fwd_label(E0, E1, softmax=False, fold=False, skew=0):
    if not fold and not softmax and E0 <= 4:
        return "thin_fwd_vec" if E1 % 4 == 0 and skew % 16 == 0 else "thin_fwd_scalar"
    return "small_fwd_%d" % (16 if E0 <= 16 else 32 if E0 <= 32 else 64) + ("_narrow" if fold else "")


def small_bwd_shape(N, E1):
    """(trips of one dW workgroup over the batch, rows of dX per workgroup) of k_linsmall_bwd"""
    cl = 32
    while cl < E1 and cl < 256:
        cl <<= 1
    per = (256 // cl) * 64
    return cdiv(N, per), max(1, min(64, 1024 // E1))


def small_bwd(N, E0, E1, cu=CU, train=1, has_dw=True, dx=True, in_place=True, tgt=False):
    """linear_small_bwd: the label of the kernel it launches, or 'refused:<why>' where it returns false"""
    tr = bool(train) and has_dw
    G = cdiv(N, THIN_RA)
    if E0 <= 4:
        if tr and 1 <= N <= 1024 and E1 >= 8:
            return "thin_bwd_cols8"
        if E1 <= 512 and N >= 1 and (dx or tr) and (not tr or (G + 1) * E0 * E1 * 4 <= WS_BYTES // 2):
            return "thin_bwd_ticket" if tr else "thin_bwd_frozen"
    ldsc = 4 * (N * E0 + E0 * LSC_CW + N * LSC_CW + 256)
    if E0 * LSC_CW + E0 <= 256 and 1 <= N <= 512 and ldsc <= LS_MAX_FLOATS * 4 and (dx or tr) and (not train or has_dw) and \
            (not tgt or cdiv(E1, LSC_CW) <= cu) and N * E1 <= 32768:
        return "small_bwd_cols"
    trips, RA = small_bwd_shape(N, E1)
    CBK = cdiv(E1, 64) if E1 > 64 and trips > 1 and E0 * cdiv(E1, 64) <= 128 else 1
    nB = E0 * CBK if tr else 0
    nA = cdiv(N, RA) if dx else 0
    alias = dx and nB > 0 and in_place
    if tgt and not alias and nB > 0:
        return "refused:target_without_alias"
    if alias and nA + nB > cu:
        return "refused:residency"
    lds = 4 * max(E0 * E1 + RA * E0, N + 768 if nB else 0)
    if lds > LS_MAX_FLOATS * 4:
        return "refused:lds"
    return "small_bwd"


def small_bwd_form(N, E0, E1):
    """(CBK, trips) of a trained k_linsmall_bwd launch"""
    trips, _ = small_bwd_shape(N, E1)
    CBK = cdiv(E1, 64) if E1 > 64 and trips > 1 and E0 * cdiv(E1, 64) <= 128 else 1
    return CBK, trips


# ----------------------------------------------------------------------------- linear.hip: the dual dW || dX launch
def dual(N, E0, E1, cu=CU):
    """linear_bwd_dual on aligned operands: None (refused), or the label with its instantiation"""
    if (E0 & 3) or (E1 & 3) or N < 1:
        return None
    big = lambda m, n: cdiv(m, 128) * cdiv(n, 128) >= cu * 3 // 4
    splits = lambda m, n, k: t64(m, n) * 2 <= cu and k >= 256
    sp = splits(E0, E1, N) or splits(N, E1, E0)
    if big(E0, E1) or big(N, E1) or (sp and (N > DUAL_MAXK or E0 > DUAL_MAXK)):
        return None
    t1, t2, riders = t64(E0, E1), t64(N, E1), cdiv(E0, 64)
    if t1 + riders + t2 > cu or N > 4096:
        return None
    a1, a2, ar = t32(E0, E1), t32(N, E1), cdiv(E0, 64)
    if a1 + ar + a2 <= 4 * cu - 32 and a1 <= 512 and N <= 1024 and E0 <= 1024:
        if N > 512 or E0 > 512:
            return "dual_l32_rst8"
        return "dual_l32_rst4" if N > 256 or E0 > 256 else "dual_l32_4"
    f1 = N % 64 == 0 and E0 >= 4 and E1 >= 4
    f2 = E0 % 64 == 0 and E1 >= 4
    return "dual_64_f%d%d" % (f1, f2)


# ----------------------------------------------------------------------------- linear.hip: the one-launch head backward
def head_bwd_lds(N, EA, EB):
    kd = cdiv(max(N, EA), 32) * 32
    lt = 8192 + kd * HB_AP
    lr = N * EB + EB * HB_CW + N * HB_CW + 256
    return 4 * max(lt, lr, N * EB)


def head_resident(N, EA, EB):
    """resident workgroups of k_head_bwd_l32 per CU, what head_bwd_ok asks the runtime for: the smaller of the register and the LDS limit.
    The GPU sweep checks this argument by comparing head_bwd_ok's verdict with t4k_mlp_head_bwd_ok for every head case"""
    return min(HB_WAVES, LDS_PER_CU // head_bwd_lds(N, EA, EB))


def head_bwd_ok(N, E1, EA, EB, cu=CU, nb=None):
    if N < 1 or N > 256 or EA < 4 or EA > 256 or (EA & 3) or EB < 1 or EB > 16 or E1 < 4 or (E1 & 3):
        return False
    nb = head_resident(N, EA, EB) if nb is None else nb
    if nb < 1:
        return False
    a1, a2, nr = t32(EA, E1), t32(N, E1), 1 + cdiv(EA, HB_CW)
    return a1 + a2 + nr <= nb * cu - 32 and a1 <= 512 and a1 + a2 + nr <= 768


# ----------------------------------------------------------------------------- the entries
def _stage_launches(stages):
    """the element-wise layers behind a product as launches of their own: one stage = (mask draw) + activate, two = one fused run"""
    if not stages:
        return 0
    if len(stages) == 2:
        return 1
    return 2 if stages[0] == "drop" else 1


def _separate_bwd(N, E0, E1, cu, train, has_dw, dx):
    """t4k_linear_bwd2's last resort: dW (+ dB) and dX as gemm_launch calls"""
    n, label = 0, []
    if train and has_dw:
        g = gemm_plan(E0, E1, N, 1, 0, cu, cs_rows=N)
        n += g[1]
        if g[3]:
            label.append("separate_colsum_rider")
        else:
            label.append("separate_colsum_add"); n += colsum_add_launches(N)
        label.append("dw_" + g[0])
    if dx:
        g = gemm_plan(N, E1, E0, 0, 0, cu, plain=True)
        n += g[1]; label.append("dx_" + g[0])
    return "+".join(label), n


def _bwd2(N, E0, E1, cu, train, has_dw, dx, in_place, masks, tgt=False):
    """t4k_linear_bwd2 (masks = 0 | 1) -> (label, launches)"""
    if masks and not small_ok(E0, E1):
        lab, n = _bwd2(N, E0, E1, cu, train, has_dw, dx, in_place, 0)
        return lab, n + 1
    if small_ok(E0, E1):
        s = small_bwd(N, E0, E1, cu, train, has_dw, dx, in_place, tgt)
        if not s.startswith("refused"):
            return s, 1
        if masks:
            lab, n = _bwd2(N, E0, E1, cu, train, has_dw, dx, in_place, 0)
            return s + "->" + lab, n + 1
    else:
        s = None
    pre = s + "->" if s else ""
    if train and has_dw and dx:
        d = dual(N, E0, E1, cu)
        if d:
            return pre + d, 1
    lab, n = _separate_bwd(N, E0, E1, cu, train, has_dw, dx)
    return pre + lab, n


def plan_of(entry, N, E0, E1, *, cu=CU, train=1, has_dw=True, in_place=True, tgt=False, masks=0, dx=True, base_skew=0,
            stages=(), copy=False, softmax=False, H=0, nb=None):
    """(label, launches) of one call.  entry: linear_fwd | linear_softmax_fwd | linear_act_fwd | linear_block_fwd | mlp_head_fwd |
    linear_bwd | loss_linear_bwd | linear_block_bwd | mlp_head_bwd | mlp_block_bwd.  masks: mask tensors of the chain (0 .. 2); stages: the
    element-wise layers behind a forward product ('relu' | 'leaky' | 'tanh' | 'drop'); base_skew: bytes X sits off a 16-byte boundary
    (forward thin head only); mlp_head_fwd: layer 1 is E1 -> H with stages[0] behind it, layer 2 H -> E0 (+ softmax);
    mlp_head_bwd / mlp_block_bwd: (N, E0, E1) = (N, EB, E1) with H = EA"""
    if entry in ("linear_fwd", "linear_softmax_fwd", "linear_act_fwd", "linear_block_fwd"):
        if entry == "linear_softmax_fwd":
            softmax = True
        if small_ok(E0, E1):
            lab = small_fwd_label(E0, E1, softmax, False, base_skew)
            fused = len(stages) == 1
            n = 1 + (0 if fused else _stage_launches(stages)) + (1 if copy else 0)
            return lab + ("+softmax" if softmax else "") + ("+stage" if fused else ""), n
        g = gemm_plan(N, E0, E1, 0, 1, cu, plain=not stages and not copy and entry == "linear_fwd")
        n = g[1]
        if entry == "linear_block_fwd":
            rides = g[2] and bool(stages or copy)
            if not g[2]:
                n += _stage_launches(stages) + (1 if copy else 0)
            elif not stages:
                pass                                         # the copy rides alone
        else:
            rides = g[2] and bool(stages)
            if not g[2]:
                n += _stage_launches(stages)
        n += 1 if softmax else 0
        return "gemm_" + g[0] + ("+riders" if rides else "+separate" if (stages or copy) else ""), n
    if entry == "mlp_head_fwd":
        if not small_ok(H, E1) and small_ok(E0, H):
            g = gemm_plan(N, H, E1, 0, 1, cu, defer=True)
            if g[4]:
                return "gemm_" + g[0] + "+" + small_fwd_label(E0, H, softmax, True), g[1] + 1
            lab2, n2 = plan_of("linear_softmax_fwd" if softmax else "linear_fwd", N, E0, H, cu=cu)
            return "gemm_" + g[0] + "+separate+" + lab2, g[1] + _stage_launches(stages) + n2
        lab1, n1 = plan_of("linear_act_fwd", N, H, E1, cu=cu, stages=stages)
        lab2, n2 = plan_of("linear_softmax_fwd" if softmax else "linear_fwd", N, E0, H, cu=cu)
        return lab1 + "|" + lab2, n1 + n2
    if entry == "linear_bwd":
        return _bwd2(N, E0, E1, cu, train, has_dw, dx, in_place, masks)
    if entry == "loss_linear_bwd":
        if small_ok(E0, E1):
            s = small_bwd(N, E0, E1, cu, train, has_dw, dx, in_place, True)
            if not s.startswith("refused"):
                return s, 1
        lab, n = _bwd2(N, E0, E1, cu, train, has_dw, dx, in_place, masks)
        return ("%s->" % s if small_ok(E0, E1) else "") + lab, n + 1
    if entry == "linear_block_bwd":
        assert masks in (1, 2) and dx
        pre = ""
        if small_ok(E0, E1):
            s = small_bwd(N, E0, E1, cu, train, has_dw, True, in_place, tgt)
            if not s.startswith("refused"):
                return s, 1
            pre = s + "->"
        n = 1 if tgt else 0
        if small_ok(E0, E1):
            s = small_bwd(N, E0, E1, cu, train, has_dw, True, in_place, False)
            if not s.startswith("refused"):
                return pre + s, n + 1
            if not tgt:
                pre = s + "->"
        if train and has_dw:
            d = dual(N, E0, E1, cu)
            if d:
                return pre + d, n + 1
        if not (train and has_dw) and not small_ok(E0, E1):
            g = gemm_plan(N, E1, E0, 0, 0, cu)
            if g[2]:
                return "dx_only_fold_rider:" + g[0], n + g[1]
            return "dx_only_unfused:" + g[0], n + g[1] + 1
        lab, m = _bwd2(N, E0, E1, cu, train, has_dw, True, in_place, 0)
        return pre + lab, n + m + 1                         # + the run's backward as one launch
    if entry in ("mlp_head_bwd", "mlp_block_bwd"):
        if head_bwd_ok(N, E1, H, E0, cu, nb) and H % 4 == 0:
            return ("head_bwd" if entry == "mlp_head_bwd" else "head_bwd_runs") + ("" if train else "_frozen"), 1
        return "head_bwd_refused", 0
    raise ValueError(entry)


# ----------------------------------------------------------------------------- the table
class Case:
    """one call: the entry, its shape and flags, the label plan_of must give at 256 CUs, and why the shape is what it is"""

    def __init__(self, label, entry, N, E0, E1, why, launches=None, **kw):
        self.label, self.entry, self.N, self.E0, self.E1, self.why, self.launches, self.kw = label, entry, N, E0, E1, why, launches, kw
        self.id = "%s-%s-N%d-E0_%d-E1_%d%s" % (label.replace(":", "_").replace("->", "_to_").replace("+", "_").replace("|", "_"), entry, N, E0, E1,
                                                "".join("-%s_%s" % (k, "".join(str(x) for x in v) if isinstance(v, tuple) else v) for k, v in sorted(kw.items())))

    def plan(self, cu=CU, **over):
        kw = dict(self.kw); kw.update(over)
        return plan_of(self.entry, self.N, self.E0, self.E1, cu=cu, **kw)


def F(label, entry, N, E0, E1, why, **kw):
    return Case(label, entry, N, E0, E1, why, **kw)


# forward.  The product depth is E1; every label's first row is the smallest shape that reaches it
FWD_CASES = (
    # thin heads: E0 <= 4 without a softmax; 16-byte loads need E1 % 4 == 0 and X, W on 16-byte boundaries
    F("thin_fwd_vec", "linear_fwd", 5, 1, 256, "E0 = 1 <= 4, E1 % 4 == 0; N = 5: the second workgroup holds one live wave of four"),
    F("thin_fwd_vec", "linear_fwd", 8, 4, 260, "E0 = 4 the last thin width; E1 = 260: lane 1 alone takes a second trip (k = 256 + 4)"),
    F("thin_fwd_scalar", "linear_fwd", 3, 2, 2, "E1 % 4 != 0 -> scalar loads; N = 3 % 4 != 0: ragged last workgroup"),
    F("thin_fwd_scalar", "linear_fwd", 6, 3, 67, "E1 = 67: lanes 0..2 take a second trip (k = 64 + lane), N = 6 ragged"),
    F("thin_fwd_scalar", "linear_fwd", 5, 2, 64, "E1 % 4 == 0 but X sits 4 bytes off a 16-byte boundary", base_skew=4),
    F("thin_fwd_vec+stage", "linear_act_fwd", 7, 1, 128, "a stage rides in the thin kernel's epilogue", stages=("drop",)),
    # k_linsmall_fwd<LG>: LG = 16 / 32 / 64 by E0 <= 16 / 32 / 64; 4 * 64 / LG rows per workgroup
    F("small_fwd_16", "linear_fwd", 17, 5, 33, "E0 = 5 the first width off the thin kernel; 16 rows per workgroup, N = 17: one row in the second"),
    F("small_fwd_16", "linear_fwd", 16, 16, 65, "E0 = 16 = LG: every lane live; E1 = 65 = one k past a wave's stride"),
    F("small_fwd_32", "linear_fwd", 9, 17, 40, "E0 = 17 the first with LG = 32; 8 rows per workgroup, N = 9"),
    F("small_fwd_32", "linear_fwd", 8, 32, 100, "E0 = 32 = LG"),
    F("small_fwd_64", "linear_fwd", 5, 33, 70, "E0 = 33 the first with LG = 64; 4 rows per workgroup, N = 5"),
    F("small_fwd_64", "linear_fwd", 4, 64, 128, "E0 = 64, E1 = 128 the last the LDS admits: 64 * 128 + 64 * 64 = 12288"),
    F("small_fwd_16+softmax", "linear_softmax_fwd", 33, 10, 100, "the classifier head, N = 33 ragged"),
    F("small_fwd_16+softmax", "linear_softmax_fwd", 5, 1, 20, "E0 = 1 with a softmax stays off the thin kernel: P = 1 everywhere"),
    F("small_fwd_32+softmax", "linear_softmax_fwd", 9, 20, 64, "LG = 32"),
    F("small_fwd_64+softmax", "linear_softmax_fwd", 6, 40, 64, "LG = 64"),
    F("small_fwd_16+stage", "linear_act_fwd", 17, 16, 40, "one stage rides", stages=("drop",)),
    F("small_fwd_16+stage", "linear_act_fwd", 17, 16, 40, "tanh: held to the witness's 4 ulps in both passes", stages=("tanh",)),
    F("small_fwd_32+stage", "linear_block_fwd", 9, 24, 40, "one stage rides, the layer-0 copy is a launch of its own", stages=("leaky",), copy=True),
    F("small_fwd_64", "linear_block_fwd", 5, 48, 40, "two stages: the head kernel carries none, the run is one launch behind it", stages=("relu", "drop")),
    # the linear_small_ok boundary pairs: one side a vector-ALU kernel, the other an MFMA sliver
    F("small_fwd_64", "linear_fwd", 6, 64, 128, "admitted: 64 * 128 + 64 * 64 = 12288 (the backward inequality binds at E0 = 64, not the forward one)"),
    F("gemm_unsplit", "linear_fwd", 6, 64, 129, "refused: 64 * 129 + 64 * 64 = 12352 > 12288; E1 = 129 % 4 != 0: no DMA blocks, the register-staged kernel"),
    F("gemm_sliver", "linear_fwd", 6, 64, 152, "refused as well (64 * 152 + 4096 = 13824): E1 % 4 == 0, the sliver kernel"),
    F("gemm_unsplit", "linear_fwd", 6, 64, 153, "... and E1 = 153 % 4 != 0: the register-staged kernel"),
    F("small_fwd_16", "linear_fwd", 6, 7, 512, "admitted: 7 * 513 + 16 * 512 = 11783"),
    F("gemm_sliver", "linear_fwd", 6, 8, 512, "refused: 8 * 513 + 8192 = 12296 > 12288; K = 512 <= 832 and % 4 == 0: the sliver kernel"),
    F("gemm_sliver", "linear_fwd", 6, 65, 16, "E0 = 65 > 64"),
    F("gemm_sliver", "linear_fwd", 6, 4, 516, "E1 = 516 > 512 (a thin width)"),
    F("gemm_splitk", "linear_fwd", 6, 4, 513, "E1 = 513 > 512, % 4 != 0: no sliver; K >= 256 on one tile: 5 slabs of 128 and a fold"),
    # the GEMM forms
    F("gemm_sliver+riders", "linear_block_fwd", 33, 68, 100, "E0 = 68 > 64; one ragged 32-tile each way, K = 100: a tail of 4 behind three blocks; run of two and the copy ride", stages=("leaky", "drop"), copy=True),
    F("gemm_sliver+riders", "linear_act_fwd", 64, 96, 48, "K = 48: half a block behind one", stages=("relu",)),
    F("gemm_splitk+riders", "linear_block_fwd", 40, 72, 896, "K = 896 > 832: off the sliver kernel; 2 tiles, K >= 256: split, everything in the fold launch", stages=("drop", "leaky"), copy=True),
    F("gemm_splitk+riders", "linear_block_fwd", 40, 72, 896, "tanh in the fold launch, the dropout behind it on the stored tanh", stages=("tanh", "drop")),
    F("gemm_sliver+riders", "linear_block_fwd", 33, 68, 100, "tanh in the sliver kernel's epilogue", stages=("drop", "tanh")),
    F("gemm_splitk+riders", "linear_act_fwd", 64, 128, 1024, "whole 64-deep slabs", stages=("drop",)),
    F("gemm_unsplit+separate", "linear_block_fwd", 20, 70, 130, "E1 = 130 % 4 != 0: no sliver; K = 130 < 256: unsplit; copy, run as launches of their own", stages=("relu", "drop"), copy=True),
    F("gemm_unsplit+separate", "linear_act_fwd", 20, 70, 130, "one stage: mask draw + activate", stages=("drop",)),
    F("gemm_sliver", "linear_softmax_fwd", 9, 100, 64, "E0 = 100 > 64: product, then the softmax kernel"),
    # t4k_mlp_head_fwd: the NARROW fold form needs layer 1 off the head kernels and split, layer 2 head-sized
    F("gemm_sliver_deferred+small_fwd_16_narrow", "mlp_head_fwd", 33, 10, 512, "H = 100: layer 1 (K = 512 >= 256) splits over idle CUs as slabs, the 100 -> 10 head folds them", H=100, stages=("drop",), softmax=True),
    F("gemm_sliver_deferred+small_fwd_32_narrow", "mlp_head_fwd", 9, 20, 300, "H = 72, LG = 32, no softmax, K = 300: ragged slabs", H=72, stages=("relu",), softmax=False),
    F("gemm_sliver_deferred+small_fwd_64_narrow", "mlp_head_fwd", 5, 40, 256, "H = 68, LG = 64: one row per workgroup", H=68, stages=("leaky",), softmax=True),
    F("gemm_sliver+separate+small_fwd_16+softmax", "mlp_head_fwd", 9, 10, 100, "K = 100 < 256: unsplit, layer by layer", H=68, stages=("drop",), softmax=True),
)

# backward.  dW's depth is N, dX's E0
BWD_CASES = (
    # thin heads, E0 <= 4
    F("thin_bwd_cols8", "linear_bwd", 1, 1, 8, "trained, E1 = 8 the first stripe width; N = 1"),
    F("thin_bwd_cols8", "linear_bwd", 33, 4, 9, "E1 = 9: a second stripe of one column; N = 33: row group 0 of 32 takes a second row"),
    F("thin_bwd_cols8", "loss_linear_bwd", 257, 1, 17, "E1 = 17: three stripes; N = 257: a second trip of the 256-row walk; target behind the ticket", masks=1),
    F("thin_bwd_cols8", "linear_block_bwd", 1024, 2, 256, "N = 1024 the last batch of the stripes", masks=2, tgt=True),
    F("thin_bwd_ticket", "linear_bwd", 3, 2, 2, "trained, E1 = 2 < 8"),
    F("thin_bwd_ticket", "linear_block_bwd", 9, 4, 7, "E1 = 7 < 8; N = 9: a second row group of one row", masks=2, tgt=True),
    F("thin_bwd_ticket", "linear_bwd", 1025, 1, 256, "N = 1025 > 1024: 129 row groups, the fold's fifth trip of 32 holds one"),
    F("thin_bwd_ticket", "loss_linear_bwd", 1032, 3, 300, "E1 = 300 > 256: the second column of a thread", masks=1),
    F("thin_bwd_frozen", "linear_block_bwd", 9, 1, 256, "train = 0: dX only", masks=2, tgt=True, train=0),
    F("thin_bwd_frozen", "linear_bwd", 5, 4, 3, "dX only through DW = NULL", has_dw=False),
    # column slices: 5 <= E0 <= 51, N <= 512, N (E0 + 4) + 4 E0 + 256 <= 12288, N E1 <= 32768
    F("small_bwd_cols", "linear_bwd", 1, 5, 5, "N = 1; E1 = 5: a second slice of one column"),
    F("small_bwd_cols", "linear_block_bwd", 33, 10, 100, "the classifier head", masks=1, tgt=True),
    F("small_bwd_cols", "linear_bwd", 128, 5, 256, "N E1 = 32768 the last"),
    F("small_bwd_cols", "loss_linear_bwd", 512, 16, 64, "N = 512 the last; E0 = 16: 16 x 4 outputs, 4 thread groups; N x CW = 2048 = ZI x 256", masks=1),
    F("small_bwd_cols", "linear_bwd", 200, 51, 12, "E0 = 51 the last: 51 x 5 = 255 <= 256"),
    F("small_bwd_cols", "linear_block_bwd", 40, 17, 33, "E0 = 17: 68 outputs, 3 thread groups; frozen", masks=2, tgt=True, train=0),
    # the general head kernel: what the column slices refuse
    F("small_bwd", "linear_bwd", 5, 52, 12, "E0 = 52: 52 x 5 = 260 > 256; one trip, CBK = 1"),
    F("small_bwd", "linear_bwd", 129, 5, 256, "N E1 = 32768 + E1; E1 = 256: 64 rows a trip, 3 trips -> CBK = 4 (5 x 4 <= 128)"),
    F("small_bwd", "linear_block_bwd", 65, 6, 512, "N E1 = 33280 > 32768, E1 = 512: N = 65 is the first second trip -> CBK = 8; two columns per thread are off", masks=2, tgt=True),
    F("small_bwd", "linear_bwd", 164, 40, 200, "N E1 = 32800; 40 x 4 = 160 > 128: CBK = 1, three dependent trips of 64 rows"),
    F("small_bwd", "loss_linear_bwd", 513, 8, 40, "N = 513 > 512; E1 = 40 <= 64: CBK = 1, 64 lanes x 4 groups, 3 trips of 256 rows (U = 64)", masks=1),
    F("small_bwd", "linear_bwd", 64, 64, 128, "E0 = 64, E1 = 128 the corner of linear_small_ok; N = 64: half a trip at CL = 128"),
    F("small_bwd", "linear_block_bwd", 300, 52, 16, "frozen with a target: no dW workgroups, the dX workgroups store out - target themselves", masks=1, tgt=True, train=0),
    F("refused:residency->separate_colsum_add+dw_splitk+dx_unsplit", "linear_bwd", 600, 7, 512,
      "N = 600 > 512, E1 = 512: 2 rows of dX per workgroup -> nA = 300, nB = 7 x 8: 356 > 256 CUs, in place refused; E0 % 4 != 0 keeps it off the dual launch and the slivers: dW on slabs (K = 600 >= 256) + fold, column sums in one chunk, dX unsplit"),
    F("small_bwd", "linear_bwd", 600, 7, 512, "the same shape apart stays on the head kernel (356 workgroups, nobody waits)", in_place=False),
    F("small_bwd", "linear_bwd", 400, 7, 512, "in place, nA + nB = 200 + 56 = 256 = the CU count: the last the arrival counter admits", in_place=True),
    F("refused:residency->separate_colsum_add+dw_splitk+dx_unsplit", "linear_bwd", 402, 7, 512, "... 201 + 56 = 257", in_place=True),
    F("refused:target_without_alias->small_bwd", "linear_block_bwd", 129, 5, 256, "target, dX apart: the first attempt is refused, out -= target goes first", masks=2, tgt=True, in_place=False),
    # dual dW || dX on 32 x 32 tiles: E0, E1 % 4 == 0, off the head kernels
    F("dual_l32_4", "linear_bwd", 33, 68, 36, "E0 = 68 > 64; ragged 32-tiles in E0, E1 and N; K = N = 33: a tail of 1 behind a block"),
    F("dual_l32_4", "linear_block_bwd", 36, 128, 516, "E1 = 516 > 512; K tail of 4 in N, ragged E1", masks=2),
    F("dual_l32_4", "linear_block_bwd", 256, 256, 48, "N = E0 = 256 the last without blocks in registers; E1 = 48: half a tile; out -= target as a launch in front", masks=1, tgt=True),
    F("dual_l32_rst4", "linear_bwd", 257, 68, 36, "N = 257 > 256"),
    F("dual_l32_rst4", "linear_block_bwd", 48, 260, 64, "E0 = 260 > 256: the dX half walks blocks 2, 3; K = N = 48: half a block behind one", masks=2),
    F("dual_l32_rst8", "linear_bwd", 513, 68, 36, "N = 513 > 512"),
    F("dual_l32_rst8", "linear_block_bwd", 40, 516, 64, "E0 = 516 > 512", masks=2),
    F("dual_l32_4", "linear_bwd", 64, 256, 2048, "a1 = 8 x 64 = 512 the last"),
    F("dual_l32_4", "linear_bwd", 64, 64, 7872, "a1 + ar + a2 = 492 + 1 + 492 = 985 <= 4 x 256 - 32 = 992: more workgroups than fit the chip, the in-place gate rests on dispatch in id order"),
    F("dual_64_f11", "linear_bwd", 64, 64, 7936, "... 496 + 1 + 496 = 993 > 992 with t1 + riders + t2 = 249 <= 256"),
    # dual dW || dX on 64 x 64 tiles: a1 > 512 with t1 + riders + t2 <= 256
    F("dual_64_f11", "linear_block_bwd", 64, 1024, 544, "a1 = 32 x 17 = 544 > 512; t1 + riders + t2 = 144 + 16 + 9; N % 64 == 0 and E0 % 64 == 0", masks=2),
    F("dual_64_f00", "linear_block_bwd", 60, 1020, 548, "a1 = 32 x 18; ragged everywhere", masks=2),
    F("dual_64_f10", "linear_bwd", 64, 1020, 548, "N % 64 == 0 only"),
    F("dual_64_f01", "linear_bwd", 60, 1024, 544, "E0 % 64 == 0 only"),
    # the dual launch refused: gemm_launch per product
    F("separate_colsum_rider+dw_unsplit+dx_unsplit", "linear_bwd", 40, 70, 36, "E0 = 70 % 4 != 0: no dual launch, no vector loads: the generic kernel carries the column sums"),
    F("separate_colsum_rider+dw_unsplit+dx_unsplit", "linear_block_bwd", 40, 68, 70, "E1 = 70 % 4 != 0; the run's backward as a launch of its own", masks=2),
    F("separate_colsum_add+dw_splitk+dx_sliver", "linear_bwd", 2048, 68, 64, "N = 2048 > 1024 with a product that would split: dW on 32 slabs + fold, column sums in 8 chunks + fold"),
    # frozen, off the head kernels: dX only
    F("dx_only_fold_rider:sliver", "linear_block_bwd", 33, 68, 100, "frozen: the chain rides in the sliver kernel", masks=2, train=0),
    F("dx_only_fold_rider:splitk", "linear_block_bwd", 40, 896, 72, "K = E0 = 896 > 832: split, the chain rides in the fold", masks=2, train=0),
    F("dx_only_unfused:unsplit", "linear_block_bwd", 20, 130, 70, "E0 = 130 % 4 != 0, K < 256: unsplit, the run's backward behind it", masks=2, train=0),
)

# the one-launch head backward: (N, EB, E1) with H = EA; a1 = t32(EA, E1), a2 = t32(N, E1), nr = 1 + EA / 4
HEAD_CASES = (
    F("head_bwd", "mlp_head_bwd", 1, 1, 4, "N = 1, EA = 4, EB = 1, E1 = 4: every lower edge at once", H=4),
    F("head_bwd", "mlp_head_bwd", 37, 16, 36, "EB = 16 the last; ragged N and E1 tiles", H=52),
    F("head_bwd", "mlp_head_bwd", 33, 3, 260, "EA = 256 the last; 2 resident workgroups per CU at 66.5 KB of LDS", H=256),
    F("head_bwd", "mlp_head_bwd", 128, 10, 2784, "a1 + a2 + nr = 348 + 348 + 33 = 729 <= 3 x 256 - 32 = 736", H=128),
    F("head_bwd_refused", "mlp_head_bwd", 128, 10, 2816, "... 352 + 352 + 33 = 737 > 736", H=128),
    F("head_bwd_refused", "mlp_head_bwd", 16, 17, 64, "EB = 17 > 16", H=64),
    F("head_bwd_refused", "mlp_head_bwd", 16, 4, 64, "EA = 260 > 256", H=260),
    F("head_bwd_refused", "mlp_head_bwd", 257, 4, 64, "N = 257 > 256", H=64),
    F("head_bwd_refused", "mlp_head_bwd", 16, 4, 66, "E1 % 4 != 0", H=64),
    F("head_bwd_runs", "mlp_block_bwd", 40, 1, 132, "two masks behind the head, two behind the big layer", H=96, masks=2),
    F("head_bwd_runs", "mlp_block_bwd", 64, 4, 128, "one mask each", H=64, masks=1),
    F("head_bwd_runs_frozen", "mlp_block_bwd", 40, 1, 132, "train = 0: no dW tiles", H=96, masks=2, train=0),
)

# labels of section 1 of the issue that no shape reaches in the release build at 256 CUs, and why
UNREACHABLE = {
    "head_bwd: a1 + a2 + nr on either side of 768": "k_head_bwd_l32 takes 144 VGPRs: at most 3 workgroups per CU, so nb * cu - 32 = 736 < 768 binds first "
                                                    "(HEAD_CASES holds 729 | 737); the 768 slots bind only from 267 CUs",
    "small_bwd: the trip boundary N = 64 | 65 at E1 = 256": "N E1 <= 32768 keeps every N <= 128 at E1 = 256 on the column slices, and E0 >= 52 does not fit linear_small_ok at "
                                                            "E1 = 256; the boundary is taken at E1 = 512 instead (65 x 6 x 512: the first second trip)",
    "small_bwd refused:lds": "needs N + 768 > 12288 floats with dW workgroups - a batch of 11521: outside a sweep of seconds",
    "thin_bwd_ticket workspace refusal": "(G + 1) E0 E1 x 4 bytes > 32 MiB needs N > 32768 at E0 E1 = 2048",
}

ALL_CASES = FWD_CASES + BWD_CASES + HEAD_CASES
REQUIRED_LABELS = (
    "thin_fwd_vec", "thin_fwd_scalar", "small_fwd_16", "small_fwd_32", "small_fwd_64", "+softmax", "+stage", "_narrow", "gemm_sliver+riders",
    "gemm_splitk+riders", "gemm_unsplit+separate", "thin_bwd_cols8", "thin_bwd_ticket", "thin_bwd_frozen", "small_bwd_cols", "small_bwd",
    "refused:residency", "refused:target_without_alias", "dual_l32_4", "dual_l32_rst4", "dual_l32_rst8", "dual_64_f00", "dual_64_f01",
    "dual_64_f10", "dual_64_f11", "separate_colsum_rider", "separate_colsum_add", "dx_only_fold_rider", "dx_only_unfused", "head_bwd",
    "head_bwd_runs", "head_bwd_runs_frozen", "head_bwd_refused")

# the linear_small_ok boundary pairs: (admitted, refused)
# (64, 152) | (64, 153) is the pair as the issue names it: E0 E1 + 64 E0 <= 12288 refuses both (E1 <= 128 at E0 = 64), they still differ
# (DMA blocks | register-staged); (64, 128) | (64, 129) is the boundary itself
BOUNDARY_PAIRS = (((64, 152), (64, 153)), ((7, 512), (8, 512)), ((64, 16), (65, 16)), ((4, 512), (4, 513)), ((64, 128), (64, 129)))


# ----------------------------------------------------------------------------- operands
def exact_operands(rng, shape, lo=-2, hi=2):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def exact_masks(rng, shape):
    return rng.integers(0, 3, shape).astype(np.float32)


def exact_bound(case):
    """(terms, magnitude of a term) of the deepest sum any tensor of the case holds on the exact pass's operands: X, W, dY, target, DW / DB in
    {-2 .. 2}, masks in {0, 1, 2}.  out - target <= 4, dX terms <= 4 x 2, a head's dY1 = dX2 x mask <= (EB x 8) x 2, masks multiply by <= 4"""
    N, E0, E1, H = case.N, case.E0, case.E1, case.kw.get("H", 0)
    if case.entry in ("mlp_head_bwd", "mlp_block_bwd"):
        dy1 = E0 * 8 * 4                                  # |dX2| <= EB x 4 x 2, two masks
        return max(N, H) + 1, dy1 * 2                     # dW1: N terms of dy1 x 2 (+ the preload); dX1: EA terms
    if case.entry == "mlp_head_fwd":
        return max(E1, H) + 1, (E1 * 4 + 2) * 2           # layer 2's terms: |A1| <= E1 x 4 + 2 times |W2| <= 2
    return max(N, E0, E1) + 1, 4 * 2


# ----------------------------------------------------------------------------- what the sweep holds every tensor to (GPU and CPU alike)
GUARD = np.float32(-777.25)
LEAD = 4                                                   # guard words in front of and behind every tensor (16 bytes: the alignment class is the offset's)
KIND = {"relu": "relu", "leaky": "leaky", "drop": "dropout", "tanh": "tanh"}
ALPHA = {"relu": 0.0, "leaky": 0.5, "drop": 0.5, "tanh": 0.0}          # leaky 0.5: exact on integers; tanh is held to its witness's allowance in both passes


def guarded(shape, off=0, data=None):
    """(host image, index of the first element, elements) of a tensor `off` bytes into a 16-byte aligned allocation with guard words on either
    side; NaN where no data is given: an element the call leaves unwritten fails every witness"""
    n, k = int(np.prod(shape)), LEAD + off // 4
    a = np.full(k + n + LEAD, GUARD, np.float32)
    a[k:k + n] = np.nan if data is None else np.asarray(data, np.float32).ravel()
    return a, k, n


def unguard(a, k, n, shape, name=""):
    assert np.all(a[:k] == GUARD) and np.all(a[k + n:] == GUARD), "%s: guard word overwritten" % name
    return a[k:k + n].reshape(shape)


def hold(exact, name, got, w, kind):
    """exact pass: bit-equal to the float64 result; float pass: inside the witness's bound"""
    if exact:
        return wt.equal(name, got, w.exact, kind="linear exact: " + kind)
    return wt.check(name, got, w, kind="linear: " + kind)


def seed_of(*v):
    s = 17
    for x in v:
        s = (s * 1000003 + int(x)) % (1 << 31)
    return s


def draw(rng, exact, shape, core=None):
    """operands of a pass at `core` shape, zero-padded to `shape` (the boundary pairs: the refused side is the admitted one plus a zero column)"""
    core = tuple(np.atleast_1d(shape)) if core is None else tuple(np.atleast_1d(core))
    a = exact_operands(rng, core) if exact else rng.standard_normal(core).astype(np.float32)
    out = np.zeros(tuple(np.atleast_1d(shape)), np.float32)
    out[tuple(slice(0, c) for c in core)] = a
    return out


def draw_mask(rng, exact, shape):
    if exact:
        return exact_masks(rng, shape)
    return (np.where(rng.random(shape) < 0.5, 1.0, 0.2) * (rng.random(shape) < 0.7)).astype(np.float32)


def fwd_operands(exact, N, E0, E1, core=None):
    c0, c1 = core or (E0, E1)
    rng = np.random.default_rng(seed_of(N, c0, c1, exact, 1))
    return dict(X=draw(rng, exact, (N, E1), (N, c1)), W=draw(rng, exact, (E0, E1), (c0, c1)), B=draw(rng, exact, E0, c0))


def bwd_operands(exact, N, E0, E1, masks=0, core=None, salt=0):
    c0, c1 = core or (E0, E1)
    rng = np.random.default_rng(seed_of(N, c0, c1, exact, 2, salt))
    ops = dict(X=draw(rng, exact, (N, E1), (N, c1)), W=draw(rng, exact, (E0, E1), (c0, c1)), DY=draw(rng, exact, (N, E0), (N, c0)),
               T=draw(rng, exact, (N, E0), (N, c0)), DW0=draw(rng, exact, (E0, E1), (c0, c1)), DB0=draw(rng, exact, E0, c0))
    for i in range(masks):
        ops["M%d" % i] = draw_mask(rng, exact, (N, E1))        # M0 multiplies dX, M1 the product
    return ops


def check_fwd(tag, exact, ops, got, stages=(), us=(), softmax=False, copy=False):
    """got: Y, (F0, A0, F1, A1), (P), (C) as the call left them, X / W / B re-read.  Each stage is witnessed on the input the call stored"""
    hold(exact, tag + " Y", got["Y"], wt.linear(ops["X"], ops["W"], ops["B"]), "Y")
    x = got["Y"]
    for i, st in enumerate(stages):
        wo, wm = wt.act(KIND[st], x, ALPHA[st], us[0].reshape(x.shape) if st == "drop" else None)
        ex = exact and st != "tanh"                          # the one stage that is no linear function of the operands
        hold(ex, "%s %s mask" % (tag, st), got["F%d" % i], wm, "stage mask" + ("" if st != "tanh" else " (tanh)"))
        hold(ex, "%s %s out" % (tag, st), got["A%d" % i], wo, "stage out" + ("" if st != "tanh" else " (tanh)"))
        x = got["A%d" % i]
    if softmax:
        wt.check(tag + " P", got["P"], wt.softmax(got["Y"]), kind="linear: softmax")
    if copy:
        wt.equal(tag + " copy of X", got["C"], ops["X"], kind="linear exact: copy")
    for k in ("X", "W", "B"):
        if k in got:
            wt.equal(tag + " %s untouched" % k, got[k], ops[k])
    return x


def check_bwd(tag, exact, ops, got, *, train=1, has_dw=True, tgt=False, masks=0, in_place=True):
    """got: DX, (D0, D1), DW, DB, DY (= OUT), (OUT2), W, T, (M0, M1), and X when dX went apart - every tensor the call wrote or had to leave"""
    dy = ops["DY"]
    if tgt:
        dy = ops["DY"] - ops["T"]                           # one fp32 subtraction: IEEE, bit-equal everywhere
        wt.equal(tag + " out - target in place", got["DY"], dy, kind="linear exact: out - target")
        wt.equal(tag + " out - target, second destination", got["OUT2"], dy, kind="linear exact: out - target")
    else:
        wt.equal(tag + " dY untouched", got["DY"], ops["DY"])
    hold(exact, tag + " dX", got["DX"], wt.gemm(dy, ops["W"]), "dX")
    g = got["DX"]
    for i in range(masks):
        hold(exact, tag + " mask chain stage %d" % i, got["D%d" % i], wt.mul(g, ops["M%d" % i]), "mask chain")
        wt.equal(tag + " mask %d untouched" % i, got["M%d" % i], ops["M%d" % i])
        g = got["D%d" % i]
    if train and has_dw:
        hold(exact, tag + " dW", got["DW"], wt.gemm(dy, ops["X"], O0=ops["DW0"], beta=1.0, tA=1), "dW")
        hold(exact, tag + " dB", got["DB"], wt.dlinear_db(dy, ops["DB0"]), "dB")
    else:
        wt.equal(tag + " DW untouched (no training pass)", got["DW"], ops["DW0"])
        wt.equal(tag + " DB untouched (no training pass)", got["DB"], ops["DB0"])
    if not in_place:
        wt.equal(tag + " X untouched (dX apart)", got["X"], ops["X"])
    wt.equal(tag + " W untouched", got["W"], ops["W"]); wt.equal(tag + " target untouched", got["T"], ops["T"])
