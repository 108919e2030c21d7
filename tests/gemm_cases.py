"""Cases of the GEMM sweep and a Python mirror of the dispatch ladder they are chosen against - shared by the GPU sweep
(tests/test_gpu_gemm_sweep.py) and its CPU self-test (tests/test_gemm_cases.py), the arrangement of linear_cases.py.

The mirror restates gemm_plan, the planner gemm_launch runs (tensorforth_amd/csrc/gemm.hip), inequality by inequality, with every GemmLab switch at
its release default (gemm_types.h).  It returns the string t4k_gemm_last_plan() reports and the launch count; the GPU sweep asserts both
for every row, so a heuristic that moves a shape to another kernel fails the sweep instead of leaving it green on the wrong kernel.
Everything is sized for the MI355X's 256 CUs; the sweep passes the device's count and FAILS a row that no longer reaches its label.

Storage: A is [K, M] when tA else [M, K], B is [N, K] when tB else [K, N], O is [M, N] (each x C channel-interleaved), row-major."""
import numpy as np

import f64_witness as wt

CU = 256                                    # the MI355X
S32_MAXK = 832                              # GemmLab::s32_maxk: deepest K one sliver workgroup walks
WS_BYTES = 64 << 20                         # runtime.hip: a stream's workspace
KG = 64                                     # split-K granularity
MOAT = 256                                  # NaN floats in front of and behind every operand of the sweep


def cdiv(a, b):
    return -(-a // b)


def _fill(tiles, cu):
    return tiles / float(cdiv(tiles, cu) * cu)


# ----------------------------------------------------------------------------- the ladder
def ladder(M, N, K, tA, tB, C=1, cu=CU, aligned=True, alpha=1.0, beta=0.0, bias=False, lane=0, capturing=False,
           defer=False, cs_rows=0, riders=False, gates=True, ws=WS_BYTES):
    """gemm_launch as a dict: plan (the hook's string), launches, base (the kernel form alone), nsplit, kchunk, and what the linear layers
    ask about: riders_ride, cs_ride, deferred.  aligned: A and B on 16-byte boundaries; lane: 0 the default stream, i + 1 a library stream;
    riders: an activation / mask-chain / copy rider is requested; cs_rows: a column-sum request over that many rows; defer: the caller folds"""
    def out(base, nsplit=1, fold=False, kchunk=0, riders_ride=False, cs_ride=False, deferred=False):
        plan = base + ("x%d" % nsplit if nsplit > 1 else "") + ("+fold" if fold else "")
        return dict(plan=plan, launches=1 + (1 if fold else 0), base=base, nsplit=nsplit, kchunk=kchunk, fold=fold,
                    riders_ride=riders_ride, cs_ride=cs_ride, deferred=deferred)
    if M == 0 or N == 0:
        return dict(out("none"), launches=0)
    if K == 0:
        return out("k0")
    plain = alpha == 1.0 and beta == 0.0
    cs_ok = 0 < cs_rows <= 4096
    a_contig, b_contig = (M if tA else K), (K if tB else N)
    vec = C == 1 and aligned and a_contig % 4 == 0 and b_contig % 4 == 0
    t128 = cdiv(M, 128) * cdiv(N, 128)
    big = t128 >= cu * 3 // 4
    bm = 128 if big else 64
    tiles = cdiv(M, bm) * cdiv(N, bm)
    dma32 = M * K * 4 < (1 << 32) and K * N * 4 < (1 << 32)
    interior64 = M % 64 == 0 and N % 64 == 0
    # slivers
    akc, bkc = not tA, bool(tB)
    al = (not akc or (K % 4 == 0 and aligned)) and (not bkc or (K % 4 == 0 and aligned))
    t32 = cdiv(M, 32) * cdiv(N, 32)
    ns, kc = 1, cdiv(K, 8) * 8
    if defer and plain and K >= 256:
        want = min(cdiv(cu, t32), K // 128, 16)
        if want > 1:
            kc = cdiv(cdiv(K, want), 8) * 8; ns = cdiv(K, kc)
        if ns * M * N * 4 > ws // 2:
            ns, kc = 1, cdiv(K, 8) * 8
    dma_ok = aligned and (K % 4 == 0 if akc else M % 4 == 0) and (K % 4 == 0 if bkc else N % 4 == 0)
    if C == 1 and not big and tiles * 2 <= cu and K >= 1 and kc <= S32_MAXK and al and dma_ok and not capturing:
        nblk = cdiv(kc, 32)
        w8 = nblk > 16 or (nblk >= 6 and t32 * ns <= cu)
        rst = nblk > (16 if w8 else 8)
        return out("l32/w%d%s" % (8 if w8 else 4, "/rst" if rst else ""), ns, False, kc, ns == 1, cs_ok and ns == 1, ns > 1)
    # two workgroups per tile
    if gates and not big and vec and C == 1 and interior64 and K % 256 == 0 and K >= 512 and tiles * 2 <= cu and tiles * 3 > cu and tiles <= 2048 and \
            not defer and not riders and not cs_rows and lane == 0 and tiles * 4096 * 4 <= ws // 2 and dma32:
        return out("pair", kchunk=K)
    # split K
    nsplit, kchunk = 1, max(cdiv(K, KG) * KG, KG)
    if not big and C == 1 and tiles * 2 <= cu and K >= 4 * KG:
        want = min(cdiv(cu, tiles), K // KG, 64)
        if want > 1:
            kchunk = cdiv(cdiv(K, want), KG) * KG; nsplit = cdiv(K, kchunk)
            if nsplit * M * N * 4 > ws // 2:
                nsplit, kchunk = 1, cdiv(K, KG) * KG
    whole_k = kchunk % 64 == 0 and K % kchunk == 0
    ragged8 = not big and vec and C == 1 and nsplit == 1 and not interior64 and whole_k and M >= 4 and N >= 4 and dma32
    ragk = not big and vec and C == 1 and not whole_k and nsplit == 1 and M >= 4 and N >= 4 and K >= 8 and dma32
    full64 = not big and vec and interior64 and whole_k
    generic = big or not vec or not (full64 or ragged8 or ragk)
    cs = cs_ok and generic and nsplit == 1 and C == 1
    t128i, t64i = (M // 128) * (N // 128), cdiv(M, 64) * cdiv(N, 64)
    lean = vec and C == 1 and nsplit == 1 and not cs and dma32
    if lean and M % 128 == 0 and N % 128 == 0 and (K % 64 == 0 or K % 4 == 0) and K >= 256 and t128i >= cu and _fill(t128i, cu) * 1.035 > _fill(t64i, cu):
        base = plain128(M, N, K, cu); kchunk = K         # the lean kernels walk K itself, tail and all (GemmP::kchunk = K)
    elif lean and interior64 and K > 128 and K % 128 != 0:
        base = "plain_ragk"; kchunk = K
    elif big and vec and C == 1 and not tA and not tB and plain and not bias and not cs and interior64 and K % 128 == 0 and dma32:
        base = "nn_plain"
    elif big and lean and interior64 and K % 128 == 0:
        base = "plain_any"
    elif big and gates and lean and K % 64 == 0 and K >= 2048 and M >= 4 and N >= 4:
        base = "glds8<128>" if K % 128 == 0 else "glds8<64>"
    elif big:
        full = vec and kchunk % 32 == 0 and K % kchunk == 0 and M >= 4 and N >= 4
        base = "mfma<128,128,32,vec,full>" if full else "mfma<128,128,32,vec,skew>" if vec else "mfma<128,128,32>"
    elif not vec:
        base = "mfma<64,64,32>"
    elif ragk:
        base = "glds8<128,ragk>" if K >= 128 and (nsplit == 1 or kchunk % 128 == 0) else "glds8<64,ragk>"
    elif ragged8:
        base = "glds8<128>" if kchunk % 128 == 0 else "glds8<64>"
    elif interior64 and whole_k:
        if not dma32:
            base = "mfma<64,64,64,vec,full>"
        elif kchunk % 128 == 0 and not tA and not tB and nsplit == 1 and plain and not bias:
            base = "nn_plain"
        elif kchunk % 128 == 0 and nsplit == 1:
            base = "plain_any"
        else:
            base = "glds8<128>" if kchunk % 128 == 0 else "glds8<64>"
    else:
        base = "mfma<64,64,64,vec,skew>"                 # GemmLab::fullk = 0: the full form stays with operands of 4 GiB
    deferred = nsplit > 1 and defer and plain
    fold = nsplit > 1 and not deferred
    return out(base, nsplit, fold, kchunk, fold, cs, deferred)


def plain128(M, N, K, cu=CU):
    """launch_plain128: the 256-tile kernel, else 128-tiles on 32-deep stages, with a K tail, or 64-deep"""
    t256 = (M // 256) * (N // 256); t128 = 4 * t256
    if M % 256 == 0 and N % 256 == 0 and K % 32 == 0 and K >= 64 and t256 >= cu and _fill(t256, cu) * 1.04 > _fill(t128, cu) and \
            M * K < (1 << 30) and N * K < (1 << 30):
        return "plain256"
    if K % 32 == 0 and (M // 128) * (N // 128) >= 2 * cu:
        return "plain128/bk32"
    return "plain128/ragk" if K % 64 != 0 else "plain128"


# ----------------------------------------------------------------------------- the planner itself
GP_A16, GP_B16, GP_EPILOGUE, GP_BIAS, GP_RIDER, GP_DEFER, GP_LANE, GP_CAPTURING, GP_GATES_OFF = (1 << i for i in range(9))      # T4K_GP_* (include/t4k.h)


def plan_entry(lib, M, N, K, C, tA, tB, flags, cs_rows=0, cu=CU, ws=0):
    """t4k_gemm_plan: what gemm_launch's own planner answers on the host, in ladder()'s terms -
    (plan, launches, nsplit, kchunk, riders_ride, cs_ride, deferred)"""
    import ctypes
    text, out = ctypes.create_string_buffer(64), (ctypes.c_int * 6)()
    rc = lib.t4k_gemm_plan(M, N, K, C, tA, tB, flags, cs_rows, cu, ws, text, out)
    assert rc == 0, (M, N, K, C, tA, tB, flags, cs_rows, cu, ws, rc)
    return (text.value.decode(), out[2], out[0], out[1], bool(out[3]), bool(out[4]), bool(out[5]))


def plan_flags(a_ptr, b_ptr, alpha=1.0, beta=0.0, lane=0, capturing=False, more=0):
    """the flags word of a call as it is made: the real alignment of A and B, its epilogue, its stream and capture state"""
    return ((GP_A16 if a_ptr % 16 == 0 else 0) | (GP_B16 if b_ptr % 16 == 0 else 0) | (0 if (alpha, beta) == (1.0, 0.0) else GP_EPILOGUE) |
            (GP_LANE if lane else 0) | (GP_CAPTURING if capturing else 0) | more)


def gemm_kernel_plan(M, N, K, tA, tB, C=1, cu=CU, aligned=True, alpha=1, beta=0, lane=0, capturing=False):
    """(what t4k_gemm_last_plan() reports after t4k_gemm of this shape, kernel launches of the call)"""
    r = ladder(M, N, K, tA, tB, C, cu, aligned, float(alpha), float(beta), False, lane, capturing)
    return r["plan"], r["launches"]


# ----------------------------------------------------------------------------- the table
class Row:
    """one t4k_gemm call: the shape, layout and flags, the plan gemm_kernel_plan must give at 256 CUs for (alpha, beta) = (1, 0), and the
    inequality that sizes each extent.  skew: floats A and B sit off a 16-byte boundary"""

    def __init__(self, label, M, N, K, tA, tB, why, C=1, skew=0):
        self.label, self.M, self.N, self.K, self.tA, self.tB, self.why, self.C, self.skew = label, M, N, K, tA, tB, why, C, skew
        self.id = "%s-%dx%dx%d-%s%s%s%s" % (label.replace("<", "_").replace(">", "").replace(",", "_").replace("/", "_").replace("+", "_"), M, N, K,
                                           "T" if tA else "N", "T" if tB else "N", "-C%d" % C if C > 1 else "", "-skew" if skew else "")

    def plan(self, cu=CU, **kw):
        return gemm_kernel_plan(self.M, self.N, self.K, self.tA, self.tB, self.C, cu, aligned=not self.skew, **kw)

    def flops(self):
        return 2 * self.M * self.N * self.K * self.C


R = Row
ROWS = (
    # ---- slivers (k_gemm_l32): 64-tiles * 2 <= 256, kc = ceil8(K) <= 832, DMA lanes whole: K % 4 == 0 on a K-contiguous operand, else M / N % 4 == 0.
    #      nblk = ceil(kc / 32); w8 = nblk > 16 or (nblk >= 6 and t32 <= 256); rst = nblk > (16 if w8 else 8)
    R("l32/w4", 33, 68, 100, 0, 1, "nblk = 4 < 6; K = 100: K % 8 = 4, a tail of 4 behind three blocks; one ragged 32-tile each way"),
    R("l32/w4", 36, 40, 13, 1, 0, "no operand K-contiguous: any K >= 1, M % 4 = N % 4 = 0; K = 13 = one partial block"),
    R("l32/w4", 4, 4, 1, 1, 0, "K = 1 the least the rung takes (K >= 1); M = N = 4 the least whole DMA lane"),
    R("l32/w4", 576, 576, 256, 0, 0, "nblk = 8 >= 6 but t32 = 324 > 256: 4 waves; 8 blocks = the last without blocks in registers"),
    R("l32/w4/rst", 576, 572, 300, 0, 0, "nblk = 10 > 8, t32 = 324 > 256 with 81 64-tiles <= 128; K % 8 = 4; N = 572 a ragged edge tile"),
    R("l32/w4/rst", 572, 576, 512, 1, 1, "nblk = 16 the last of the 4-wave form; ragged M, both operands transposed"),
    R("l32/w8", 70, 68, 208, 0, 0, "nblk = 7 >= 6, t32 = 9 <= 256; K = 208: a tail of 16 (half a block); ragged M and N"),
    R("l32/w8", 100, 36, 512, 1, 0, "nblk = 16 the last without blocks in registers; A transposed"),
    R("l32/w8/rst", 64, 96, 516, 1, 1, "nblk = 17 > 16; a tail of 4"),
    R("l32/w8/rst", 64, 64, 832, 0, 1, "kc = 832 = s32_maxk the last depth of the sliver rung"),
    # ---- two workgroups per tile (PAIR): 86 .. 128 interior 64-tiles, K % 256 == 0; K >= 1024 (K <= 832 is a sliver), default stream
    R("pair", 576, 640, 1024, 0, 0, "90 tiles: 90 * 3 = 270 > 256 the first count of the form; K = 1024 the first K % 256 == 0 past 832"),
    R("pair", 1024, 512, 1024, 1, 1, "128 tiles = 256 / 2 the last; both operands transposed"),
    R("pair", 640, 576, 1280, 0, 1, "K = 1280: five 128-deep stages per half"),
    # ---- split K + k_splitk_fold: 64-tiles * 2 <= 256, K >= 256, the sliver refused (K > 832, or K % 4 != 0 on a K-contiguous operand)
    R("glds8<128>x4+fold", 512, 512, 1024, 0, 0, "64 tiles: want = 4, kchunk = 256 % 128 == 0 (64 * 3 = 192 <= 256: no pair)"),
    R("glds8<64>x2+fold", 1024, 512, 896, 0, 1, "128 tiles: want = 2, kchunk = 448 % 128 != 0; K = 896 % 256 != 0: no pair"),
    R("glds8<64>x16+fold", 64, 128, 1024, 1, 0, "2 tiles: want = min(128, K / 64) = 16, kchunk = 64"),
    R("glds8<64>x64+fold", 64, 64, 4096, 0, 0, "one tile, K = 4096: nsplit at its cap of 64"),
    R("mfma<64,64,64,vec,skew>x14+fold", 40, 72, 896, 0, 1, "ragged M and N: slabs on the skewed register-staged kernel; kchunk = 64"),
    R("mfma<64,64,64,vec,skew>x8+fold", 64, 64, 900, 0, 0, "interior, K = 900 not in whole chunks: kchunk = 128, the last slab holds 4"),
    R("mfma<64,64,32>x5+fold", 6, 4, 513, 0, 1, "K = 513 % 4 != 0 on K-contiguous operands: no vector loads; kchunk = 128, the last slab holds 1"),
    # ---- unsplit on 64-tiles: 129 .. 767 of them (768 x 704 = 132 the smallest interior grid), t128 < 192
    R("nn_plain", 768, 704, 128, 0, 0, "plain product, K % 128 == 0"),
    R("plain_any", 768, 704, 128, 1, 0, "another layout: the lean kernel with its layout arguments"),
    R("plain_any", 768, 704, 256, 0, 1, "two stages"),
    R("plain_any", 768, 704, 128, 1, 1, "both transposed"),
    R("plain_ragk", 768, 704, 132, 0, 1, "K = 132 > 128, K % 128 = 4: a tail of 4"),
    R("plain_ragk", 768, 704, 192, 1, 0, "K % 128 = 64: GemmLab::plain_ragk = 2 takes whole 64s too"),
    R("glds8<64>", 768, 704, 64, 0, 0, "K = 64 < 128: one 64-deep stage"),
    R("glds8<128>", 770, 704, 128, 0, 1, "ragged M, whole K stages: clamped source rows, predicated stores"),
    R("glds8<64>", 768, 708, 192, 1, 0, "ragged N, kchunk = 192 % 128 != 0"),
    R("glds8<128,ragk>", 770, 704, 784, 0, 0, "K = 784 = 6 x 128 + 16, ragged M (interior would be plain_ragk)"),
    R("glds8<128,ragk>", 768, 708, 132, 1, 1, "K = 132: one stage and a tail of 4; ragged N"),
    R("glds8<64,ragk>", 768, 704, 100, 0, 1, "K = 100 < 128 (interior: K > 128 fails for plain_ragk): a 64-deep stage and a tail of 36"),
    R("glds8<64,ragk>", 768, 704, 12, 0, 0, "K = 12: the tail alone"),
    R("glds8<64,ragk>", 772, 704, 8, 1, 0, "K = 8 the least the form takes"),
    R("mfma<64,64,64,vec,skew>", 768, 704, 4, 0, 0, "K = 4 < 8"),
    R("mfma<64,64,64,vec,skew>", 2, 8256, 64, 0, 0, "M = 2 < 4 (the clamp needs 4 rows); N = 8256: 129 tiles keep it off the sliver rung"),
    R("mfma<64,64,64,vec,skew>", 8256, 3, 64, 0, 1, "N = 3 < 4 with B transposed (K contiguous)"),
    R("mfma<64,64,32>", 768, 704, 64, 0, 0, "A and B 4 bytes off a 16-byte boundary", skew=1),
    R("mfma<64,64,32>", 770, 702, 64, 0, 0, "N = 702 % 4 != 0 contiguous in B"),
    R("mfma<64,64,32>", 33, 20, 40, 0, 0, "C = 2: channel-interleaved operands", C=2),
    R("mfma<64,64,32>", 20, 12, 9, 1, 1, "C = 3", C=3),
    # ---- big: t128 >= 192 (1536 x 2048 = 12 x 16 the smallest; 1792 x 1792 = 196)
    R("nn_plain", 1536, 2048, 128, 0, 0, "K = 128 < 256 keeps it off the 128-tiles; several 64-tiles per CU"),
    R("plain_any", 1792, 1792, 128, 1, 0, "another layout"),
    R("plain_ragk", 1536, 2048, 192, 0, 1, "K = 192 < 256, K % 128 != 0"),
    R("plain128", 2048, 2048, 256, 0, 1, "t128i = 256 >= 256 and fill 1.0 x 1.035 > 1.0 of the 64-tiles; K = 256 the least; 256 < 512 tiles: 64-deep stages"),
    R("plain128/ragk", 2048, 2048, 300, 1, 0, "K = 300 % 64 != 0, % 4 == 0: a tail of 44"),
    R("plain128/bk32", 2048, 4096, 288, 0, 0, "512 tiles >= 2 x 256, K = 288 % 32 == 0 (not % 64)"),
    R("plain256", 4096, 4096, 256, 0, 0, "t256 = 256 >= 256, fill 1.0 x 1.04 > 1.0; K = 256 the least the 128-tile rung in front admits"),
    R("plain256", 4096, 4096, 256, 0, 1, "B transposed"),
    R("plain256", 4096, 4096, 288, 1, 0, "A transposed; K % 32 == 0, not % 64"),
    R("plain256", 4096, 4096, 320, 1, 1, "both transposed"),
    R("nn_plain", 4096, 4352, 256, 0, 0, "1088 128-tiles fill 0.85 x 1.035 < 1.0 of the 4352 64-tiles: neither 128- nor 256-tiles"),
    R("glds8<128>", 1540, 2048, 2048, 1, 0, "ragged M, K = 2048 the least of big_dma"),
    R("glds8<64>", 1540, 2048, 2112, 0, 1, "K = 2112 % 128 = 64"),
    R("mfma<128,128,32,vec,full>", 1540, 2048, 64, 0, 0, "ragged M, K = 64 < 2048 in whole stages"),
    R("mfma<128,128,32,vec,full>", 1536, 2044, 128, 1, 1, "ragged N"),
    R("mfma<128,128,32,vec,skew>", 1536, 2048, 72, 0, 1, "K = 72 % 64 != 0 (kchunk = 128)"),
    R("mfma<128,128,32>", 1536, 2048, 8, 0, 0, "C = 2", C=2),
    R("mfma<128,128,32>", 1536, 2046, 40, 0, 0, "N % 4 != 0"),
)

# labels of the ladder that no call of t4k_gemm reaches in the release build at 256 CUs, with the arithmetic
UNREACHABLE = {
    "split-K workspace fallback (nsplit = 1)": "split K needs 64-tiles <= 128, so M N <= 128 x 4096 floats, and nsplit <= ceil(256 / tiles): nsplit M N x 4 bytes "
                                                "<= 256 x 4096 x 4 = 4 MiB (one tile at nsplit = 64: 1 MiB) against ws / 2 = 32 MiB",
    "pair workspace refusal": "tiles x 4096 x 4 bytes <= 128 x 16 KiB = 2 MiB < 32 MiB; tiles <= 2048 follows from tiles x 2 <= 256",
    "mfma<64,64,64,vec,full> (!dma32)": "an operand of 4 GiB: M K or K N >= 2^30 floats; GemmLab::fullk = 0 leaves the form no other way in",
    "plain256 refused by M K >= 2^30": "a 4 GiB operand again (4096 rows x 262144)",
    "glds8<128,ragk> on split-K slabs": "GemmLab::ragged_k = 1: unsplit products only",
}

REQUIRED = ("l32/w4", "l32/w4/rst", "l32/w8", "l32/w8/rst", "pair", "nn_plain", "plain_any", "plain_ragk", "plain128", "plain128/ragk", "plain128/bk32",
            "plain256", "glds8<128>", "glds8<64>", "glds8<128,ragk>", "glds8<64,ragk>", "mfma<128,128,32,vec,full>", "mfma<128,128,32,vec,skew>",
            "mfma<128,128,32>", "mfma<64,64,64,vec,skew>", "mfma<64,64,32>", "glds8<128>x4+fold", "glds8<64>x64+fold", "mfma<64,64,64,vec,skew>x14+fold",
            "mfma<64,64,32>x5+fold")
# every base form the mirror can return for t4k_gemm (ladder()'s `base`); test_gemm_cases.py holds the table against it
ALL_BASES = ("l32/w4", "l32/w4/rst", "l32/w8", "l32/w8/rst", "pair", "nn_plain", "plain_any", "plain_ragk", "plain128", "plain128/ragk", "plain128/bk32",
             "plain256", "glds8<128>", "glds8<64>", "glds8<128,ragk>", "glds8<64,ragk>", "mfma<128,128,32,vec,full>", "mfma<128,128,32,vec,skew>",
             "mfma<128,128,32>", "mfma<64,64,64,vec,skew>", "mfma<64,64,32>")

# the drifted cases of test_gpu_parity.py: (M, N, K, tA, tB, the kernel the comment above them named, what the ladder gives)
DRIFTED = (
    (1024, 512, 512, 1, 0, "pair", "l32/w4/rst"), (576, 832, 768, 1, 1, "pair", "l32/w8/rst"),
    (4096, 4096, 160, 0, 0, "plain256", "plain_ragk"), (4096, 4096, 96, 1, 1, "plain256", "mfma<128,128,32,vec,skew>"),
    (4096, 4352, 224, 0, 1, "plain256", "plain_ragk"), (4352, 4096, 64, 1, 0, "plain256", "mfma<128,128,32,vec,full>"),
)


def euler_walk(n):
    """a closed walk over the complete directed graph on n nodes that takes every edge once: every node follows every other"""
    out = {i: [j for j in range(n) if j != i] for i in range(n)}
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def first(label):
    return next(r for r in ROWS if r.label == label)


# ----------------------------------------------------------------------------- operands and witnesses
def seed_of(*v):
    s = 23
    for x in v:
        s = (s * 1000003 + int(x)) % (1 << 31)
    return s


def shapes(r):
    ch = (r.C,) if r.C > 1 else ()
    return ((r.K, r.M) if r.tA else (r.M, r.K)) + ch, ((r.N, r.K) if r.tB else (r.K, r.N)) + ch, (r.M, r.N) + ch


def operands(r, exact, K=None):
    """A, B as stored and O0; K: a reduced depth (CPU self-test)"""
    q = Row(r.label, r.M, r.N, r.K if K is None else K, r.tA, r.tB, r.why, r.C, r.skew)
    rng = np.random.default_rng(seed_of(q.M, q.N, q.K, q.tA, q.tB, q.C, exact))
    sa, sb, so = shapes(q)
    if exact:
        return (rng.integers(-2, 3, sa).astype(np.float32), rng.integers(-2, 3, sb).astype(np.float32), rng.integers(-3, 4, so).astype(np.float32))
    return rng.standard_normal(sa).astype(np.float32), rng.standard_normal(sb).astype(np.float32), rng.standard_normal(so).astype(np.float32)


class Product:
    """the float64 product of a row's operands and its magnitude, computed once (float64 BLAS) and shared by every (alpha, beta)"""

    def __init__(self, r, A, B):
        self.K = A.shape[0] if r.tA else A.shape[1]
        if r.C > 1:
            a = np.moveaxis(wt.f64(A), -1, 0); b = np.moveaxis(wt.f64(B), -1, 0)
            a = a.transpose(0, 2, 1) if r.tA else a; b = b.transpose(0, 2, 1) if r.tB else b
            self.ex = np.moveaxis(a @ b, 0, -1); self.mg = None
            self._ab = (np.abs(a), np.abs(b))
        else:
            a = wt.f64(A).T if r.tA else wt.f64(A); b = wt.f64(B).T if r.tB else wt.f64(B)
            self.ex = a @ b; self.mg = None
            self._ab = (np.abs(a), np.abs(b))
        self.C = r.C

    def mag(self):
        if self.mg is None:
            m = self._ab[0] @ self._ab[1]
            self.mg = np.moveaxis(m, 0, -1) if self.C > 1 else m
        return self.mg

    def exact(self, alpha, beta, O0):
        """bit-exact result on integer operands (every partial sum an integer below 2^24)"""
        return alpha * self.ex + (beta * wt.f64(O0) if beta != 0 else 0.0)

    def witness(self, alpha, beta, O0):
        """f64_witness.gemm's witness as it stands: c n 2^-24 mag with n = K + 2"""
        ex, mg = alpha * self.ex, abs(alpha) * self.mag()
        if beta != 0:
            ex = ex + beta * wt.f64(O0); mg = mg + abs(beta) * np.abs(wt.f64(O0))
        return wt.W(ex, mg, self.K + 2)


def exact_ok(r):
    """the precondition of the bit-equal pass: K terms of |a b| <= 4 (doubled by alpha = 2) plus |O0| <= 3 stay below 2^24"""
    return wt.is_int_exact(r.K + 1, 8)


def moated(data, skew=0, moat=MOAT):
    """(host image, index of the first element) of a tensor inside a larger allocation: `moat` NaN floats in front and behind, `skew` more in front"""
    d = np.asarray(data, np.float32).ravel()
    a = np.full(moat + skew + d.size + moat, np.nan, np.float32)
    a[moat + skew:moat + skew + d.size] = d
    return a, moat + skew


def check_moat(name, img, k, n, before=None):
    """the floats round a tensor are bit-identical to what was uploaded (NaN, compared as bits)"""
    want = np.full(img.size, np.nan, np.float32) if before is None else before
    a, b = img.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(a[:k], b[:k]), "%s: a float in front of the tensor was overwritten (index %d of the moat)" % (name, int(np.argmax(a[:k] != b[:k])))
    assert np.array_equal(a[k + n:], b[k + n:]), "%s: a float behind the tensor was overwritten (%d past the end)" % (name, int(np.argmax(a[k + n:] != b[k + n:])))
    return img[k:k + n]


def hold(name, got, prod, alpha, beta, O0, exact, kind):
    """one result against the float64 product: no NaN, then bit-equal (exact pass) or inside the witness's bound (float pass)"""
    got = np.asarray(got)
    assert not np.isnan(got).any(), "%s: NaN in O at flat index %d - O read at beta = 0, or an element from outside an operand reached an MFMA" % (
        name, int(np.argmax(np.isnan(got).ravel())))
    if exact:
        return wt.equal(name, got, prod.exact(alpha, beta, O0), kind="gemm exact: " + kind)
    return wt.check(name, got, prod.witness(alpha, beta, O0), kind="gemm: " + kind)
