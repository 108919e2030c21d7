"""Cases of the conv sweep and a Python mirror of the dispatch they are chosen against - shared by the GPU sweep (tests/test_gpu_conv_sweep.py)
and its CPU self-test (tests/test_conv_cases.py), the arrangement of gemm_cases.py.

The mirror restates the host side of conv.hip, conv_few.hip, conv_img.hip, conv_big.hip, colsum.hip and dconv.hip inequality by inequality, with
every ConvLab switch at its release default (conv_types.h).  It returns the string t4k_conv_last_plan() reports (include/t4k.h lists the tokens)
and the kernel launches of the call; memcpys are not launches.  Everything is sized for the MI355X's 256 CUs; the sweep passes the device's
count and FAILS a row that no longer reaches its label.

Tensors are NHWC, filters [C1][K][K][C0].  `skew` maps a tensor's name (I, O, F, B, ICOPY, DO, DX, DX2, DF, DB, and the block's PRE, PREM, POOL,
POST, POSTM, COPY) to the floats it starts past a 16-byte boundary (0: aligned)."""
import numpy as np

import f64_witness as wt
from gemm_cases import cdiv, euler_walk, seed_of   # noqa: F401  (euler_walk: the sweep's back-to-back walk takes it from here)

CU = 256                                    # the MI355X
WS_BYTES = 64 << 20                         # runtime.hip: a stream's workspace
LDS_FILTER_FLOATS = 8192                    # conv_types.h
GEO = {1: (1, 1, 0), 3: (3, 1, 1), 4: (4, 2, 1), 5: (5, 1, 2)}   # launch.h with_geometry: the four admitted (K, S, P)
L_RELU, L_TANH, L_LEAKY, L_DROPOUT, L_AVGPOOL, L_MAXPOOL, L_MINPOOL = 4, 5, 8, 10, 13, 14, 15   # t4_layer, include/t4k.h


def out_hw(H1, W1, K):
    _, S, P = GEO[K]
    return (H1 + 2 * P - K) // S + 1, (W1 + 2 * P - K) // S + 1


def al16(skew, name):
    return skew.get(name, 0) % 4 == 0


def al8(skew, name):
    return skew.get(name, 0) % 2 == 0


# ----------------------------------------------------------------------------- admission tests
def conv_supported(K, S, P):
    return K in GEO and GEO[K] == (K, S, P)


def conv_few_ok(K, Cin, Cout):
    """conv_few.hip: (G, NG) or None"""
    if Cin > 4 or Cout > 32 or K not in (3, 5):
        return None
    G = 4 if Cout <= 4 else 12
    NG = cdiv(Cout, G)
    if K * K * Cin * NG * G > LDS_FILTER_FLOATS:
        return None
    return G, NG


def few_token(name, K, Cin, Cout, x_al8):
    G, _ = conv_few_ok(K, Cin, Cout)
    v2 = Cin % 2 == 0 and x_al8
    return "%s<%d,%d,%d>" % (name, G, 1 if Cin == 1 else 4, 1 if Cin == 1 else 2 if v2 else 1)


def conv_big_ok(Cin, Cout):
    return Cin >= 32 and Cin % 32 == 0 and Cout >= 16 and Cout % 4 == 0


def same3x3(K, H1, W1, H0, W0):
    return K == 3 and H0 == H1 and W0 == W1


def conv_gemm_ksplit(npix, Cout, Cin, K):
    waves = cdiv(npix, 32) * cdiv(Cout, 32)
    return 2 if waves < 1536 and ((Cin + 1) // 2) * K * K >= 18 else 1


def gather_filter(C1, K, C0):
    return "raw" if C1 * K * K * C0 <= LDS_FILTER_FLOATS else "staged"


def gather_chunks(Cin, K, C1, C0):
    """trips of conv_gemm_body's chunk loop: one on the raw path, ceil(pairs / pairs per chunk) on the staged one"""
    if gather_filter(C1, K, C0) == "raw":
        return 1
    return cdiv((Cin + 1) // 2, LDS_FILTER_FLOATS // (K * K * 2 * 32))


def thin_fwd(N, H, W, C1, C0, skew, icopy, bn):
    """conv_img.hip conv_thin_fwd: None, or (token, workgroups, batch-norm chunks)"""
    npix = N * H * W
    if C1 < 1 or C1 > 4 or C0 not in (32, 64) or npix >= 0x7fffff00:
        return None
    if not al16(skew, "I") or not al16(skew, "O") or (icopy and not al16(skew, "ICOPY")):
        return None
    wg = min(cdiv(cdiv(npix, 32), 4), 512)
    stat = bn and npix % 32 == 0 and wg * 2 * C0 <= WS_BYTES // 8
    return "thin" + ("+copy" if icopy else "") + ("+stat" if stat else ""), wg, (wg if stat else 0)


def thin_df(N, H, W, C1, C0):
    """conv_thin_df: slab rows (workgroups), or 0.  Its loads are single floats: no alignment enters"""
    npix = N * H * W
    if C1 < 1 or C1 > 3 or C0 not in (32, 64) or W < 2 or npix >= 0x7fffff00:
        return 0
    wg = min(cdiv(cdiv(npix, 32), 4), 512)
    while wg > 1 and wg * (9 * C1 + 1) * C0 * 4 > WS_BYTES // 2:
        wg >>= 1
    return wg if wg * (9 * C1 + 1) * C0 * 4 <= WS_BYTES // 2 else 0


IMG_COUT = (4, 6, 8, 10, 12, 16)


def img_block_ok(H, W, C1, C0, blk, skew):
    if C1 not in (1, 3) or C0 > 16 or H % 2 or W % 2 or blk["KS"] != 2 or not blk["pool"]:
        return False
    if blk["pre"] == L_DROPOUT or blk["post"] == L_DROPOUT:
        return False
    if C0 % 2 == 0 and not all(al16(skew, t) for t in ("O", "POOL", "PRE", "PREM", "POST", "POSTM", "COPY")):
        return False
    return C0 in IMG_COUT


def fusable(blk, H0, W0, C1, C0, K):
    return bool(blk["pool"]) and blk["KS"] == 2 and H0 % 2 == 0 and W0 % 2 == 0 and K in (3, 5) and blk["post"] != L_DROPOUT and not conv_big_ok(C1, C0)


def big_token(bwd, cu, K, N, Hx, Wx, Cin, Hy, Wy, Cout, C0f, bn=False):
    """launch_conv_big: (token, batch-norm chunks).  X / Cin: the gathered tensor, Y / Cout: the produced one"""
    S, P = GEO[K][1:]
    npix = N * Hy * Wy
    tiles_m = cdiv(npix, 128)
    wide = Cout > 64 and tiles_m * cdiv(Cout, 128) >= cu                      # wide_tiles(.., 1): big8 and (wide_mul = 1) big alike
    BN = 128 if wide else 64
    big8 = (S == 1 and P == K // 2 and K in (1, 3, 5) and Cin % 64 == 0 and Cout % 4 == 0 and Hx == Hy and Wx == Wy and npix >= 128 and
            npix * Cin < (1 << 29) and max(Cin, Cout) * K * K * C0f < (1 << 29))
    if not big8:
        return "%s<%d>" % ("dx_big" if bwd else "big", BN), 0
    rider = (not bwd) and bn and npix % 128 == 0 and Cout % BN == 0 and tiles_m * 2 * 2 * Cout <= WS_BYTES // 8
    two = tiles_m * cdiv(Cout, BN) >= 2 * cu
    return "%s<%d,%s>%s" % ("dx_big8" if bwd else "big8", BN, "bk32" if two else "bk64", "+bn" if rider else ""), (tiles_m * 2 if rider else 0)


def big_df(cu, K, N, H1, W1, C1, H0, W0, C0):
    """launch_conv_big_df: (token, slices, pixels per slice) or None (workspace too small)"""
    S, P = GEO[K][1:]
    npix, KK = N * H0 * W0, K * K
    part_floats = WS_BYTES // 8
    if S == 1 and K in (1, 3, 5) and H1 == H0 and W1 == W0 and C1 % 128 == 0 and C0 % 64 == 0 and npix * C1 < (1 << 29) and npix * C0 < (1 << 29):
        ntw = 2 if C0 % 128 == 0 else 1
        tilesw = KK * (C1 // 128) * (C0 // (64 * ntw))
        ns = max(1, cu // tilesw)
        pp = max(cdiv(cdiv(npix, ns), 64) * 64, 256)
        ns = cdiv(npix, pp)
        if ns * C1 * KK * C0 <= part_floats:
            return "dfw<128,%d>x%d" % (ntw, ns), ns, pp
    if npix * max(C0, C1) // 4 + 4 * W1 * C1 < (1 << 31):                    # df8_shape
        tp2 = C1 == 32
        kks = (KK + 1) // 2 if tp2 else KK
        tiles8 = kks * cdiv(C1, 64) * cdiv(C0, 64)
        ns = max(1, cu * 2 // tiles8)                                         # 64 KiB of LDS: two workgroups per CU
        pp = max(cdiv(cdiv(npix, ns), 64) * 64, 256)
        ns = cdiv(npix, pp)
        if ns * C1 * KK * C0 > part_floats:
            return None
        return "df8<tp%d>x%d" % (2 if tp2 else 1, ns), ns, pp
    raise AssertionError("k_convbig_df: behind df8_shape (UNREACHABLE)")


def colsum(rows):
    """colsum_add: (token, launches, chunks, rows per chunk)"""
    want = max(1, min(cdiv(rows, 256), 2048))
    if rows <= 1024:
        want = 1
    rpc = cdiv(rows, want)
    n = cdiv(rows, rpc)
    return "colsum<%d>%s" % (n, "+fold" if n > 1 else ""), (1 if n == 1 else 2), n, rpc


def df_mfma_slices(N, H0, C1, K, C0):
    rows, nrow1 = N * H0, C1 * K * K + 1
    tiles = cdiv(nrow1, 32) * cdiv(C0, 32)
    ns = max(1, min(cdiv(512, tiles), cdiv(rows, 4)))
    while ns > 1 and ns * nrow1 * C0 * 4 > WS_BYTES // 8:
        ns >>= 1
    rpw = cdiv(rows, ns * 4)
    return cdiv(rows, rpw * 4), rpw


# ----------------------------------------------------------------------------- the entries
def fwd_tokens(cu, N, H1, W1, C1, C0, K, icopy=False, skew=None, bn=False):
    """conv2d_fwd_impl: (tokens, launches, batch-norm chunks the conv kernel left)"""
    skew = skew or {}
    H0, W0 = out_hw(H1, W1, K)
    same = H0 == H1 and W0 == W1
    if conv_few_ok(K, C1, C0):
        t = [few_token("few", K, C1, C0, al8(skew, "I"))]
        if icopy and not same:
            t.append("memcpy")
        return t, 1, 0
    if same3x3(K, H1, W1, H0, W0):
        th = thin_fwd(N, H0, W0, C1, C0, skew, icopy, bn)
        if th:
            return [th[0]], 1, th[2]
    t = ["memcpy"] if icopy else []
    if conv_big_ok(C1, C0) and al16(skew, "I") and al16(skew, "F"):
        tok, chunks = big_token(False, cu, K, N, H1, W1, C1, H0, W0, C0, C0, bn)
        return t + [tok], 1, chunks
    return t + ["gather<%s,ks%d>" % (gather_filter(C1, K, C0), conv_gemm_ksplit(N * H0 * W0, C0, C1, K))], 1, 0


def bwd_tokens(cu, N, H1, W1, C1, C0, K, dx=True, df=True, skew=None):
    """t4k_conv2d_bwd2 (train = 1): (tokens, launches, info).  info: slices / pixels or rows per slice of the dF engine, for the CPU second order"""
    skew = skew or {}
    H0, W0 = out_hw(H1, W1, K)
    t, n, nfold, info = [], 0, 0, {}
    if df:
        done = False
        if conv_big_ok(C1, C0) and al16(skew, "I") and al16(skew, "DO"):
            b = big_df(cu, K, N, H1, W1, C1, H0, W0, C0)
            if b:
                tok, ns, pp = b
                cs = colsum(N * H0 * W0)
                t += [tok, "fold_add" if ns <= 32 else "df_fold", cs[0]]; n += 2 + cs[1]
                info = dict(slices=ns, pix_per_slice=pp, chunks=cs[2], rows_per_chunk=cs[3]); done = True
        if not done:
            wg = thin_df(N, H0, W0, C1, C0) if same3x3(K, H1, W1, H0, W0) else 0
            if wg:
                t.append("thin_dfx%d+b" % wg); info = dict(slices=wg, tiles32=True)
            else:
                ns, rpw = df_mfma_slices(N, H0, C1, K, C0)
                t.append("df_mfmax%d+b" % ns); info = dict(slices=ns, pix_per_slice=rpw * 4 * W0)
            n += 1; nfold = 1
    dx_big = dx and conv_big_ok(C0, C1) and al16(skew, "DO") and al16(skew, "F")
    need = 15 if C0 % 4 == 0 else 7 if C0 % 2 == 0 else 3
    dx_few = dx and not dx_big and C1 <= 4 and C1 * K * K * C0 <= LDS_FILTER_FLOATS and (skew.get("DO", 0) * 4) & need == 0
    dx_fewch = dx and not dx_big and not dx_few and conv_few_ok(K, C0, C1) is not None
    if nfold and (not dx or dx_big or dx_fewch):
        t.append("df_fold"); n += 1; nfold = 0
    if not dx:
        return t, n, info
    f = "+fold" if nfold else ""
    if dx_big:
        t.append(big_token(True, cu, K, N, H0, W0, C0, H1, W1, C1, C0)[0])
    elif dx_few:
        wide = K == 3 and C0 in (32, 64, 128) and al16(skew, "DO") and al16(skew, "F")
        t.append(("dx_wide<%d>" % (C0 // 4) if wide else "dx_few") + f)
    elif dx_fewch:
        t.append(few_token("fewch", K, C0, C1, al8(skew, "DO")))
    else:
        t.append("dx_and_fold<%s,ks%d>%s" % (gather_filter(C1, K, C0), conv_gemm_ksplit(N * H1 * W1, C1, C0, K), f))
    return t, n + 1, info


BLK_NONE = dict(pre=0, pool=0, post=0, KS=1, copy=False)


def block_tokens(cu, N, H, W, C1, C0, K, blk, icopy=False, skew=None):
    """t4k_conv2d_block_fwd on a shared pixel grid (K 3 or 5): fused blocks only - the unfused one is t4k_conv2d_fwd2 + t4k_poolblock_fwd"""
    skew = skew or {}
    assert fusable(blk, H, W, C1, C0, K), "the table holds fused blocks"
    if K == 3 and img_block_ok(H, W, C1, C0, blk, skew):
        return ["img_block"], 1
    t = ["memcpy"] if icopy and C1 > 4 else []
    return t + ["gather_pool<%s,ks%d>" % (gather_filter(C1, K, C0), conv_gemm_ksplit(N * H * W, C0, C1, K))], 1


def bn_tokens(cu, N, H1, W1, C1, C0, K, icopy=False, skew=None):
    """t4k_conv2d_bn_fwd: the conv with the rider asked for, then k_bn_fin + k_bn_apply (rider) or the statistics pass + k_bn_apply"""
    t, n, chunks = fwd_tokens(cu, N, H1, W1, C1, C0, K, icopy, skew, bn=True)
    H0, W0 = out_hw(H1, W1, K)
    stats = 1 if chunks or N * H0 * W0 < 2048 else 2                           # reduce.hip bn_fwd_stats: one launch below 2048 pixels, chunk partials + fold from there
    return t, n + stats + 1


def dconv_fwd_tokens(cu, N, H1, W1, C1, C0, K):
    """t4k_dconv2d_fwd: the filter transposed, the dX of the virtual conv O -> I, the bias"""
    H0, W0 = dconv_out(H1, W1, K)
    t, n, _ = bwd_tokens(cu, N, H0, W0, C0, C1, K, dx=True, df=False)
    return ["xpose"] + t + ["bias"], n + 2


def dconv_bwd_tokens(cu, N, H1, W1, C1, C0, K, dx=True, df=True):
    H0, W0 = dconv_out(H1, W1, K)
    t, n, info = [], 0, {}
    if df:
        t, n, info = bwd_tokens(cu, N, H0, W0, C0, C1, K, dx=False, df=True)
        cs = colsum(N * H0 * W0)
        t = t + ["xpose", cs[0]]; n += 1 + cs[1]
        info = dict(info, chunks=cs[2], rows_per_chunk=cs[3])
    if dx:
        ft, fn, _ = fwd_tokens(cu, N, H0, W0, C0, C1, K)
        t = t + ["xpose"] + ft; n += 1 + fn
    return t, n, info


def dconv_out(H1, W1, K):
    _, S, P = GEO[K]
    return (H1 - 1) * S - 2 * P + K, (W1 - 1) * S - 2 * P + K


# ----------------------------------------------------------------------------- the table
class Row:
    def __init__(self, id, entry, N, H1, W1, C1, C0, K, label, why, icopy=False, skew=None, blk=None, dx=True):
        self.id, self.entry, self.N, self.H1, self.W1, self.C1, self.C0, self.K = id, entry, N, H1, W1, C1, C0, K
        self.label, self.why, self.icopy, self.skew, self.blk, self.dx = label, why, icopy, dict(skew or {}), blk, dx

    def out_hw(self):
        return dconv_out(self.H1, self.W1, self.K) if self.entry.startswith("dconv") else out_hw(self.H1, self.W1, self.K)

    def plan(self, cu=CU, dx=None, df=True, skew=None):
        """(the hook's string, launches) of the row's call; backward rows: with / without DX and DF"""
        sk = self.skew if skew is None else skew
        dx = self.dx if dx is None else dx
        a = (cu, self.N, self.H1, self.W1, self.C1, self.C0, self.K)
        if self.entry == "fwd":
            t, n, _ = fwd_tokens(*a, icopy=self.icopy, skew=sk)
        elif self.entry == "bn":
            t, n = bn_tokens(*a, icopy=self.icopy, skew=sk)
        elif self.entry == "block":
            t, n = block_tokens(*a, blk=self.blk, icopy=self.icopy, skew=sk)
        elif self.entry == "bwd":
            t, n, _ = bwd_tokens(*a, dx=dx, df=df, skew=sk)
        elif self.entry == "dconv_fwd":
            t, n = dconv_fwd_tokens(*a)
        else:
            t, n, _ = dconv_bwd_tokens(*a, dx=dx, df=df)
        return " ".join(t), n

    def info(self, cu=CU):
        if self.entry == "bwd":
            return bwd_tokens(cu, self.N, self.H1, self.W1, self.C1, self.C0, self.K, dx=self.dx, skew=self.skew)[2]
        if self.entry == "dconv_bwd":
            return dconv_bwd_tokens(cu, self.N, self.H1, self.W1, self.C1, self.C0, self.K, dx=self.dx)[2]
        return {}

    def pixels(self):
        H0, W0 = self.out_hw()
        return self.N * H0 * W0


def blk(pre=0, pool=L_MAXPOOL, post=L_RELU, copy=True, KS=2):
    return dict(pre=pre, pool=pool, post=post, KS=KS, copy=copy)


R = Row
ROWS = [
    # ------------------------------------------------------------------ forward: the rung file's rows, re-derived
    R("few_cin1_ch1_g4", "fwd", 3, 11, 9, 1, 3, 3, "few<4,1,1>", "conv_few_ok: Cin <= 4, Cout <= 32, K 3; Cin == 1 -> CH 1; Cout <= 4 -> G 4; 297 pixels: two workgroups, ragged", icopy=True),
    R("few_cin3_vw1_g12", "fwd", 3, 11, 9, 3, 5, 3, "few<12,4,1>", "odd Cin in 2..4 -> CH 4, VW 1; Cout 5 > 4 -> G 12"),
    R("few_cin2_vw2", "fwd", 3, 11, 9, 2, 4, 3, "few<4,4,2>", "even Cin, I on an 8-byte boundary -> VW 2"),
    R("few_cin4_unaligned_vw1", "fwd", 2, 6, 5, 4, 4, 3, "few<4,4,1>", "even Cin, I 4 bytes past the boundary -> VW 1", skew={"I": 1}),
    R("few_g12_two_groups", "fwd", 2, 6, 5, 2, 13, 3, "few<12,4,2>", "Cout 13 > 12: two channel groups, the second with one valid channel"),
    R("few_k5", "fwd", 2, 6, 5, 1, 3, 5, "few<4,1,1>", "K 5"),
    R("gather_k4s2_icopy_memcpy", "fwd", 2, 6, 6, 1, 3, 4, "memcpy gather<raw,ks1>",
      "K 4 is no few-channel kernel: the layer-0 copy is a memcpy in front of the gather kernel; pairs K K = 16 < 18 -> ksplit 1", icopy=True),
    R("thin_fwd", "fwd", 2, 5, 7, 3, 64, 3, "thin", "conv_thin_fwd: K 3, C1 in 1..4, C0 in {32, 64}; conv_few_ok takes C0 <= 32 first, so C0 = 64; 70 pixels: ragged last tile"),
    R("thin_fwd_icopy", "fwd", 2, 5, 7, 4, 64, 3, "thin+copy", "the layer-0 copy from the same launch", icopy=True),
    R("gather_ksplit1_k1", "fwd", 2, 5, 7, 3, 5, 1, "memcpy gather<raw,ks1>", "K 1 is no few-channel kernel, C1 % 32 != 0 no many-channel one; pairs K K = 2 < 18 -> ksplit 1", icopy=True),
    R("gather_ksplit2", "fwd", 2, 5, 7, 5, 7, 3, "gather<raw,ks2>", "3 pairs x 9 >= 18 and 3 waves < 1536 -> ksplit 2"),
    R("gather_k4s2", "fwd", 2, 6, 8, 3, 5, 4, "gather<raw,ks2>", "(4,2,1) on the gather kernel: 2 x 16 >= 18"),
    R("gather_staged_filter", "fwd", 1, 4, 5, 40, 72, 3, "gather<staged,ks2>", "40 x 9 x 72 = 25920 > 8192 floats: staged per chunk of 14 channel pairs (20 pairs: two chunks), three channel tiles"),
    R("gather_1536_waves", "fwd", 6, 64, 64, 5, 33, 3, "gather<raw,ks1>", "768 pixel tiles x 2 channel tiles = 1536 waves: not < 1536 -> ksplit 1 by size"),
    R("convbig_cin32", "fwd", 2, 8, 8, 32, 16, 3, "big<64>", "conv_big_ok: Cin >= 32, % 32, Cout >= 16, % 4; big8 wants Cin % 64 == 0"),
    R("convbig_k4s2", "fwd", 2, 8, 8, 64, 16, 4, "big<64>", "stride 2 is no big8 shape"),
    R("convbig_under_128_pixels", "fwd", 1, 5, 5, 64, 16, 3, "big<64>", "25 pixels < 128"),
    R("convbig_wide", "fwd", 8, 64, 64, 32, 68, 1, "big<128>", "Cout 68 > 64 and 256 pixel tiles x 1 >= 256 CUs"),
    R("convbig8_n64", "fwd", 2, 8, 8, 64, 16, 3, "big8<64,bk64>", "S 1, P K/2, Cin % 64 == 0, same grid, 128 pixels"),
    R("convbig8_k5", "fwd", 2, 8, 8, 64, 20, 5, "big8<64,bk64>", "K 5"),
    R("convbig8_n128", "fwd", 8, 64, 64, 64, 128, 1, "big8<128,bk64>", "Cout 128 > 64 and 256 tiles >= CUs -> 128-wide; 256 < 2 per CU -> 64-deep"),
    R("convbig8_bk32", "fwd", 16, 64, 64, 64, 64, 1, "big8<64,bk32>", "512 tiles >= 2 per CU -> 32-deep stages"),
    R("convbig8_n128_bk32", "fwd", 8, 64, 64, 64, 256, 1, "big8<128,bk32>", "256 pixel tiles x 2 channel tiles = 512"),
    R("convbig8_ragged", "fwd", 5, 6, 7, 64, 68, 3, "big8<64,bk64>", "210 pixels: ragged second pixel tile; 68 channels: ragged second 64-wide tile"),
    # ------------------------------------------------------------------ forward: what the rung file does not reach
    R("gather_raw_skewed_f", "fwd", 2, 5, 7, 5, 7, 3, "gather<raw,ks2>", "the raw path's scalar copy: F 4 bytes off 16", skew={"F": 1}),
    R("big_refused_by_skewed_i", "fwd", 2, 8, 8, 64, 16, 3, "gather<staged,ks2>", "big_path wants I on 16 bytes: the gather kernel takes the layer, 64 x 9 x 16 = 9216 > 8192 staged", skew={"I": 1}),
    R("thin_fwd_past_cap", "fwd", 1, 257, 256, 4, 64, 3, "thin", "65 792 pixels > 512 workgroups x 4 waves x 32 = 65 536: a wave's second trip, ragged"),
    R("thin_refused_by_skewed_o", "fwd", 2, 5, 7, 3, 64, 3, "gather<raw,ks2>", "conv_thin_fwd wants O on 16 bytes", skew={"O": 1}),
    R("few_past_8192_workgroups", "fwd", 1, 1025, 2048, 1, 3, 3, "few<4,1,1>", "2 099 200 pixels > 8192 workgroups x 256: the grid-stride second trip"),
    R("bn_thin_rider", "bn", 2, 8, 8, 3, 64, 3, "thin+stat", "128 pixels % 32 == 0: the sums ride"),
    R("bn_thin_refused", "bn", 2, 5, 7, 3, 64, 3, "thin", "70 pixels % 32 != 0: the statistics pass runs"),
    R("bn_big8_rider", "bn", 2, 8, 8, 64, 64, 3, "big8<64,bk64>+bn", "128 pixels % 128 == 0, Cout % 64 == 0"),
    R("bn_big8_refused", "bn", 5, 6, 7, 64, 64, 3, "big8<64,bk64>", "210 pixels % 128 != 0"),
    R("bn_thin_rider_icopy", "bn", 2, 8, 8, 3, 64, 3, "thin+copy+stat", "the layer-0 copy and the sums from one launch", icopy=True),
    R("bn_big8_n64_bk32_rider", "bn", 16, 64, 64, 64, 64, 1, "big8<64,bk32>+bn", "the rider on 32-deep stages: 512 tiles, 1024 chunk rows"),
    R("bn_big8_n128_rider", "bn", 8, 64, 64, 64, 128, 1, "big8<128,bk64>+bn", "the rider on 128-wide tiles: Cout % 128 == 0"),
    R("bn_big8_n128_bk32_rider", "bn", 8, 64, 64, 64, 256, 1, "big8<128,bk32>+bn", "the rider on both"),
    R("few_cin1_g12", "fwd", 3, 11, 9, 1, 5, 3, "few<12,1,1>", "Cin == 1 with Cout 5 > 4: CH 1 on G 12"),
    R("gather_staged_ks1", "fwd", 1, 128, 128, 40, 72, 3, "gather<staged,ks1>", "512 pixel tiles x 3 channel tiles = 1536 waves on a staged filter"),
    # ------------------------------------------------------------------ the block entry
    R("gemm_pool_k3", "block", 2, 6, 10, 2, 5, 3, "gather_pool<raw,ks1>", "C1 = 2 is no image layer; 1 pair x 9 < 18", icopy=True, blk=blk()),
    R("gemm_pool_k5", "block", 2, 6, 10, 5, 3, 5, "memcpy gather_pool<raw,ks2>", "K 5 is no image layer; C1 = 5 > 4: the copy is a memcpy; 3 x 25 >= 18", icopy=True, blk=blk()),
    R("img_block_odd_c0_falls", "block", 2, 10, 14, 3, 5, 3, "gather_pool<raw,ks2>", "C0 = 5 is none of 4, 6, 8, 10, 12, 16; 2 pairs x 9 >= 18", icopy=True, blk=blk()),
    R("gather_pool_staged_ks2", "block", 2, 6, 10, 40, 72, 3, "memcpy gather_pool<staged,ks2>", "conv_big_ok(40, 72) fails, so the block is fusable; 25920 floats: staged under the pool epilogue", icopy=True, blk=blk()),
    R("gather_pool_staged_ks1", "block", 1, 128, 128, 40, 72, 3, "gather_pool<staged,ks1>", "1536 waves", blk=blk()),
] + [
    R("img_block_c%d_to_%d" % (c1, c0), "block", 2, 10, 14, c1, c0, 3, "img_block", "C1 in {1, 3}, C0 in {4 .. 16}: 70 pool windows, two workgroups", icopy=True,
      blk=blk(pre=(L_RELU if c0 % 4 == 0 else 0), pool=(L_MAXPOOL, L_MINPOOL, L_AVGPOOL)[(c0 // 2) % 3]))
    for c1 in (1, 3) for c0 in IMG_COUT
] + [
    # ------------------------------------------------------------------ backward: the rung file's rows
    R("dfw__fold_add__dx_convbig8", "bwd", 2, 8, 8, 128, 64, 3, "dfw<128,1>x1 fold_add colsum<1> dx_big8<64,bk64>", "C1 % 128 == 0, C0 % 64 == 0; 128 pixels: one slice; colsum in place"),
    R("dfw_48_slices__df_fold", "bwd", 3, 64, 64, 128, 64, 1, "dfw<128,1>x48 df_fold colsum<48>+fold dx_big8<64,bk64>", "12 288 pixels / 256 = 48 slices > 32: the wave-per-output fold"),
    R("df8_tp2__dx_convbig8", "bwd", 2, 8, 8, 32, 64, 3, "df8<tp2>x1 fold_add colsum<1> dx_big8<64,bk64>", "C1 = 32: two taps per tile"),
    R("df8_48_slices__df_fold__dx_gather", "bwd", 3, 64, 64, 64, 16, 1, "df8<tp1>x48 df_fold colsum<48>+fold dx_and_fold<raw,ks1>", "C0 = 16 < 32 is no many-channel dX; 8 pairs x 1 < 18"),
    R("df8_k4s2", "bwd", 2, 8, 8, 64, 16, 4, "df8<tp1>x1 fold_add colsum<1> dx_and_fold<staged,ks2>", "(4,2,1) on df8; 32 output pixels; 64 x 16 x 16 = 16384 floats staged"),
    R("df_mfma__fold_alone__dx_convbig", "bwd", 2, 8, 8, 16, 32, 3, "df_mfmax4+b df_fold dx_big<64>", "conv_big_ok(16, 32) fails; dX gathers 32 channels: k_convbig, which carries no fold"),
    R("thin_df__dx_wide_c32", "bwd", 2, 5, 7, 1, 32, 3, "thin_dfx1+b dx_wide<8>+fold", "thin_df: C1 in 1..3, C0 in {32, 64}"),
    R("thin_df__dx_wide_c64", "bwd", 2, 5, 7, 3, 64, 3, "thin_dfx1+b dx_wide<16>+fold", "16 lanes per pixel"),
    R("df_mfma__dx_wide_c128", "bwd", 2, 5, 7, 4, 128, 3, "df_mfmax3+b dx_wide<32>+fold", "C0 = 128 is no thin layer; C1 = 4"),
    R("df_mfma_one_slice__dx_and_fold", "bwd", 1, 4, 5, 5, 7, 3, "df_mfmax1+b dx_and_fold<raw,ks2>+fold", "4 rows: one wave row each"),
    R("df_mfma_slices__dx_and_fold", "bwd", 3, 11, 9, 5, 7, 3, "df_mfmax9+b dx_and_fold<raw,ks2>+fold", "33 rows -> 9 slices"),
    R("dx_and_fold_k1", "bwd", 2, 5, 7, 5, 7, 1, "df_mfmax3+b dx_and_fold<raw,ks1>+fold", "K 1"),
    R("dx_and_fold_k4s2", "bwd", 2, 6, 8, 5, 7, 4, "df_mfmax2+b dx_and_fold<raw,ks2>+fold", "(4,2,1)"),
    R("dx_and_fold_k5", "bwd", 2, 5, 7, 5, 7, 5, "df_mfmax3+b dx_and_fold<raw,ks2>+fold", "K 5: 5 x 25 x 7 = 875 floats, raw"),
    R("dx_fewch", "bwd", 3, 11, 9, 7, 3, 3, "df_mfmax9+b df_fold fewch<12,4,1>", "conv_few_ok(K, C0, C1): C0 <= 4, C1 <= 32; carries no fold"),
    R("dx_fewch_k5_g12_two_groups", "bwd", 2, 6, 5, 13, 2, 5, "df_mfmax3+b df_fold fewch<12,4,2>", "K 5, two channel groups, even C0 on 8 bytes"),
] + [
    R("dx_few_c%d_k%d" % (c1, k), "bwd", 3, 11 if k != 4 else 12, 9 if k != 4 else 10, c1, (5, 6, 8, 3)[c1 - 1], k, None,
      "dx_few: C1 <= 4 on every geometry; C0 = 5 / 6 / 8 / 3: the scalar, 8-byte and 16-byte channel loops; 297 input pixels")
    for c1 in (1, 2, 3, 4) for k in (1, 3, 4, 5)
] + [
    # ------------------------------------------------------------------ backward: what the rung file does not reach
    R("df_mfma_w15_second_trip", "bwd", 2, 6, 15, 5, 7, 3, "df_mfmax3+b dx_and_fold<raw,ks2>+fold", "W0 = 15 > 14: 8 pixel pairs, the second trip of the 7-pair loop, odd W0"),
    R("df_mfma_w14_one_trip", "bwd", 2, 6, 14, 5, 7, 3, "df_mfmax3+b dx_and_fold<raw,ks2>+fold", "W0 = 14: exactly one trip, no tail"),
    R("df_mfma_w29_third_trip", "bwd", 2, 6, 29, 5, 7, 3, "df_mfmax3+b dx_and_fold<raw,ks2>+fold", "W0 = 29: 15 pairs, three trips"),
    R("df_mfma_k4s2_w15", "bwd", 2, 6, 30, 5, 7, 4, "df_mfmax2+b dx_and_fold<raw,ks2>+fold", "K 4 / S 2 with W1 = 30: W0 = 15"),
    R("dx_gather_staged_k3", "bwd", 2, 8, 8, 40, 72, 3, "df_mfmax4+b dx_and_fold<staged,ks2>+fold", "dX gathers 72 channels: 36 pairs > 14 per chunk, three chunks of the flipped staged filter"),
    R("dx_gather_staged_k5", "bwd", 2, 8, 8, 40, 72, 5, "df_mfmax4+b dx_and_fold<staged,ks2>+fold", "K 5: 5 pairs per chunk"),
    R("thin_df__dx_wide8_past_caps", "bwd", 1, 257, 256, 3, 32, 3, "thin_dfx512+b dx_wide<8>+fold", "65 792 pixels > 65 536: thin_df's and dx_wide<8>'s (2048 workgroups x 32 pixels) second trip, ragged"),
    R("thin_df__dx_wide16_past_cap", "bwd", 1, 129, 256, 3, 64, 3, "thin_dfx258+b dx_wide<16>+fold", "33 024 pixels > 2048 workgroups x 16 = 32 768"),
    R("df_mfma__dx_wide32_past_cap", "bwd", 1, 129, 128, 3, 128, 3, "df_mfmax33+b dx_wide<32>+fold", "16 512 pixels > 2048 workgroups x 8 = 16 384"),
    R("dx_few_past_8192_workgroups", "bwd", 1, 1025, 2048, 1, 3, 3, "df_mfmax257+b dx_few+fold", "2 099 200 input pixels > 8192 workgroups x 256"),
    R("dx_few_refused_by_skewed_do", "bwd", 3, 11, 9, 3, 8, 3, "df_mfmax9+b dx_and_fold<raw,ks2>+fold", "C0 % 4 == 0: k_conv_dx_few reads dO 16 bytes at a time - DO 4 bytes off goes to the gather kernel", skew={"DO": 1}),
    R("dx_wide_refused_by_skewed_do", "bwd", 2, 5, 7, 3, 64, 3, "thin_dfx1+b dx_and_fold<raw,ks2>+fold", "dx_wide and dx_few both want DO on 16 bytes at C0 = 64", skew={"DO": 1}),
    R("dx_wide_refused_by_skewed_f", "bwd", 2, 5, 7, 3, 64, 3, "thin_dfx1+b dx_few+fold", "dx_wide wants F on 16 bytes; k_conv_dx_few copies F float by float", skew={"F": 1}),
    R("dx_big8_n128_k1", "bwd", 8, 64, 64, 128, 64, 1, "dfw<128,1>x128 df_fold colsum<128>+fold dx_big8<128,bk64>", "dX: Cout = C1 = 128 > 64 and 256 tiles >= CUs: 128-wide, 64-deep"),
    R("dx_big8_bk32_k1", "bwd", 16, 64, 64, 64, 64, 1, "df8<tp1>x256 df_fold colsum<256>+fold dx_big8<64,bk32>", "512 tiles: 32-deep"),
    R("dx_big8_n128_bk32_k1", "bwd", 8, 64, 64, 256, 64, 1, "dfw<128,1>x128 df_fold colsum<128>+fold dx_big8<128,bk32>", "256 x 2 tiles: both"),
    R("dx_big8_n128_k3", "bwd", 8, 64, 64, 128, 64, 3, "dfw<128,1>x27 fold_add colsum<128>+fold dx_big8<128,bk64>", "K 3: the tap walk crosses the stage-buffer parity; 28 slots -> 1216 pixels per slice -> 27 slices"),
    R("dx_big8_bk32_k3", "bwd", 16, 64, 64, 64, 64, 3, "df8<tp1>x54 df_fold colsum<256>+fold dx_big8<64,bk32>", "K 3, 32-deep"),
    R("dx_big_wide", "bwd", 8, 64, 64, 68, 32, 1, "df_mfmax128+b df_fold dx_big<128>", "dX gathers C0 = 32 (no big8), produces C1 = 68 > 64 on 256 pixel tiles"),
    R("dfw_ntw2", "bwd", 2, 8, 8, 128, 128, 3, "dfw<128,2>x1 fold_add colsum<1> dx_big8<64,bk64>", "C0 % 128 == 0: two column blocks"),
    R("dfw_two_row_tiles", "bwd", 2, 8, 8, 256, 64, 1, "dfw<128,1>x1 fold_add colsum<1> dx_big8<64,bk64>", "C1 = 256: two 128-channel row tiles"),
    R("dfw_ragged_slices_k3", "bwd", 2, 64, 64, 128, 64, 3, "dfw<128,1>x26 fold_add colsum<32>+fold dx_big8<64,bk64>", "256 / 9 = 28 slots -> 320 pixels per slice -> 26 slices, the last holds 192"),
    R("df8_ragged_channel_tiles", "bwd", 2, 8, 8, 96, 20, 3, "df8<tp1>x1 fold_add colsum<1> dx_and_fold<staged,ks2>", "C1 = 96: a ragged second 64-channel tile; C0 = 20"),
    R("df8_tp2_even_taps", "bwd", 2, 8, 8, 32, 16, 4, "df8<tp2>x1 fold_add colsum<1> dx_and_fold<raw,ks2>", "16 taps in 8 pairs"),
    R("df8_ragged_slice", "bwd", 5, 6, 7, 64, 68, 3, "df8<tp1>x1 fold_add colsum<1> dx_and_fold<staged,ks2>", "210 pixels in one 256-pixel slice: ragged last stage; C0 = 68: ragged second tile (68 % 32 != 0: no many-channel dX)"),
    R("dfw_refused_by_skewed_i", "bwd", 2, 8, 8, 128, 64, 3, "df_mfmax4+b df_fold dx_big8<64,bk64>", "big_path wants I on 16 bytes: dF falls to k_conv_df_mfma, dX (DO, F aligned) stays", skew={"I": 1}),
    R("fewch_g4_vw1_skewed_do", "bwd", 3, 11, 9, 3, 4, 3, "df_mfmax9+b df_fold fewch<4,4,1>", "C1 <= 4 reaches k_conv_few<BWD> only when dx_few refuses: C0 = 4 with DO 4 bytes off; odd 8-byte phase: VW 1", skew={"DO": 1}),
    R("fewch_g4_vw2_skewed_do", "bwd", 3, 11, 9, 3, 4, 3, "df_mfmax9+b df_fold fewch<4,4,2>", "DO 8 bytes off 16: dx_few refuses (16-byte loads), k_conv_few loads pairs", skew={"DO": 2}),
    R("fewch_cin1_g12", "bwd", 2, 6, 5, 7, 1, 3, "df_mfmax3+b df_fold fewch<12,1,1>", "C0 = 1: CH 1; C1 = 7 > 4"),
    R("dx_gather_staged_ks1", "bwd", 6, 64, 64, 40, 72, 3, "df_mfmax14+b dx_and_fold<staged,ks1>+fold", "768 pixel tiles x 2 channel tiles = 1536 waves on the flipped staged filter"),
    # ------------------------------------------------------------------ the transposed convolution
    R("dconv_fwd", "dconv_fwd", 2, 5, 6, 6, 5, 4, "xpose dx_and_fold<raw,ks2> bias", "the forward is the dX of the virtual conv O -> I"),
    R("dconv_bwd", "dconv_bwd", 2, 5, 6, 6, 5, 4, "df_mfmax3+b df_fold xpose colsum<1> xpose gather<raw,ks2>", "dF of the virtual conv with its fold alone, dB a column sum, dX the conv forward"),
    R("dconv_colsum_12_chunks", "dconv_bwd", 1, 75, 10, 2, 70, 4, "df_mfmax10+b df_fold xpose colsum<12>+fold", "3000 rows > 1024: 12 chunks of 250 and the fold; 70 columns: two groups, the second ragged", dx=False),
    R("dconv_colsum_cap", "dconv_bwd", 1, 513, 256, 1, 4, 4, "df_mfmax129+b df_fold xpose colsum<2045>+fold", "525 312 rows -> want 2052 capped at 2048 -> 257 rows per chunk -> 2045 chunks", dx=False),
]
for _r in ROWS:
    if _r.label is None:
        _r.label = _r.plan()[0]                 # the 16 dx_few rows: df_mfmaxN+b dx_few+fold, N by geometry (asserted as a family in test_conv_cases.py)

BY_ID = {r.id: r for r in ROWS}

UNREACHABLE = {
    "dfxN (k_convbig_df)": "behind df8_shape: npix max(C0, C1) / 4 + 4 W1 C1 >= 2^31 needs a 2 GiB tensor, and ConvLab::df8 = 64 in the release build",
    "big8 / dfw refused by the 2^29 offset limits": "npix Cin >= 2^29 floats is a 2 GiB operand",
    "thin_fwd / thin_df refused by pixels >= 0x7fffff00": "a 2^31-pixel batch",
    "big_df returning 0 (workspace)": "ns C1 K K C0 > 8 Mi floats: ns <= 2 CUs / tiles and tiles >= K K ceil(C1 / 64) ceil(C0 / 64), so ns C1 K K C0 <= 512 x 64 x 64 floats = 2 Mi",
    "df_mfma / thin_df workspace halving": "512 slices x (9 x 3 + 1) x 64 floats = 3.5 MiB < 8 MiB; df_mfma: nslice <= 512 / tiles, so nslice nrow1 C0 <= 512 x 32 x 32 floats",
    "colsum workspace refusal": "2048 chunks x E floats > 32 MiB needs E > 4096 channels",
    "few refused by K K Cin NG G > 8192": "25 x 4 x 36 = 3600 at most",
    "fewch<4,1,1>": "k_conv_few<BWD> with C0 = 1 and C1 <= 4: dx_few takes C1 <= 4 first unless DO is off the boundary of its loads, and at C0 = 1 (odd) it loads float by float",
    "dx_few refused by C1 K K C0 > 8192 with C1 <= 4": "reachable only with C0 > 81 at K 5 and no other engine changes; covered by the staged dX rows, not a rung of its own",
    "df8 32 / 128-pixel stages, 3 - 5 stage buffers, dfw 32-pixel stages, dfw<64|32,..>": "ConvLab::df8, df8_nst, dfw: LAB-only values",
    "big8 with non-temporal stores, big<128> from wide_mul > 1": "ConvLab::big8_nt, wide_mul: LAB only",
}

# every kernel form the mirror can name (the token up to its slice count / suffix); test_conv_cases.py holds the table against it
ALL_FORMS = ("few<4,1,1>", "few<4,4,1>", "few<4,4,2>", "few<12,1,1>", "few<12,4,1>", "few<12,4,2>", "fewch<4,4,1>", "fewch<4,4,2>", "fewch<4,1,1>", "fewch<12,1,1>",
             "fewch<12,4,1>", "fewch<12,4,2>", "thin", "thin+copy", "thin+stat", "thin+copy+stat", "img_block", "memcpy",
             "gather<raw,ks1>", "gather<raw,ks2>", "gather<staged,ks1>", "gather<staged,ks2>", "gather_pool<raw,ks1>", "gather_pool<raw,ks2>",
             "gather_pool<staged,ks1>", "gather_pool<staged,ks2>", "big<64>", "big<128>", "big8<64,bk64>", "big8<64,bk32>", "big8<128,bk64>", "big8<128,bk32>",
             "big8<64,bk64>+bn", "big8<64,bk32>+bn", "big8<128,bk64>+bn", "big8<128,bk32>+bn",
             "dx_big<64>", "dx_big<128>", "dx_big8<64,bk64>", "dx_big8<64,bk32>", "dx_big8<128,bk64>", "dx_big8<128,bk32>",
             "dfw<128,1>", "dfw<128,2>", "df8<tp1>", "df8<tp2>", "thin_df", "df_mfma", "fold_add", "df_fold", "colsum",
             "dx_wide<8>", "dx_wide<16>", "dx_wide<32>", "dx_few", "dx_and_fold<raw,ks1>", "dx_and_fold<raw,ks2>", "dx_and_fold<staged,ks1>", "dx_and_fold<staged,ks2>",
             "xpose", "bias")
def form_of(token):
    """a token without its slice count, fold suffix or bias-row mark"""
    t = token.split("+fold")[0]
    for fam in ("dfw<128,1>", "dfw<128,2>", "df8<tp1>", "df8<tp2>", "thin_df", "df_mfma", "colsum"):
        if t.startswith(fam):
            return fam
    return t


# ids of tests/test_gpu_conv_rungs.py whose comments named an engine the hook does not report: (id, what the comment said, what runs).  None: every
# comment of that file names the engines the mirror gives for its shape (test_conv_cases.py holds the ids against the table)
DRIFTED = ()


# ----------------------------------------------------------------------------- operands and witnesses
def operands(r, exact, N=None):
    """the row's tensors as a dict of fp32 arrays; N: a reduced batch (CPU self-test)"""
    N = r.N if N is None else N
    H0, W0 = r.out_hw()
    rng = np.random.default_rng(seed_of(N, r.H1, r.W1, r.C1, r.C0, r.K, exact, len(r.entry)))
    g = (lambda *s: rng.integers(-2, 3, s).astype(np.float32)) if exact else (lambda *s: rng.standard_normal(s).astype(np.float32))
    o = dict(I=g(N, r.H1, r.W1, r.C1), F=g(r.C1, r.K, r.K, r.C0), B=g(r.C0))
    if r.entry in ("bwd", "dconv_bwd"):
        o.update(DO=g(N, H0, W0, r.C0), DF0=g(r.C1, r.K, r.K, r.C0), DB0=g(r.C0))
    if r.entry == "bn":
        o.update(G=g(r.C0), BB=g(r.C0))
    return o


def exact_ok(r):
    """the precondition of the bit-equal pass: every partial sum an integer below 2^24.  Forward / dX: K K max(C1, C0) products of at most 4 and a
    bias; dF | dB: one product per output pixel and the preloaded gradient; the batch-norm sums are checked by the test on the values themselves"""
    H0, W0 = r.out_hw()
    npix = r.N * max(H0 * W0, r.H1 * r.W1)
    return wt.is_int_exact(r.K * r.K * max(r.C1, r.C0) + 1, 4) and wt.is_int_exact(npix + 1, 4)


def witnesses(r, o):
    """name -> f64_witness.W of every tensor the row's call writes, on the operands as stored"""
    _, S, P = GEO[r.K]
    if r.entry in ("fwd", "block", "bn"):
        return dict(O=wt.conv_fwd(o["I"], o["F"], o["B"], S, P))
    if r.entry == "bwd":
        return dict(DX=wt.conv_dx(o["DO"], o["F"], r.H1, r.W1, S, P), DF=wt.conv_df(o["I"], o["DO"], r.K, S, P, acc=o["DF0"]), DB=wt.conv_db(o["DO"], acc=o["DB0"]))
    H0, W0 = r.out_hw()
    if r.entry == "dconv_fwd":
        return dict(O=wt.dconv_fwd(o["I"], o["F"], o["B"], H0, W0, S, P))
    dx, df, db = wt.dconv_bwd(o["I"], o["DO"], o["F"], o["DF0"], o["DB0"], S, P)
    return dict(DX=dx, DF=df, DB=db)


def hold(name, got, w, exact, kind):
    """one written tensor against its witness: no NaN, then bit-equal (exact pass) or inside the witness's bound as it stands (float pass)"""
    got = np.asarray(got)
    assert not np.isnan(got).any(), "%s: NaN at flat index %d - an element was skipped, or one from outside an operand reached the sum" % (name, int(np.argmax(np.isnan(got).ravel())))
    if exact:
        return wt.equal(name, got, w.exact, kind="conv exact: " + kind)
    return wt.check(name, got, w, kind="conv: " + kind)


def hold_all(name, got, w, o, exact, plan):
    """everything a call wrote (got: name -> array) against its witnesses: O / DX / DF / DB by hold, the layer-0 copy bit-equal to I as uploaded,
    the second dX copy bit-equal to the first"""
    toks = plan.split()
    for k in ("O", "DX", "DF", "DB"):
        if k in got:
            eng = toks[-1] if k == "DX" else (toks[0].split("x")[0] + (" dF" if k == "DF" else " dB")) if k in ("DF", "DB") else plan
            hold(name + " " + k, got[k], w[k], exact, eng)
    if "ICOPY" in got:
        wt.equal(name + " ICOPY", got["ICOPY"], o["I"], kind="conv exact: layer-0 copy")
    if "DX2" in got:
        wt.equal(name + " DX2 == DX", got["DX2"], got["DX"], kind="conv exact: second dX copy")


def hold_bn(name, got, o, exact, plan):
    """the batch-norm half on the conv output the call stored (got["O"]): statistics [1 / (sigma + eps) | mean], x-hat and the output, each against
    the witness of its own op on the tensor in front of it as stored"""
    y = got["O"].reshape(-1, got["O"].shape[-1]); C = y.shape[1]; st = got["ST"]
    assert not np.isnan(st[:2 * C]).any() and not np.isnan(got["XH"]).any() and not np.isnan(got["Y"]).any(), name + ": NaN in a batch-norm tensor"
    wm, wr = wt.bn_stats(y)
    if exact:                                              # the sums are integers below 2^24: the mean is one correctly rounded division
        assert np.abs(y).sum(0).max() < 2 ** 24
        wt.equal(name + " mean", st[C:2 * C], (y.astype(np.float64).sum(0) / y.shape[0]).astype(np.float32), kind="conv exact: bn mean " + plan)
    wt.check(name + " mean", st[C:2 * C], wm, kind="conv: bn mean " + plan)
    wt.check(name + " 1/(sigma+eps)", st[:C], wr, kind="conv: bn rstd " + plan)
    wt.check(name + " x-hat", got["XH"], wt.bn_xhat(y, st), kind="conv: bn x-hat " + plan)
    wt.check(name + " bn out", got["Y"], wt.bn_y(got["XH"], o["G"], o["BB"]), kind="conv: bn out " + plan)


# ----------------------------------------------------------------------------- loop structure the table is sized from
def df_mfma_trips(W0):
    """trips of k_conv_df_mfma's 7-pixel-pair loop over one image row"""
    return cdiv(cdiv(W0, 2), 7)


def grid_trips(engine, pixels, cu=CU, C0=0):
    """grid-stride trips of a capped kernel's busiest workgroup (wave) over `pixels`"""
    per = {"few": 8192 * 256, "dx_few": 8192 * 256, "thin": 512 * 4 * 32, "thin_df": 512 * 4 * 32,
           "dx_wide": 8 * cu * 4 * (64 // max(1, C0 // 4))}[engine]
    return cdiv(pixels, per)
