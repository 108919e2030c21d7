"""CPU half of the conv sweep (tests/test_gpu_conv_sweep.py): the case table against the Python mirror of the conv dispatch at 256 CUs, the
sweep's own assertions (conv_cases.hold_all, hold_bn) run on two honest fp32 implementations - the oracle, and a second summation order (the
pixels in the slices of the row's dF engine, a slice in blocks of 32 summed pairwise, the slices folded in order; forward and dX as fp32 matrix
products) - which must pass both the exact and the float bar on every row, and on injected defects, each of which must fail the row its test
names.  No GPU needed.  Rows too large for the CPU run with N = 1 and a reduced H1 (W1 and the channels, which size the loops, stay)."""
import numpy as np
import pytest

import conv_cases as cc
import f64_witness as wt

CPU_FLOPS = 2e8


# ----------------------------------------------------------------------------- the table and the mirror
def test_every_row_is_on_its_label_at_256_cus():
    ids = [r.id for r in cc.ROWS]
    assert len(set(ids)) == len(ids)
    for r in cc.ROWS:
        lab, n = r.plan(256)
        assert lab == r.label, "%s: the mirror says %s (%d launches)" % (r.id, lab, n)
        assert r.why and cc.exact_ok(r) and n >= len([t for t in lab.split() if t != "memcpy" and not t.startswith("colsum")])
        assert all(v in (1, 2) for v in r.skew.values())
    for c1 in (1, 2, 3, 4):                                # the dx_few family: every C1 on every geometry, the fold riding
        for k in (1, 3, 4, 5):
            lab = cc.BY_ID["dx_few_c%d_k%d" % (c1, k)].label.split()
            assert len(lab) == 2 and lab[0].startswith("df_mfmax") and lab[1] == "dx_few+fold", lab


def forms_of(r):
    out = set()
    for dx, df in (((None, True), (False, True), (True, False)) if r.entry == "bwd" else ((None, True),)):
        out |= {cc.form_of(t) for t in r.plan(dx=dx, df=df)[0].split()}
    return out


def test_every_form_of_the_mirror_has_a_row_or_a_reason():
    forms = set().union(*(forms_of(r) for r in cc.ROWS))
    assert forms <= set(cc.ALL_FORMS), forms - set(cc.ALL_FORMS)
    assert set(cc.ALL_FORMS) - forms == {"fewch<4,1,1>"} and "fewch<4,1,1>" in cc.UNREACHABLE, set(cc.ALL_FORMS) - forms
    assert all(isinstance(v, str) and v for v in cc.UNREACHABLE.values())
    labels = {r.label for r in cc.ROWS}
    for want in ("thin_dfx512+b dx_wide<8>+fold", "dfw<128,2>x1 fold_add colsum<1> dx_big8<64,bk64>", "df_mfmax129+b df_fold xpose colsum<2045>+fold", "img_block"):
        assert want in labels
    assert {(r.C1, r.C0) for r in cc.ROWS if r.label == "img_block"} == {(a, b) for a in (1, 3) for b in cc.IMG_COUT}
    # a random walk over shapes finds no form the table does not name
    rng = np.random.default_rng(5)
    pick = lambda *v: int(rng.choice(v))
    for _ in range(6000):
        K = pick(1, 3, 4, 5)
        N, H, W = pick(1, 2, 3, 8, 16), pick(4, 6, 8, 16, 64, 130), pick(4, 6, 8, 14, 16, 30, 64, 256)
        C1, C0 = pick(1, 2, 3, 4, 5, 7, 16, 32, 40, 64, 68, 96, 128, 256), pick(1, 2, 3, 4, 5, 8, 13, 16, 20, 32, 33, 64, 68, 72, 128, 256)
        sk = {k: pick(0, 0, 0, 1, 2) for k in ("I", "F", "DO", "O", "ICOPY")}
        for entry in ("fwd", "bn", "bwd"):
            r = cc.Row("walk", entry, N, H, W, C1, C0, K, None, "walk", icopy=bool(rng.integers(2)) and entry != "bwd", skew=sk)
            assert forms_of(r) <= set(cc.ALL_FORMS), (entry, N, H, W, C1, C0, K, sk, forms_of(r) - set(cc.ALL_FORMS))
        if K in (3, 5) and H % 2 == 0 and W % 2 == 0 and not cc.conv_big_ok(C1, C0):
            r = cc.Row("walk", "block", N, H, W, C1, C0, K, None, "walk", icopy=True, blk=cc.blk(), skew={"POOL": sk["O"]})
            assert forms_of(r) <= set(cc.ALL_FORMS)
        if K == 4:
            for entry in ("dconv_fwd", "dconv_bwd"):
                assert forms_of(cc.Row("walk", entry, N, H, W, C1, C0, K, None, "walk")) <= set(cc.ALL_FORMS)


def test_the_mirror_at_the_edges_the_table_is_sized_from():
    B = lambda *a, **k: " ".join(cc.bwd_tokens(256, *a, **k)[0])
    F = lambda *a, **k: " ".join(cc.fwd_tokens(256, *a, **k)[0])
    assert cc.df_mfma_trips(14) == 1 and cc.df_mfma_trips(15) == 2 and cc.df_mfma_trips(28) == 2 and cc.df_mfma_trips(29) == 3          # W0 14 | 15
    assert cc.BY_ID["df_mfma_w14_one_trip"].out_hw()[1] == 14 and cc.BY_ID["df_mfma_w15_second_trip"].out_hw()[1] == 15 and cc.BY_ID["df_mfma_k4s2_w15"].out_hw()[1] == 15
    assert cc.grid_trips("thin", 65536) == 1 and cc.grid_trips("thin", 65537) == 2 and cc.grid_trips("thin_df", 65792) == 2             # 65 536 | 65 537 pixels
    assert cc.grid_trips("dx_wide", 65536, C0=32) == 1 and cc.grid_trips("dx_wide", 65792, C0=32) == 2
    assert cc.grid_trips("dx_wide", 32768, C0=64) == 1 and cc.grid_trips("dx_wide", 33024, C0=64) == 2
    assert cc.grid_trips("dx_wide", 16384, C0=128) == 1 and cc.grid_trips("dx_wide", 16512, C0=128) == 2
    assert cc.grid_trips("few", 8192 * 256) == 1 and cc.grid_trips("few", 2099200) == 2 == cc.grid_trips("dx_few", 2099200)
    for rid, eng in (("thin_fwd_past_cap", "thin"), ("thin_df__dx_wide8_past_caps", "thin_df"), ("few_past_8192_workgroups", "few"), ("dx_few_past_8192_workgroups", "dx_few")):
        r = cc.BY_ID[rid]
        assert cc.grid_trips(eng, r.N * r.H1 * r.W1) == 2, rid
    assert F(8, 64, 64, 64, 128, 1) == "big8<128,bk64>" and F(8, 64, 63, 64, 128, 1) == "big8<64,bk64>"                                # 256 | 252 pixel tiles
    assert F(8, 64, 64, 32, 68, 1) == "big<128>" and F(8, 64, 63, 32, 68, 1) == "big<64>"
    assert F(16, 64, 64, 64, 64, 1) == "big8<64,bk32>" and F(16, 64, 63, 64, 64, 1) == "big8<64,bk64>"                                  # 512 | 504 tiles
    assert B(2, 8, 8, 128, 64, 3).startswith("dfw<128,1>x1") and B(2, 8, 8, 96, 64, 3).startswith("df8<tp1>x1")                         # C1 128 | 96
    assert B(2, 64, 64, 128, 64, 1).split()[:2] == ["dfw<128,1>x32", "fold_add"] and B(2, 64, 66, 128, 64, 1).split()[:2] == ["dfw<128,1>x33", "df_fold"]   # nbig 32 | 33
    assert cc.colsum(1024)[:3] == ("colsum<1>", 1, 1) and cc.colsum(1025)[:3] == ("colsum<5>+fold", 2, 5)                              # 1024 | 1025 rows
    assert cc.colsum(525312)[2:] == (2045, 257)
    assert cc.big_df(256, 3, 2, 64, 64, 128, 64, 64, 64)[1:] == (26, 320) and 2 * 64 * 64 - 25 * 320 == 192
    assert cc.gather_chunks(72, 3, 40, 72) == 3 and cc.gather_chunks(72, 5, 40, 72) == 8 and cc.gather_chunks(40, 3, 40, 72) == 2
    assert cc.conv_gemm_ksplit(6 * 64 * 64, 33, 5, 3) == 1 and cc.conv_gemm_ksplit(6 * 64 * 64 - 32, 33, 5, 3) == 2                     # 1536 | 1534 waves
    assert B(3, 11, 9, 3, 8, 3).endswith("dx_few+fold") and B(3, 11, 9, 3, 8, 3, skew={"DO": 2}).endswith("dx_and_fold<raw,ks2>+fold")  # 16-byte loads of dO at C0 % 4 == 0
    assert B(3, 11, 9, 2, 6, 3, skew={"DO": 2}).endswith("dx_few+fold") and B(3, 11, 9, 2, 6, 3, skew={"DO": 1}).endswith("dx_and_fold<raw,ks2>+fold")   # 8-byte loads at even C0
    assert B(3, 11, 9, 1, 5, 3, skew={"DO": 1}).endswith("dx_few+fold")                                                                 # odd C0: float by float
    blk = cc.blk()
    assert cc.img_block_ok(10, 14, 3, 6, blk, {}) and not cc.img_block_ok(10, 14, 3, 6, blk, {"POST": 1}) and cc.img_block_ok(10, 14, 3, 6, blk, {"POST": 4})
    assert not cc.img_block_ok(10, 14, 3, 6, blk, {"COPY": 2}) and not cc.img_block_ok(10, 14, 2, 6, blk, {}) and not cc.img_block_ok(10, 14, 3, 5, blk, {})
    from test_gpu_conv_rungs import BWD, FWD                                                                                            # the rung file's ids are rows of the table, same shapes
    for c in FWD:
        r = cc.BY_ID[c[0]]
        assert (r.N, r.H1, r.W1, r.C1, r.C0, r.K, r.icopy, r.skew.get("I", 0)) == tuple(c[1:]), c[0]
    for c in BWD:
        r = cc.BY_ID[c[0]]
        assert (r.N, r.H1, r.W1, r.C1, r.C0, r.K) == tuple(c[1:]), c[0]


# ----------------------------------------------------------------------------- two honest fp32 implementations
def cpu_row(r):
    """the row at a size the CPU affords: N = 1, then a smaller (even) H1; W1, the channels and K stay"""
    cost = lambda N, H: 2.0 * N * H * r.W1 * r.K * r.K * r.C1 * r.C0 * (3 if "bwd" in r.entry else 1)
    N, H = r.N, r.H1
    if cost(N, H) > CPU_FLOPS:
        N = 1
    while cost(N, H) > CPU_FLOPS and H > 8:
        H = max(8, (H // 2 + 1) // 2 * 2)
    return cc.Row(r.id, r.entry, N, H, r.W1, r.C1, r.C0, r.K, r.label, r.why, icopy=r.icopy, skew=r.skew, blk=r.blk, dx=r.dx)


def pairwise(parts):
    """[n, ...] -> the pairwise (tree) sum over axis 0, in fp32"""
    parts = np.asarray(parts, np.float32)
    while parts.shape[0] > 1:
        if parts.shape[0] % 2:
            parts = np.concatenate([parts, np.zeros_like(parts[:1])])
        parts = parts[0::2] + parts[1::2]
    return parts[0]


def sliced_sum(A, d, pps, defect=None, W0=0):
    """sum over pixels of A[p, :, None] * d[p, None, :] in fp32: slices of pps pixels, a slice in blocks of 32 summed pairwise, the slices folded in order"""
    npix = A.shape[0]
    tot = np.zeros((A.shape[1], d.shape[1]), np.float32)
    starts = list(range(0, npix, pps))
    if defect == "fold_drops_last_slice" and len(starts) > 1:
        starts = starts[:-1]
    for s0 in starts:
        e = min(npix, s0 + pps)
        if defect == "ragged_slice_cut_at_stage" and s0 == starts[-1]:
            e = s0 + (e - s0) // 64 * 64
        a, g = A[s0:e], d[s0:e]
        if defect == "dropped_second_pair_trip":           # pixel pairs 7.. of every image row never enter
            keep = (np.arange(s0, e) % W0) < 14
            a, g = a[keep], g[keep]
        if not len(a):
            continue
        pad = (-len(a)) % 32
        a = np.concatenate([a, np.zeros((pad, a.shape[1]), np.float32)]).reshape(-1, 32, a.shape[1])
        g = np.concatenate([g, np.zeros((pad, g.shape[1]), np.float32)]).reshape(-1, 32, g.shape[1])
        tot = tot + pairwise(np.matmul(a.transpose(0, 2, 1), g))
    return tot


def second_order(r, o, defect=None):
    """the row's call in fp32 numpy, in an order of its own; returns what the call writes"""
    K, S, P = cc.GEO[r.K]
    f32 = lambda a: np.asarray(a, np.float32)
    if r.entry in ("fwd", "bn", "block"):
        A, H0, W0 = wt._cols(o["I"], K, S, P)
        O = (f32(A) @ f32(wt._fmat(o["F"])) + o["B"]).astype(np.float32).reshape(r.N, H0, W0, r.C0)
        if defect == "single_grid_pass":
            O.reshape(-1, r.C0)[8192 * 256:] = np.nan
        got = {"O": O}
        if r.icopy:
            got["ICOPY"] = o["I"].copy()
        if r.entry == "bn":
            y = O.reshape(-1, r.C0)
            ys = y[:len(y) // 32 * 32] if defect == "rider_skips_ragged_tile" else y
            mean = (ys.sum(0, dtype=np.float32) / np.float32(len(y))).astype(np.float32)
            var = ((ys * ys).sum(0, dtype=np.float32) / np.float32(len(y)) - mean * mean).astype(np.float32)
            rstd = (np.float32(1.0) / (np.sqrt(np.maximum(var, 0)) + np.float32(wt.EPS))).astype(np.float32)
            xh = ((y - mean) * rstd).astype(np.float32)
            got.update(ST=np.concatenate([rstd, mean, np.zeros(r.C0, np.float32)]), XH=xh, Y=(xh * o["G"] + o["BB"]).astype(np.float32))
        return got
    if r.entry == "dconv_fwd":
        H0, W0 = r.out_hw()
        Fv = np.ascontiguousarray(o["F"].transpose(3, 1, 2, 0)[:, ::-1, ::-1, :])
        return {"O": (dx32(o["I"], Fv, H0, W0, K, S, P) + o["B"]).astype(np.float32)}
    info = r.info()
    H0, W0 = r.out_hw()
    got = {}
    if r.entry == "bwd":
        if r.dx:
            got["DX"] = dx32(o["DO"], o["F"], r.H1, r.W1, K, S, P, flip=defect != "unflipped")
            got["DX2"] = np.zeros_like(got["DX"]) if defect == "dx2_stale" else got["DX"].copy()
        A, _, _ = wt._cols(o["I"], K, S, P)
        d = f32(o["DO"]).reshape(-1, r.C0)
        pps = 128 if info.get("tiles32") else info["pix_per_slice"]
        df = sliced_sum(f32(A), d, pps, defect, W0).reshape(K, K, r.C1, r.C0).transpose(2, 0, 1, 3)
        got["DF"] = (o["DF0"] + df).astype(np.float32)
        db = sliced_sum(np.ones((len(d), 1), np.float32), d, info.get("rows_per_chunk", pps), defect, W0)[0]
        got["DB"] = o["DB0"].copy() if defect == "no_bias_row" else (o["DB0"] + db).astype(np.float32)
        return got
    # dconv_bwd: the virtual conv's roles swapped
    Fv = np.ascontiguousarray(o["F"].transpose(3, 1, 2, 0))
    if r.dx:
        A, h, w_ = wt._cols(o["DO"], K, S, P)
        got["DX"] = (f32(A) @ f32(wt._fmat(Fv))).astype(np.float32).reshape(r.N, h, w_, r.C1)
    A, _, _ = wt._cols(o["DO"], K, S, P)
    d = f32(o["I"]).reshape(-1, r.C1)
    dfv = sliced_sum(f32(A), d, info["pix_per_slice"], defect).reshape(K, K, r.C0, r.C1).transpose(2, 0, 1, 3)
    got["DF"] = (o["DF0"] + dfv.transpose(3, 1, 2, 0)).astype(np.float32)
    g = f32(o["DO"]).reshape(-1, r.C0)
    got["DB"] = (o["DB0"] + sliced_sum(np.ones((len(g), 1), np.float32), g, info["rows_per_chunk"], defect)[0]).astype(np.float32)
    return got


def dx32(dO, F, H1, W1, K, S, P, flip=True):
    """f64_witness.conv_dx's scatter in fp32"""
    dO = np.asarray(dO, np.float32); N, H0, W0, _ = dO.shape; C1 = F.shape[0]
    Ff = np.asarray(F, np.float32)[:, ::-1, ::-1, :] if flip else np.asarray(F, np.float32)
    ex = np.zeros((N, H1 + 2 * P + K, W1 + 2 * P + K, C1), np.float32)
    for ky in range(K):
        for kx in range(K):
            ex[:, ky:ky + S * H0:S, kx:kx + S * W0:S] += dO @ Ff[:, ky, kx, :].T
    return np.ascontiguousarray(ex[:, P:P + H1, P:P + W1])


def oracle_run(oracle, r, o):
    lib, P = oracle.lib(), oracle.P
    K, S, Pd = cc.GEO[r.K]
    H0, W0 = r.out_hw()
    geo = (r.N, r.H1, r.W1, r.C1, H0, W0, r.C0, K, S, Pd)
    c = lambda a: np.ascontiguousarray(a, np.float32)
    I, F, B = c(o["I"]), c(o["F"]), c(o["B"])
    if r.entry in ("fwd", "block", "dconv_fwd"):
        O = np.zeros((r.N, H0, W0, r.C0), np.float32)
        assert (lib.t4o_conv2d_fwd if r.entry != "dconv_fwd" else lib.t4o_dconv2d_fwd)(P(I), P(O), P(F), P(B), *geo) == 0
        return dict({"O": O}, **({"ICOPY": I.copy()} if r.icopy else {}))
    DO, DF, DB = c(o["DO"]), c(o["DF0"]).copy(), c(o["DB0"]).copy()
    DX = np.zeros_like(I)
    assert (lib.t4o_conv2d_bwd if r.entry == "bwd" else lib.t4o_dconv2d_bwd)(P(I), P(DO), P(DX) if r.dx else None, P(F), P(DF), P(DB), *geo, 1) == 0
    got = {"DF": DF, "DB": DB}
    if r.dx:
        got["DX"] = DX
        if r.entry == "bwd":
            got["DX2"] = DX.copy()
    return got


def held(r, got, o, exact):
    w = cc.witnesses(r, o)
    cc.hold_all(r.id, got, w, o, exact, r.label)
    if r.entry == "bn":
        cc.hold_bn(r.id, got, o, exact, r.label)


@pytest.mark.parametrize("row", cc.ROWS, ids=[r.id for r in cc.ROWS])
def test_both_implementations_pass_the_sweeps_bars(oracle, row):
    r = cpu_row(row)
    assert r.W1 == row.W1 and (r.C1, r.C0, r.K) == (row.C1, row.C0, row.K)
    for exact in (True, False):
        o = cc.operands(r, exact)
        held(r, second_order(r, o), o, exact)
        if r.entry != "bn":
            held(r, oracle_run(oracle, r, o), o, exact)


# ----------------------------------------------------------------------------- injected defects: each must fail the row its test names
DEFECTS = [
    ("unflipped", "df_mfma_slices__dx_and_fold", "few_cin1_ch1_g4"),
    ("fold_drops_last_slice", "dfw_ragged_slices_k3", "dfw__fold_add__dx_convbig8"),
    ("no_bias_row", "thin_df__dx_wide_c32", None),
    ("single_grid_pass", "few_past_8192_workgroups", "few_cin1_ch1_g4"),
    ("dropped_second_pair_trip", "df_mfma_w15_second_trip", "df_mfma_w14_one_trip"),
    ("ragged_slice_cut_at_stage", "df8_ragged_slice", "df8_tp2__dx_convbig8"),
    ("dx2_stale", "dx_and_fold_k1", None),
    ("rider_skips_ragged_tile", "bn_thin_refused", "bn_thin_rider"),
]


@pytest.mark.parametrize("defect,fails,passes", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_an_injected_defect_fails_the_row_that_pins_it(defect, fails, passes):
    """`fails`: the row sized for the defect, at its full shape; `passes`: a neighbour the defect cannot touch (one slice, one trip, no ragged tile),
    which shows that the row's size is what catches it"""
    r = cc.BY_ID[fails]
    for exact in (True, False):
        o = cc.operands(r, exact)
        held(r, second_order(r, o), o, exact)
        with pytest.raises(AssertionError):
            held(r, second_order(r, o, defect), o, exact)
    if passes:
        q = cc.BY_ID[passes]
        o = cc.operands(q, True)
        held(q, second_order(q, o, defect), o, True)
