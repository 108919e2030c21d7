"""CPU half of the feed / label sweep (tests/feed_label_cases.py): the mirrors against csrc/t4k_common.h, the numpy witnesses against the oracle on EVERY case
of the tables (the oracle restates the reference's Model::hit, Model::onehot and Dataset::_load, so the witnesses hang on the reference, the specials
included), and the tables against nine injected defects: each must fail the cases named for it and nothing but plausible neighbours."""
import ctypes
import os
import re

import numpy as np
import pytest

import feed_label_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFILL = 0xA5A5A5A5


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


# ---------------------------------------------------------------- mirrors and tables
def test_mirror_matches_the_header():
    text = open(os.path.join(ROOT, "tensorforth_amd", "csrc", "t4k_common.h")).read()
    got = {k: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % k, text).group(1)) for k in ("BLK", "MAX_WG")}
    assert got == {"BLK": fc.BLK, "MAX_WG": fc.MAX_WG} and fc.CAP == fc.BLK * fc.MAX_WG == 524288
    assert re.search(r"if \(g > MAX_WG\) g = MAX_WG;", text)                   # grid_for caps, so a kernel must stride
    launch = open(os.path.join(ROOT, "tensorforth_amd", "csrc", "reduce.hip")).read()
    assert re.search(r"if \(E <= 32\)\s+T4K_LAUNCH\(k_hit<1>", launch) and re.search(r"else if \(E <= 256\)\s+T4K_LAUNCH\(k_hit<8>", launch)
    assert re.search(r"else\s+T4K_LAUNCH\(k_hit<64>", launch)
    stage = open(os.path.join(ROOT, "tensorforth_amd", "csrc", "elementwise.hip")).read()
    assert "const int vec = ((uintptr_t)src & 3) == 0 && aligned16(dst);" in stage


def test_mirror_functions():
    assert [fc.hit_lanes(E) for E in (1, 32, 33, 256, 257, 1000)] == [1, 1, 8, 8, 64, 64]
    assert [fc.hit_trip(E) for E in (10, 40, 257)] == [256, 32, 4]
    assert fc.stage_vec(0, 0) and fc.stage_vec(4, 16) and not fc.stage_vec(1, 0) and not fc.stage_vec(0, 4) and not fc.stage_vec(0, 8)
    assert fc.grid_for(fc.CAP) == fc.MAX_WG == fc.grid_for(fc.CAP + 1) and fc.grid_for(fc.CAP - 256) == fc.MAX_WG - 1 and fc.grid_for(0) == 1


def test_tables_hold_what_the_launch_code_asks_for():
    for table in (fc.HIT_CASES, fc.ONEHOT_HIT_CASES, fc.ONEHOT_CASES, fc.NORM_CASES, fc.STAGE_CASES):
        names = [c.name for c in table]
        assert len(set(names)) == len(names)
    assert {c.E for c in fc.HIT_CASES if c.kind == "lanes"} == {1, 2, 31, 32, 33, 40, 255, 256, 257, 300, 1000}
    for E in (10, 40, 257):                                                    # both sides of one trip and of two, and no row at all
        t = fc.hit_trip(E)
        assert {c.N for c in fc.HIT_CASES if c.kind == "trip" and c.E == E} == {0, t - 1, t, t + 1, 2 * t + 1}
    ties = fc.by_name(fc.HIT_CASES, "ties-E40")
    assert ties.N == 780 and (9, 16) in ties.pairs and 16 % 8 < 9 % 8          # j's lane below i's
    assert fc.by_name(fc.HIT_CASES, "ties-E300").N == 21
    assert {c.special for c in fc.HIT_CASES if c.kind == "special" and c.E == 300} == set(fc.special_rows(300)) and len(fc.special_rows(10)) == 9
    assert {fc.hit_lanes(E) for E in fc.SPECIAL_E} == {1, 8, 64}
    sizes = {c.N * c.E for c in fc.ONEHOT_CASES}
    assert {fc.CAP, fc.CAP + 12, 2 * fc.CAP + 7, 2 * fc.CAP + 24, 1} <= sizes
    assert {c.n for c in fc.NORM_CASES} >= set(fc.SIZES) and {c.n for c in fc.STAGE_CASES} >= set(fc.SIZES)
    assert {(c.src_off, c.dst_off) for c in fc.OFFSET_GROUP} == {(s, d) for s in (0, 1, 2, 3) for d in (0, 4, 8)}
    assert {c.vec for c in fc.OFFSET_GROUP} == {True, False} and sum(c.vec for c in fc.OFFSET_GROUP) == 1
    assert {(c.n, c.nlab) for c in fc.STAGE_CASES} >= {(3, 0), (3, 1), (3, 700), (0, fc.CAP), (0, fc.CAP + 1), (1003, fc.CAP), (1003, fc.CAP + 1), (1003, 2 * fc.CAP + 5)}
    for c in fc.ONEHOT_HIT_CASES:
        lab, _ = c.build()
        assert {c.E - 1, c.E, c.E + 1, fc.ALL_ONES} <= set(int(x) for x in lab)
    lab = fc.by_name(fc.STAGE_CASES, "stage-n1003-nlab%d" % (2 * fc.CAP + 5)).build()[1]
    assert lab[0] == fc.ALL_ONES and lab.size == 2 * fc.CAP + 5
    for c in fc.HIT_CASES:
        a, b = c.build(), c.build()
        assert same(a[0], b[0]) and same(a[1], b[1]) and a[0].shape == (c.N, c.E)


# ---------------------------------------------------------------- witness == oracle
def o_hit(oracle, out, hot):
    out, hot = np.ascontiguousarray(out, np.float32), np.ascontiguousarray(hot, np.float32)
    c = ctypes.c_int(0x5a5a5a5a)
    oracle.lib().t4o_hit(oracle.P(out), oracle.P(hot), out.shape[0], out.shape[1], ctypes.byref(c))
    return c.value


def o_onehot(oracle, lab, N, E):
    hot = np.full((N, E), np.nan, np.float32)
    oracle.lib().t4o_onehot(oracle.P(np.ascontiguousarray(lab, np.uint32)), oracle.P(hot), N, E)
    return hot


def o_norm(oracle, u8, mean, scale):
    u8 = np.ascontiguousarray(u8, np.uint8); dst = np.full(u8.size, np.nan, np.float32)
    oracle.lib().t4o_u8_normalize(oracle.P(u8), oracle.P(dst), u8.size, mean, scale)
    return dst


@pytest.mark.parametrize("case", fc.HIT_CASES, ids=repr)
def test_hit_witness_is_the_oracle(oracle, case):
    out, hot = case.build()
    assert fc.hit(out, hot) == o_hit(oracle, out, hot)
    if case.kind == "special":
        assert fc.hit(out, hot) == 3
    if case.kind == "ties":
        assert fc.hit(out, hot) == case.N and np.array_equal(fc.argmax(out), [i for i, _ in case.pairs])
    if case.kind == "maxpos":
        assert np.array_equal(fc.argmax(out), np.arange(case.E)) and 0 < fc.hit(out, hot) < case.N
    if case.kind == "hotvals":
        assert fc.hit(out, hot) == 2 * (2 + 0 + 0 - 1 + 3)


@pytest.mark.parametrize("E", fc.SPECIAL_E)
def test_special_rows_pick_the_reference_class(oracle, E):
    for name, (row, want) in fc.special_rows(E).items():
        assert fc.argmax(row[None])[0] == want, name
        probe = np.zeros((1, E), np.float32); probe[0, want] = 1.0            # the oracle counts exactly this class
        assert o_hit(oracle, row[None], probe) == 1, name


@pytest.mark.parametrize("case", fc.ONEHOT_HIT_CASES, ids=repr)
def test_onehot_hit_witness_is_the_oracle(oracle, case):
    lab, out = case.build()
    hot = fc.onehot(lab, case.N, case.E)
    assert same(hot, o_onehot(oracle, lab, case.N, case.E))
    assert fc.hit(out, hot) == o_hit(oracle, out, hot) and 0 < fc.hit(out, hot)


@pytest.mark.parametrize("case", fc.ONEHOT_CASES, ids=repr)
def test_onehot_witness_is_the_oracle(oracle, case):
    lab = case.build()
    hot = fc.onehot(lab, case.N, case.E)
    assert same(hot, o_onehot(oracle, lab, case.N, case.E)) and hot.sum() == case.N


@pytest.mark.parametrize("case", fc.NORM_CASES + fc.STAGE_CASES, ids=repr)
def test_normalize_witness_is_the_oracle(oracle, case):
    u8 = case.build() if case.kind == "norm" else case.build()[0]
    assert u8.size == (256 if "bytes" in case.name else case.n)
    assert same(fc.normalize(u8, case.mean, case.scale), o_norm(oracle, u8, case.mean, case.scale))
    if case.kind == "stage":
        lab = case.build()[1]
        assert same(fc.stage(u8, case.mean, case.scale, lab)[1], lab) and lab.size == case.nlab


# ---------------------------------------------------------------- injected defects
def hit_failures(defect):
    bad = set()
    for c in fc.HIT_CASES:
        out, hot = c.build()
        if defect(out, hot) != fc.hit(out, hot):
            bad.add(c.name)
    return bad


def names(table, pred):
    return {c.name for c in table if pred(c)}


def has_tied_maximum(c):
    out, _ = c.build()
    with np.errstate(invalid="ignore"):
        return any(np.sum(r == np.max(r[~np.isnan(r)])) > 1 for r in out if not np.all(np.isnan(r)))


def test_defect_scan_started_at_flt_max():
    """the kernel in front of the sweep: exactly the two special rows, at every lane count"""
    assert hit_failures(fc.defect_hit_from_flt_max) == {"special-E%d-%s" % (E, s) for E in fc.SPECIAL_E for s in ("lead-nan", "ninf-then-fltmax")}


def test_defect_higher_index_wins_a_tie():
    bad = hit_failures(fc.defect_hit_higher_tie)
    assert bad >= {"ties-E40", "ties-E300"} | {"special-E%d-%s" % (E, s) for E in fc.SPECIAL_E for s in ("pinf-twice", "zero-signs")}
    assert bad <= names(fc.HIT_CASES, has_tied_maximum)
    assert not bad & names(fc.HIT_CASES, lambda c: c.kind in ("maxpos", "hotvals"))


def test_defect_only_the_first_trip_counts():
    bad = hit_failures(fc.defect_hit_first_trip)
    assert bad >= names(fc.HIT_CASES, lambda c: c.kind == "trip" and c.N > fc.hit_trip(c.E)) | {"ties-E40", "ties-E300", "maxpos-E40", "maxpos-E257"}
    assert bad <= names(fc.HIT_CASES, lambda c: c.N > fc.hit_trip(c.E))


def test_defect_tail_lanes_see_nothing():
    bad = hit_failures(fc.defect_hit_tail_lanes)
    assert bad >= {"maxpos-E257", "ties-E300"} | {"lanes-E%d" % E for E in (33, 255, 257, 300, 1000)}
    assert bad <= names(fc.HIT_CASES, lambda c: c.E % fc.hit_lanes(c.E) != 0)


def test_defect_rounding_for_truncation():
    assert hit_failures(fc.defect_hit_rounds) == {"hotvals-E%d" % E for E in fc.SPECIAL_E}


def test_defect_onehot_without_the_clamp():
    outside = lambda c: bool(np.any((c.build() if c.kind == "onehot" else c.build()[0]) >= c.E))
    bad = names(fc.ONEHOT_CASES, lambda c: not same(fc.defect_onehot_no_clamp(c.build(), c.N, c.E), fc.onehot(c.build(), c.N, c.E)))
    assert bad == names(fc.ONEHOT_CASES, outside) and bad >= {"onehot-5243x100", "onehot-4096x128", "onehot-10486x100", "onehot-1048583x1", "onehot-37x1"}
    assert not bad & {"onehot-1x1-inrange", "onehot-37x10-inrange"}
    bad = names(fc.ONEHOT_HIT_CASES, lambda c: not same(fc.defect_onehot_no_clamp(c.build()[0], c.N, c.E), fc.onehot(c.build()[0], c.N, c.E)))
    assert bad == {c.name for c in fc.ONEHOT_HIT_CASES}


def test_defect_normalize_distributed():
    def fails(c):
        u8 = c.build() if c.kind == "norm" else c.build()[0]
        return not same(fc.defect_normalize_distributed(u8, c.mean, c.scale), fc.normalize(u8, c.mean, c.scale))
    bad = names(fc.NORM_CASES + fc.STAGE_CASES, fails)
    assert bad >= {"norm-bytes-2", "norm-bytes-3", "stage-bytes-2-vec", "stage-bytes-3-scalar"} | {"norm-n1003-s%dd%d" % (s, d) for s in (0, 1, 2, 3) for d in (0, 4, 8)}
    assert not bad & ({"norm-bytes-0", "norm-bytes-1", "stage-bytes-0-vec", "stage-bytes-1-vec"} | names(fc.NORM_CASES + fc.STAGE_CASES, lambda c: c.n == 0 or c.mean == 128.0))


def stage_failures(defect):
    bad = set()
    for c in fc.STAGE_CASES:
        u8, lab = c.build()
        got, want = defect(u8, c.mean, c.scale, lab, PREFILL, c.vec), fc.stage(u8, c.mean, c.scale, lab)
        if not (same(got[0], want[0]) and same(got[1], want[1])):
            bad.add(c.name)
    return bad


def test_defect_stage_drops_the_labels_past_the_cap():
    assert stage_failures(fc.defect_stage_labels_stop_at_cap) == names(fc.STAGE_CASES, lambda c: c.nlab > fc.CAP) == {
        "stage-n0-nlab%d" % (fc.CAP + 1), "stage-n1003-nlab%d" % (fc.CAP + 1), "stage-n1003-nlab%d" % (2 * fc.CAP + 5)}


def test_defect_stage_swaps_two_bytes_of_a_word():
    bad = stage_failures(fc.defect_stage_swapped_bytes)
    assert bad == names(fc.STAGE_CASES, lambda c: c.vec and c.n >= 4)
    assert "stage-n1003-s0d0" in bad and "stage-n1003-s1d0" not in bad and "stage-n%d-s0d0" % (4 * fc.CAP + 5) in bad and "stage-n3-s0d0" not in bad
