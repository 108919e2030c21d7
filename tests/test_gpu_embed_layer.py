"""t4k_embed_fwd / _bwd (include/t4k.h, csrc/embed.hip) through the C ABI: the token-embedding lookup, the learned position table, or both.

The forward is held bit for bit against the NumPy float32 restatement of the rule (tests/embed_witness.py: at most one add per element), the backward
against the float64 witness with its derived bound (h roundings for a table row of h hits, N for a position) AND bit for bit against the float32 restatement
of the kernels' order; with small-integer dY every sum is exact and DTABLE / DPOS must be the integer sums.  Outputs are pre-filled with NaN between guard
floats (Dev of tests/test_gpu_bcast.py): an element that was not written shows, and so does a store outside the tensor.  The rung, the load path, P and the
launch counts come from t4k_embed_plan, the function the entries call.  No input here is meant to fault: ids outside [0, V) are padding by the rule."""
import ctypes
import zlib

import numpy as np
import pytest

import embed_witness as ew
from test_gpu_bcast import Dev
from test_gpu_pool_geo import guards_intact, lcount

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
WS = 32 << 20
R = ew.R_SLAB
F = np.float32


def plan(h, T, L, V, E, pos, aligned=1):
    out = I8()
    assert h.lib.t4k_embed_plan(T, L, V, E, pos, aligned, WS, out) == OK, h.lib.t4k_last_error()
    return list(out)


def nan(k):
    return np.full(k, np.nan, F)


def bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).ravel().view(np.uint32), np.ascontiguousarray(b, F).ravel().view(np.uint32))


def run_case(h, name, N, L, V, E, pos, off=None, train=1, ids="mixed", dy="normal", rung=None, P=None, inplace=False, ids_fn=None):
    """forward, then backward; every stored tensor against its witness; launches against the plan; operands intact; guards.  off: floats a pointer starts
    off 16 bytes, by name.  Returns (O, DTABLE, DPOS, DX)"""
    off = off or {}
    o = lambda k: off.get(k, 0)
    T = N * L
    rng = np.random.default_rng(zlib.crc32(repr((name, N, L, V, E, pos)).encode()))
    tok = V >= 1
    IDS = ew.make_ids(rng, T, V, ids) if tok else None
    if ids_fn is not None:
        IDS = ids_fn(IDS)
    X = None if tok else rng.normal(0.0, 1.0, (T, E)).astype(F)
    TAB = rng.normal(0.0, 1.0, (V, E)).astype(F) if tok else None
    POS = rng.normal(0.0, 0.02, (L, E)).astype(F) if pos else None
    if dy == "int":
        DY = rng.integers(-8, 9, (T, E)).astype(F); DT0 = rng.integers(-100, 101, (max(V, 1), E)).astype(F); DP0 = rng.integers(-100, 101, (L, E)).astype(F)
    else:
        DY = rng.normal(0.0, 1.0, (T, E)).astype(F); DT0 = rng.normal(0.0, 1.0, (max(V, 1), E)).astype(F); DP0 = rng.normal(0.0, 1.0, (L, E)).astype(F)
    used_f = ["IDS" if tok else "X", "O"] + (["TABLE"] if tok else []) + (["POS"] if pos else [])
    used_b = ["DY"] + (["IDS", "DTABLE"] if tok and train else ["IDS"] if tok else ["DX"]) + (["DPOS"] if pos and train else [])
    al_f, al_b = all(o(k) % 4 == 0 for k in used_f), all(o(k) % 4 == 0 for k in used_b)
    pf, pb = plan(h, T, L, V, E, pos, int(al_f)), plan(h, T, L, V, E, pos, int(al_b))
    tag = "%s n%d l%d v%d e%d p%d %s" % (name, N, L, V, E, pos, sorted(off.items()))
    if rung is not None:
        assert pf[0] == rung, (tag, pf)
    assert pf[0] == (0 if not tok else 1 if pf[3] == 1 else 2) and (pf[3] == 1 or T >= 128), (tag, pf)      # the rung is the plan's: parts need two id loads
    if P is not None:
        assert pf[3] == P, (tag, pf)
    assert pf[1] == (4 if E % 4 == 0 and al_f else 1) and pb[1] == (4 if E % 4 == 0 and al_b else 1), (tag, pf, pb)
    p = lambda d: d.p if d is not None else None
    dev = lambda a, k: Dev(a, o(k)) if a is not None else None
    dI, dX, dT, dP, dO = dev(IDS, "IDS"), dev(X, "X"), dev(TAB, "TABLE"), dev(POS, "POS"), Dev(nan(T * E), o("O"))
    l0 = lcount(h)
    h.call("t4k_embed_fwd", p(dI), p(dX), p(dT), p(dP), dO.p, T, L, V, E, None)
    assert lcount(h) - l0 == pf[4] == 1, (tag, pf)
    O = dO.get(h, (T, E)).copy()
    want = ew.fwd32(IDS if tok else X, TAB, POS, T, L, V, E)
    assert bits(O, want), tag + ": forward"
    assert np.max(np.abs(O.astype(np.float64) - ew.fwd64(IDS if tok else X, TAB, POS, T, L, V, E))) <= 2.0 ** -24 * max(1e-30, np.max(np.abs(want))), tag
    for d, a in ((dI, IDS), (dX, X), (dT, TAB), (dP, POS)):
        if d is not None:
            assert bits(d.get(h, a.shape), a), tag + ": an operand changed"
    # backward
    dDY = Dev(DY, o("DY"))
    dDT, dDP = (Dev(DT0[:V], o("DTABLE")) if tok else None), (Dev(DP0, o("DPOS")) if pos else None)
    dDX = None if tok else (dDY if inplace else Dev(nan(T * E), o("DX")))
    null = train == "null"
    l0 = lcount(h)
    h.call("t4k_embed_bwd", p(dI), dDY.p, None if null else p(dDT), None if null else p(dDP), p(dDX), T, L, V, E, 1 if train == 1 else 0, None)
    nl = lcount(h) - l0
    if train == 1:
        assert nl == pb[5] == (pb[0] if tok else 1), (tag, nl, pb)
    else:
        assert nl == (0 if tok or inplace else 1), (tag, nl)
    DT = dDT.get(h, (V, E)).copy() if tok else None
    DP = dDP.get(h, (L, E)).copy() if pos else None
    DX = dDX.get(h, (T, E)).copy() if dDX is not None else None
    t1 = 1 if train == 1 else 0
    rDT, rDP = ew.bwd32(IDS, DY, DT0[:V] if tok else None, DP0 if pos else None, T, L, V, E, pb[3])
    if tok:
        ew.check(tag + " dtable", DT, ew.em_dtable(IDS, DY, DT0[:V], V, E, t1))
        assert bits(DT, rDT if t1 else DT0[:V]), tag + ": dtable is not the restated order's"
    if pos:
        ew.check(tag + " dpos", DP, ew.em_dpos(DY, DP0, T, L, E, t1))
        assert bits(DP, rDP if t1 else DP0), tag + ": dpos is not the restated order's"
    if DX is not None:
        assert bits(DX, DY), tag + ": dx"
    if not inplace:
        assert bits(dDY.get(h, (T, E)), DY), tag
    if tok:
        assert bits(dI.get(h, (T,)), IDS), tag + ": the ids changed"
    guards_intact(*[d for d in (dI, dX, dT, dP, dO, dDY, dDT, dDP, dDX) if d is not None])
    return O, DT, DP, DX


VS = [1, R - 1, R, R + 1, 2 * R + 3]
LN = [(L, N) for L in (1, 5, 64, 65) for N in (1, 2, 3)]


def es(i):
    return [1, 3, 4, 20, 64, 260, 68][i % 7]                               # 260 = one 16-byte chunk + 4, 68 = one dword chunk + 4


@pytest.mark.parametrize("V", VS)
def test_token_mode_over_the_shapes(t4k, V):
    """V on both sides of a slab, E on both sides of the load paths and a chunk, L and N over the issue's list: every (L, N) pair once per V, E cycling"""
    for i, (L, N) in enumerate(LN):
        E = es(i + V)
        run_case(t4k, "grid", N, L, V, E, i % 2, rung=1 if N * L < 128 else None)


@pytest.mark.parametrize("E", [1, 3, 4, 20, 64, 68, 260])
def test_every_width_with_and_without_positions(t4k, E):
    for pos in (0, 1):
        run_case(t4k, "e", 2, 65, 2 * R + 3, E, pos, rung=2)
        run_case(t4k, "e0", 1, 65, 2 * R + 3, E, pos, rung=1)
        run_case(t4k, "e1", 3, 5, R + 1, E, pos, off={k: 1 for k in ("IDS", "O", "TABLE", "POS", "DY", "DTABLE", "DPOS")})


@pytest.mark.parametrize("T", [63, 64, 65, 255, 256, 257])
def test_both_sides_of_an_id_load(t4k, T):
    run_case(t4k, "t", 1, T, R + 1, 8, 1, rung=1 if T < 128 else 2)
    run_case(t4k, "tn", T, 1, 3, 4, 1, rung=1 if T < 128 else 2)                           # L = 1: every token at position 0, N = T samples for dPOS


@pytest.mark.parametrize("N,L,V,E,P", [(2, 64, 5, 8, 2), (8, 64, 5, 8, 8), (9, 64, 35, 20, 9), (4, 196, 65, 4, 7), (16, 64, 3, 260, 16), (1, 129, 3, 4, 2)])
def test_parts_and_the_fold(t4k, N, L, V, E, P):
    """a small vocabulary at a modest T: rung 2, P parts (hand-counted: min(ceil(1024 / units), T / 64), re-counted from whole id loads) and the fold launch"""
    run_case(t4k, "parts", N, L, V, E, 1, rung=2, P=P)
    run_case(t4k, "parts0", N, L, V, E, 0, rung=2, P=P, dy="int")
    run_case(t4k, "partsd", N, L, V, E, 1, off={"DTABLE": 1}, P=P)


def test_position_mode(t4k):
    for N, L, E in ((1, 1, 1), (2, 5, 3), (3, 65, 4), (17, 5, 20), (33, 3, 64), (2, 64, 260)):
        run_case(t4k, "pos", N, L, 0, E, 1, rung=0)
        run_case(t4k, "posi", N, L, 0, E, 1, rung=0, inplace=True)            # DX = DY
        run_case(t4k, "poso", N, L, 0, E, 1, off={"X": 1, "O": 1, "POS": 1, "DY": 1, "DX": 1, "DPOS": 1})
    run_case(t4k, "pos0", 3, 5, 0, 4, 1, train=0)                              # the copy alone
    run_case(t4k, "pos0i", 3, 5, 0, 4, 1, train=0, inplace=True)               # nothing to do
    run_case(t4k, "posn", 3, 5, 0, 4, 1, train="null")


def test_exact_integer_sums(t4k):
    """small-integer dY: every partial sum is an integer below 2^24, so any order gives the same bits - DTABLE / DPOS are the integer sums"""
    V, E, N, L = 2 * R + 3, 20, 3, 65
    cases = {
        "same":  lambda a: np.full_like(a, 7.0),                          # every token the same id
        "ends":  lambda a: np.where(np.arange(a.size) % 2 == 0, F(0), F(V - 1)).astype(F),       # ids 0 and V - 1
        "frac":  lambda a: (np.trunc(np.nan_to_num(np.clip(a, 0, V - 1), nan=0.0)) + F(0.75)).astype(F),
        "pads":  lambda a: np.where(np.arange(a.size) % 3 == 0, np.resize(np.array([-1.0, -0.5, V, 1e9, np.nan, np.inf, -np.inf], F), a.size), a).astype(F),
        "allpad": lambda a: np.full_like(a, -1.0),
    }
    for name, fn in cases.items():
        for pos in (0, 1):
            O, DT, DP, _ = run_case(t4k, name, N, L, V, E, pos, dy="int", ids_fn=fn)
    # an id no token has: its row keeps its previous bits (run_case holds every row to the witness; here the row is named)
    O, DT, DP, _ = run_case(t4k, "hole", N, L, V, E, 1, dy="int", ids="plain", ids_fn=lambda a: np.where(a == 5.0, F(6.0), a).astype(F))


def test_padding_gets_a_zero_vector_and_no_gradient(t4k):
    V, E, L, N = R + 1, 4, 8, 1
    pads = np.array([-1.0, -0.5, V, 1e9, np.nan, np.inf, -np.inf, 3.0], F)
    O, DT, DP, _ = run_case(t4k, "padrow", N, L, V, E, 0, ids_fn=lambda a: pads, dy="int")
    assert not O[:7].any() and O[7].any()
    O, DT, DP, _ = run_case(t4k, "padpos", N, L, V, E, 1, ids_fn=lambda a: pads, dy="int")


def test_train_0_touches_no_gradient(t4k):
    run_case(t4k, "t0", 2, 65, R + 1, 20, 1, train=0)
    run_case(t4k, "tnull", 2, 65, R + 1, 20, 1, train="null")
    run_case(t4k, "t0p", 8, 64, 5, 8, 1, train=0)


def test_the_same_bits_on_two_calls(t4k):
    for args in ((3, 65, 2 * R + 3, 20, 1), (8, 64, 5, 8, 1), (3, 65, 0, 20, 1)):
        a = run_case(t4k, "twice", *args)
        b = run_case(t4k, "twice", *args)
        for x, y in zip(a, b):
            assert (x is None and y is None) or bits(x, y)


@pytest.mark.parametrize("which", ["IDS", "TABLE", "POS", "O", "DY", "DTABLE", "DPOS", "all"])
def test_a_pointer_off_16_bytes_takes_the_dword_path(t4k, which):
    """every pointer, and each single pointer, 4 bytes off: the dword path, with the results of the aligned call"""
    names = ("IDS", "TABLE", "POS", "O", "DY", "DTABLE", "DPOS")
    off = {k: 1 for k in names} if which == "all" else {which: 1}
    for args in ((2, 65, 2 * R + 3, 20, 1), (8, 64, 5, 8, 1)):
        a = run_case(t4k, "off", *args)
        b = run_case(t4k, "off", *args, off=off)
        for x, y in zip(a, b):
            assert (x is None and y is None) or bits(x, y)
    if which in ("POS", "O", "DY", "DPOS", "all"):
        o2 = {"X": 1, "DX": 1, **off} if which == "all" else off
        a = run_case(t4k, "offp", 3, 65, 0, 20, 1); b = run_case(t4k, "offp", 3, 65, 0, 20, 1, off=o2)
        for x, y in zip(a, b):
            assert (x is None and y is None) or bits(x, y)


def test_rejections_launch_and_write_nothing(t4k):
    h = t4k
    T, L, V, E = 10, 5, 7, 4
    ids, tab, pos = Dev(np.zeros(T, F)), Dev(np.ones((V, E), F)), Dev(np.ones((L, E), F))
    x, dy = Dev(np.ones((T, E), F)), Dev(np.ones((T, E), F))
    can = lambda k: Dev(np.full(k, 77.0, F))
    O, DT, DP, DX = can(T * E), can(V * E), can(L * E), can(T * E)

    def refused(code, fn, *a):
        l0 = lcount(h)
        rc = getattr(h.lib, fn)(*a)
        assert rc == code and lcount(h) == l0 and h.lib.t4k_last_error(), (fn, rc, h.lib.t4k_last_error())
    f, b = "t4k_embed_fwd", "t4k_embed_bwd"
    refused(ERR_ARG, f, ids.p, x.p, tab.p, pos.p, O.p, T, L, V, E, None)               # both modes at once
    refused(ERR_ARG, f, None, None, tab.p, pos.p, O.p, T, L, V, E, None)               # neither
    refused(ERR_ARG, f, ids.p, None, None, pos.p, O.p, T, L, V, E, None)               # token mode without TABLE
    refused(ERR_ARG, f, ids.p, None, tab.p, pos.p, O.p, T, L, 0, E, None)              # token mode with V = 0
    refused(ERR_ARG, f, None, x.p, None, None, O.p, T, L, 0, E, None)                  # position mode without POS
    refused(ERR_ARG, f, None, x.p, None, pos.p, O.p, T, L, V, E, None)                 # position mode with V != 0
    refused(ERR_ARG, f, ids.p, None, tab.p, pos.p, None, T, L, V, E, None)
    refused(ERR_ARG, f, ids.p, None, tab.p, pos.p, O.p, T, 3, V, E, None)              # T % L
    refused(ERR_ARG, f, ids.p, None, tab.p, pos.p, O.p, 0, L, V, E, None)
    refused(ERR_ARG, f, ids.p, None, tab.p, pos.p, O.p, T, L, V, 0, None)
    refused(ERR_UNSUPPORTED, f, ids.p, None, tab.p, None, O.p, 1 << 21, 1, V, 1 << 10, None)
    refused(ERR_UNSUPPORTED, f, ids.p, None, tab.p, None, O.p, T, L, 1 << 21, 1 << 10, None)
    refused(ERR_ARG, f, ids.p, None, tab.p, pos.p, tab.p, T, L, V, E, None)            # O over TABLE
    refused(ERR_ARG, f, None, x.p, None, pos.p, x.p, T, L, 0, E, None)                 # O over X
    refused(ERR_ARG, b, ids.p, None, DT.p, DP.p, None, T, L, V, E, 1, None)            # no DY
    refused(ERR_ARG, b, None, dy.p, DT.p, DP.p, None, T, L, V, E, 1, None)             # token mode without IDS
    refused(ERR_ARG, b, ids.p, dy.p, None, DP.p, None, T, L, V, E, 1, None)            # train without DTABLE
    refused(ERR_ARG, b, None, dy.p, None, None, DX.p, T, L, 0, E, 1, None)             # position mode, train without DPOS
    refused(ERR_ARG, b, None, dy.p, None, DP.p, None, T, L, 0, E, 1, None)             # position mode without DX
    refused(ERR_ARG, b, ids.p, dy.p, None, DP.p, DX.p, T, L, 0, E, 1, None)            # position mode with IDS
    refused(ERR_ARG, b, ids.p, dy.p, DT.p, DP.p, None, T, 3, V, E, 1, None)
    refused(ERR_ARG, b, ids.p, dy.p, dy.p, DP.p, None, T, L, V, E, 1, None)            # DTABLE over DY
    refused(ERR_ARG, b, ids.p, dy.p, DT.p, DT.p, None, T, L, V, E, 1, None)            # DPOS over DTABLE
    refused(ERR_ARG, b, None, dy.p, None, DP.p, ctypes.c_void_p(dy.p.value + 4), T - 1, 1, 0, E, 1, None)      # DX overlaps DY but is not DY
    refused(ERR_UNSUPPORTED, b, ids.p, dy.p, DT.p, None, None, T, L, 1 << 21, 1 << 10, 1, None)
    for d, n in ((O, T * E), (DT, V * E), (DP, L * E), (DX, T * E)):
        assert (d.get(h, (n,)) == 77.0).all()
    assert (dy.get(h, (T * E,)) == 1.0).all() and (tab.get(h, (V * E,)) == 1.0).all()
    guards_intact(ids, tab, pos, x, dy, O, DT, DP, DX)
