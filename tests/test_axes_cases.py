"""tests/axes_cases.py against the library and against itself, on the CPU: the table lands on its plans, covers what the planner can reach, the
mirror equals t4k_reduce_axes_plan / t4k_softmax_axes_geometry on a random walk, and the sweep's pass criteria notice the faults they are meant for."""
import ctypes

import numpy as np
import pytest

import axes_cases as ac

I4, I8 = ctypes.c_int * 4, ctypes.c_int * 8
OK, ERR_ARG, ERR_NODEVICE = 0, -1, -5
WALK = 24000


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def entry(lib, kernel):
    return lib.t4k_reduce_axes_plan if kernel == "reduce" else lib.t4k_softmax_axes_geometry


def report(lib, kernel, dim, mask, aligned, ws_bytes):
    out = I8()
    rc = entry(lib, kernel)(I4(*dim), mask, int(aligned), ctypes.c_long(ws_bytes), out)
    return rc, list(out)


# ----------------------------------------------------------------------------------------------------------------- the table
def test_the_table_lands_on_its_plans(lib):
    """every row: the mirror gives the fields the row asserts, and so does the library, with no device"""
    for r in ac.TABLE:
        for k in ac.KERNELS:
            p = r.plan(k)
            assert p.fields() == r.want(k), (r.id, k, p)
            assert report(lib, k, r.dim, r.mask, True, ac.WS_BYTES) == (OK, r.want(k)), (r.id, k)
        p = r.plan("softmax")
        assert (p.regime, p.chunks) == (r.regime, r.chunks), (r.id, p)
    assert len({r.id for r in ac.TABLE}) == len(ac.TABLE)
    assert max(r.size for r in ac.TABLE) == 2100 * 8196 and sorted(r.size for r in ac.TABLE)[-2] < 4_500_000


def test_every_factor_value_and_every_crossing_has_a_row():
    labels = ac.all_labels()
    for k in ac.KERNELS:
        for fam in (ac.ROW, ac.COL):
            mine = [L for L in labels if L.kernel == k and L.family == fam]
            assert {L.vec for L in mine} == {0, 1} and {L.split for L in mine} == {ac.NONE, ac.INNER, ac.OUTER}
            assert {L.lanes for L in mine} == ({0, 1, 2, 3, 4, 5, 6, 8} if fam == ac.ROW else {0, 1, 2, 3, 4, 5, 6}), (k, fam)    # k0 = 2, 3 take sx = 1 scalar: sx = 0 is float4 k0 = 4
            assert {L.outer for L in mine} == {False, True} and {L.second for L in mine} == {False, True} and {L.wrap for L in mine} == {False, True}
            assert {L.tiles for L in mine} == ({False, True} if fam == ac.COL else {False})
            assert {L.regime for L in mine} == ({None} if k == "reduce" else {ac.REG, ac.ONLINE, ac.MULTI})
            assert {L.loop for L in mine} == ({"short", "long"} if (k, fam) == ("reduce", ac.ROW) else {None})
    for k, name, pred in ac.CROSSINGS:
        assert any(pred(r.plan(k), ac.label(r.plan(k))) for r in ac.TABLE), (k, name)
    for r in ac.TABLE:                                                  # what UNREACHABLE names, no row reaches either
        for k in ac.KERNELS:
            assert not any(f(r.plan(k)) for f in ac.UNREACHABLE.values())


def test_rows_are_the_smallest_kind():
    """no row could go without losing a pair of factor values or a crossing, the issue's named rows apart"""
    named = [r for r in ac.TABLE if r.name != r.id]
    assert len(named) == 16
    full = ac.all_pairs()
    for r in ac.TABLE:
        if r in named:
            continue
        rest = set()
        for o in ac.TABLE:
            if o is not r:
                for k in ac.KERNELS:
                    rest |= ac.pairs(ac.label(o.plan(k)))
        assert rest != full, r.id


# ----------------------------------------------------------------------------------------------------------------- the walk
def test_random_walk_mirror_equals_the_library_and_stays_inside_the_table(lib):
    """WALK draws at the library's workspace size: the eight fields equal, field by field; every pair of factor values seen is one the table
    holds; nothing UNREACHABLE is reached"""
    have, seen, worst_split = ac.all_pairs(), set(), 0
    for dim, mask, aligned in ac.walk(20241, WALK):
        for k in ac.KERNELS:
            rc, got = report(lib, k, dim, mask, aligned, ac.WS_BYTES)
            try:
                p = (ac.reduce_plan if k == "reduce" else ac.softmax_plan)(dim, mask, aligned)
            except ValueError:
                assert rc == ERR_ARG, (dim, mask)
                continue
            assert rc == OK and got == p.fields(), (k, dim, mask, aligned, got, p)
            for name, f in ac.UNREACHABLE.items():
                assert not f(p), (name, dim, mask, aligned, p)
            ps = ac.pairs(ac.label(p))
            assert ps <= have, (k, dim, mask, aligned, sorted(ps - have, key=str))
            seen |= ps
            if p.S > 1:
                worst_split = max(worst_split, p.nitem)
    assert len(seen) >= 0.97 * len(have), (len(seen), len(have))         # the walk is wide enough to mean something
    assert 1900 <= worst_split <= 2047, worst_split


def test_random_walk_with_a_small_workspace_reaches_the_cap(lib):
    """ws_bytes = 4 KiB: split_for's workspace term decides, in both kernels and both families, and the mirror still equals the library"""
    capped = set()
    for dim, mask, aligned in ac.walk(20242, WALK):
        for k in ac.KERNELS:
            rc, got = report(lib, k, dim, mask, aligned, 4096)
            try:
                p = (ac.reduce_plan if k == "reduce" else ac.softmax_plan)(dim, mask, aligned, 4096)
            except ValueError:
                assert rc == ERR_ARG
                continue
            assert rc == OK and got == p.fields(), (k, dim, mask, aligned, got, p)
            big = (ac.reduce_plan if k == "reduce" else ac.softmax_plan)(dim, mask, aligned)
            if p.capped:
                capped.add((k, p.family, p.S > 1))
                assert p.S <= big.S and (p.S == 1 or (p.S * p.nout if k == "reduce" else 2 * (p.S + 1) * p.nout) <= 1024), (dim, mask, p, big)     # what the parts leave fits the 1024 floats
            else:
                assert p.fields() == big.fields()
    assert capped == {(k, f, s) for k in ac.KERNELS for f in (0, 1) for s in (False, True)}, capped


def test_plan_entries_arguments(lib):
    for k in ac.KERNELS:
        f = entry(lib, k)
        dim, out = I4(2, 3, 4, 5), I8()
        assert f(dim, 5, 1, ctypes.c_long(4096), None) == ERR_ARG and f(None, 5, 1, ctypes.c_long(4096), out) == ERR_ARG
        assert f(dim, 0, 1, ctypes.c_long(4096), out) == ERR_ARG and f(dim, 16, 1, ctypes.c_long(4096), out) == ERR_ARG
        assert f(I4(2, 0, 4, 5), 5, 1, ctypes.c_long(4096), out) == ERR_ARG
        assert f(dim, 5, 1, ctypes.c_long(-4), out) == ERR_ARG and b"ws_bytes" in lib.t4k_last_error()
        assert f(I4(1 << 11, 1 << 10, 1 << 10, 1 << 10), 6, 1, ctypes.c_long(4096), out) == ERR_ARG
        assert f(dim, 5, 1, ctypes.c_long(1), out) == OK and list(out)[5] == 1      # a workspace of no float at all: no split, no division by it


def test_own_workspace_needs_init(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_axes_sweep.py asks with ws_bytes = 0 after t4k_init")
    for k in ac.KERNELS:
        assert entry(lib, k)(I4(2, 3, 4, 5), 5, 1, ctypes.c_long(0), I8()) == ERR_NODEVICE


# ----------------------------------------------------------------------------------------------------------------- the criteria bite
CPU_MAX = 1_200_000                 # floats: the mutations are shown on rows up to this size, the honest evaluation on every row


def fails(f, *a, **kw):
    try:
        f(*a, **kw)
    except AssertionError:
        return True
    return False


def judged_reduce(r, mutate):
    """[(name, exact, failed)] of every pass of the row under the evaluation by plan"""
    p, out = r.plan("reduce"), []
    for name, op, x, c, exact in ac.reduce_passes(r.dim, r.mask):
        got = ac.reduce_by_plan(op, x, c, p, mutate).reshape(ac.kept(r.dim, r.mask))
        out.append((name, exact, fails(ac.judge_reduce, name, op, x, r.mask, c, got, exact)))
    return out


def judged_softmax(r, mutate):
    p, out = r.plan("softmax"), []
    for name, x, exact in ac.softmax_passes(r.dim, r.mask):
        got = ac.softmax_by_plan(x, p, mutate)
        out.append((name, exact, fails(ac.judge_softmax, name, x, r.mask, got, p.rescales, exact)))
    return out


SMALL = [r for r in ac.TABLE if r.size <= CPU_MAX]


@pytest.mark.parametrize("r", ac.TABLE, ids=[r.id for r in ac.TABLE])
def test_an_honest_fp32_evaluation_in_another_order_passes(r):
    assert not [j for j in judged_reduce(r, None) if j[2]]
    assert not [j for j in judged_softmax(r, None) if j[2]]


SPLIT = [r for r in SMALL if r.plan("reduce").S > 1]
WRAP = [ac.row((2100, 2, 1, 3), 4), ac.row((2100, 2, 1, 260), 4), ac.row((2049, 2, 1, 7), 4), ac.row((1, 1, 524300, 1), 1), ac.row((9, 2100, 5, 4), 10)]
TWICE = [ac.row(*k) for k in [((1, 1, 1, 4097), 1), ((40, 2, 3, 5), 10), ((3, 2, 40, 64), 10), ((2, 3, 3, 683), 5), ((4, 4, 8, 4), 5), ((8, 1, 1, 1), 12), ((2100, 2, 1, 3), 4)]]
ONLINE = [r for r in SMALL if r.regime == ac.ONLINE]
MULTI = [r for r in SMALL if r.regime == ac.MULTI]


@pytest.mark.parametrize("r", SPLIT, ids=[r.id for r in SPLIT])
def test_a_dropped_last_part_fails_the_exact_passes(r):
    """every split row of the table: the integer SUM and both integer NVAR of the reduction, the constant tensor of the softmax"""
    assert r.plan("softmax").S > 1
    j = {n: f for n, e, f in judged_reduce(r, "drop_last_part")}
    assert j["int op 0"] and j["int op 1"] and j["int nvar NULL"], j
    j = {n: f for n, e, f in judged_softmax(r, "drop_last_part")}
    assert j["constant"], j


@pytest.mark.parametrize("r", WRAP, ids=[r.id for r in WRAP])
def test_a_single_pass_of_the_grid_stride_loop_fails_every_pass(r):
    """outputs behind the first 2048 work items keep the NaN prefill"""
    for k in ac.KERNELS:
        dead = ac.groups_beyond_first_trip(r.plan(k))
        assert 0 < dead.sum() < dead.size, (k, r.id)
    assert all(f for _, _, f in judged_reduce(r, "single_trip"))
    assert all(f for _, _, f in judged_softmax(r, "single_trip"))


@pytest.mark.parametrize("r", TWICE, ids=[r.id for r in TWICE])
def test_an_element_taken_twice_fails_the_exact_passes(r):
    j = {n: f for n, e, f in judged_reduce(r, "twice")}
    assert j["int op 0"] and j["int nvar NULL"], j                      # the element doubled is not 0: the sum and the sum of squares move
    assert not j["int op 2"] and not j["int op 3"]                      # (max and min cannot see it)
    j = {n: f for n, e, f in judged_softmax(r, "twice")}
    assert j["constant"], j


@pytest.mark.parametrize("r", MULTI, ids=[r.id for r in MULTI])
def test_a_merge_without_the_rescale_fails_the_float_bound(r):
    j = {n: f for n, e, f in judged_softmax(r, "merge_unscaled")}
    assert j["normal"] and j["wide"] and not j["constant"], j          # (the constant tensor's maxima are equal: the factor is 1)


@pytest.mark.parametrize("r", ONLINE, ids=[r.id for r in ONLINE])
def test_a_running_sum_that_forgets_the_rescale_fails_the_float_bound(r):
    j = {n: f for n, e, f in judged_softmax(r, "online_unscaled")}
    assert j["normal"] and j["wide"] and not j["constant"], j
