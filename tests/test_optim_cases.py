"""The CPU half of the optimizer sweep: the case table of tests/optim_cases.py against itself.  The oracle's three update kernels stay inside the
float64 witness over every size for three consecutive steps; a second implementation (NumPy float32, one rounding per line in the order sgd1 / adam1 /
adamw1 of csrc/optim.hip spell out) gives the oracle's bits, at the edges of the arithmetic too - it is the reference of the GPU test there, where a
float64 witness cannot model fp32 overflow; the branch labels and the `pad` prefix are what optim.hip computes from the same numbers; and every check the
GPU test applies FAILS on an implementation with a known defect, on the rows named here and on no other."""
import numpy as np
import pytest

import optim_cases as oc


def _chain(oracle, kname, defect=None, snapshot=False):
    """every record of SIZES through STEPS steps, a fresh gradient each step; the NumPy implementation (with `defect`) is the one under test.  Returns the
    records (index) whose checks failed."""
    rng = np.random.default_rng(77)
    failed = set()
    for i, n in enumerate(oc.SIZES):
        ini = oc.operands(rng, n)
        for step in range(oc.STEPS):
            orc = oc.oracle_step(oracle, kname, *ini, oc.NW[i])
            got = oc.np_step(kname, *ini, oc.NW[i], defect)
            try:
                oc.check_record("%s n=%d step %d" % (kname, n, step), kname, ini, got[:4], orc, oc.NW[i], report="optimizer sweep (NumPy)")
                if defect is None:
                    for t, g, o in zip("wgmv", got[:4], orc):
                        oc.same_bits("%s n=%d step %d NumPy vs oracle %s" % (kname, n, step, t), g, o)
                if snapshot:
                    oc.same_bits("snapshot", got[4], ini[0])
            except AssertionError:
                if defect is None:
                    raise
                failed.add(i)
            ini = (orc[0], oc.fresh_gradient(rng, n), orc[2], orc[3])            # the next step starts from the oracle's state
    return failed


@pytest.mark.parametrize("kname", list(oc.KINDS))
def test_oracle_inside_float64_and_numpy_bit_equal_for_three_steps(oracle, kname):
    assert _chain(oracle, kname, snapshot=True) == set()


@pytest.mark.parametrize("kname", list(oc.KINDS))
def test_numpy_gives_the_oracle_bits_at_the_specials(oracle, kname):
    """gradients 0, -0, subnormal, d * d underflowing and overflowing, infinite, NaN against moments {0, 1e-38, 1, 1e30} and weights {0, +-1, +-1e30}: the
    same bits, and NaN at the same places (the payload of a NaN an operation produces is the implementation's)"""
    ini = oc.specials()
    assert len(set(zip(*(oc.bits(a).tolist() for a in ini[:3])))) == 17 * 4 * 5                 # every gradient x moment x weight
    for Nw in (1, 3):
        orc = oc.oracle_step(oracle, kname, *ini, Nw); got = oc.np_step(kname, *ini, Nw)
        for t, g, o in zip("wgmv", got[:4], orc):
            oc.same_values("%s specials Nw=%d %s" % (kname, Nw, t), g, o)
        assert not oc.bits(got[1]).any()
        assert np.isnan(got[0]).any() and np.isfinite(got[0]).any()


def test_branch_labels_follow_the_pointers():
    """BRANCH is what line 90 of optim.hip decides from the four pointers of each record, for every kind's aliasing, on a 256-byte aligned base"""
    base = 0x7f0000000000
    for layout in oc.LAYOUTS:
        for kname in oc.KINDS:
            pl = oc.Plan(oc.SIZES, layout, kname)
            got = tuple(oc.branch_of(*pl.pointers(base, i)) for i in range(len(oc.SIZES)))
            assert got == oc.BRANCH[layout], (layout, kname, got)
            for i in range(len(oc.SIZES)):                                        # every tensor inside its allocation, NaN moats of 64 floats on both sides
                for t in oc.TENSORS:
                    s, n = pl.rec[i][t]
                    assert n == oc.SIZES[i] and pl.moat[s - oc.MOAT:s - oc.LAYOUTS[layout][t]].all() and pl.moat[s + n:s + n + oc.MOAT].all() and not pl.moat[s:s + n].any()
                G, DG, M, V = pl.pointers(base, i)
                if layout == "host_alias":
                    assert (M == G and V == G) if kname == "sgd0" else (V == M and M != G) if kname == "sgdm" else len({G, DG, M, V}) == 4
                else:
                    assert len({G, DG, M, V}) == 4
    # a snapshot destination 4 bytes off drops an aligned record to the scalar branch - that record alone
    assert oc.branch_of(0x1000, 0x2000, 0x3000, 0x4000, 0x1000, 0x5004) == "scalar" and oc.branch_of(0x1000, 0x2000, 0x3000, 0x4000, 0x9000, 0x5004) == "vec"
    assert oc.branch_of(0x1000, 0x2000, 0x3000, 0x4000, 0x1000, 0x5000) == "vec"


def test_pad_prefix_is_the_running_sum_of_chunks():
    pad, chunks = oc.pads(oc.SIZES)
    want = np.concatenate([[0], np.cumsum([-(-n // 1024) for n in oc.SIZES])])
    assert pad == want[:-1].tolist() and chunks == want[-1] == 18
    e = oc.SIZES.index(0)
    assert pad[e] == pad[e + 1] and pad[e - 1] + 3 == pad[e]                      # the empty record has no chunk: it shares its pad with the record behind it
    # the scan of k_opt_chunked (`while (i + 1 < nt && b >= tab[i + 1].pad) i++`) gives every chunk to a record that has it, never to the empty one
    for b in range(chunks):
        i = 0
        while i + 1 < len(pad) and b >= pad[i + 1]: i += 1
        assert 0 <= (b - pad[i]) * 1024 < oc.SIZES[i], (b, i)
    import struct
    raw, c = oc.Plan(oc.SIZES, "aligned", "adam").table(1 << 20)
    assert c == chunks and len(raw) == 48 * len(oc.SIZES)
    assert [struct.unpack_from("<QQQQqii", raw, 48 * i)[4:] for i in range(len(oc.SIZES))] == [(n, nw, q) for n, nw, q in zip(oc.SIZES, oc.NW, pad)]


_ALL = tuple(oc.KINDS)
_NONEMPTY = {i for i, n in enumerate(oc.SIZES) if n > 0}
_HAS_V0 = {i for i, n in enumerate(oc.SIZES) if n > 5}                           # element 5 has dg = 0 and v = 0: v' = 0, the place where eps alone divides
# defect -> (the kinds, the records) whose checks must fail; every other (kind, record) must pass
DEFECT_ROWS = {
    "wd_times_m":            (("adamw",), _NONEMPTY),
    "eps_inside_root":       (("adam", "adamw"), _HAS_V0),
    "v_from_d":              (("adam", "adamw"), _NONEMPTY),
    "momentum_not_stored":   (("sgdm", "adam", "adamw"), _NONEMPTY),
    "gradient_not_zeroed":   (_ALL, _NONEMPTY),
    "dg_over_batch":         (("sgd0", "sgdm"), _NONEMPTY),
    "last_three_skipped":    (_ALL, _NONEMPTY),
    "snapshot_after_update": (_ALL, _NONEMPTY),
}


@pytest.mark.parametrize("defect", oc.DEFECTS)
def test_injected_defect_fails_the_named_rows(oracle, defect):
    """the defect goes into the NumPy implementation, never into a kernel; the checks are the GPU test's own (optim_cases.check_record, same_bits)"""
    kinds, recs = DEFECT_ROWS[defect]
    for kname in oc.KINDS:
        failed = _chain(oracle, kname, defect, snapshot=True)
        want = recs if kname in kinds else set()
        if defect == "eps_inside_root" and kname in kinds:
            assert want <= failed, (defect, kname, sorted(failed))                 # (a small v' elsewhere may show it too)
        else:
            assert failed == want, (defect, kname, sorted(failed), sorted(want))
    assert set(DEFECT_ROWS) == set(oc.DEFECTS)
