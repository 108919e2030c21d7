"""t4k_linalg_batched_plan (include/t4k.h, csrc/linalg_batched.hip) on the host alone: nothing is launched, no device is needed.

out = { regime (0 wave, 1 workgroup, 2 global, 3 blocked), threads per group, NB (0 outside blocked), LDS bytes, launches, workgroups, load path, 0 }
for entry 0 inverse, 1 plu, 2 lu_inverse, 3 det.  The rule, worked by hand in ROWS: wave up to K = 32 (four matrices per workgroup), workgroup up to
K = 140 (inverse, lu_inverse) or 200 (plu, det); inverse and lu_inverse are global up to KB = 192; above that every entry is blocked (NB = 32) up to
K = 1024."""
import ctypes

import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
SENTINEL = [-7] * 8
INV, PLU, LUINV, DET = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, entry, K, batch, aligned=1):
    out = I8(*SENTINEL)
    return lib.t4k_linalg_batched_plan(entry, K, batch, aligned, out), list(out)


def words(K, mats):                                                        # A (and X) at pitch K | 1, colz, perm, 12 slots; rounded up to 4 words
    return (mats * K * (K | 1) + 2 * K + 12 + 3) & ~3


def blocked_lds(K, two=False):                                             # the panel [rows to 32][33], 32 pivots, perm, 12 slots;
    panel = ((K + 31) & ~31) * 33                                          # inverse, lu_inverse: at least four waves' two tiles [32][33]
    return 4 * (((max(panel, 8 * 32 * 33) if two else panel) + 32 + K + 12 + 3) & ~3)


# ((entry, K, batch, aligned), out): both sides of every boundary
ROWS = [
    ((INV, 32, 7, 1),     [0, 256, 0, 16 * words(32, 2), 1, 2, 4, 0]),
    ((INV, 33, 7, 1),     [1, 256, 0, 4 * words(33, 2), 1, 7, 1, 0]),       # 33 * 33 % 4 != 0: dwords
    ((LUINV, 140, 3, 1),  [1, 256, 0, 159088, 1, 3, 4, 0]),
    ((LUINV, 141, 3, 1),  [2, 256, 0, 4 * words(141, 0), 1, 3, 1, 0]),
    ((INV, 140, 2, 1),    [1, 256, 0, 159088, 1, 2, 4, 0]),
    ((INV, 141, 2, 1),    [2, 256, 0, 4 * words(141, 0), 1, 2, 1, 0]),
    ((INV, 192, 2, 1),    [2, 256, 0, 4 * words(192, 0), 1, 2, 1, 0]),      # KB
    ((INV, 193, 2, 1),    [3, 256, 32, blocked_lds(193, True), 1, 2, 1, 0]),   # KB + 1: 224 panel rows are fewer words than the substitution's tiles
    ((LUINV, 32, 4, 1),   [0, 256, 0, 16 * words(32, 2), 1, 1, 4, 0]),
    ((LUINV, 33, 4, 1),   [1, 256, 0, 4 * words(33, 2), 1, 4, 1, 0]),
    ((LUINV, 192, 3, 0),  [2, 256, 0, 4 * words(192, 0), 1, 3, 1, 0]),
    ((LUINV, 193, 3, 0),  [3, 256, 32, 4 * 8688, 1, 3, 1, 0]),
    ((LUINV, 256, 3, 1),  [3, 256, 32, 4 * (256 * 33 + 32 + 256 + 12), 1, 3, 4, 0]),
    ((INV, 1024, 1, 1),   [3, 256, 32, 139440, 1, 1, 4, 0]),
    ((PLU, 33, 9, 0),     [1, 256, 0, 4 * words(33, 1), 1, 9, 1, 0]),
    ((DET, 32, 5, 1),     [0, 256, 0, 16 * words(32, 1), 1, 2, 4, 0]),
    ((DET, 33, 5, 1),     [1, 256, 0, 4 * words(33, 1), 1, 5, 1, 0]),
    ((PLU, 32, 9, 0),     [0, 256, 0, 16 * words(32, 1), 1, 3, 1, 0]),
    ((PLU, 200, 2, 1),    [1, 256, 0, 162448, 1, 2, 4, 0]),
    ((PLU, 201, 2, 1),    [3, 256, 32, blocked_lds(201), 1, 2, 1, 0]),      # the first blocked K, odd: dwords
    ((DET, 200, 5, 1),    [1, 256, 0, 162448, 1, 5, 4, 0]),
    ((DET, 201, 5, 1),    [3, 256, 32, blocked_lds(201), 1, 5, 1, 0]),
    ((DET, 204, 5, 1),    [3, 256, 32, blocked_lds(204), 1, 5, 4, 0]),
    ((PLU, 204, 5, 0),    [3, 256, 32, blocked_lds(204), 1, 5, 1, 0]),      # a base off the 16-byte grid
    ((PLU, 1024, 1, 1),   [3, 256, 32, 139440, 1, 1, 4, 0]),
]


@pytest.mark.parametrize("args,out", ROWS, ids=["e%d_k%d_b%d_a%d" % r[0] for r in ROWS])
def test_hand_worked_rows(lib, args, out):
    rc, got = plan(lib, *args)
    assert rc == OK and got == out, (args, got, lib.t4k_last_error())
    assert got[3] <= 160 * 1024 and got[4] == 1


@pytest.mark.parametrize("entry", (INV, PLU, LUINV, DET))
def test_limits_and_refusals(lib, entry):
    assert plan(lib, entry, 1024, 3)[0] == OK
    assert plan(lib, entry, 4, 0) == (OK, [0, 256, 0, 16 * words(4, 2 if entry in (INV, LUINV) else 1), 1, 0, 4, 0])
    for K, batch, code in ((1025, 1, ERR_UNSUPPORTED), (0, 1, ERR_ARG), (-3, 1, ERR_ARG), (4, -1, ERR_ARG)):
        assert plan(lib, entry, K, batch) == (code, SENTINEL), (K, batch)
        assert lib.t4k_last_error()
    assert lib.t4k_linalg_batched_plan(entry, 4, 1, 1, None) == ERR_ARG
    for bad in (-1, 4):
        assert plan(lib, bad, 4, 1) == (ERR_ARG, SENTINEL)
    assert plan(lib, entry, 5, 2**31 - 1)[1][5] == 2**29                     # ceil(batch / 4) taken in 64 bits
