"""t4k_token_ce_plan (include/t4k.h, csrc/token_ce.hip) on the host alone: nothing is launched and no device is needed.

out = { rung, load path, lanes of a team, tokens a wave has in flight, passes, rescales R, launches of the score, workspace bytes }; the rule is the header's,
worked by hand in ROWS on both sides of every switch.  tools/token_ce_plan_check.cpp walks the same function around every limit."""
import ctypes

import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
WS = 32 << 20
SENTINEL = [-7] * 8


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, T, V, aligned=1, ws=WS):
    out = I8(*SENTINEL)
    return lib.t4k_token_ce_plan(T, V, aligned, ws, out), list(out)


ROWS = [
    ((16384, 65, 1, WS),      [0, 1, 32, 2, 1, 0, 2, 1024]),     # a character model: 65 dwords, 17 lanes would do: a team of 32, two tokens a wave; 64 score workgroups
    ((32, 11, 1, WS),         [0, 1, 4, 16, 1, 0, 1, 0]),        # 11 items: 3 lanes -> 4; T <= 256: the score is one launch
    ((8192, 4096, 1, WS),     [1, 4, 256, 1, 1, 0, 2, 512]),     # 1024 items: the workgroup, in registers
    ((64, 2048, 1, WS),       [0, 4, 64, 1, 1, 0, 1, 0]),        # 512 items: the last a wave holds
    ((64, 2052, 1, WS),       [1, 4, 256, 1, 1, 0, 1, 0]),       # 513
    ((64, 8192, 1, WS),       [1, 4, 256, 1, 1, 0, 1, 0]),       # 2048 items: the last a workgroup holds
    ((64, 8196, 1, WS),       [2, 4, 256, 1, 2, 3, 1, 0]),       # 2049: two passes, two chunks + 1
    ((64, 8196, 0, WS),       [2, 1, 256, 1, 2, 6, 1, 0]),       # ... in dwords 8196 items: five chunks + 1
    ((4096, 32768, 1, WS),    [2, 4, 256, 1, 2, 5, 2, 256]),     # a BPE vocabulary: 8192 items, four chunks + 1
    ((257, 8, 1, 31),         [0, 4, 1, 64, 1, 0, 1, 0]),        # two score workgroups need 32 bytes: 31 do not hold them
    ((257, 8, 1, 32),         [0, 4, 1, 64, 1, 0, 2, 32]),
    ((127, 1 << 24, 1, WS),   [2, 4, 256, 1, 2, 2049, 1, 0]),    # the largest V at the largest T it admits
]


@pytest.mark.parametrize("args,want", ROWS, ids=["t%d_v%d_a%d_w%d" % r[0] for r in ROWS])
def test_hand_worked_rows(lib, args, want):
    assert plan(lib, *args) == (OK, want)


@pytest.mark.parametrize("args,code", [((0, 8, 1, WS), ERR_ARG), ((-1, 8, 1, WS), ERR_ARG), ((8, 1, 1, WS), ERR_ARG), ((8, 0, 1, WS), ERR_ARG),
                                       ((8, -3, 1, WS), ERR_ARG), ((8, 8, 1, -1), ERR_ARG), ((1, (1 << 24) + 1, 1, WS), ERR_UNSUPPORTED),
                                       ((128, 1 << 24, 1, WS), ERR_UNSUPPORTED), ((1 << 28, 8, 1, WS), ERR_UNSUPPORTED), ((1 << 31, 2, 1, WS), ERR_UNSUPPORTED),
                                       ((1 << 62, 4, 1, WS), ERR_UNSUPPORTED)])
def test_rejections_leave_out_untouched(lib, args, code):
    assert plan(lib, *args) == (code, SENTINEL) and lib.t4k_last_error()
    assert lib.t4k_token_ce_plan(8, 8, 1, WS, None) == ERR_ARG
