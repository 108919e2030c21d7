"""t4k_pool_geo_plan (include/t4k.h, csrc/pool_geo.hip): admission, output extents and channel vector widths of the run-time-geometry
pooling, on the host alone - nothing is launched and no device is needed, so these rows run wherever the library loads.

out = { H0, W0, channel vector width of the forward (4 | 1), of the backward (4 | 1) }.  The extents are a FLOOR grid, (H1 + 2P - K) / S + 1 and the
same from W1 - torch's max_pool2d / avg_pool2d output shape.  A width of 4 needs C % 4 == 0 and the pass's tensors on 16 bytes: `aligned` bit 0
speaks for I and O (the forward), bit 1 for DY and DX (the backward)."""
import ctypes

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I4 = ctypes.c_int * 4


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def layer_ids():
    """T4K_L_AVGPOOL / MAXPOOL / MINPOOL from the header's layer enumeration"""
    import os
    import re
    from tensorforth_amd.lib import root_dir
    text = open(os.path.join(root_dir(), "include", "t4k.h")).read()
    body = re.search(r"T4K_L_NONE\s*=\s*0(.*?)\}", text, re.S).group(0)
    names = re.findall(r"T4K_L_\w+", body)
    return {n: i for i, n in enumerate(names)}


def plan(lib, layer, N, H1, W1, C, K, S, P, aligned=3):
    out = I4()
    rc = lib.t4k_pool_geo_plan(layer, N, H1, W1, C, K, S, P, aligned, out)
    return rc, list(out)


def admitted():
    for K in range(1, 17):
        for S in range(1, 17):
            for P in range(0, K // 2 + 1):
                yield K, S, P


def test_layer_ids_are_what_the_header_says():
    ids = layer_ids()
    assert ids["T4K_L_NONE"] == 0 and {"T4K_L_AVGPOOL", "T4K_L_MAXPOOL", "T4K_L_MINPOOL", "T4K_L_USAMPLE", "T4K_L_CONV"} <= set(ids)


def test_extent_rule_against_torch(lib):
    """every admitted (K, S, P) with K <= 16 at H1 = 1..20 and W1 = 1..20: the plan admits exactly the images whose padded extent holds the window, and H0, W0
    are torch's output shape - W0 from W1, on rectangular images too.  torch is asked once per (K, S, P, extent) on a one-row image (its rule is separable)"""
    L = layer_ids()["T4K_L_MAXPOOL"]
    n = 0
    for K, S, P in admitted():
        ext = {}
        for H1 in range(1, 21):
            if K <= H1 + 2 * P:
                o = torch.nn.functional.max_pool2d(torch.zeros(1, 1, H1, K), K, S, (P, 0))       # the width K holds one window without padding
                assert o.shape[3] == 1
                ext[H1] = o.shape[2]
                assert ext[H1] == (H1 + 2 * P - K) // S + 1
        for H1 in range(1, 21):
            for W1 in (1, 2, 3, 5, 8, 13, 20, H1):
                rc, out = plan(lib, L, 2, H1, W1, 3, K, S, P)
                fits = H1 in ext and W1 in ext
                assert rc == (OK if fits else ERR_UNSUPPORTED), (K, S, P, H1, W1, rc)
                if fits:
                    assert out[:2] == [ext[H1], ext[W1]], (K, S, P, H1, W1, out)
                    n += 1
    assert n > 100000
    for K, S, P, H1, W1 in ((3, 2, 1, 11, 9), (7, 4, 1, 8, 13), (16, 3, 8, 11, 9), (2, 3, 0, 20, 7)):   # whole rectangular calls, and avg_pool2d's shape beside
        o = torch.nn.functional.max_pool2d(torch.zeros(1, 1, H1, W1), K, S, P)
        a = torch.nn.functional.avg_pool2d(torch.zeros(1, 1, H1, W1), K, S, P, count_include_pad=True)
        assert plan(lib, L, 1, H1, W1, 1, K, S, P)[1][:2] == [o.shape[2], o.shape[3]] == [a.shape[2], a.shape[3]]
    with pytest.raises(RuntimeError):
        torch.nn.functional.max_pool2d(torch.zeros(1, 1, 8, 8), 4, 2, 3)                             # P <= K / 2 is torch's rule


def test_rejections(lib):
    ids = layer_ids()
    good = dict(layer=ids["T4K_L_MAXPOOL"], N=3, H1=11, W1=9, C=4, K=3, S=2, P=1)
    call = lambda **kw: plan(lib, **{**good, **kw})[0]
    assert call() == OK
    assert lib.t4k_pool_geo_plan(good["layer"], 3, 11, 9, 4, 3, 2, 1, 3, None) == ERR_ARG
    for name in ("T4K_L_AVGPOOL", "T4K_L_MAXPOOL", "T4K_L_MINPOOL"):
        assert call(layer=ids[name]) == OK
    for name in ("T4K_L_USAMPLE", "T4K_L_CONV", "T4K_L_RELU", "T4K_L_NONE"):                       # no avg / max / min pool
        assert call(layer=ids[name]) == ERR_UNSUPPORTED, name
        assert b"layer" in lib.t4k_last_error()
    assert call(layer=-1) == ERR_UNSUPPORTED and call(layer=1000) == ERR_UNSUPPORTED
    for name in ("N", "H1", "W1", "C"):                                                              # an extent below 1: a bad argument
        assert call(**{name: 0}) == ERR_ARG and call(**{name: -2}) == ERR_ARG, name
        assert b"extent" in lib.t4k_last_error()
    for kw in (dict(K=0), dict(K=17), dict(K=-3), dict(S=0), dict(S=17), dict(S=-1), dict(P=-1), dict(P=2), dict(K=1, P=1), dict(K=2, P=2), dict(K=7, P=4)):
        assert call(**kw) == ERR_UNSUPPORTED, kw
        assert b"not supported" in lib.t4k_last_error()
    assert call(K=16, S=16, P=8, H1=1, W1=1) == OK and call(K=7, P=3) == OK and call(K=2, P=1) == OK and call(K=1, S=16, P=0) == OK
    assert call(H1=2, K=6, P=2) == OK                                                                # an image smaller than the window, inside its padding
    assert call(H1=2, K=7, P=2) == ERR_UNSUPPORTED and b"does not fit" in lib.t4k_last_error()     # 2 + 4 < 7
    assert call(W1=2, K=5, P=1) == ERR_UNSUPPORTED and b"does not fit" in lib.t4k_last_error()     # ... on W alone
    assert call(H1=11, W1=11, K=11, P=0) == OK and call(H1=11, W1=10, K=11, P=0) == ERR_UNSUPPORTED
    assert call(N=1 << 20, H1=64, W1=32, K=1, S=1, P=0) == ERR_UNSUPPORTED and b"2^31" in lib.t4k_last_error()
    assert call(N=(1 << 20) - 1, H1=64, W1=32, K=1, S=1, P=0) == OK
    assert call(N=1 << 20, H1=64, W1=32, K=2, S=2, P=0) == ERR_UNSUPPORTED                           # ... on the input side alone
    assert call(N=(1 << 21) - 1, H1=32, W1=32, K=2, S=1, P=1) == ERR_UNSUPPORTED                     # ... on the output side alone: 33 x 33 outputs
    assert call(N=(1 << 21) - 1, H1=32, W1=32, K=2, S=1, P=0) == OK


@pytest.mark.parametrize("C", [3, 4, 8])
@pytest.mark.parametrize("aligned", [0, 1, 2, 3])
def test_vector_widths(lib, C, aligned):
    """a width of 4 needs C % 4 == 0 and the pass's own alignment bit - the forward bit 0, the backward bit 1 - for every layer kind"""
    ids = layer_ids()
    for name in ("T4K_L_AVGPOOL", "T4K_L_MAXPOOL", "T4K_L_MINPOOL"):
        rc, out = plan(lib, ids[name], 3, 11, 9, C, 3, 2, 1, aligned)
        assert rc == OK
        assert out == [6, 5, 4 if (C % 4 == 0 and aligned & 1) else 1, 4 if (C % 4 == 0 and aligned & 2) else 1], (name, C, aligned, out)
