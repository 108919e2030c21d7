"""t4k_gateact_plan (include/t4k.h, csrc/gateact.hip) on the host alone, and the float64 rule the GPU tests hold the kernels to.

out = { rung, load path, items a lane has in flight, workgroups forward, workgroups backward, launches forward, launches backward, 0 }; the rule is the
header's, worked by hand in ROWS on both sides of every switch.  tools/gateact_plan_check.cpp walks the same function around every limit.

reference(kind, a) is f and f' in float64, written so that the tails keep their relative accuracy (erfc, sigmoid(-z)); it is checked against torch's
functions and their autograd.  bound() is the issue's |got - ref| <= k u (|ref| + cond) plus FLT_MIN (1 + |scale|): float32 has no normal number below
2^-126, so a factor or a product below it may come out as zero whatever the arithmetic - without that term the correctly rounded reference itself
misses the bound wherever f' underflows (GELU' at -14, SiLU' at -104).  With it the rounded reference passes at k = 1, which is checked here."""
import ctypes
import math

import numpy as np
import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
SENTINEL = [-7] * 8
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
EXTREMES = [0.0, 88.0, -88.0, 1e4, -1e4, 3.4e38, -3.4e38]


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, *a):
    out = I8(*SENTINEL)
    return lib.t4k_gateact_plan(*a, out), list(out)


def reference(kind, a):
    """(f(a), f'(a)) for a float64 tensor"""
    if kind == 0:
        Phi = 0.5 * torch.erfc(-a / math.sqrt(2.0))
        return a * Phi, Phi + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
    if kind == 3:
        t, s = torch.tanh(torch.nn.functional.softplus(a)), torch.sigmoid(a)
        return a * t, t + a * (1.0 - t * t) * s
    k0 = math.sqrt(2.0 / math.pi)
    z, c = (2.0 * k0 * (a + 0.044715 * a ** 3), 2.0 * k0 * (1.0 + 3.0 * 0.044715 * a * a)) if kind == 1 else (a, torch.ones_like(a))
    s, s1 = torch.sigmoid(z), torch.sigmoid(-z)
    return a * s, s * (1.0 + a * c * s1)


def torch_f(kind, a):
    fn = torch.nn.functional
    return (fn.gelu(a), fn.gelu(a, approximate="tanh"), fn.silu(a), fn.mish(a))[kind]


def sweep(n, seed):
    """n values of a: [-30, 30] with a third each near 0 and near +-6, and the extreme points at the end (the last n of them where n is smaller)"""
    rng = np.random.default_rng(seed)
    m = max(n - len(EXTREMES), 0)
    a = np.concatenate([rng.uniform(-30.0, 30.0, m - 2 * (m // 3)), rng.normal(0.0, 0.5, m // 3), rng.choice([-6.0, 6.0], m // 3) + rng.normal(0.0, 0.5, m // 3)])
    return np.concatenate([rng.permutation(a), EXTREMES])[-n:].astype(np.float32)


def operands(gate, T, C, seed):
    """X [T, C] with the sweep in A (or all of X), dY ~ N(0, 1) [T, Hc], B ~ N(0, 1); at +-3.4e38 B and dY are 0.5, so that the products stay floats"""
    rng = np.random.default_rng(seed)
    Hc = C // 2 if gate else C
    A = sweep(T * Hc, seed).reshape(T, Hc)
    DY, B = rng.normal(0.0, 1.0, (T, Hc)).astype(np.float32), rng.normal(0.0, 1.0, (T, Hc)).astype(np.float32)
    DY[np.abs(A) > 1e30] = B[np.abs(A) > 1e30] = 0.5
    return (np.concatenate([A, B], 1) if gate else A), DY


def bound(k, ref, cond, scale):
    return k * U * (np.abs(ref) + cond) + FLT_MIN * (1.0 + np.abs(scale))


def rule(kind, gate, X, DY):
    """float64 (Y, DX) and their cond terms for X [T, C], DY [T, Hc] - the issue's: |a| for a value of f, |a f'| + |f| for f', times what multiplies them"""
    x, dy = torch.from_numpy(X.astype(np.float64)), DY.astype(np.float64)
    Hc = X.shape[1] // 2 if gate else X.shape[1]
    a = x[:, :Hc]
    f, d = (t.numpy() for t in reference(kind, a))
    a = a.numpy()
    cf, cd = np.abs(a), np.abs(a * d) + np.abs(f)
    if not gate:
        return (f, cf, np.ones_like(f)), (dy * d, cd * np.abs(dy), dy)
    b = x[:, Hc:].numpy()
    return (f * b, cf * np.abs(b), b), (np.concatenate([dy * b * d, dy * f], 1), np.concatenate([cd * np.abs(b * dy), cf * np.abs(dy)], 1), np.concatenate([b * dy, dy], 1))


# (T, C, kind, gate, aligned) -> out
ROWS = [
    ((65, 8, 0, 0, 1),        [0, 4, 4, 1, 1, 1, 1, 0]),       # 520 floats, 130 items: one workgroup
    ((65, 8, 0, 0, 0),        [1, 1, 4, 1, 1, 1, 1, 0]),       # ... off 16 bytes: 520 dwords
    ((3, 10, 2, 0, 1),        [1, 1, 4, 1, 1, 1, 1, 0]),       # 30 floats: no whole items
    ((1025, 4, 1, 0, 1),      [0, 4, 4, 2, 2, 1, 1, 0]),       # 1025 items: the second workgroup has one
    ((256, 16, 3, 0, 1),      [0, 4, 4, 1, 1, 1, 1, 0]),       # 1024 items: the last a workgroup holds
    ((3, 10, 2, 1, 1),        [3, 1, 4, 1, 1, 1, 1, 0]),       # Hc = 5: B's rows leave 16 bytes
    ((65, 8, 2, 1, 1),        [2, 4, 4, 1, 1, 1, 1, 0]),       # Hc = 4
    ((65, 8, 2, 1, 0),        [3, 1, 4, 1, 1, 1, 1, 0]),
    ((4, 6, 0, 1, 1),         [3, 1, 4, 1, 1, 1, 1, 0]),       # Hc = 3, T Hc = 12 a multiple of 4: the flat rule does not apply to a gated tensor
    ((8192, 4096, 2, 1, 1),   [2, 4, 4, 4096, 4096, 1, 1, 0]), # SwiGLU 8192 x 2 x 2048: 4 194 304 items
    ((25088, 768, 0, 0, 1),   [0, 4, 4, 4704, 4704, 1, 1, 0]), # ViT-tiny
    ((1, (1 << 31) - 1, 3, 0, 1), [1, 1, 4, 2097152, 2097152, 1, 1, 0]),   # the largest tensor
]


@pytest.mark.parametrize("args,want", ROWS, ids=["t%d_c%d_k%d_g%d_a%d" % r[0] for r in ROWS])
def test_hand_worked_rows(lib, args, want):
    assert plan(lib, *args) == (OK, want)


@pytest.mark.parametrize("args,code", [((0, 8, 0, 0, 1), ERR_ARG), ((-1, 8, 0, 0, 1), ERR_ARG), ((8, 0, 0, 0, 1), ERR_ARG), ((8, -2, 0, 0, 1), ERR_ARG),
                                       ((8, 8, 4, 0, 1), ERR_ARG), ((8, 8, -1, 0, 1), ERR_ARG), ((8, 8, 0, 2, 1), ERR_ARG), ((8, 8, 0, -1, 1), ERR_ARG),
                                       ((8, 7, 2, 1, 1), ERR_ARG), ((1 << 28, 8, 0, 0, 1), ERR_UNSUPPORTED), ((1 << 31, 1, 0, 0, 1), ERR_UNSUPPORTED),
                                       ((1 << 62, 4, 2, 1, 1), ERR_UNSUPPORTED)])
def test_rejections_leave_out_untouched(lib, args, code):
    assert plan(lib, *args) == (code, SENTINEL) and lib.t4k_last_error()
    assert lib.t4k_gateact_plan(8, 8, 0, 0, 1, None) == ERR_ARG


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_the_float64_rule_is_torchs(kind):
    a = torch.from_numpy(sweep(4096, kind).astype(np.float64)).requires_grad_(True)
    y = torch_f(kind, a)
    g, = torch.autograd.grad(y.sum(), a)
    f, d = reference(kind, a.detach())
    assert torch.isfinite(f).all() and torch.isfinite(d).all()
    assert (torch.abs(f - y.detach()) <= 1e-12 * (1.0 + torch.abs(f))).all() and (torch.abs(d - g) <= 1e-12 * (1.0 + torch.abs(d))).all()


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("gate", [0, 1])
def test_the_rounded_reference_is_inside_the_bound_at_k_1(kind, gate):
    X, DY = operands(gate, 2048, 2, 10 * kind + gate)
    for ref, cond, scale in rule(kind, gate, X, DY):
        with np.errstate(over="ignore"):
            r32 = ref.astype(np.float32)
        assert np.isfinite(r32).all() and (np.abs(r32.astype(np.float64) - ref) <= bound(1.0, ref, cond, scale)).all()
