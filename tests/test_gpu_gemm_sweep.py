"""t4k_gemm at every rung of gemm_launch (tensorforth_amd/csrc/gemm.hip), with the rung asserted.

Every row of tests/gemm_cases.py names the plan it is meant to reach.  The plan is recomputed from the device's CU count with the Python
mirror of the ladder and the row FAILS when it no longer reaches its label; t4k_gemm_last_plan() must report the mirror's string and
t4k_launch_count() the mirror's launch count, for every (alpha, beta) a row runs.  A, B and O each sit inside a larger allocation with 256
NaN floats in front and behind (skewed-base rows: one float more in front): O's moat must be bit-identical after the call, A and B
entirely, and no NaN may appear in O - an element from outside an operand that reaches an MFMA, even times zero, shows as one.
  exact   operands in {-2 .. 2}, O0 in {-3 .. 3}: (1, 0) over an O prefilled with NaN (beta = 0 must not read O), (2, -1) on O0, (1, 0) again
          (tickets, flags and slabs were left clean) - each bit-equal to the float64 product (K <= 4096: every partial sum below 2^24);
  float   standard-normal operands, (0.5, 2.0): element by element inside f64_witness.gemm's bound c (K + 2) 2^-24 mag; a row whose kernel
          changes with the epilogue (nn_plain -> plain_any) also runs (1, 0) over NaN, so its own kernel sees float operands too."""
import ctypes
import time

import numpy as np
import pytest

import f64_witness as wt
import gemm_cases as gc
from test_gpu_parity import Dev, p

pytestmark = pytest.mark.gpu

ARG = -1                                                   # T4K_ERR_ARG (include/t4k.h)
EXACT_PASSES = ((1.0, 0.0, "nan"), (2.0, -1.0, "o0"), (1.0, 0.0, "keep"))
FLOAT_PASSES = ((0.5, 2.0, "o0"),)
CLOCK = {}


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    CLOCK["t0"] = time.time()
    return Dev(t4k)


def launches(t4k):
    return int(t4k.lib.t4k_launch_count())


def last_plan(t4k):
    return t4k.lib.t4k_gemm_last_plan().decode()


def cu_count(t4k):
    cu, khz, hbm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    t4k.call("t4k_device_info", ctypes.byref(cu), ctypes.byref(khz), ctypes.byref(hbm))
    assert cu.value > 0
    return cu.value


def entry_plan(t4k, r, a_ptr, b_ptr, alpha, beta, lane=0, capturing=False):
    """t4k_gemm_plan's text for the call as it was made: the device's CU count, the real alignment of A and B, the stream and capture state"""
    return gc.plan_entry(t4k.lib, r.M, r.N, r.K, r.C, r.tA, r.tB, gc.plan_flags(a_ptr, b_ptr, alpha, beta, lane, capturing), cu=cu_count(t4k))[0]


def call(t4k, name, *a):
    """t4k.call; a HIP error (a fault on the device) ends the session there: nothing more is started on a device that has faulted"""
    try:
        return t4k.call(name, *a)
    except Exception as e:
        if "(-2)" in str(e) or "illegal" in str(e):
            pytest.exit("%s: %s" % (name, e), returncode=3)
        raise


def free(dev):
    del dev.keep[:]; dev.torch.cuda.empty_cache()


class Buf:
    """a device tensor inside a larger allocation: gemm_cases.moated"""

    def __init__(self, dev, data, skew=0):
        self.dev, self.n = dev, int(np.asarray(data).size)
        self.img, self.k = gc.moated(data, skew)
        self.t = dev.up(self.img); assert p(self.t) % 16 == 0
        self.ptr = p(self.t) + 4 * self.k

    def put(self, data):
        self.img[self.k:self.k + self.n] = np.asarray(data, np.float32).ravel()
        self.t.copy_(self.dev.torch.from_numpy(self.img))

    def get(self, name, shape, stream=None):
        """the tensor as the device holds it, its moat checked bit for bit"""
        call(self.dev.h, "t4k_sync", stream)
        got = self.t.cpu().numpy()
        return gc.check_moat(name, got, self.k, self.n).reshape(shape).copy()

    def untouched(self, name):
        got = self.t.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), self.img.view(np.uint32)), "%s: an operand was written" % name


PRODUCTS = {}


def product(r, exact):
    """operands and float64 product of a row, computed once; the large ones are not kept"""
    key = (r.id, exact)
    if key not in PRODUCTS:
        A, B, O0 = gc.operands(r, exact)
        v = (A, B, O0, gc.Product(r, A, B))
        if r.M * r.N > (1 << 20):
            return v
        PRODUCTS[key] = v
    return PRODUCTS[key]


def run_row(t4k, dev, r, exact, passes=None, stream=None, lane=0, oskew=0, check_plan=True, want_label=None, tag=""):
    """the passes of one row on one set of buffers; returns the last O"""
    assert gc.exact_ok(r), r.id
    cu = cu_count(t4k)
    A, B, O0, prod = product(r, exact)
    shape = gc.shapes(r)[2]
    bA, bB, bO = Buf(dev, A, r.skew), Buf(dev, B, r.skew), Buf(dev, np.full(shape, np.nan, np.float32), oskew)
    dev.torch.cuda.synchronize()
    prev, got = None, None
    for i, (alpha, beta, fill) in enumerate(passes or (EXACT_PASSES if exact else FLOAT_PASSES)):
        name = "%s%s %s pass %d (%g, %g)" % (tag, r.id, "exact" if exact else "float", i, alpha, beta)
        if fill == "nan":
            bO.put(np.full(shape, np.nan, np.float32)); before = O0
        elif fill == "o0":
            bO.put(O0); before = O0
        else:
            before = prev
        dev.torch.cuda.synchronize()
        want, want_n = r.plan(cu, alpha=alpha, beta=beta, lane=lane)
        if check_plan and i == 0 and alpha == 1.0 and beta == 0.0:
            lab = r.label if want_label is None else want_label
            assert want == lab, "%s: with %d CUs this row takes the plan %s, not %s - resize the table (tests/gemm_cases.py)" % (r.id, cu, want, lab)
        l0 = launches(t4k)
        call(t4k, "t4k_gemm", bA.ptr, bB.ptr, bO.ptr, alpha, beta, r.tA, r.tB, r.M, r.N, r.K, r.C, stream)
        n, plan = launches(t4k) - l0, last_plan(t4k)
        assert entry_plan(t4k, r, bA.ptr, bB.ptr, alpha, beta, lane) == plan, "%s: t4k_gemm_plan() does not say what the launch did, %s" % (name, plan)
        if check_plan:
            assert plan == want, "%s: t4k_gemm_last_plan() says %s, the mirror %s" % (name, plan, want)
            assert n == want_n, "%s: %d launches, the plan %s makes %d" % (name, n, want, want_n)
        got = bO.get(name + " O", shape, stream)
        gc.hold(name, got, prod, alpha, beta, before, exact, plan)
        prev = got
    bA.untouched(r.id + " A"); bB.untouched(r.id + " B")
    return got


# ----------------------------------------------------------------------------- 1. every rung
@pytest.mark.parametrize("row", gc.ROWS, ids=[r.id for r in gc.ROWS])
def test_every_rung_exact_and_float(t4k, dev, row):
    run_row(t4k, dev, row, True)
    if row.label != "plain256" or row is gc.first("plain256"):         # the 4096^2 rows: one layout is enough in the float pass
        run_row(t4k, dev, row, False)
        cu = cu_count(t4k)
        if row.plan(cu)[0] != row.plan(cu, alpha=0.5, beta=2.0)[0]:    # the epilogue moves the row to another kernel (nn_plain -> plain_any):
            run_row(t4k, dev, row, False, passes=((1.0, 0.0, "nan"),))  # the row's own kernel on float operands too, over an O of NaN
    free(dev)


def test_the_drifted_parity_cases_take_the_rungs_the_mirror_says(t4k, dev):
    """shapes of test_gpu_parity.py whose comments named PAIR / k_gemm_plain256: what the hook reports for them (pytest -s prints it)"""
    cu = cu_count(t4k)
    for M, N, K, tA, tB, named, taken in gc.DRIFTED:
        r = gc.Row(taken, M, N, K, tA, tB, "drifted")
        A, B, O0 = gc.operands(r, True)
        bA, bB, bO = Buf(dev, A), Buf(dev, B), Buf(dev, O0)
        call(t4k, "t4k_gemm", bA.ptr, bB.ptr, bO.ptr, 1.0, 0.0, tA, tB, M, N, K, 1, None)
        plan = last_plan(t4k)
        print("drifted %dx%dx%d tA=%d tB=%d: named %s, t4k_gemm_last_plan() = %s" % (M, N, K, tA, tB, named, plan))
        assert plan == r.plan(cu)[0] and (cu != gc.CU or plan == taken) and plan != named
        call(t4k, "t4k_sync", None)
        free(dev)


# ----------------------------------------------------------------------------- 2. degenerate extents
def test_zero_extents(t4k, dev):
    """M = 0 or N = 0: OK, nothing launched, nothing written.  Negative extents and C = 0: T4K_ERR_ARG.  K = 0: O = alpha 0 + beta O on the
    fold kernel (no K-loop kernel is launched: the lean ones fetch their first stage before they look at the stage count), operands unread -
    A and B are handed over as the last float of a moat, so a single stage-0 fetch would run past the allocation's data"""
    SENT = np.float32(4242.5)
    one = Buf(dev, np.ones(4, np.float32))
    for M, N, K in ((0, 8, 8), (8, 0, 8), (0, 0, 0)):
        bO = Buf(dev, np.full(64, SENT))
        l0 = launches(t4k)
        t4k.call("t4k_gemm", one.ptr, one.ptr, bO.ptr, 1.0, 0.0, 0, 0, M, N, K, 1, None)
        assert launches(t4k) == l0 and last_plan(t4k) == "none"
        assert np.all(bO.get("empty product", 64) == SENT)
    bO = Buf(dev, np.full(64, SENT))
    for M, N, K, C in ((-1, 8, 8, 1), (8, -1, 8, 1), (8, 8, -1, 1), (8, 8, 8, 0), (8, 8, 8, -2)):
        l0 = launches(t4k)
        assert t4k.lib.t4k_gemm(one.ptr, one.ptr, bO.ptr, 1.0, 0.0, 0, 0, M, N, K, C, None) == ARG, (M, N, K, C)
        assert launches(t4k) == l0
    assert np.all(bO.get("refused product", 64) == SENT)
    for M, N, C, tA, tB in ((5, 7, 1, 0, 0), (64, 64, 1, 1, 1), (1536, 2048, 1, 0, 0), (9, 6, 3, 0, 1)):
        rng = np.random.default_rng(M + N + C)
        O0 = rng.integers(-3, 4, (M, N, C)).astype(np.float32)
        bO = Buf(dev, np.full(O0.shape, np.nan, np.float32))
        for alpha, beta, fill, want in ((1.0, 0.0, None, np.zeros_like(O0)), (2.0, -1.0, O0, -O0), (0.5, 2.0, O0, 2.0 * O0)):
            if fill is not None:
                bO.put(fill)
            dev.torch.cuda.synchronize()
            l0 = launches(t4k)
            t4k.call("t4k_gemm", one.ptr + 12, one.ptr + 12, bO.ptr, alpha, beta, tA, tB, M, N, 0, C, None)
            assert launches(t4k) - l0 == 1 and last_plan(t4k) == "k0" == gc.gemm_kernel_plan(M, N, 0, tA, tB, C)[0]
            wt.equal("K = 0, %dx%dx%d (%g, %g)" % (M, N, C, alpha, beta), bO.get("K = 0", O0.shape), want)
        free(dev)
    one.untouched("the one-float operand")


# ----------------------------------------------------------------------------- 3. streams and capture
def test_streams_and_capture(t4k, dev):
    """the pair row on a library stream takes split-K (tickets are the default stream's); a sliver row under capture takes the rung the
    mirror gives for capturing = True; both bit-equal to the default-stream result.  A captured (1, 1) split-K product replayed three times
    gives three times the product: the workspace slabs are rewritten by every replay.  Linear graphs on a private stream."""
    cu = cu_count(t4k)
    s = ctypes.c_void_p(); t4k.call("t4k_stream_create", ctypes.byref(s))
    try:
        r = gc.first("pair")
        ref = run_row(t4k, dev, r, True, passes=((1.0, 0.0, "nan"),))
        lab = r.plan(cu, lane=1)[0]
        assert "x" in lab and lab.endswith("+fold"), lab
        got = run_row(t4k, dev, r, True, passes=((1.0, 0.0, "nan"), (2.0, -1.0, "o0"), (1.0, 0.0, "keep")), stream=s, lane=1, want_label=lab, tag="library stream ")
        assert np.array_equal(got, ref)
        free(dev)
        for r in (gc.first("l32/w4"), gc.first("l32/w8"), gc.first("l32/w8/rst")):
            A, B, O0, prod = product(r, True)
            shape = gc.shapes(r)[2]
            ref = run_row(t4k, dev, r, True, passes=((1.0, 0.0, "nan"),))
            want, want_n = gc.gemm_kernel_plan(r.M, r.N, r.K, r.tA, r.tB, r.C, cu, lane=1, capturing=True)
            assert not want.startswith("l32"), want
            bA, bB, bO = Buf(dev, A), Buf(dev, B), Buf(dev, np.full(shape, np.nan, np.float32))
            dev.torch.cuda.synchronize()
            g = ctypes.c_void_p()
            t4k.call("t4k_graph_begin", s)
            l0 = launches(t4k)
            rc = t4k.lib.t4k_gemm(bA.ptr, bB.ptr, bO.ptr, 1.0, 0.0, r.tA, r.tB, r.M, r.N, r.K, r.C, s)
            n, plan = launches(t4k) - l0, last_plan(t4k)
            during = entry_plan(t4k, r, bA.ptr, bB.ptr, 1.0, 0.0, lane=1, capturing=True)
            t4k.call("t4k_graph_end", s, ctypes.byref(g))
            assert rc == 0 and plan == want and n == want_n, (r.id, rc, plan, want, n, want_n)
            assert during == plan and entry_plan(t4k, r, bA.ptr, bB.ptr, 1.0, 0.0, lane=1).startswith("l32"), (r.id, during, plan)   # the capture alone moved it
            t4k.call("t4k_graph_launch", g, s)
            got = bO.get(r.id + " captured", shape, s)
            gc.hold(r.id + " captured", got, prod, 1.0, 0.0, O0, True, "captured")
            assert np.array_equal(got, ref)
            t4k.call("t4k_graph_destroy", g)
            # (1, 1) replayed three times over zeros: 3 x the product
            bO.put(np.zeros(shape, np.float32)); dev.torch.cuda.synchronize()
            t4k.call("t4k_graph_begin", s)
            rc = t4k.lib.t4k_gemm(bA.ptr, bB.ptr, bO.ptr, 1.0, 1.0, r.tA, r.tB, r.M, r.N, r.K, r.C, s)
            t4k.call("t4k_graph_end", s, ctypes.byref(g))
            assert rc == 0
            for _ in range(3):
                t4k.call("t4k_graph_launch", g, s)
            got = bO.get(r.id + " replayed", shape, s)
            assert wt.is_int_exact(3 * r.K + 3, 4)
            wt.equal(r.id + " three replays of (1, 1)", got, 3.0 * prod.ex)
            t4k.call("t4k_graph_destroy", g)
            bA.untouched("A"); bB.untouched("B")
            free(dev)
    finally:
        t4k.call("t4k_stream_destroy", s)


# ----------------------------------------------------------------------------- 4. state between launches
B2B = ("l32/w8", "pair", "glds8<128>x4+fold", "glds8<64>x16+fold", "mfma<64,64,64,vec,skew>x14+fold", "mfma<64,64,32>x5+fold", "plain_any", "glds8<128,ragk>",
       "mfma<64,64,64,vec,skew>")


def test_rungs_back_to_back(t4k, dev):
    """one exact row of each family that owns tickets, flags, the zero block or the workspace, on one stream, in an order in which every one
    follows every other (a closed walk over all ordered pairs); every output checked, (1, 0) over NaN then (2, -1)"""
    reps = [gc.first(lab) for lab in B2B]
    walk = gc.euler_walk(len(reps))
    steps = set(zip(walk, walk[1:]))
    assert all((a, b) in steps for a in range(len(reps)) for b in range(len(reps)) if a != b)
    for n, i in enumerate(walk):
        run_row(t4k, dev, reps[i], True, passes=((1.0, 0.0, "nan"), (2.0, -1.0, "o0")))
        if n % 8 == 7:
            free(dev)
    free(dev)
    assert t4k.lib.t4k_sync(None) == 0


# ----------------------------------------------------------------------------- 5. O off its 16-byte boundary
SKEWED = ("l32/w4", "l32/w8/rst", "pair", "glds8<64>x2+fold", "nn_plain", "plain_ragk", "glds8<128>", "glds8<64,ragk>", "mfma<64,64,64,vec,skew>", "plain128",
          "plain128/bk32", "mfma<128,128,32,vec,full>")


@pytest.mark.parametrize("label", SKEWED)
def test_outputs_from_skewed_bases(t4k, dev, label):
    """O 4, then 8 bytes into its allocation: the dispatch looks at A and B alone, so plan and launch count stay; every kernel that stores
    16-byte vectors or rows of them must fall back or be right, the exact pass stays bit-equal and the moat intact"""
    r = gc.first(label)
    for off in (1, 2):
        run_row(t4k, dev, r, True, oskew=off, tag="O + %d bytes " % (4 * off))
    free(dev)


def test_zz_report_worst_ratios_and_wall_time():
    """the worst |error| / bound per kernel form over the float passes above, and the file's wall time (pytest -s prints both;
    tests/README.md quotes them)"""
    print("\nGEMM sweep, worst |err| / bound per kernel form:")
    for kind in sorted(k for k in wt.WORST if k.startswith("gemm:")):
        print("  %-40s %.3g   %s" % (kind, wt.WORST[kind][0], wt.WORST[kind][1]))
        assert wt.WORST[kind][0] <= 1.0
    print("GEMM sweep wall time: %.1f s" % (time.time() - CLOCK.get("t0", time.time())))
