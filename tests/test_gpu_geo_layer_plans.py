"""The run-time-geometry layers - conv2d of any geometry (t4k_conv2d_geo_*), grouped conv2d (t4k_conv2d_grp_*), the vector form of the pools (t4k_pool_geo_*),
upsample of any factor and method (t4k_upsample_*) - under every launch plan of host/model.cpp.  The plan switches (T4_FUSE, T4_GRAPH, T4_SIDE, T4_LAZY_DX0)
are read when libten4.so is loaded, so every plan is a child process of its own (tests/geo_plan_worker.py), one after the other: three nets stepped four
times on the same input and target, every tensor in an .npz.  tests/README.md ("The geometry layers under every launch plan") lists the branch of model.cpp
each plan and net reaches, the observables and the mutations tried.

  1. default plan: every output, dX, dF, dB of every layer at steps 1 and 4 inside the float64 witness bound of its own op on the operands the VM itself stored
     (f64_witness.py and the `witness` helpers of the four kernel test files; nothing is carried from layer to layer); the updated weights against
     w - lr dw / Nw in float64.
  2. nets A and B: every tensor of every other plan BIT-equal to the default child's, the captured and the replayed steps included.  Net C (neighbours that
     run other kernels when unfused): every plan held to (1); what one of the four families' entries wrote is bit-equal wherever its operands are.
  3. the plan was in force: launch counts and t4k_conv_last_plan(), per plan.
  4. frozen (`0 trainable`), default and side stream: no gradient tensor moves, every dX bit-equal to the trainable backprop's on the same operands.

A child that ends by a signal, an abort or its time limit, or whose output names a HIP fault, ends the series: no further child is started, and every test
that needs one fails with that child's output."""
import os
import subprocess
import sys

import numpy as np
import pytest

import f64_witness as fw
import geo_plan_worker as gw
from test_gpu_conv_geo import witness as geo_witness
from test_gpu_conv_grp import witness as grp_witness
from test_gpu_pool_geo import witness as pool_witness
from test_gpu_upsample import witness as up_witness
from vm_util import ROOT

pytestmark = pytest.mark.gpu

PLANS = [("default", {}), ("unfused", {"T4_FUSE": "0"}), ("hipgraph", {"T4_GRAPH": "1"}), ("sidestream", {"T4_SIDE": "1"}),
         ("graph+side", {"T4_SIDE": "1", "T4_GRAPH": "1", "T4_FUSE": "0"}), ("eager-dx0", {"T4_LAZY_DX0": "0"})]
IDS = [p for p, _ in PLANS]
SWITCHES = ("T4_FUSE", "T4_GRAPH", "T4_SIDE", "T4_LAZY_DX0", "T4_STACK", "T4_STACK_HEAD", "T4_HEAD_BWD", "T4_OPT_FOLD")
CHILD_LIMIT = 120                                                         # seconds; a child takes 2.0 .. 2.2 s on the MI355X (tests/README.md): VM start and module load vary
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorIllegal", "hipErrorLaunchFailure", "Aborted", "core dumped",
               "Segmentation fault")
SKIP_KEYS = (".launches", ".last_plan", ".frozen_launches")


class Run:
    def __init__(self, plan):
        self.plan, self.data, self.rc, self.tail, self.fatal, self.seconds = plan, None, None, "not started", False, 0.0


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """one child per plan, in the table's order, never two at a time; the series ends at the first child that faulted, aborted or ran into its limit"""
    import time
    d = tmp_path_factory.mktemp("geo_plans")
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    out, ended_by = {p: Run(p) for p in IDS}, None
    for plan, env in PLANS:
        r = out[plan]
        if ended_by:
            r.tail = "not started: the %s child ended the series\n%s" % (ended_by.plan, ended_by.tail)
            continue
        path = str(d / (plan.replace("+", "_") + ".npz"))
        t0 = time.time()
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "geo_plan_worker.py"), path], env=dict(base, **env), capture_output=True, text=True,
                               timeout=CHILD_LIMIT)
            r.rc, r.tail = p.returncode, p.stdout[-2000:] + p.stderr[-3000:]
        except subprocess.TimeoutExpired as e:
            r.rc, r.fatal = "time limit of %d s" % CHILD_LIMIT, True
            r.tail = "".join((x.decode(errors="replace") if isinstance(x, bytes) else x or "")[-2500:] for x in (e.stdout, e.stderr))
        r.seconds = time.time() - t0
        if isinstance(r.rc, int) and (r.rc < 0 or r.rc in (134, 139) or any(w in r.tail for w in FAULT_WORDS)):
            r.fatal = True
        if r.fatal:
            ended_by = r
        elif r.rc == 0:
            r.data = dict(np.load(path))
        print("geo plan child %-10s rc=%s %.1f s" % (plan, r.rc, r.seconds))
    return out


def need(runs, plan):
    r = runs[plan]
    assert r.data is not None, "the %s child gave no tensors (rc = %s):\n%s" % (plan, r.rc, r.tail)
    return r.data


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------- (1) one pass of one net against float64
def _bn_xhat_from_input(X, C):
    """x-hat = (x - mean) rstd with the statistics of X in float64: the stored mean and rstd lie within bn_stats's bounds bm, br of them, then the two roundings
    of bn_xhat - |err| <= |r| bm + |x - m| br + bm br + 2 u (|x - m| + bm)(|r| + br)"""
    wm, wr = fw.bn_stats(X)
    x = fw.f64(X).reshape(-1, C); m, r, bm, br = wm.exact, wr.exact, wm.bound(), wr.bound()
    d = np.abs(x - m)
    bound = np.abs(r) * bm + d * br + bm * br + 2.0 * fw.U * (d + bm) * (np.abs(r) + br)
    return fw.W((x - m) * r, bound / fw.U, 1, 1.0), wr


def _bn_dx(gamma, DY, XH, wr, s1w, s2w):
    """bn_dx with rstd, mean dy and mean dy x-hat in float64: the stored three lie within their own bounds br, b1, b2, which move dx by
    |dx| br / r + |k| b1 + |k| |xh| b2 on top of bn_dx's five roundings"""
    C = DY.shape[-1]
    w = fw.bn_dx(gamma, DY, XH, np.concatenate([wr.exact, s1w.exact, s2w.exact]))
    k = np.abs(wr.exact * fw.f64(gamma)); xh = np.abs(fw.f64(XH).reshape(-1, C))
    extra = np.abs(w.exact) * wr.bound() / wr.exact + k * s1w.bound() + k * xh * s2w.bound()
    return fw.W(w.exact, (1.01 * w.bound() + extra) / fw.U, 1, 1.0)


def check_pass(t4k, name, what, acts, grads, parm, target, train=True):
    """one forward + backprop of net `name`: acts / grads are the layer tensors after the two words, parm(word, i) the layer's parameter tensors as the pass
    read (w, b) and left (dw, db, the gradients zero before it) them, ex masks / x-hat.  Every tensor against the witness of its own op"""
    net = gw.NETS[name]
    ops, n = net["ops"], len(net["ops"])
    for i, s in enumerate(net["shapes"]):
        assert acts[i].shape == (gw.N,) + s and grads[i].shape == (gw.N,) + s, (what, i, acts[i].shape, grads[i].shape)
    last = grads[n]
    if ops[-1][0] == "softmax":                                           # cross entropy: out -= target, one rounding
        p = fw.f64(acts[n]); t = fw.f64(target)
        fw.check("%s dLoss" % what, last, fw.W(p - t, np.abs(p) + np.abs(t), 1, 1.0))
    else:
        assert same_bits(last, target), "%s: the loss derivative of an MSE net is the target" % what
    for i, op in enumerate(ops):
        tag = "%s op %d %s" % (what, i, op[0])
        I, O, dY, dX = acts[i], acts[i + 1], grads[i + 1], grads[i]
        if op[0] == "conv":
            _, C1, C0, K, S, P, D, G = op
            F, B = parm("w", i), parm("b", i).ravel()
            assert F.shape == (C1 // G, K, K, C0), (tag, F.shape)
            a = dict(I=I, F=F, B=B, G=dY, DF0=np.zeros_like(F), DB0=np.zeros_like(B))
            wo, wdx, wdf, wdb = grp_witness("float", a, K, S, P, D, G) if G > 1 else geo_witness("float", a, K, S, P, D)
            fw.check(tag + " O", O, wo); fw.check(tag + " dX", dX, wdx)
            if train:
                fw.check(tag + " dF", parm("dw", i), wdf); fw.check(tag + " dB", parm("db", i), wdb)
        elif op[0] == "pool":
            _, kind, K, S, P = op
            wo, wdx, _ = pool_witness(kind, "float", I, dY, K, S, P)
            fw.check(tag + " O", O, wo); fw.check(tag + " dX", dX, wdx)
        elif op[0] == "up":
            wo, wdx, _ = up_witness(t4k, op[1], op[2], I, dY, "float")
            fw.check(tag + " O", O, wo); fw.check(tag + " dX", dX, wdx)
        elif op[0] == "relu":
            mask = (I > 0).astype(np.float32)
            ex = parm("ex", i)
            assert ex is None or same_bits(ex, mask), tag + " mask"
            assert same_bits(O, np.maximum(I, 0)), tag + " O"
            fw.check(tag + " dX", dX, fw.mul(dY, mask))
        elif op[0] == "flatten":
            assert same_bits(O.ravel(), I.ravel()) and same_bits(dX.ravel(), dY.ravel()), tag
        elif op[0] == "softmax":
            fw.check(tag + " O", O.reshape(gw.N, -1), fw.softmax(I.reshape(gw.N, -1)))
            assert same_bits(dX, dY), tag + " passes dY through"
        elif op[0] == "linear":
            _, E1, E0 = op
            Wt, B = parm("w", i).reshape(E0, E1), parm("b", i).ravel()
            x, dy = I.reshape(gw.N, E1), dY.reshape(gw.N, E0)
            fw.check(tag + " O", O.reshape(gw.N, E0), fw.linear(x, Wt, B))
            fw.check(tag + " dX", dX.reshape(gw.N, E1), fw.gemm(dy, Wt))
            if train:
                fw.check(tag + " dW", parm("dw", i).reshape(E0, E1), fw.gemm(dy, x, tA=1))
                fw.check(tag + " dB", parm("db", i).ravel(), fw.dlinear_db(dy, np.zeros(E0, np.float32)))
        elif op[0] == "bn":
            C = I.shape[-1]
            gamma, beta, XH = parm("w", i).ravel(), parm("b", i).ravel(), parm("ex", i)
            wxh, wr = _bn_xhat_from_input(I, C)
            fw.check(tag + " x-hat", XH.reshape(-1, C), wxh)
            fw.check(tag + " O", O.reshape(-1, C), fw.bn_y(XH, gamma, beta))
            s1w, s2w, wdw, wdb = fw.bn_bwd_stats(dY, XH, np.zeros(C, np.float32), np.zeros(C, np.float32), 1 if train else 0)
            if train:
                fw.check(tag + " dW", parm("dw", i).ravel(), wdw); fw.check(tag + " dB", parm("db", i).ravel(), wdb)
            fw.check(tag + " dX", dX.reshape(-1, C), _bn_dx(gamma, dY, XH, wr, s1w, s2w))
        else:
            raise AssertionError(op)


def check_update(name, what, D, step):
    """nn.sgd without momentum, optim.hip sgd1 spelled out as the reference writes it: d = dw / Nw (Nw = the parameter tensor's N), w' = w - lr d - a quotient,
    a product and a difference, ONE fp32 rounding each.  Against float64 on the fetched tensors: inside f64_witness.sgd's bound (those three roundings of
    |w| + |lr d|), and bit-equal to the three operations carried out in IEEE fp32 - which pins every bit, so no looser figure is left to assert.  (A bound of
    one unit in the last place of the float64 RESULT is not what three rounded operations give where |lr d| is large beside |w'|: on `10 linear`'s small
    weights the fp32 evaluation of the reference's own expression lies up to 4 ulps of w' from it.)"""
    lr32 = np.float32(gw.LR)
    for i in gw.params(name):
        for w, dw in (("w", "dw"), ("b", "db")):
            g, dg, new = (D["%s.s%d.%s%d" % (name, step, k, i)] for k in (w, dw, "new." + w))
            Nw = g.shape[0] if g.ndim == 4 else 1
            tag = "%s step %d layer %d %s" % (what, step, i, w)
            wit = fw.sgd(g, dg, None, Nw, gw.LR, 0.0)[0]
            fw.check(tag, new, wit)
            assert same_bits(new, g - lr32 * (dg / np.float32(Nw))), tag + ": not the fp32 evaluation of w - lr (dw / Nw)"


def step_pass(t4k, name, what, D, step, train=True):
    n = len(gw.NETS[name]["shapes"])
    acts = [D["%s.s%d.a%d" % (name, step, i)] for i in range(n)]
    grads = [D["%s.s%d.g%d" % (name, step, i)] for i in range(n)]
    assert same_bits(acts[0], D[name + ".x"]), "%s: layer 0 holds the batch" % what
    check_pass(t4k, name, "%s step %d" % (what, step), acts, grads, lambda w, i: D.get("%s.s%d.%s%d" % (name, step, w, i)), D[name + ".t"], train)


# ----------------------------------------------------------------------------- the tests
def test_children_ran(runs):
    for plan in IDS:
        r = runs[plan]
        assert r.rc == 0 and r.data is not None, "%s: rc = %s\n%s" % (plan, r.rc, r.tail)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_default_plan_against_float64(runs, t4k, name):
    D = need(runs, "default")
    for step in (1, 4):
        step_pass(t4k, name, "default " + name, D, step)
        if gw.NETS[name]["opt"]:
            check_update(name, "default " + name, D, step)


def test_default_plan_steps_differ(runs):
    """the four steps are no copies of each other: the weights move, and so does every tensor behind them (a replay that ran on stale operands would show)"""
    D = need(runs, "default")
    for name in ("A", "C"):
        last = len(gw.NETS[name]["shapes"]) - 1
        assert not same_bits(D["%s.s1.a%d" % (name, last)], D["%s.s4.a%d" % (name, last)]), name
        assert not same_bits(D["%s.s1.w0" % name], D["%s.s4.w0" % name]), name
    assert not same_bits(D["A.s1.a10"], D["A.s2.a10"])


@pytest.mark.parametrize("plan", IDS[1:])
def test_plans_agree_bit_for_bit_on_nets_a_and_b(runs, plan):
    D0, D = need(runs, "default"), need(runs, plan)
    keys = sorted(k for k in D0 if k[0] in "AB" and not k.endswith(SKIP_KEYS))
    assert len(keys) > 150 and all(k in D for k in keys), [k for k in keys if k not in D]
    bad = [k for k in keys if not same_bits(D0[k], D[k])]
    assert not bad, "%s: %d of %d tensors differ from the default plan's: %s" % (plan, len(bad), len(keys), bad[:12])


@pytest.mark.parametrize("plan", IDS[1:])
def test_net_c_under_every_plan(runs, t4k, plan):
    D0, D = need(runs, "default"), need(runs, plan)
    for step in (1, 4):
        step_pass(t4k, "C", plan + " C", D, step)
        check_update("C", plan + " C", D, step)
        # what the geometry entries wrote: (tensor, its operands); bit-equal to the default child's wherever the operands are
        k = lambda s: "C.s%d.%s" % (step, s)
        for out, operands in ((k("a1"), (k("a0"), k("w0"), k("b0"))), (k("g0"), (k("g1"), k("w0"))), (k("dw0"), (k("a0"), k("g1"))), (k("db0"), (k("g1"),)),
                              (k("a4"), (k("a3"),)), (k("g3"), (k("g4"), k("a3")))):
            if all(same_bits(D0[o], D[o]) for o in operands):
                assert same_bits(D0[out], D[out]), "%s: %s differs from the default plan's on bit-equal operands" % (plan, out)
    assert same_bits(D0["C.s1.a1"], D["C.s1.a1"])                        # step 1's conv operands are the worker's own draws, equal in every child: the condition above held


def _launches(D, name):
    return D[name + ".launches"]                                          # [step, (forward, backprop, optimizer)]


def test_default_plan_is_the_lazy_fused_one(runs):
    D = need(runs, "default")
    for p in D["A.last_plan"]:                                            # layer 0's backward is dF | dB alone; dX0 waits for a word that asks
        assert p.startswith("grp_dfx") and "grp_dx" not in p, p
    for name in ("A", "B", "C"):                                          # every eager step launches what the one before launched (the first forward also builds the gradient slab)
        L = _launches(D, name)
        assert np.all(L[1:] == L[1]) and np.all(L[0, 1:] == L[1, 1:]) and L[0, 0] >= L[1, 0], (name, L)


@pytest.mark.parametrize("plan", IDS[1:])
def test_the_plan_was_in_force(runs, plan):
    D0, D = need(runs, "default"), need(runs, plan)
    A0, A, C0, C = _launches(D0, "A"), _launches(D, "A"), _launches(D0, "C"), _launches(D, "C")
    if plan in ("hipgraph", "graph+side"):                                # t4k_graph_launch goes past the launch counter (runtime.hip): a replayed word counts no kernel
        for name in ("A", "B", "C"):
            L, L0 = _launches(D, name), _launches(D0, name)
            words = 3 if gw.NETS[name]["opt"] else 2
            assert np.all(L[0, :words] > 0) and np.all(L[2:, :words] < L[0, :words]) and np.all(L[2:, :words] < L0[3, :words]), (plan, name, L, L0)
        for p in D["A.last_plan"][:2]:                                    # no lazy dX0 under graphs: the eager and the captured call run layer 0's dX
            assert "grp_dx" in p, p
    if plan == "unfused":                                                 # linear and softmax apart, `out -= target` apart, the layer-0 copy a kernel
        assert np.all(C.sum(1) > C0.sum(1)), (C, C0)
        assert np.all(A[:, 0] == A0[:, 0] + 1), (A, A0)
    if plan in ("sidestream", "graph+side"):                              # dF | dB and dX are calls of their own, the `in = dX` copies are kernels
        assert A[0, 1] > A0[0, 1] + 4, (A, A0)
        for p in D["A.last_plan"][:1 if plan == "graph+side" else None]:  # layer 0's last entry is the dX call on the main stream: no dF token
            assert "dfx" not in p and "fold" not in p and p.startswith("grp_dx"), p
    if plan == "eager-dx0":                                               # layer 0's dX inside backprop: one kernel more than the lazy plan, before any fetch
        assert np.all(A[:, 1] == A0[:, 1] + 1) and np.all(A[:, 0] == A0[:, 0]) and np.all(C[:, 1] == C0[:, 1] + 1), (A, A0, C, C0)
        for p in D["A.last_plan"]:
            assert p.startswith("grp_dfx") and "grp_dx" in p, p


@pytest.mark.parametrize("plan", ["default", "sidestream"])
def test_frozen_model(runs, t4k, plan):
    D = need(runs, plan)
    n = len(gw.NETS["A"]["shapes"])
    moved = 0
    for i in gw.params("A"):
        for w in ("dw", "db"):
            assert same_bits(D["A.pre.%s%d" % (w, i)], D["A.frz.%s%d" % (w, i)]), "%s: layer %d %s moved under `0 trainable`" % (plan, i, w)
            moved += int(np.count_nonzero(D["A.pre.%s%d" % (w, i)]))
        for w in ("w", "b"):
            assert same_bits(D["A.frz.%s%d" % (w, i)], D["A.s4.new.%s%d" % (w, i)]), (plan, i, w)
    assert moved > 1000                                                   # the trainable pass in front left gradients to keep
    acts = [D["A.frz.a%d" % i] for i in range(n)]
    grads = [D["A.frz.g%d" % i] for i in range(n)]
    for i in range(n):                                                    # same weights, same batch, same target: the trainable backprop's dX, bit for bit
        assert same_bits(grads[i], D["A.pre.g%d" % i]), "%s: frozen dX of layer %d differs from the trainable backprop's" % (plan, i)
    check_pass(t4k, "A", plan + " frozen A", acts, grads, lambda w, i: D.get("A.frz.%s%d" % (w, i)), D["A.t"], train=False)
    (f1, b1), (f0, b0) = D["A.frozen_launches"]
    assert f0 == f1 and b0 < b1, "the frozen backprop launches no dF | dB: %s" % (D["A.frozen_launches"],)
