"""One launch PLAN of the host (tests/test_gpu_geo_layer_plans.py starts this program once per plan, with the plan's T4_* switches in the environment -
host/model.cpp reads them when libten4.so is loaded): three nets of run-time-geometry layers (conv2d of any geometry, grouped conv2d, the vector form of
the pools, upsample of any factor and method) built on the product VM, stepped four times on the same input and target, every tensor written to one .npz.
usage: geo_plan_worker.py <out.npz>

The nets, their layer tables and the step protocol are this module's constants: the test imports them for its witnesses, tests/test_geo_layer_plans_oracle.py
builds the same texts on the CPU oracle VM.  Not a test module."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 3                                                                     # the batch of every net
NEAREST, LINEAR, BILINEAR, CUBIC = range(4)                               # T4K_UP_* of include/t4k.h
STEPS = 4                                                                 # with T4_GRAPH=1: call 1 eager, call 2 captured and launched, calls 3 and 4 replays
LR = 2.0 ** -10                                                           # nn.sgd, no momentum.  A power of two: a scalar cell of the VM gives up the last bit of
LR_TEXT = "0.0009765625"                                                  # its mantissa to the object tag (0.001 reaches the kernel one ulp short), this one loses nothing

# op kinds: ("conv", C1, C0, K, S, P, D, G)  ("pool", kind, K, S, P)  ("up", method, K)  ("relu",)  ("bn",)  ("flatten",)  ("linear", E1, E0)  ("softmax",)
NETS = {
    # the hourglass: a GROUPED layer 0 (the layer-0 copy, both dX0 plans and materialize_dx0 on t4k_conv2d_grp_*), a dense and a grouped run-time-geometry
    # layer inside (the forked and the single-stream backward on both entries), a max and an avg pool of the vector form, a bilinear and a bicubic upsample
    "A": dict(
        text="%d 12 12 8 nn.model 0.5 8 5 vector{ 3 1 1 1 8 } conv2d relu 3 vector{ 3 2 1 } maxpool 0.5 16 4 vector{ 3 1 2 2 } conv2d relu "
             "3 vector{ 2 2 0 } avgpool 2 2 upsample 0.5 16 5 vector{ 3 1 1 1 4 } conv2d 3 2 upsample 0.5 4 4 vector{ 3 2 1 1 } conv2d" % N,
        ops=[("conv", 8, 8, 3, 1, 1, 1, 8), ("relu",), ("pool", "max", 3, 2, 1), ("conv", 8, 16, 3, 1, 2, 2, 1), ("relu",), ("pool", "avg", 2, 2, 0),
             ("up", BILINEAR, 2), ("conv", 16, 16, 3, 1, 1, 1, 4), ("up", CUBIC, 2), ("conv", 16, 4, 3, 2, 1, 1, 1)],
        shapes=[(12, 12, 8), (12, 12, 8), (12, 12, 8), (6, 6, 8), (6, 6, 16), (6, 6, 16), (3, 3, 16), (6, 6, 16), (6, 6, 16), (12, 12, 16), (6, 6, 4)],
        opt=True, record=(1, 2, 4), frozen=True),
    # no parameters, a RECTANGULAR grid all the way: min pool, nearest x4 through the new entry, the linear method, an avg pool whose 16 x 16 window (the
    # largest admitted K) takes the padded 48 x 40 grid in 3 x 3 windows - the in-place dX chain with no convolution in between
    "B": dict(
        text="%d 6 5 8 nn.model 3 vector{ 3 1 1 } minpool 4 upsample 1 2 upsample 3 vector{ 16 16 4 } avgpool" % N,
        ops=[("pool", "min", 3, 1, 1), ("up", NEAREST, 4), ("up", LINEAR, 2), ("pool", "avg", 16, 16, 4)],
        shapes=[(6, 5, 8), (6, 5, 8), (24, 20, 8), (48, 40, 8), (3, 3, 8)],
        opt=False, record=(1, 4), frozen=False),
    # neighbours whose launches change with the plan: batch-norm behind the conv, linear + softmax (one launch fused, two apart; `out -= target` inside the linear
    # backward or apart), the flatten copy and the linear backward forked under the side stream
    "C": dict(
        text="%d 12 12 3 nn.model 0.5 8 4 vector{ 3 2 1 1 } conv2d 0.1 batchnorm relu 3 vector{ 3 2 1 } maxpool flatten 10 linear softmax" % N,
        ops=[("conv", 3, 8, 3, 2, 1, 1, 1), ("bn",), ("relu",), ("pool", "max", 3, 2, 1), ("flatten",), ("linear", 72, 10), ("softmax",)],
        shapes=[(12, 12, 3), (6, 6, 8), (6, 6, 8), (6, 6, 8), (3, 3, 8), (1, 72, 1), (1, 10, 1), (1, 10, 1)],
        opt=True, record=(1, 4), frozen=False),
}
# the layer table `network` prints, line for line (tests/test_geo_layer_plans_oracle.py holds the oracle VM to it, the worker the product VM)
TABLES = {
    "A": """NN Model[10/128]
[  0] conv2d : T4[3,12,12,8] #p=3616 T4[1,3,3,8] T1[8] T4[3,12,12,8] bias=0.5, C=8, K=3, S=1, P=1, G=8
[  1] relu   : T4[3,12,12,8] #p=3456 T4[3,12,12,8]@
[  2] maxpool: T4[3,12,12,8] #p=216 T4[3,6,6,2] 3x3, S=2, P=1
[  3] conv2d : T4[3,6,6,8] #p=3200 T4[8,3,3,16] T1[16] T4[3,6,6,8] bias=0.5, C=16, K=3, S=1, P=2, D=2
[  4] relu   : T4[3,6,6,16] #p=1728 T4[3,6,6,16]@
[  5] avgpool: T4[3,6,6,16] #p=0 2x2, S=2, P=0
[  6] upsampl: T4[3,3,3,16] #p=0 2x2 bilinear
[  7] conv2d : T4[3,6,6,16] #p=2912 T4[4,3,3,16] T1[16] T4[3,6,6,16] bias=0.5, C=16, K=3, S=1, P=1, G=4
[  8] upsampl: T4[3,6,6,16] #p=0 2x2 cubic
[  9] conv2d : T4[3,12,12,16] #p=8072 T4[16,3,3,4] T1[4] T4[3,12,12,16] bias=0.5, C=4, K=3, S=2, P=1
[ 10] output : T4[3,6,6,4] #p=0@
""",
    "B": """NN Model[4/128]
[  0] minpool: T4[3,6,5,8] #p=180 T4[3,6,5,2] 3x3, S=1, P=1
[  1] upsampl: T4[3,6,5,8] #p=0 4x4 nearest
[  2] upsampl: T4[3,24,20,8] #p=0 2x2 linear
[  3] avgpool: T4[3,48,40,8] #p=0 16x16, S=16, P=4
[  4] output : T4[3,3,3,8] #p=0@
""",
    "C": """NN Model[7/128]
[  0] conv2d : T4[3,12,12,3] #p=1744 T4[3,3,3,8] T1[8] T4[3,12,12,3] bias=0.5, C=8, K=3, S=2, P=1
[  1] batchnm: T4[3,6,6,8] #p=896 T1[8] T1[8] T4[3,6,6,8] mtum=0.1
[  2] relu   : T4[3,6,6,8] #p=864 T4[3,6,6,8]@
[  3] maxpool: T4[3,6,6,8] #p=54 T4[3,3,3,2] 3x3, S=2, P=1
[  4] flatten: T4[3,3,3,8] #p=0@
[  5] linear : T4[3,1,72,1] #p=1460 T4[1,10,72,1] T1[10] bias=1, H=10
[  6] softmax: T4[3,1,10,1] #p=10 T4[1,1,10,1]@
[  7] output : T4[3,1,10,1] #p=0@
""",
}
TABLES = {k: v.replace("@", " ") for k, v in TABLES.items()}           # (the printer's trailing blank, kept out of the source text)


def operand(rng, *shape):
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def params(name):
    """the ops of net `name` that hold parameters"""
    return [i for i, op in enumerate(NETS[name]["ops"]) if op[0] in ("conv", "bn", "linear")]


def check_table(name, txt):
    assert TABLES[name] in txt, (name, txt)


class Recorder:
    def __init__(self, vm, k):
        self.vm, self.k, self.out = vm, k, {}
        k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
        k.lib.t4k_conv_last_plan.restype = ctypes.c_char_p

    def ev(self, src):
        """a line of Forth whose text must report nothing; the kernels counted while it ran"""
        l0 = int(self.k.lib.t4k_launch_count())
        txt = self.vm.eval(src)
        assert "not supported" not in txt and "failed" not in txt and "error" not in txt and "wrong shape" not in txt, (src, txt)
        return int(self.k.lib.t4k_launch_count()) - l0

    def get(self, key, expr):
        self.out[key] = self.vm.fetch(expr).copy(); self.vm.eval("drop drop")

    def layers(self, name, tag):
        for i in range(len(NETS[name]["shapes"])):                       # layer 0 first: under the lazy plan this fetch has dX0 produced, as in the words tests
            self.get("%s.%s%d" % (name, tag, i), "net%s %d n@" % (name, i))

    def parms(self, name, tag, words):
        for i in params(name):
            for w in words:
                self.get("%s.%s.%s%d" % (name, tag, w, i), "net%s %d nn.%s" % (name, i, w))


def build(vm, name, rng):
    """net `name` as the constant net<name>; conv weights as `operand` draws, filters scaled by 1 / (K sqrt(Cg1)) so that the activations keep their size"""
    net = NETS[name]
    vm.eval(net["text"] + " constant net" + name)
    check_table(name, vm.eval("net%s network drop" % name))
    for i, op in enumerate(net["ops"]):
        if op[0] != "conv":
            continue
        _, C1, C0, K, S, P, D, G = op
        Cg1 = C1 // G
        F = operand(rng, Cg1, K, K, C0) / np.float32(K * np.sqrt(Cg1)); B = operand(rng, C0)
        vm.store(F, "net%s %d %d %d %d tensor" % (name, Cg1, K, K, C0)); out = vm.eval("%d nn.w=" % i)
        vm.store(B, "%d vector" % C0); out += vm.eval("%d nn.b= drop" % i)
        assert "?" not in out and "shape" not in out, out
    H, W, C = net["shapes"][0]
    X = operand(rng, N, H, W, C)
    vm.store(X, "%d %d %d %d tensor constant x%s x%s" % (N, H, W, C, name, name)); vm.eval("drop")
    h, w, c = net["shapes"][-1]
    if net["ops"][-1][0] == "softmax":                                   # cross entropy: one-hot rows
        T = np.zeros((N, h, w, c), np.float32); T[np.arange(N), 0, rng.integers(0, w, size=N), 0] = 1.0
    else:
        T = operand(rng, N, h, w, c)
    vm.store(T, "%d %d %d %d tensor constant t%s t%s" % (N, h, w, c, name, name)); vm.eval("drop")
    return X, T


def run_net(rec, name, rng):
    net, k = NETS[name], rec.k
    rec.out[name + ".x"], rec.out[name + ".t"] = build(rec.vm, name, rng)
    fwd, bwd, opt = "net%s x%s forward drop" % (name, name), "net%s t%s backprop drop" % (name, name), "net%s %s 0.0 nn.sgd drop" % (name, LR_TEXT)
    counts, plans = [], []
    for step in range(1, STEPS + 1):
        keep = step in net["record"]
        tag = "s%d" % step
        f = rec.ev(fwd)
        if keep:
            rec.layers(name, tag + ".a")
            for i, op in enumerate(net["ops"]):
                if op[0] in ("bn", "relu"):                              # x-hat, the mask
                    rec.get("%s.%s.ex%d" % (name, tag, i), "net%s %d nn.ex" % (name, i))
        b = rec.ev(bwd)
        plans.append(k.lib.t4k_conv_last_plan().decode())               # the last conv entry of the pass: layer 0's (read BEFORE a fetch has dX0 produced)
        if keep:
            rec.layers(name, tag + ".g")
            rec.parms(name, tag, ("dw", "db", "w", "b"))
        o = rec.ev(opt) if net["opt"] else 0
        if keep and net["opt"]:
            rec.parms(name, tag + ".new", ("w", "b"))
        counts.append((f, b, o))
    rec.out[name + ".launches"] = np.array(counts, np.int64)
    rec.out[name + ".last_plan"] = np.array(plans)
    if not net["frozen"]:
        return
    # a fifth pass without the optimizer (the gradients stay), then the same pass frozen
    f = rec.ev(fwd); b = rec.ev(bwd)
    rec.layers(name, "pre.g"); rec.parms(name, "pre", ("dw", "db"))
    rec.ev("net%s 0 trainable drop" % name)
    f0 = rec.ev(fwd); rec.layers(name, "frz.a")
    b0 = rec.ev(bwd); rec.layers(name, "frz.g"); rec.parms(name, "frz", ("dw", "db", "w", "b"))
    rec.out[name + ".frozen_launches"] = np.array([(f, b), (f0, b0)], np.int64)


def main():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tensorforth_amd import lib as t4lib
    from tensorforth_amd.vm import VM
    k = t4lib.load()
    vm = VM(device=0, seed=11)
    rec = Recorder(vm, k)
    rng = np.random.default_rng(2024)
    for name in ("A", "B", "C"):
        run_net(rec, name, rng)
    rc = k.lib.t4k_sync(None)
    if rc != 0:
        print("SYNC_ERROR %d %s" % (rc, k.lib.t4k_last_error().decode(errors="replace")), flush=True)
        return 3
    np.savez(sys.argv[1], **rec.out)
    vm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
