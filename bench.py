#!/usr/bin/env python3
"""bench.py - headline benchmark of the MI355X tensorForth backend (contract in the task brief).

One "step" = one CNN training step (copy-in + forward + backprop + SGD, reference words
`forward backprop 0.01 nn.sgd`) of the LeNet-style `nn_f` network (examples/t4_30e.4th:19-23)
on a synthetic, HBM-resident 28x28x1 batch of 128 images PER GPU, through libt4hip.so.
With --gpus N the batch is sharded by sample (N x 128, weak scaling) and the gradient slab is
all-reduced (SUM) over RCCL before the optimizer kernel.

A plain run sets up, warms up, times --steps steps and prints the line; `roofline_step` carries the
HBM roofline of the CNN step.  --dump-outputs DIR writes what the last timed step computed (see
dump_outputs).  Everything else needs --full: the run then also times the 1024x1024x1024 fp32
`matmul` kernel (BASELINE config #2) with HIP events and reports it against the fp32 MFMA peak in
`roofline`, runs the sustained loop and the extras (GAN, batch 1024, t4_40a, CIFAR, dataset feed,
first-layer dX on demand, data-parallel overhead), and `cpu_baseline` is the CPU oracle timed on
this box's cores.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BASELINE_METRIC = 'CNN train images/sec + fp32 GEMM TFLOP/s (% MI355X MFMA peak), 1→8 GPUs'    # BASELINE.json "metric"
PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: 256 CU x 2.4 GHz x 256 FLOP/clk/CU
PEAK_HBM_GBS = 8000.0            # spec; ~6300 achievable


def measured_traffic():
    """HBM-side bytes per launch / per step from the LATEST counter pass under profiles/ (profiles/rNN_bench_traffic.json, written by
    tools/profile_bench.sh -> tools/traffic_json.py from the TCC_EA0 request counters of a separate --pmc run of this very command, reads
    x2-corrected on gfx950).  Nothing is pasted by hand: no file -> `traffic` is null."""
    import glob
    fs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_traffic.json")))
    if not fs:
        return None, None, None
    try:
        with open(fs[-1]) as f:
            d = json.load(f)
        return d.get("gemm_bytes_per_launch"), d.get("step_bytes"), "profiles/" + os.path.basename(fs[-1]) + " (" + d.get("source", "") + ")"
    except Exception:
        return None, None, None


# algorithmic bytes per image and parameter count (SURVEY.md 8d / BASELINE.md 3)
NETS = {"nn_f": dict(bytes_per_img=494720, params=101030, flop_per_img=3134160),
        "nn_c": dict(bytes_per_img=294800, params=197210, flop_per_img=1605360)}
# the layers of each net that hold parameters (nn.w / nn.b), by index in NET_WORDS
PARAM_LAYERS = {"nn_f": (0, 3, 8, 10), "nn_c": (0, 4, 6)}


def dump_outputs(vm, net, d):
    """What the timed path hands its caller after its last step, one float32 .npy per array under `d`: every parameter tensor of
    the net after the last nn.sgd (l<layer>_w, l<layer>_b) and the output layer's tensor as the step left it (`output`; the
    reference's backprop writes its loss derivative there in place): under 1 MB of parameters plus 40 B per image.  The net sits
    on the VM's stack; every fetch pushes it again and drops both."""
    import numpy as np
    arrays = {}
    for L in PARAM_LAYERS[net]:
        for kind in ("w", "b"):
            arrays["l%d_%s" % (L, kind)] = vm.fetch("net %d nn.%s" % (L, kind)); vm.eval("drop drop")
    arrays["output"] = vm.fetch("net -1 n@"); vm.eval("drop drop")
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a, np.float32))


def dry_run(rank, world, args):
    """The N-rank plumbing without a GPU: gloo rendezvous on 127.0.0.1, the bench contract's barrier and MAX-over-ranks time
    reduction, one JSON line from rank 0 with n_gpus = ranks that really joined.  No metric is measured (`value` is null)."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=pg_timeout())
    dist.barrier()
    ones = torch.ones(1); dist.all_reduce(ones, op=dist.ReduceOp.SUM)             # "negotiation": who is there
    if os.environ.get("T4_BENCH_TEST_DIE_RANK") == str(rank):                    # test hook (tests/test_bench_launch.py): a rank that dies behind the negotiation
        os._exit(7)
    t0 = time.perf_counter(); dist.barrier(); dt = time.perf_counter() - t0
    tmax = torch.tensor([dt]); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    all_alive(dist, torch, world, None)                                          # a line is printed only by a job whose ranks are ALL still there
    if rank == 0:
        print(json.dumps({"metric": BASELINE_METRIC, "value": None, "unit": "images/s", "n_gpus": int(ones.item()), "steps": 0, "warmup": 0,
                          "dry_run": True, "config": {"workload": "launch / rendezvous / reduction plumbing only", "parallelism": "dp%d" % world,
                                                      "allreduce": "gloo"}}), flush=True)
    dist.barrier(); dist.destroy_process_group()
    return 0


def pg_timeout():
    """Bound of every torch.distributed collective of the bench (T4_BENCH_PG_TIMEOUT_S, default 600 s): a rank that dies behind the rendezvous makes the
    survivors' next collective fail - they exit non-zero instead of waiting for the default 30 minutes (VERDICT r5 #9c)."""
    import datetime
    return datetime.timedelta(seconds=float(os.environ.get("T4_BENCH_PG_TIMEOUT_S", "600")))


def all_alive(dist, torch, world, device):
    """Every rank answers, or the caller dies with the collective's error (non-zero exit, no JSON line)."""
    t = torch.ones(1, device=device) if device is not None else torch.ones(1)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    if int(round(float(t.item()))) != world:
        raise SystemExit("bench: %d of %d ranks alive at the end of the run" % (int(round(float(t.item()))), world))


def cpu_workers(mode_args, n_workers, timeout=120):
    """Run n_workers copies of oracle/cpu_baseline.py side by side (plain subprocesses: this process holds a HIP runtime and must
    not fork); returns their parsed stdout lines."""
    import subprocess
    script = os.path.join(ROOT, "oracle", "cpu_baseline.py")
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, script] + [str(a) for a in mode_args], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, text=True)
             for _ in range(n_workers)]
    out = []
    for p_ in procs:
        try:
            o, _ = p_.communicate(timeout=timeout)
            out.append([float(x) for x in o.split()])
        except Exception:
            p_.kill()
    return [o for o in out if o]


GAN_SRC = """0 trace
256 constant N
N 1 1 1 tensor ones  constant REAL
N 1 1 1 tensor zeros constant FAKE
N 28 28 1 nn.model 512 linear 0.2 leakyrelu 0.3 dropout 256 linear 0.2 leakyrelu 0.3 dropout 1 linear sigmoid constant D
N 128 1 1 nn.model 256 linear 0.2 leakyrelu 512 linear 0.2 leakyrelu 784 linear tanh constant G
N 28 28 1 tensor rand constant real
N 128 1 1 tensor randn constant Z
: F ( -- t4 ) G Z forward -1 n@ N 28 28 1 reshape4 swap drop ;
: train_d ( D -- D ) 1 trainable real forward REAL backprop F forward FAKE backprop 0.0001 0.5 nn.adam ;
: train_g ( D -- D ) 0 trainable F forward REAL backprop 0 n@ G swap backprop 0.0004 0.5 nn.adam drop ;
: rounds ( D n -- D ) 1- for train_d train_g next ;
D 20 rounds real forward REAL loss.bce drop
"""


def gan_round_bytes(n=256):
    """Algorithmic HBM bytes of one `train_d train_g` round of the t4_40b nets (examples/t4_40b.4th), by the rule of SURVEY 8(d): every
    layer-boundary tensor written once and read once per pass (8 B per activation element forward, 8 B backward), every derivative /
    dropout mask written forward and read backward (8 B), parameters read once per pass they take part in (4 B), dW|dB read-modify-write
    when the net trains (8 B), Adam 7 floats per parameter (w rw, dw r + zero, m rw, v rw)."""
    D = [(784, 512, "ld"), (512, 256, "ld"), (256, 1, "s")]      # l = leakyrelu mask, d = dropout mask, s = sigmoid (pass-through)
    G = [(128, 256, "l"), (256, 512, "l"), (512, 784, "t")]

    def acts(net):
        a = net[0][0]; m = 0
        for _i, o, k in net:
            a += o * (1 + len(k)); m += o * sum(1 for c in k if c in "ldt")
        return a, m

    def params(net):
        return sum(i * o + o for i, o, _k in net)
    aD, mD = acts(D); aG, mG = acts(G); pD, pG = params(D), params(G)
    fwd = lambda a, m, p_: 4 * (n * (2 * a + m) + p_)
    bwd = lambda a, m, p_, train: 4 * (n * (2 * a + m) + p_ + (2 * p_ if train else 0))
    train_d = fwd(aD, mD, pD) + bwd(aD, mD, pD, True) + fwd(aG, mG, pG) + fwd(aD, mD, pD) + bwd(aD, mD, pD, True) + 28 * pD
    train_g = fwd(aG, mG, pG) + fwd(aD, mD, pD) + bwd(aD, mD, pD, False) + bwd(aG, mG, pG, True) + 28 * pG
    flops = 2 * n * (sum(i * o for i, o, _ in D) * (3 + 3 + 2) + sum(i * o for i, o, _ in G) * (1 + 3))   # GEMMs per weight matrix: D (fwd + dW + dX) x 2 in train_d, fwd + dX in train_g; G fwd in train_d, fwd + dW + dX in train_g
    return train_d + train_g, flops


def extras(vm_cls, local, ms_step, args, torch):
    """BASELINE configs #3 (sustained), #4 (GAN) and the dataset-fed step, all device-synchronised; rank 0 of a 1-GPU run only."""
    import subprocess
    import tempfile
    out = {}
    # The extras run on the product's DEFAULT launch plan (first layer's dX on demand), as in every earlier round - only the headline loop above and `gan_round_eager_ms`
    # below store it every step.  The switch is process-wide (ten4_set_lazy_dx0) and read at every backprop.
    from tensorforth_amd import vm as t4vm
    headline_plan = t4vm.set_lazy_dx0(1)
    out["extras_plan"] = "product default (first layer's dX on demand, T4_LAZY_DX0=1); the headline loop ran with T4_LAZY_DX0=%d" % headline_plan
    # ---- config #4: t4_40b GAN nets, N = 256, Adam beta1 = 0.5 (tools/forth/gan_steps.4th), one `train_d train_g` round
    g = vm_cls(device=local, seed=4321)
    txt = g.eval(GAN_SRC)
    assert "?" not in txt.replace("-> ok", ""), txt
    torch.cuda.synchronize()
    rounds = 300
    t0 = time.perf_counter(); g.eval("%d rounds real forward REAL loss.bce drop\n" % rounds); torch.cuda.synchronize()     # the loss read-back is a device sync as well
    gdt = (time.perf_counter() - t0) / rounds
    gb, gf = gan_round_bytes(256)
    out["gan_round_ms"] = round(gdt * 1e3, 4)
    out["gan"] = {"workload": "examples/t4_40b.4th nets (D 784-512-256-1 leakyrelu+dropout+sigmoid, G 128-256-512-784 leakyrelu+tanh), N=256, BCE, Adam b1=0.5, one train_d + train_g round, HBM-resident batch",
                  "rounds_timed": rounds, "algorithmic_bytes_per_round": gb, "hbm_frac": round(gb / gdt / 1e9 / PEAK_HBM_GBS, 5),
                  "flop_per_round": gf, "mfma_frac": round(gf / gdt / 1e12 / PEAK_F32_MFMA_TFLOPS, 5)}
    g.close()
    # the same round with every layer's dX stored every step, the generator's and the discriminator's first layers included (the reference's work)
    t4vm.set_lazy_dx0(0)
    g = vm_cls(device=local, seed=4321)
    txt = g.eval(GAN_SRC)
    assert "?" not in txt.replace("-> ok", ""), txt
    torch.cuda.synchronize()
    t0 = time.perf_counter(); g.eval("%d rounds real forward REAL loss.bce drop\n" % rounds); torch.cuda.synchronize()
    out["gan_round_eager_ms"] = round((time.perf_counter() - t0) / rounds * 1e3, 4)
    g.close()
    t4vm.set_lazy_dx0(1)
    # ---- config #5's strong-scaling denominator: the same net at batch 1024 on ONE GPU (8 x 128 sharded is the weak-scaling line above)
    b = vm_cls(device=local, seed=1234)
    txt = b.eval("0 trace\n1024 28 28 1 nn.model 0.5 10 conv2d 2 maxpool relu 0.5 20 conv2d 0.5 dropout 2 maxpool relu flatten 100 linear 0.5 dropout 10 linear softmax constant net\n"
                 "1024 28 28 1 tensor rand constant img\n: hot ( T -- T ) 1024 0 do 1 i 10 * i 7 * 10 mod + t! loop ;\n10240 vector zeros hot 1024 1 10 1 reshape4 constant lbl\n"
                 ": steps ( N n -- N ) 1- for img forward lbl backprop 0.01 0.0 nn.sgd next ;\nnet 5 steps\n")
    assert "?" not in txt.replace("-> ok", ""), txt
    torch.cuda.synchronize()
    t0 = time.perf_counter(); b.eval("100 steps\n"); torch.cuda.synchronize()
    out["batch1024_1gpu_ms_per_step"] = round((time.perf_counter() - t0) / 100 * 1e3, 4)
    b.close()
    # ---- the net BASELINE config #4 names literally (examples/t4_40a.4th:10-13 `nn_c`: conv10-pool-relu-flatten-lin100-relu-lin10-softmax, N = 256, nn.adam):
    # single-stage conv stack with the classifier head inside its forward, HBM-resident batch (its TensorBoard words are not part of the step)
    c = vm_cls(device=local, seed=40)
    txt = c.eval("0 trace\n256 28 28 1 nn.model 0.5 10 conv2d 2 maxpool relu flatten 100 linear relu 10 linear softmax constant net\n"
                 "256 28 28 1 tensor rand constant img\n: hot ( T -- T ) 256 0 do 1 i 10 * i 7 * 10 mod + t! loop ;\n2560 vector zeros hot 256 1 10 1 reshape4 constant lbl\n"
                 ": steps ( N n -- N ) 1- for img forward lbl backprop 0.001 nn.adam next ;\nnet 5 steps\n")
    assert "?" not in txt.replace("-> ok", ""), txt
    torch.cuda.synchronize()
    t0 = time.perf_counter(); c.eval("200 steps\n"); torch.cuda.synchronize()
    out["t4_40a_net_ms_per_step"] = round((time.perf_counter() - t0) / 200 * 1e3, 4)
    c.close()
    # ---- the reference's t4_42a-style CIFAR net (3 x [conv3x3 + batchnorm + relu + maxpool + dropout] + linear head, N = 256, AdamW) - the words of
    # tools/forth/cifar_steps.4th, HBM-resident synthetic batch; bytes / FLOP by SURVEY 8(d)'s rule (tools/cifar_roofline.py).  The reference quotes sec / epoch
    # for this net (examples/t4_42a.4th:49); here it is a per-step figure under the driver's clock.
    try:
        cf = vm_cls(device=local, seed=42)
        src = open(os.path.join(ROOT, "tools", "forth", "cifar_steps.4th")).read().split("net 5 steps")[0]
        txt = cf.eval(src + "net 5 steps\n")
        assert "?" not in txt.replace("-> ok", ""), txt
        torch.cuda.synchronize()
        nst = 60
        t0 = time.perf_counter(); cf.eval("%d steps\n" % nst); torch.cuda.synchronize()
        cms = (time.perf_counter() - t0) / nst * 1e3
        cf.close()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cifar_roofline.py"), "%.5f" % cms], capture_output=True, text=True, timeout=60)
        cr = json.loads(r.stdout.strip().splitlines()[-1])
        out["cifar_step_ms"] = round(cms, 4)
        out["cifar"] = {"workload": cr["workload"], "steps_timed": nst, "images_per_s": round(256 / (cms * 1e-3), 1), "algorithmic_bytes_per_step": cr["algorithmic_bytes_per_step"],
                        "flop_per_step": cr["flop_per_step"], "bound": cr["bound"], "mfma_frac": cr["mfma_frac"], "hbm_frac": cr["hbm_frac"]}
    except Exception as ex:                                      # never lose the main line over an extra
        out["cifar_note"] = "cifar leg failed: %r" % (ex,)
    # ---- the product's DEFAULT plan: the same timed loop with the first layer's dX left to the first word that reads it (T4_LAZY_DX0=1).  The switch is
    # read when the host library loads, so the figure comes from a child process of this very script.
    if os.environ.get("T4_LAZY_DX0", "1") == "0":
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--net", args.net, "--batch", str(args.batch),
                                "--no-extras", "--no-cpu-baseline", "--gemm-iters", "1", "--sustain-s", "0"], capture_output=True, text=True, timeout=600,
                               env=dict(os.environ, T4_LAZY_DX0="1"))
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode == 0 and line:
                e = json.loads(line[-1])
                out["lazy_dx0_ms_per_step"] = e["ms_per_step"]
                out["lazy_dx0_note"] = "T4_LAZY_DX0=1 (the product's default: the first layer's dX produced when a word reads it, not every step): %s launches per step, %s images/s, roofline_step.frac %s on %d algorithmic bytes" % (
                    e["config"]["launches_per_step"], e["value"], e["roofline_step"]["frac"], e["roofline_step"]["algorithmic_bytes_per_step"])
            else:
                out["lazy_dx0_note"] = "lazy leg failed: " + (r.stderr or r.stdout)[-300:]
        except Exception as ex:                                  # never lose the main line over an extra
            out["lazy_dx0_note"] = "lazy leg failed: %r" % (ex,)
    # ---- dataset-fed step: IDX file -> pinned double buffer (reader thread) -> one staging launch -> forward backprop nn.sgd
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_mnist.py"), os.path.join(d, "data", "MNIST", "raw"), "8192", "256"], check=True, capture_output=True)
        os.chdir(d)
        try:
            v = vm_cls(device=local, seed=99)
            txt = v.eval("0 trace\n128 28 28 1 nn.model 0.5 10 conv2d 2 maxpool relu 0.5 20 conv2d 0.5 dropout 2 maxpool relu flatten 100 linear 0.5 dropout 10 linear softmax constant net\n"
                         # the reference's idiom (examples/t4_30e.4th:62-83): a word that asks for host service (dataset / fetch / rewind, the `next` of a
                         # dataset loop) ends its input line - the VM drops what follows it, as the reference's does - so the epochs live in a colon word
                         "128 dataset mnist_train\nconstant ds0\n: epoch ( N D -- N ) for forward backprop 0.01 0.0 nn.sgd next ;\n"
                         ": epochs ( N n -- N ) 1- for ds0 epoch ds0 rewind drop next ;\nnet 1 epochs\n")
            assert "?" not in txt.replace("-> ok", ""), txt
            torch.cuda.synchronize()
            epochs = 6
            t0 = time.perf_counter()
            v.eval("%d epochs\nnn.hit drop\n" % epochs); torch.cuda.synchronize()
            out["dataset_fed_ms_per_step"] = round((time.perf_counter() - t0) / (epochs * 64) * 1e3, 4)
            out["dataset_fed_note"] = "synthetic MNIST-shaped IDX corpus (8192 images, tools/make_synth_mnist.py), batches of 128 through the dataset words: host read + pinned staging + on-GPU normalise + the same training step; %d steps" % (epochs * 64)
            v.close()
        finally:
            os.chdir(cwd)
    t4vm.set_lazy_dx0(headline_plan)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--net", default="nn_f", choices=list(NETS))
    ap.add_argument("--batch", type=int, default=128, help="images per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--gemm-iters", type=int, default=200)
    ap.add_argument("--sustain-s", type=float, default=3.0, help="--full: length of the sustained loop behind the timed region (seconds; 0 = skip)")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the GAN / dataset-fed / sustained legs")
    ap.add_argument("--allow-fallback", action="store_true", help="print the line even when the timed step did not take the conv-stack path (default: exit 4)")
    ap.add_argument("--dry-run", action="store_true", help="launch / rendezvous / reduction plumbing only (gloo, no GPU work, no metric): CPU test of the N-rank path")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: GEMM roofline, sustained loop, extras, CPU baseline, N > 1 exchange figures")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last step computed (parameters, output layer) as DIR/<name>.npy, float32")
    args = ap.parse_args()

    # ---- N > 1 asked for from a plain `python bench.py --gpus N`: become N ranks (one process per GPU) or fail - never a 1-rank record
    from tensorforth_amd import launch
    if launch.need_spawn(args.gpus):
        sys.exit(launch.spawn_ranks(os.path.abspath(__file__), args.gpus, sys.argv[1:], dry_run=args.dry_run))
    rank, world, local = launch.check_world(args.gpus)
    if args.dry_run:
        return dry_run(rank, world, args)

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (RCCL across processes); must be set before the HIP runtime starts
    # The headline step does the REFERENCE's work: the first layer's dX is stored every step (backprop.cu:185,240).  The product's default leaves that tensor
    # to the first word that reads it (T4_LAZY_DX0=1); its figure is the `lazy_dx0_ms_per_step` extra.  The switch is read when the host library loads.
    os.environ.setdefault("T4_LAZY_DX0", "0")
    import numpy as np
    import torch
    import torch.distributed as dist

    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback in the product path)"
    if local >= torch.cuda.device_count():
        sys.stderr.write("bench: rank %d has no device %d (%d visible)\n" % (rank, local, torch.cuda.device_count())); sys.exit(2)
    torch.cuda.set_device(local)
    dp = world > 1 or os.environ.get("T4_BENCH_FORCE_DP") == "1"     # FORCE_DP: exercise the all-reduce path on one GPU
    if dp:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local), timeout=pg_timeout())

    from tensorforth_amd import lib as t4lib, pymodel
    from tensorforth_amd.vm import VM
    N = args.batch
    build = pymodel.nn_c if args.net == "nn_c" else pymodel.nn_f      # layer lists shared with the oracle baseline
    # ---- the product: native C++ eForth VM (libten4.so) driving libt4hip.so; the model, the synthetic HBM-resident
    # batch and the training step are all plain tensorForth words (same source runs under the stand-alone `ten4`)
    vm = VM(device=local, seed=1234)
    NET_WORDS = {"nn_f": "0.5 10 conv2d 2 maxpool relu 0.5 20 conv2d 0.5 dropout 2 maxpool relu flatten 100 linear 0.5 dropout 10 linear softmax",
                 "nn_c": "0.5 10 conv2d 2 maxpool relu flatten 100 linear relu 10 linear softmax"}
    vm.eval("0 trace\n%d 28 28 1 nn.model %s constant net\n" % (N, NET_WORDS[args.net]))
    k = t4lib.load()
    # replicas are identical (same Philox seed, same draws so far).  The synthetic batch is the rank's rows of the WHOLE batch's draw
    # (stream slice [rank*n, (rank+1)*n) of a world*n-element draw), like the dropout masks later (t4k_rand_set_shard):
    # N ranks x 128 images see exactly the data and masks of 1 rank x 128N images
    n_img = N * 28 * 28
    off0 = vm.rand_tell()
    vm.rand_seek(off0 + rank * n_img)
    vm.eval("%d 28 28 1 tensor rand constant img\n" % N)
    vm.rand_seek(off0 + world * n_img)
    out_txt = vm.eval(
        ": hot ( T -- T ) %d 0 do 1 i 10 * i 7 * %d + 10 mod + t! loop ;\n"
        "%d vector zeros hot %d 1 10 1 reshape4 constant lbl\n"
        ": fb ( N -- N ) img forward lbl backprop ;\n"
        ": opt ( N -- N ) 0.01 0.0 nn.sgd ;\n"
        ": steps ( N n -- N ) 1- for fb opt next ;\n"
        "net 2 steps\n" % (N, rank, N * 10, N))
    assert "?" not in out_txt.replace("-> ok", ""), out_txt
    # ---- data parallel: the VM owns an RCCL communicator (t4k_comm_*) and sums its gradient slab in-order on its own
    # stream inside `nn.sgd`, so the training loop stays inside the VM exactly as on one GPU.  torch.distributed only
    # carries the 128-byte communicator id to the ranks (and the barrier / max-time reduction of the bench contract).
    native = False
    xchg = False
    neg = None
    if dp:
        # the ladder (library's own RCCL communicator -> one-shot peer exchange inside the optimizer launch, each rung agreed on by all ranks and the
        # exchange checked against a known sum before it is trusted) lives in tensorforth_amd/dp.py, where the CPU tests drive it with scripted failures
        from tensorforth_amd import dp as t4dp
        neg = t4dp.negotiate_reduction(k.lib, rank, world, torch.device("cuda", local),
                                       want_native=os.environ.get("T4_DP_NATIVE", "1") == "1", want_xchg=os.environ.get("T4_DP_XCHG", "1") == "1",
                                       log=(lambda m: sys.stderr.write("bench: %s (%s)\n" % (m, k.lib.t4k_last_error().decode(errors="replace")[-300:]))) if rank == 0 else None)
        native, xchg = neg["native"], neg["xchg"]
        if native and not xchg:
            k.call("t4k_rand_set_shard", rank, world)         # (a destroyed exchange resets the shard it had set; t4k_comm_init set it before)
    if dp and not native:
        k.call("t4k_rand_set_shard", rank, world)         # torch.distributed reduces the slab; the masks are still keyed by sample
    joined = k.lib.t4k_comm_world() if native else (dist.get_world_size() if dp else 1)
    if joined != world:
        sys.stderr.write("bench: %d ranks joined the reduction, %d asked for\n" % (joined, world)); sys.exit(3)
    slab = vm.grad_slab() if (dp and not native) else None
    vstream = vm.stream() if (dp and not native) else None
    reducer = None
    if slab is not None and os.environ.get("T4_DP_TORCH_OVERLAP", "0") == "1":   # torch path only: reduce the slab's tail under conv backprop
        from tensorforth_amd.dp import OverlappedSlabReducer
        reducer = OverlappedSlabReducer(slab, vstream)
        vm.set_grad_hook(reducer.on_layer)

    def run(n):
        if not dp or native:
            vm.eval("%d steps" % n)                       # the whole loop runs inside the VM (all-reduce included when native)
            return
        for _ in range(n):
            vm.eval("fb")
            if reducer:
                reducer.finish()                          # tail already in flight since mid-backprop
            else:
                with torch.cuda.stream(vstream):          # ordered with the VM's kernels; SUM: raw batch-sum gradients (quirk a-19)
                    dist.all_reduce(slab, op=dist.ReduceOp.SUM)
            vm.eval("opt")

    def barrier():
        torch.cuda.synchronize()
        if dp:
            dist.barrier()
        torch.cuda.synchronize()

    if args.warmup > 0:
        run(args.warmup)
    barrier()
    k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    l0 = k.lib.t4k_launch_count()
    t0 = time.perf_counter()
    run(args.steps)
    barrier()
    dt = time.perf_counter() - t0
    launches = (k.lib.t4k_launch_count() - l0) / args.steps          # MEASURED: every launch site of the library counts itself
    # ---- the timed path must be the one `config.workload` describes: the sample-resident conv stack (forward with the classifier head,
    # banded backward) and the fold inside the optimizer launch.  A box where hipRTC is missing / a compile failed would silently run the
    # per-layer kernels (12+ launches): say so and fail instead of printing a line that describes another path.
    cj, cd, cf = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    k.lib.t4k_conv_stack_stats.restype = None
    k.lib.t4k_conv_stack_stats(ctypes.byref(cj), ctypes.byref(cd), ctypes.byref(cf))
    stack_mode = "off" if (cj.value + cd.value == 0) else ("jit" if cj.value else "prebuilt")
    want = {"nn_f": 4, "nn_c": 6}[args.net] + (1 if (dp and native and not xchg) else 0)    # nn_f: cs_fwd(+head), head backward with the linear backward in front of it (k_head_bwd_l32: riders + dW || dX tiles), cs_bwd_b, optimizer (+ fold [+ exchange]); with RCCL between them the fold keeps its launch.  nn_c (one conv stage, relu head): single-stage stack forward with the head, head backward (2 launches), linear backward, cs_bwd_b, optimizer
    if N > 256:
        want += 1                                              # the one-launch head backward takes batches up to 256 per GPU; larger ones the column-stripe head + the dual GEMM
    if N > 512:
        want += 3                                              # the column-stripe head backward holds the batch in LDS (N <= 512): larger batches take the gated head kernels (3 more launches)
    if not args.allow_fallback and os.environ.get("T4_STACK", "1") != "0" and (stack_mode == "off" or cf.value or launches > want + 0.01):
        sys.stderr.write("bench: the timed step is NOT the described path: conv_stack=%s (jit %d, cache %d, failed %d), %.2f launches per step (expected <= %d); "
                         "%s\n(--allow-fallback prints the line anyway)\n" % (stack_mode, cj.value, cd.value, cf.value, launches, want, k.lib.t4k_last_error().decode(errors="replace")[-600:]))
        sys.exit(4)
    if dp:
        tmax = torch.tensor([dt], device="cuda"); dist.all_reduce(tmax, op=dist.ReduceOp.MAX); dt = float(tmax.cpu()[0])
    ms_step = dt / args.steps * 1e3
    img_s = world * N * args.steps / dt
    # ---- what the last timed step computed, before anything below steps the net again (replicas are identical: rank 0 writes)
    if args.dump_outputs and rank == 0:
        dump_outputs(vm, args.net, args.dump_outputs)
    # ---- sustained loop (same work, >= 3 s): what a long training run sees, and long enough for an external GPU-busy sampler
    sustained = None
    if args.full and args.sustain_s > 0 and not args.no_extras:
        n_sus = max(args.steps, int(args.sustain_s / (ms_step * 1e-3)))
        barrier()
        t0 = time.perf_counter(); run(n_sus); barrier()
        sdt = time.perf_counter() - t0
        if dp:
            tmax = torch.tensor([sdt], device="cuda"); dist.all_reduce(tmax, op=dist.ReduceOp.MAX); sdt = float(tmax.cpu()[0])
        sustained = (sdt / n_sus * 1e3, n_sus)
    loss_txt = vm.eval("img forward lbl loss.ce .") if args.full else None   # a fresh forward: after backprop the output tensor holds out - target (reference in-place convention)
    # ---- N > 1, day-one numbers of the exchange (VERDICT r5 #9a; never measured on real xGMI so far): every rank's known-sum probe times, and the EXPOSED
    # exchange time per step = the step above minus the same loop run by every rank on its own (exchange and communicator dropped: the single-GPU step, same
    # process, same clocks).  DESIGN section 6 predicts 5-8 us at 8 ranks.  The replicas diverge from here on - nothing after this reads their weights.
    dp_extra = None
    if args.full and dp and native and world > 1 and os.environ.get("T4_BENCH_DP_EXTRA", "1") != "0":
        try:
            probes = [None] * world
            dist.all_gather_object(probes, (neg or {}).get("xchg_probe_us"))
            if xchg:
                k.lib.t4k_xchg_destroy()
            k.lib.t4k_comm_destroy()
            run(max(args.warmup, 5)); barrier()
            t1 = time.perf_counter(); run(args.steps); barrier()
            solo = torch.tensor([(time.perf_counter() - t1) / args.steps * 1e3], device="cuda"); dist.all_reduce(solo, op=dist.ReduceOp.MAX)
            dp_extra = {"xchg_probe_us_per_rank": probes, "solo_ms_per_step": round(float(solo.cpu()[0]), 4),
                        "exchange_exposed_us_per_step": round((dt / args.steps * 1e3 - float(solo.cpu()[0])) * 1e3, 2),
                        "note": "exposed = ms_per_step (all ranks, exchange inside the optimizer launch) - the same loop with every rank stepping alone (max over ranks)"}
        except Exception as ex:                                  # an extra never costs the line (T4_BENCH_DP_EXTRA=0 skips it)
            dp_extra = {"note": "dp extra failed: %r" % (ex,)}

    out = None
    if dp and rank != 0:
        all_alive(dist, torch, world, torch.device("cuda", local))       # (rank 0 asks in front of its print)
    if rank == 0:
        net = NETS[args.net]
        gemm_traffic, step_traffic, traffic_src = measured_traffic()
        if args.net != "nn_f" or N != 128:
            step_traffic = None                                # the counter pass is of the default workload
        step_bytes_eager = N * net["bytes_per_img"] + 4 * net["params"] * 7      # k_opt = 7 for SGD; SURVEY 8(d): every layer-boundary tensor incl. the first layer's dX
        lazy_dx0 = os.environ.get("T4_LAZY_DX0", "1") != "0"
        # a step run with T4_LAZY_DX0=1 does not produce the first layer's dX (nobody reads it in a training loop; it is made on demand): its write + read
        # (2 x 4 B per input element) is then not counted as work done.  The headline (default of this script) is the eager, reference-equal step.
        step_bytes = step_bytes_eager - (2 * 4 * N * 28 * 28 if lazy_dx0 else 0)
        out = {
            "metric": BASELINE_METRIC,   # `value` = CNN train images/sec; the GEMM TFLOP/s (% of MFMA peak) part is the `roofline` object
            "value": round(img_s, 1), "unit": "images/s", "n_gpus": joined, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "t4_30e %s LeNet-style CNN (examples/t4_30e.4th), 28x28x1, batch %d per GPU, "
                                   "copy-in + forward + backprop + nn.sgd(0.01), dropout on, %s" % (args.net, N, "first layer's dX left to the first reader (T4_LAZY_DX0=1)" if lazy_dx0 else "every layer's dX stored every step incl. the first layer's (the reference's work)"),
                       "global_batch": N * world, "parallelism": "dp%d" % world, "host": "C++ eForth VM (libten4.so) -> C-ABI (libt4hip.so)", "launches_per_step": round(launches, 2), "launches_source": "t4k_launch_count() around the timed loop", "conv_stack": stack_mode, "allreduce": ("one-shot peer exchange inside the optimizer launch (csrc/xchg.hip)" if xchg else ("rccl-native-in-vm" if native else ("torch.distributed" if dp else None))),
                       "allreduce_fallback_reason": neg["reason"] if neg else None, "ranks_seen": neg["ranks_seen"] if neg else None},
            "roofline_step": {"bound": "hbm", "achieved": round(step_bytes / (ms_step * 1e-3) / 1e9, 2), "peak": PEAK_HBM_GBS,
                              "unit": "GB/s", "frac": round(step_bytes / (ms_step * 1e-3) / 1e9 / PEAK_HBM_GBS, 5),
                              "traffic": step_traffic, "traffic_source": traffic_src,
                              "algorithmic_bytes_per_step": step_bytes, "algorithmic_bytes_per_step_eager": step_bytes_eager,
                              "first_layer_dx": "on demand (T4_LAZY_DX0=1): its 2 x 4 B per input element are not in algorithmic_bytes_per_step" if lazy_dx0 else "stored every step"},
        }
        if loss_txt is not None:
            out["config"]["final_loss_ce"] = loss_txt.split()[0] if loss_txt.split() else None
            out["config"]["final_loss_note"] = "random images and labels, batch-SUM gradients (reference semantics): a throughput run, not a convergence test; training parity vs the oracle is in tests/"
        if dp_extra:
            out["dp"] = dp_extra
        if sustained:
            out["sustained_ms_per_step"] = round(sustained[0], 4)
            out["sustained_steps"] = sustained[1]
        if args.full and world == 1 and not dp and not args.no_extras:
            # ---- what the data-parallel machinery itself costs on ONE GPU: the same loop with a one-rank exchange in self mode - the optimizer
            # launch takes its exchanging form (k_opt_step<true>: pushes to nobody, adds its own element out of the same code path)
            h = (ctypes.c_ubyte * 64)()
            if k.lib.t4k_xchg_create(1 << 17, 0, 1, h) == 0 and k.lib.t4k_xchg_connect(bytes(h)) == 0:
                k.lib.t4k_xchg_self(1)
                run(args.warmup or 5); torch.cuda.synchronize()
                l1 = k.lib.t4k_launch_count()
                t0 = time.perf_counter(); run(args.steps); torch.cuda.synchronize()
                dms = (time.perf_counter() - t0) / args.steps * 1e3
                out["dp_overhead_us"] = round((dms - ms_step) * 1e3, 2)
                out["dp_overhead_note"] = "same %d steps with the one-shot exchange connected (world 1, self mode): %.4f ms/step, %.2f launches/step" % (args.steps, dms, (k.lib.t4k_launch_count() - l1) / args.steps)
                k.lib.t4k_xchg_self(0)
            k.lib.t4k_xchg_destroy()
            out.update(extras(VM, local, ms_step, args, torch))
        if args.full:
            # ---- GEMM 1024^3 fp32 (word `matmul`), HIP events on the launch stream
            g = torch.Generator(device="cuda"); g.manual_seed(1234)
            A = torch.rand(1024, 1024, device="cuda", generator=g); B = torch.rand(1024, 1024, device="cuda", generator=g)
            O = torch.zeros(1024, 1024, device="cuda")
            e0 = ctypes.c_void_p(); e1 = ctypes.c_void_p()
            k.call("t4k_event_create", ctypes.byref(e0)); k.call("t4k_event_create", ctypes.byref(e1))
            for _ in range(1500):                             # ~35 ms of back-to-back launches: the launch time settles only after the
                k.call("t4k_gemm", A.data_ptr(), B.data_ptr(), O.data_ptr(), 1.0, 0.0, 0, 0, 1024, 1024, 1024, 1, None)   # clocks ramp (25.3 -> 22.4 us)
            best = 1e9; tot = 0.0; reps = 5
            for _ in range(reps):
                k.call("t4k_event_record", e0, None)
                for _ in range(args.gemm_iters):
                    k.call("t4k_gemm", A.data_ptr(), B.data_ptr(), O.data_ptr(), 1.0, 0.0, 0, 0, 1024, 1024, 1024, 1, None)
                k.call("t4k_event_record", e1, None); k.call("t4k_event_sync", e1)
                ms = ctypes.c_float(0); k.call("t4k_event_elapsed_ms", e0, e1, ctypes.byref(ms))
                per = ms.value / args.gemm_iters; tot += per; best = min(best, per)
            avg_ms = tot / reps
            flops = 2.0 * 1024 ** 3
            tf = flops / (avg_ms * 1e-3) / 1e12
            out["roofline"] = {"kernel": "k_gemm_nn_plain (1024^3 fp32 matmul: 64x64 tiles, 8 waves/WG = 2 k-groups x 2x2 v_mfma_f32_32x32x2_f32 accumulator pairs, LDS-DMA from inline asm, 128-deep double-buffered stages)", "bound": "mfma", "achieved": round(tf, 2),
                               "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_F32_MFMA_TFLOPS, 4),
                               "traffic": gemm_traffic, "traffic_source": traffic_src,
                               "avg_launch_us": round(avg_ms * 1e3, 2), "best_launch_us": round(best * 1e3, 2),
                               "flop_per_launch": flops}
            # ---- the same product through the Forth word, reference idiom `for @ drop next` (examples/t4_20a.4th:20-29): per call an arena
            # allocation for the result, the VM's dispatch, the launch, and `drop` freeing the tensor again
            vm.eval("1024 1024 matrix rand constant ma\n1024 1024 matrix rand constant mb\n: mx ( A B n -- A B ) 1- for matmul drop next ;\nma mb 1500 mx 2drop\n")
            torch.cuda.synchronize()
            wl = []
            for _ in range(3):
                t0w = time.perf_counter(); vm.eval("ma mb %d mx 2drop\n" % args.gemm_iters); torch.cuda.synchronize(); wl.append((time.perf_counter() - t0w) / args.gemm_iters * 1e6)
            out["roofline"]["word_level_us"] = round(sum(wl) / len(wl), 2)
            out["roofline"]["word_level_note"] = "`ma mb N mx` with `: mx 1- for matmul drop next ;` (t4_20a.4th:20-29 idiom), host clock around the VM call + device sync, %d words per sample" % args.gemm_iters
            # ---- CPU baseline: the oracle ("port"), bounded sample
            if not args.no_cpu_baseline and world == 1:       # the CPU baseline is reported by the 1-GPU run only (rank 0 of an N-GPU job just prints)
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import t4oracle
                rng = np.random.default_rng(42)
                lab = rng.integers(0, 10, N).astype(np.uint32)
                x = rng.random((N, 28, 28, 1)).astype(np.float32)
                om = build(t4oracle.OracleModel(N, 28, 28, 1, seed=1234))
                om.forward(x); om.onehot_labels(lab)
                t0 = time.perf_counter(); nst = 0
                while True:
                    om.forward(x); om.backprop(); om.sgd(0.01, 0.0); nst += 1
                    if time.perf_counter() - t0 > 3.0 or nst >= 50:
                        break
                cdt = time.perf_counter() - t0
                a = np.random.default_rng(1).random((1024, 1024)).astype(np.float32); o_ = np.zeros((1024, 1024), np.float32)
                t1 = time.perf_counter()
                t4oracle.lib().t4o_gemm_host_blocked(t4oracle.P(a), t4oracle.P(a), t4oracle.P(o_), 1.0, 0.0, 1024, 1024, 1024)
                gdt = time.perf_counter() - t1
                # all cores: one worker process per core the bench may run on, each training its own batch-N replica (the CPU analogue of
                # sample sharding), and the blocked host GEMM on row slabs of the same 1024^3 product
                try:
                    ncore = len(os.sched_getaffinity(0))
                except Exception:
                    ncore = os.cpu_count() or 1
                wr = cpu_workers(["step", args.net, N, 4.0], ncore)
                all_img_s = sum(N * r[0] / r[1] for r in wr if len(r) == 2 and r[1] > 0)
                rows = max(4, 1024 // ncore)
                gr = cpu_workers(["gemm", rows, 1024, 1024, 2.0], ncore)
                all_gflops = sum(r[0] * 2.0 * rows * 1024 * 1024 / r[1] for r in gr if len(r) == 2 and r[1] > 0) / 1e9
                out["cpu_baseline"] = {"value": round(all_img_s, 1), "unit": "images/s", "cores": len(wr), "kind": "port",
                                       "sample": "%d worker processes (one per core), each ~4 s of oracle training steps of the same %s batch-%d workload "
                                                 "(%d steps in total); single thread: %d steps in %.1f s" % (len(wr), args.net, N, int(sum(r[0] for r in wr)), nst, cdt),
                                       "single_thread_value": round(N * nst / cdt, 1),
                                       "host_cores_available": os.cpu_count(),
                                       "gemm_1024_host_blocked_ms": round(gdt * 1e3, 1),
                                       "gemm_1024_host_gflops": round(flops / gdt / 1e9, 2),
                                       "gemm_1024_host_gflops_all_cores": round(all_gflops, 1), "gemm_all_cores_workers": len(gr),
                                       "gemm_note": "reference's blocked host GEMM (tensor.cu:97-123 restated): one thread on the full 1024^3 product, then %d workers on %d-row slabs for ~2 s" % (len(gr), rows)}
        if dp:
            all_alive(dist, torch, world, torch.device("cuda", local))   # a line is printed only by a job whose ranks are ALL still there
        print(json.dumps(out), flush=True)
    if dp:
        if xchg:
            torch.cuda.synchronize(); dist.barrier(); k.lib.t4k_xchg_destroy()
        if native:
            k.lib.t4k_comm_destroy()
        dist.barrier(); dist.destroy_process_group()


if __name__ == "__main__":
    main()
