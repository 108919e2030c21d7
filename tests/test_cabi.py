"""CPU-side checks of the drop-in boundary: libt4hip.so loads, exports every symbol
include/t4k.h declares, and refuses to run without a gfx950 device (no CPU fallback)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from tensorforth_amd.lib import T4K
    h = T4K()
    assert h.missing == [], h.missing
    assert len(h.decls) >= 60
    out = subprocess.check_output(["nm", "-D", "--defined-only", h.path]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(h.decls) <= exported


def test_backend_identifies_itself_and_has_no_oracle_dependency():
    from tensorforth_amd.lib import T4K
    h = T4K()
    assert h.lib.t4k_backend_name() == b"hip-gfx950"
    ldd = subprocess.check_output(["ldd", h.path]).decode()
    assert "oracle" not in ldd and "libamdhip64" in ldd


def test_fails_loudly_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tensorforth_amd.lib import T4K, T4KError
    h = T4K()
    assert h.lib.t4k_device_count() == 0
    with pytest.raises(T4KError):
        h.init(0)
    # a compute entry point must refuse, not silently fall back
    assert h.lib.t4k_gemm(None, None, None, 1.0, 0.0, 0, 0, 4, 4, 4, 1, None) == -5
    assert b"no" in h.lib.t4k_last_error().lower() or b"init" in h.lib.t4k_last_error().lower()


def test_header_cites_reference_lines():
    text = open(os.path.join(ROOT, "include", "t4k.h")).read()
    for needle in ("k_gemm_tile_claude :478", "nmath.tcu:34", "nmath.tcu:211", "nmath.cu:419", "tensor.cu:344"):
        assert needle in text


def test_conv_stack_device_source_compiles_for_gfx950_without_a_device():
    """The sample-resident conv-stack kernels are specialised at run time (hipRTC) for a model's shapes; the embedded source must
    compile for gfx950 here, with no GPU: the LeNet front end of bench.py and a three-stage stack with every layer kind."""
    from tensorforth_amd.lib import T4K
    h = T4K()
    assert h.lib.t4k_conv_stack_selftest() == 0, h.lib.t4k_last_error().decode(errors="replace")[-3000:]


def test_release_library_has_no_lab_switches():
    """The conv-stack ablation hooks (T4K_STACK_LAB_*: kernels that skip work, wrong results) and the stamp pointer hook exist only in a
    LAB build (make -C tensorforth_amd/csrc LAB=1 -> libt4hip_lab.so); the shipped library does not even contain their names, so no
    environment variable can switch them on."""
    import re
    blob = open(os.path.join(ROOT, "tensorforth_amd", "libt4hip.so"), "rb").read()
    for name in (b"T4K_STACK_LAB_NOSTORE", b"T4K_STACK_LAB_NOW1", b"T4K_STACK_LAB_NOXCHG", b"T4K_STACK_PROF_PTR"):
        assert name + b"\0" not in blob, name               # as a C string of its own (what getenv would be handed); comments of the embedded source may mention it
    assert b"#define CS_LAB_" not in blob
    assert b"defined(CS_LAB_NOW1)" in blob                    # (the embedded device source keeps the guarded text; nothing can define the macro)
    # round 6: the engine-selection / tuning knobs (T4K_LAB_ENV, csrc/t4k_common.h) are compile-time constants of the release build
    for name in (b"T4K_GEMM_S32", b"T4K_GEMM_DUAL", b"T4K_GEMM_PLAIN128", b"T4K_CONVBIG8", b"T4K_CONV_THIN", b"T4K_STACK_SPLIT", b"T4K_LINTHIN", b"T4K_HB_LAB", b"T4K_GEMM_VARIANT"):
        assert name + b"\0" not in blob, name
    # the head-backward kernel's ablation word is compile-time too: the release kernel's last parameter is its HeadBwd block, no `int lab` behind it
    hb = set(re.findall(rb"(?<![0-9A-Za-z_])_ZN12_GLOBAL__N_114k_head_bwd_l32E[0-9A-Za-z_]*", blob))
    assert hb and all(n.endswith(b"HeadBwdE") for n in hb), hb
    # ... and the release libraries read a short documented list: every T4K_* / T4_* name they hold as a C string
    names = set(re.findall(rb"\0(T4K?_[A-Z0-9_]{3,})\0", blob + open(os.path.join(ROOT, "tensorforth_amd", "libten4.so"), "rb").read()))
    names = {n.decode() for n in names if not n.startswith((b"T4K_ERR", b"T4K_L_", b"T4K_OK", b"T4K_OP"))}
    documented = {"T4K_RCCL_PATH", "T4K_XCHG_TIMEOUT_MS", "T4K_CACHE_DIR", "T4K_STACK_JIT", "T4K_STACK_DISK_CACHE",
                  "T4_FUSE", "T4_STACK", "T4_HEAD_BWD", "T4_STACK_HEAD", "T4_LAZY_DX0", "T4_OPT_FOLD", "T4_GRAPH", "T4_SIDE", "T4_FEED_PREFETCH",
                  "T4_DP_SYNC_BN", "T4_DP_OVERLAP", "T4_DP_BUCKET", "T4_DP_TRACE", "T4_DP_XCHG", "T4_TB_FIXED_TIME", "T4_TB_LOGDIR", "T4_TB_RUN",
                  "T4_DEVICE", "T4_SEED", "T4_SLAB_MB", "T4_HOLD_WARN"}
    assert names <= documented, sorted(names - documented)
    assert len(documented) <= 30


def test_conv_stack_code_objects_are_cached_on_disk(tmp_path):
    """hipRTC output is kept on disk keyed by the hash of the specialised source: a second process (another rank, the next run, a tree
    shipped after build()) loads the code object instead of compiling.  T4K_CACHE_DIR redirects it."""
    code = ("import os, time; from tensorforth_amd.lib import T4K; h = T4K(); t0 = time.time(); "
            "assert h.lib.t4k_conv_stack_selftest() == 0; print(time.time() - t0)")
    env = dict(os.environ, T4K_CACHE_DIR=str(tmp_path), PYTHONPATH=ROOT)
    t_cold = float(subprocess.check_output(["python3", "-c", code], env=env, cwd=ROOT).decode().split()[-1])
    objs = [f for f in os.listdir(tmp_path) if f.startswith("cs_") and f.endswith(".hsaco")]
    assert len(objs) >= 5, objs
    assert all(open(os.path.join(tmp_path, f), "rb").read(4) == b"\x7fELF" for f in objs)
    t_warm = float(subprocess.check_output(["python3", "-c", code], env=env, cwd=ROOT).decode().split()[-1])
    assert t_warm < 0.5 * t_cold + 0.05, (t_cold, t_warm)
    # a truncated file is not trusted: it is recompiled and replaced
    victim = os.path.join(tmp_path, objs[0]); full = os.path.getsize(victim)
    open(victim, "wb").write(b"\x7fELFgarbage")
    subprocess.check_output(["python3", "-c", code], env=env, cwd=ROOT)
    assert os.path.getsize(victim) >= 64
