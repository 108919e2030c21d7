"""CPU side of the conv stack's streaming stores (csrc/conv_stack.hip `preamble`, csrc/conv_stack_kernels.hip.inc CS_STREAM_DEAD): the dead layer
tensors take a streaming store policy only in modules compiled for a BANDED backward.  The define that turns it on is part of the preamble, and the
preamble is part of the text the on-disk code-object cache is keyed on - a one-band module and a banded one can never load each other's object.
No device needed: t4k_conv_stack_key reports the preamble and the cache file name of a stack at a given plan."""
import ctypes
import os

from test_gpu_conv_stack import ConvStage

L_RELU, L_DROPOUT, L_MAXPOOL = 4, 10, 14           # t4k_layer (include/t4k.h)


def _lenet():
    """the LeNet front end of bench.py: the geometry t4k_conv_stack_selftest compiles banded (2 x 2) and whole-image (1 x 1)"""
    arr = (ConvStage * 2)()
    for s, (H, C1, C0) in zip(arr, ((28, 1, 10), (14, 10, 20))):
        s.H, s.W, s.C1, s.C0, s.K = H, H, C1, C0, 3
        s.F = s.B = s.O = 1                        # non-null placeholders: the query reads shapes only
        b = s.run
        b.KS, b.pool_layer, b.pool_out, b.post_layer, b.post_mask, b.post_out = 2, L_MAXPOOL, 1, L_RELU, 1, 1
    b = arr[1].run
    b.pre_layer, b.pre_alpha, b.pre_mask, b.pre_out, b.copy_out = L_DROPOUT, 0.5, 1, 1, 1
    return arr


def _key(h, arr, split, bsplit):
    pre, name = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(64)
    assert h.lib.t4k_conv_stack_key(arr, len(arr), split, bsplit, pre, len(pre), name, len(name)) == 1
    return pre.value.decode().splitlines(), name.value.decode()


def test_device_source_compiles_with_and_without_the_streaming_define():
    """the selftest's geometries cover both settings: the banded LeNet modules (with and without the head) and their one-band twins"""
    from tensorforth_amd.lib import T4K
    h = T4K()
    assert h.lib.t4k_conv_stack_selftest() == 0, h.lib.t4k_last_error().decode(errors="replace")[-3000:]
    # ... and where the disk cache is on and has a directory it could write, what the selftest compiled sits there under the names the query reports, one
    # object per setting (_lenet() is the selftest's LeNet geometry: banded 2 x 2 and whole-image 1 x 1)
    lib_dir = os.path.dirname(h.path)
    dirs = [os.environ["T4K_CACHE_DIR"]] if os.environ.get("T4K_CACHE_DIR") else [os.path.join(lib_dir, "kcache"), os.path.expanduser("~/.cache/tensorforth_amd")]
    cached = [f for d in dirs if os.path.isdir(d) for f in os.listdir(d) if f.startswith("cs_") and f.endswith(".hsaco")]
    if os.environ.get("T4K_STACK_DISK_CACHE", "1") == "0" or not cached:
        return                                     # nothing is kept on disk here: the selftest's 0 is the whole statement
    arr = _lenet()
    for split, bsplit in ((2, 2), (1, 1)):
        name = _key(h, arr, split, bsplit)[1]
        assert any(os.path.exists(os.path.join(d, name)) for d in dirs), (split, bsplit, name)


def test_banded_preamble_carries_the_define_and_its_own_cache_key():
    from tensorforth_amd.lib import T4K
    h = T4K()
    arr = _lenet()
    one, one_name = _key(h, arr, 2, 1)
    for bsplit in (2, 3, 4):
        banded, banded_name = _key(h, arr, 2, bsplit)
        assert set(banded) - set(one) == {"#define CS_BSPLIT %d" % bsplit, "#define CS_STREAM_DEAD 1"}
        assert set(one) - set(banded) == {"#define CS_BSPLIT 1"}
        assert banded_name != one_name
    assert not any("CS_STREAM" in line for line in one)
    assert one_name.startswith("cs_") and one_name.endswith(".hsaco")
    # the forward's band count alone does not switch it
    assert not any("CS_STREAM" in line for line in _key(h, arr, 4, 1)[0])


def test_query_refuses_what_is_no_stack_or_does_not_fit():
    from tensorforth_amd.lib import T4K
    h = T4K()
    arr = _lenet()
    pre, name = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(64)
    assert h.lib.t4k_conv_stack_key(arr, 2, 2, 5, pre, len(pre), name, len(name)) == 0          # more than 4 bands
    assert h.lib.t4k_conv_stack_key(arr, 2, 2, 2, pre, 16, name, len(name)) == 0                # preamble buffer too small
    arr[0].K = 4
    assert h.lib.t4k_conv_stack_key(arr, 2, 2, 2, pre, len(pre), name, len(name)) == 0          # even kernel size: no stack
