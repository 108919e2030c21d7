"""CPU: the numpy Philox witness (philox_witness.py) against the Random123 known-answer vectors, the oracle's generator against the
witness at the far positions of the stream, and proof that those positions see what they claim to see: a generator that drops the high
counter word, the high key word or the carry between the counter words draws a different mask there.

Positions (philox_witness.POSITIONS; offsets in elements, nq = ceil(n / 4)):
    P0  seed 777                  offset 0                      control
    P1  seed 0x9E3779B97F4A7C15   offset 2^34 - 4 (nq // 2)     the draw straddles the carry into the high counter word; high key word set
    P2  seed 0xFFFFFFFF00000001   offset 2^36 + 48              high counter word 16 throughout
    P3  seed 1 << 32              offset 4096                   only the high key word set
    P4  seed 5                    offset 2^64 - 4 (nq // 2)     the element offset wraps mod 2^64 inside the draw: counter 2^62, a carry into the high word

Which position catches which injected defect (CAUGHT_AT, asserted below on 64-element masks, alpha 0.5):
    counter truncated to 32 bits           P1 P2 P4     (P0, P3: high counter word is 0 anyway)
    key truncated to 32 bits               P1 P2 P3     (P0, P4: high key word is 0 anyway)
    carry dropped in base + (a >> 2)       P1 P4        (P0, P2, P3: the low word does not overflow inside the draw)
tests/test_gpu_philox_far.py runs every drawing kernel at P1 and P2 at least, so each defect is caught by a position used there."""
import numpy as np
import pytest

import philox_witness as pw

NAMES = ("P0", "P1", "P2", "P3", "P4")
SIZES = (1, 5, 64, 4099)
GPU_FILE_POSITIONS = ("P1", "P2")            # the positions EVERY entry of test_gpu_philox_far.py visits (most visit P0 .. P4)


def _hex(words):
    return " ".join("%08x" % int(x) for x in words)


# ----------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_random123_known_answers(ctr, key, want):
    assert _hex(pw.philox4x32_10(np.array([ctr], np.uint32), key)[0]) == want


def test_known_answers_in_one_batch_and_the_stream_layout():
    """rows of a batch are independent, and words() lays a 64-bit counter out as (lo, hi, 0, 0) under key (lo(seed), hi(seed))"""
    c = np.array([(0, 0, 0, 0), (7, 9, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0, 0)], np.uint32)
    key = (0x7F4A7C15, 0x9E3779B9)
    both = pw.philox4x32_10(c, key)
    for i in range(3):
        assert np.array_equal(both[i], pw.philox4x32_10(c[i:i + 1], key)[0])
    seed = 0x9E3779B97F4A7C15
    assert np.array_equal(pw.words(seed, 4 * ((9 << 32) + 7), 4), both[1])
    assert np.array_equal(pw.words(seed, 4 * (2 ** 64 - 1), 8), np.concatenate([both[2], both[0]]))  # ... and the COUNTER wraps mod 2^64
    assert np.array_equal(pw.words(seed, 4 * ((9 << 32) + 7) + 3, 4), both[1])                       # an offset inside a counter is rounded down
    u = pw.u01(np.array([0, 1, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFF7F], np.uint32))
    assert u.dtype == np.float32 and u[0] == np.float32(2.0 ** -33) and u[1] == np.float32(2.0 ** -32 + 2.0 ** -33)
    assert u[2] == np.float32(0.5) and u[3] == np.float32(1.0) and u[4] < np.float32(1.0)            # (0, 1]: never 0, 1 reachable


# ----------------------------------------------------------------------------------------------------- oracle == witness
def _oracle_uniform(oracle, seed, off, n, bias=0.0, scale=1.0):
    o = oracle.lib()
    o.t4o_rand_set_shard(0, 1)
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
    a = np.zeros(n, np.float32); o.t4o_rand(oracle.P(a), n, 0, bias, scale)
    return a, o.t4o_rand_offset()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_uniform_is_the_witness(oracle, name, n):
    seed, off = pw.position(name, n)
    a, end = _oracle_uniform(oracle, seed, off, n)
    assert np.array_equal(a, pw.uniform(seed, off, n))
    assert end == pw.end_offset(off, n) == (off + 4 * ((n + 3) // 4)) % 2 ** 64


@pytest.mark.parametrize("seed,off,n", [(777, 0, 100001), (0x9E3779B97F4A7C15, 2 ** 34 - 4000, 8001),
                                        (0xFFFFFFFF00000001, 2 ** 36 + 12, 4099), (5, 2 ** 64 - 40, 103)])
def test_oracle_uniform_is_the_witness_at_the_positions_of_the_feasibility_check(oracle, seed, off, n):
    a, end = _oracle_uniform(oracle, seed, off, n)
    assert np.array_equal(a, pw.uniform(seed, off, n))
    assert end == pw.end_offset(off, n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_sharded_mask_is_the_ranks_slice_of_the_witness(oracle, name, n):
    o = oracle.lib(); world = 3
    seed, off = pw.position(name, n * world)
    nq = (n + 3) // 4
    whole = pw.uniform(seed, off, 4 * nq * world)
    try:
        for r in range(world):
            o.t4o_rand_set_shard(r, world)
            o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
            m = np.zeros(n, np.float32); o.t4o_dropout_mask(oracle.P(m), n)
            assert np.array_equal(m, whole[r * 4 * nq: r * 4 * nq + n]), "rank %d" % r
            assert o.t4o_rand_offset() == (off + 4 * world * nq) % 2 ** 64 == pw.end_offset(off, n, world)
    finally:
        o.t4o_rand_set_shard(0, 1)


def test_oracle_offsets_are_rounded_down_to_a_whole_counter(oracle):
    """include/t4k.h: the position is kept in counters of 4 elements; the remainder of an offset is dropped, not remembered"""
    o = oracle.lib()
    seed = pw.SEED_P2
    for rem in (0, 1, 2, 3):
        base = 2 ** 36 + 48
        a, end = _oracle_uniform(oracle, seed, base + rem, 9)
        assert np.array_equal(a, pw.uniform(seed, base, 9)), rem
        assert end == base + 12 == pw.end_offset(base + rem, 9), rem
        o.t4o_rand_set_offset(base + rem)
        assert o.t4o_rand_offset() == base, rem


# ----------------------------------------------------------------------------------------------------- injected defects
def _ctr32(q, seed):                        # the high counter word never reaches the generator
    return q & pw.M32, seed


def _key32(q, seed):                        # the high key word never reaches the generator
    return q, seed & 0xFFFFFFFF


def _no_carry(q, seed):                     # base + (a >> 2) added in the low words only: hi(base) stays
    base = int(q[0])
    lo = (np.uint64(base & 0xFFFFFFFF) + (q - q[0])) & pw.M32
    return (np.uint64(base >> 32) << np.uint64(32)) | lo, seed


DEFECTS = {"counter truncated to 32 bits": _ctr32, "key truncated to 32 bits": _key32, "carry dropped": _no_carry}
CAUGHT_AT = {"counter truncated to 32 bits": ("P1", "P2", "P4"), "key truncated to 32 bits": ("P1", "P2", "P3"), "carry dropped": ("P1", "P4")}


def _mask_with(defect, seed, off, n):
    with np.errstate(over="ignore"):
        q, s = defect(pw.counters(off, n), seed)
    return (pw.u01(pw.words_at(q, s).reshape(-1)[:n]) > np.float32(0.5)).astype(np.float32)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", sorted(DEFECTS))
def test_injected_defect_is_caught_where_claimed(kind, name):
    n = 64
    seed, off = pw.position(name, n)
    good, bad = pw.mask(seed, off, n, 0.5), _mask_with(DEFECTS[kind], seed, off, n)
    if name in CAUGHT_AT[kind]:
        assert not np.array_equal(good, bad), "%s must change the mask at %s" % (kind, name)
    else:
        assert np.array_equal(good, bad), "%s does not apply at %s" % (kind, name)  # the position cannot see it: not claimed


def test_every_defect_is_caught_by_a_position_every_gpu_entry_visits():
    for kind, where in CAUGHT_AT.items():
        assert set(where) & set(GPU_FILE_POSITIONS), kind
    # at P1 the counter defects show only BEHIND the carry, in the second half of the draw: being right up to element 2^34 is not enough
    seed, off = pw.position("P1", 64)
    for kind in ("counter truncated to 32 bits", "carry dropped"):
        good, bad = pw.mask(seed, off, 64, 0.5), _mask_with(DEFECTS[kind], seed, off, 64)
        assert np.array_equal(good[:32], bad[:32]) and not np.array_equal(good[32:], bad[32:]), kind


# ----------------------------------------------------------------------------------------------------- normal draws
def _oracle_normal(oracle, seed, off, n):
    o = oracle.lib()
    o.t4o_rand_set_shard(0, 1)
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
    a = np.zeros(n, np.float32); o.t4o_rand(oracle.P(a), n, 1, 0.0, 1.0)
    return a


def normal_cases():
    """(seed, offset, n) of every normal draw NORMAL_ORACLE_WORST was measured over"""
    out = [pw.position(name, 100001) + (100001,) for name in NAMES]
    out.append((pw.SEED_P1, 2 ** 34 - 200000, 400001))
    out.append((pw.TAIL_SEED, 4 * pw.TAIL_COUNTER - 64, 256))
    return out


def test_oracle_normal_draws_stay_within_the_stored_figure(oracle):
    worst = 0.0
    for seed, off, n in normal_cases():
        r = pw.normal_ratio(_oracle_normal(oracle, seed, off, n), seed, off, n)
        print("normal: seed %#x offset %d n %d: worst |oracle - float64| = %.3f x 2^-24 rad" % (seed, off, n, r.max()))
        worst = max(worst, float(r.max()))
    print("normal: worst over all = %.3f (NORMAL_ORACLE_WORST = %.2f)" % (worst, pw.NORMAL_ORACLE_WORST))
    assert worst <= pw.NORMAL_ORACLE_WORST, worst


def test_tail_position_holds_the_smallest_u1():
    w = pw.words_at(np.array([pw.TAIL_COUNTER], np.uint64), pw.TAIL_SEED)[0]
    assert int(w[pw.TAIL_SLOT]) == pw.TAIL_WORD == 154 and pw.TAIL_SLOT in (0, 2)
    u1 = float(pw.u01(w[pw.TAIL_SLOT]))
    assert abs(u1 - 3.6e-8) < 1e-9
    v, rad = pw.normal64(pw.TAIL_SEED, 4 * pw.TAIL_COUNTER - 64, 256)
    assert abs(rad[64 + pw.TAIL_SLOT] - 5.855) < 1e-3 and rad.max() == rad[64 + pw.TAIL_SLOT] == rad[64 + pw.TAIL_SLOT + 1]


def test_oracle_normal_draw_at_the_tail(oracle):
    seed, off, n = pw.TAIL_SEED, 4 * pw.TAIL_COUNTER - 64, 256
    a = _oracle_normal(oracle, seed, off, n)
    r = pw.normal_ratio(a, seed, off, n)
    assert r.max() <= pw.NORMAL_ORACLE_WORST, r.max()
    i = 64 + pw.TAIL_SLOT
    assert abs(float(np.hypot(a[i], a[i + 1])) - 5.855) < 1e-3                   # the pair really sits 5.855 sigma out
