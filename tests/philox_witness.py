"""An independent witness of the project's random stream: Philox4x32-10 (Salmon et al., SC'11) in plain numpy uint64 arithmetic.

Nothing here is shared with oracle/ or csrc/: the round function is written from the paper (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
key increments 0x9E3779B9 / 0xBB67AE85) and pinned by the three Random123 known-answer vectors (tests/test_philox_witness.py).  The
stream contract of include/t4k.h on top of it:

    element a of a draw that starts at stream offset `off` (in elements) = word (a & 3) of Philox(counter, key) with
    counter = (off // 4 + a // 4) mod 2^64 as (lo, hi, 0, 0) and key = (lo(seed), hi(seed));
    u = fma(float(word), 2^-32, 2^-33) in (0, 1]; a dropout mask is u > alpha; a normal pair is Box-Muller on words (0, 1) and (2, 3).
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_PM0, _PM1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)

# ---- the positions the far-stream tests visit (tests/test_gpu_philox_far.py); offsets in elements, nq = counters of the first draw = ceil(n / 4)
SEED_P0, SEED_P1, SEED_P2, SEED_P3, SEED_P4 = 777, 0x9E3779B97F4A7C15, 0xFFFFFFFF00000001, 1 << 32, 5
POSITIONS = {
    "P0": (SEED_P0, lambda nq: 0),                                           # control: both high words zero
    "P1": (SEED_P1, lambda nq: 2 ** 34 - 4 * (nq // 2)),                     # the draw straddles the carry into the high counter word; high key word set
    "P2": (SEED_P2, lambda nq: 2 ** 36 + 12 * 4),                            # high counter word 16 throughout
    "P3": (SEED_P3, lambda nq: 4096),                                        # only the high key word set
    "P4": (SEED_P4, lambda nq: (2 ** 64 - 4 * (nq // 2)) % 2 ** 64),         # the element offset wraps mod 2^64 inside the draw (counter 2^62: a carry into the high word)
}


def position(name, n):
    """(seed, offset) of position `name` for a first draw of n elements"""
    seed, off = POSITIONS[name]
    return seed, off((n + 3) // 4)


# ---- the tail of the normal draw: the smallest word feeding a u1 (words 0 and 2 of a counter) within the first 2^24 counters of SEED_P1.
# Found by a scan (4.7 s on a CPU); the tests recompute this one counter only.
TAIL_SEED, TAIL_COUNTER, TAIL_SLOT, TAIL_WORD = SEED_P1, 1904343, 2, 154
# worst |oracle - normal64| / (2^-24 rad) of the CPU oracle's normal draw (glibc logf / sqrtf / cosf / sinf in fp32) over 100 001 draws at each
# of P0 .. P4, the 400 001 draws straddling element 2^34 of SEED_P1 and the 256 draws round the tail counter: measured 2.637, at P4 (tests/README.md)
NORMAL_ORACLE_WORST = 2.64


def philox4x32_10(ctr4, key):
    """ctr4: uint32[n, 4] counter words, key: two uint32 key words -> uint32[n, 4]"""
    c = np.asarray(ctr4, dtype=np.uint64).reshape(-1, 4) & M32
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _PM0 * c0, _PM1 * c2                                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def counters(off, n):
    """the 64-bit counters of a draw of n elements from stream offset `off`: off // 4 + i, wrapping mod 2^64.  `off` is a Python int and
    may exceed 2^64: a reported offset (uint64, in elements) wraps at counter 2^62, the counter itself goes on - the stage behind a draw
    that crossed element 2^64 sits at the unwrapped offset + 4 ceil(n / 4)."""
    nq = (int(n) + 3) // 4
    base = (int(off) // 4) % 2 ** 64
    lo = np.arange(nq, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return np.uint64(base) + lo                                          # uint64 addition wraps mod 2^64


def words_at(q, seed):
    """the four output words of every 64-bit counter in q under the 64-bit seed -> uint32[len(q), 4]"""
    q = np.asarray(q, dtype=np.uint64)
    z = np.zeros_like(q)
    seed = int(seed) % 2 ** 64
    return philox4x32_10(np.stack([q & M32, q >> _S32, z, z], axis=1), (seed & 0xFFFFFFFF, seed >> 32))


def words(seed, off, n):
    """the n stream words (uint32) from offset `off`"""
    return words_at(counters(off, n), seed).reshape(-1)[:int(n)]


def u01(w):
    """uint32 word -> float32 in (0, 1]: float(x) * 2^-32 + 2^-33 with ONE rounding (the sum is exact in float64), i.e. the kernels' fmaf"""
    x = np.asarray(w, dtype=np.uint32).astype(np.float32).astype(np.float64)
    return (x * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)


def uniform(seed, off, n):
    return u01(words(seed, off, n))


def mask(seed, off, n, alpha):
    """the 0 / 1 mask of a dropout layer: keep where u > alpha"""
    return (uniform(seed, off, n) > np.float32(alpha)).astype(np.float32)


def end_offset(off, n, world=1):
    """the offset reported (uint64, so mod 2^64) behind a draw of n elements; a sample-keyed draw of a `world`-rank shard moves the
    stream by the whole batch's"""
    return (int(off) // 4 * 4 + 4 * int(world) * ((int(n) + 3) // 4)) % 2 ** 64


def normal64(seed, off, n):
    """float64 witness of the Box-Muller draw: (values, rad) per element.  Only the kernels' fp32 roundings of the INPUTS are followed -
    u1, u2 as above and ang = float32(float32(2 pi) * u2) - then sqrt(-2 ln u1), cos, sin and the products in float64."""
    nq = (int(n) + 3) // 4
    u = u01(words_at(counters(off, n), seed)).reshape(nq, 2, 2)              # [counter][pair][u1, u2]
    u1, u2 = u[:, :, 0], u[:, :, 1]
    ang = (np.float32(6.2831853071795865) * u2).astype(np.float32).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    v = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=2).reshape(-1)[:int(n)]
    return v, np.repeat(rad.reshape(-1), 2)[:int(n)]


def normal_ratio(got, seed, off, n):
    """|got - normal64| / (2^-24 rad), element by element (u1 = 1 gives rad = 0: the value must then be 0 exactly)"""
    v, rad = normal64(seed, off, n)
    d = np.abs(np.asarray(got, np.float64).reshape(-1) - v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(rad > 0, d / (2.0 ** -24 * rad), np.where(d > 0, np.inf, 0.0))
