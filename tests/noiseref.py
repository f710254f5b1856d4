"""numpy restatement of csrc/noise.hip (tests/test_noise_cpu.py, tests/test_noise_gpu.py).  Not a conftest: plain functions only.

Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw, SC'11; the Random123 constants) in uint64 arithmetic, the word layout of
pbe_philox_u32 and the Box-Muller of pbe_randn_philox_f32 evaluated in float64.  u and v are exact in fp32 (24-bit integers times
2^-24), so randn64 is the mathematical value of the definition; what the device adds is the fp32 rounding of logf, sqrtf, sincospif
and two products.

MEASURED (one MI355X, the case table below, 40 236 elements): the largest |device - randn64| is 5.094e-7, recorded rounded up as
RANDN_MEASURED_MAX_ABS_ERR = 5.1e-7 - 1.07 units in the last place of r, 2.9 of the element itself (2^20 elements of another seed, not
in the table: 6.4e-7; numpy fp32 arithmetic with the angle formed as 2 pi v in fp32 gives 1.2e-6).  In units in the last place: r <= sqrt(-2 ln 2^-24) = 5.77 lies in [4, 8), where one fp32 ulp is 2^-21 = 4.77e-7; r itself carries the rounding of
logf (<= 1 ulp of a value <= 16.7, i.e. <= 1.9e-6 before the square root halves its relative size), of the product by -2 (exact), and
of sqrtf (correctly rounded, half an ulp); sin / cos carry sincospif's, and the final product half an ulp more.  The gate RANDN_ABS_TOL
is 4 x the measured maximum: the inputs change with every seed, so the margin covers unseen arguments of logf and sincospif.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)

STREAM_X_T, STREAM_POST_EPS, STREAM_STEP0 = 0, 1, 16

RANDN_MEASURED_MAX_ABS_ERR = 5.1e-7      # see the module docstring
RANDN_ABS_TOL = 4 * RANDN_MEASURED_MAX_ABS_ERR

# statistics (issue: about five standard errors at n = 16384; conditions, not measurements)
STAT_N = 16384
STAT_MEAN, STAT_STD, STAT_CORR = 0.04, 0.03, 0.04
STAT_SEEDS = (0, 1, 42, (1 << 63) + 5)

# The Random123 known answers: (counter, key, words)
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

# (n, seeds [B], sub or None, stream): a pruned table - every n with B = 1 and B = 3, every seed, sub and stream value at least twice,
# the extremes together.  n: 1, 3, 4, 5 around one counter; 1023, 1024, 1025 around a workgroup of 256 counters; 4 * 33 * 47 a latent.
N_VALUES = (1, 3, 4, 5, 1023, 1024, 1025, 4 * 33 * 47)
SEEDS = (0, 1, 1 << 32, (1 << 63) + 5, (1 << 64) - 1)
SUBS = (None, 0, 1, (1 << 31) - 1)
STREAMS = (0, 1, 16, (1 << 32) + 3)


def _cases():
    out = []
    for i, n in enumerate(N_VALUES):
        s1 = SEEDS[i % 5]
        out.append((n, (s1,), None if SUBS[i % 4] is None else (SUBS[i % 4],), STREAMS[i % 4]))
        s3 = (SEEDS[(i + 1) % 5], SEEDS[(i + 2) % 5], SEEDS[(i + 4) % 5])
        sub = SUBS[(i + 1) % 4]
        out.append((n, s3, None if sub is None else (sub, SUBS[(i + 2) % 4] or 0, SUBS[(i + 3) % 4] or 0), STREAMS[(i + 2) % 4]))
    out.append((5, ((1 << 64) - 1,), ((1 << 31) - 1,), (1 << 32) + 3))          # every field at its extreme
    out.append((1025, SEEDS[:3], (0, 1, (1 << 31) - 1), 1))
    return tuple(out)


CASES = _cases()

# (seed, sub, stream, elements): counters whose u is exactly 1 (the word's top 24 bits are all ones), found by a search over sub at q = 0.
# r = sqrt(-2 ln 1) = 0 there, so the two elements are zeros whatever the angle.
ZERO_RADIUS = ((0, 5150801, 0, (0, 1)), (0, 921823, 0, (2, 3)))


def philox4x32_10(counter, key):
    """counter: uint array [..., 4], key: [..., 2] (broadcast against each other) -> uint32 [..., 4].  uint64 arithmetic throughout."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] & MASK32 for i in range(4))
    k0, k1 = k[..., 0] & MASK32, k[..., 1] & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2             # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def words(seed: int, sub: int, stream: int, n: int) -> np.ndarray:
    """The first n words of one sample: uint32 [n], word w = x[w % 4] of counter (w // 4, sub, stream lo32, stream hi32)."""
    assert 0 <= seed < 1 << 64 and 0 <= sub < 1 << 32 and 0 <= stream < 1 << 64
    nq = (n + 3) // 4
    ctr = np.empty((nq, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nq, dtype=np.uint64)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = sub, stream & 0xFFFFFFFF, stream >> 32
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32_10(ctr, key).reshape(-1)[:n]


def uniforms(seed: int, sub: int, stream: int, n: int):
    """(u, v) float64 per PAIR of elements: u in (0, 1], v in [0, 1), both exact."""
    w = words(seed, sub, stream, (n + 3) // 4 * 4).astype(np.uint64)
    u = ((w[0::2] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    v = (w[1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u, v


def randn64(seed: int, sub: int, stream: int, n: int) -> np.ndarray:
    """The definition in float64: elements 2p, 2p + 1 = r cos(2 pi v), r sin(2 pi v), r = sqrt(-2 ln u), from word pair p."""
    u, v = uniforms(seed, sub, stream, n)
    r = np.sqrt(-2.0 * np.log(u))
    out = np.empty(2 * u.size, dtype=np.float64)
    out[0::2], out[1::2] = r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v)
    return out[:n]


def as_i64(seed: int) -> int:
    """The int64 value that holds an unsigned 64-bit seed."""
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def corr(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def check_stats(draw) -> dict:
    """The issue's conditions on draw(seed, stream, n) -> array: returns the largest figures and asserts the limits."""
    worst = {"mean": 0.0, "std": 0.0, "corr": 0.0}
    n = STAT_N
    for seed in STAT_SEEDS:
        z = np.asarray(draw(seed, 0, n), np.float64)
        worst["mean"] = max(worst["mean"], abs(float(z.mean())))
        worst["std"] = max(worst["std"], abs(float(z.std()) - 1.0))
        worst["corr"] = max(worst["corr"], abs(corr(z, draw(seed, 1, n))), abs(corr(z[:-1], z[1:])))
    worst["corr"] = max(worst["corr"], abs(corr(draw(7, 0, n), draw(8, 0, n))))
    print("noise statistics:", worst)
    assert worst["mean"] <= STAT_MEAN and worst["std"] <= STAT_STD and worst["corr"] <= STAT_CORR, worst
    return worst
