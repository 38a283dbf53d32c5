"""Philox4x32 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC'11) written from its definition on numpy uint64, and the layout of the device noise
generator's draws on top of it (csrc/noise_dev.h).  The reference of tests/test_philox_ref.py
and tests/test_noise_gpu.py; it imports nothing from torch_scae_amd.

One round on the counter (c0, c1, c2, c3) with the round key (k0, k1):

    hi0:lo0 = M0 * c0        hi1:lo1 = M1 * c2          (32 x 32 -> 64 bit products)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)

and between rounds the key is bumped by the Weyl constants (W0, W1) mod 2^32.

A draw of n floats by launch number ``launch`` of the generator seeded ``seed``: group g of
four outputs is philox4x32((g & M32, g >> 32, launch & M32, launch >> 32),
(seed & M32, seed >> 32)); output e of group g is (word_e >> 8) * 2^-24, which float32 holds
exactly; the last group is cut to n.  (g >> 32 is live only from 2^34 floats = 64 GiB in one
draw on: no test reaches it.)
"""
import numpy as np
import torch

M32 = 0xFFFFFFFF
M63 = (1 << 63) - 1
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85

# One pass of the generator's grid: it is capped at 2048 workgroups of 256 threads, each
# thread writing a group of 4 floats per pass (noise_dev.h, blocks_for).
PASS = 2048 * 256 * 4


def step_draw_sizes(B, P, O, V):
    """What SCAE._draw_noise asks for per step at batch B with P part capsules, O object
    capsules and V votes: its three slices -- part encoder (B, P), capsule (B, O, 1), votes
    (B, O, V) -- the training draw (all three) and the evaluation draw (the last two)."""
    a, b, c = B * P, B * O, B * O * V
    return [a, b, c, a + b + c, b + c]


# the sizes every device comparison runs at: the ragged tails of a group of 4 and of a
# workgroup, the existing test's size, the per-step draws at cfg-2 (B 128, 24 / 24) and at the
# 48 / 64 shape (B 1024), exactly one pass of the capped grid, one float more, and three
# passes with a ragged tail
DRAW_SIZES = sorted({1, 2, 3, 4, 5, 1023, 1024, 1025, 79872,
                     *step_draw_sizes(128, 24, 24, 24), *step_draw_sizes(1024, 48, 64, 48),
                     PASS, PASS + 1, 2 * PASS + 4099})
# torch seeds: the key's low word alone, its high word alone (2^32), both full (2^63 - 1)
SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1]
# launch counters written into the state: the carry into the counter's high word
CARRY_LAUNCHES = [2 ** 32 - 1, 2 ** 32]
NOISE_SALT = 0x123456789ABCDEF & M63     # a non-zero StepPlan.noise_salt


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def philox4x32(counter4, key2, rounds=10, multipliers=(PHILOX_M0, PHILOX_M1)):
    """-> the four output words (numpy uint64 holding uint32 values; arrays where a counter
    or key word is one).  ``counter4`` / ``key2``: words in [0, 2^32), ints or arrays."""
    c0, c1, c2, c3 = (_u64(w) for w in counter4)
    k0, k1 = (_u64(w) for w in key2)
    m0, m1 = (np.uint64(m) for m in multipliers)
    mask, s32 = np.uint64(M32), np.uint64(32)
    for w in (c0, c1, c2, c3, k0, k1):
        assert (w <= mask).all(), "words are 32 bits"
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2           # < 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & mask, (k1 + np.uint64(PHILOX_W1)) & mask
    return c0, c1, c2, c3


def counter_of(g, launch):
    """Counter words of output group(s) g of launch number ``launch``."""
    g = _u64(g)
    return g & np.uint64(M32), g >> np.uint64(32), launch & M32, launch >> 32


def uniform_ref(seed, launch, n, philox=philox4x32, counter=counter_of):
    """-> np.float32[n]: the draw of n floats by launch ``launch`` of the generator seeded
    ``seed`` (both in [0, 2^64)).  ``philox`` / ``counter``: replaced only by the deliberately
    wrong variants of tests/test_philox_ref.py."""
    assert 0 <= seed < 1 << 64 and 0 <= launch < 1 << 64 and n >= 0
    groups = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox(counter(groups, launch), (seed & M32, seed >> 32))
    k = np.stack([np.broadcast_to(w, groups.shape) for w in words], 1).reshape(-1)[:n]
    k = k >> np.uint64(8)                                   # 24 bits
    return k.astype(np.float32) * np.float32(2.0 ** -24)    # exact: k < 2^24


def effective_seed(torch_seed, salt=0):
    """The generator seed of a plan whose ``noise_salt`` is ``salt`` under torch's seed."""
    return (int(torch_seed) ^ int(salt)) & M63


def _bits(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    x = x.detach().cpu().contiguous().reshape(-1)
    assert x.dtype == torch.float32, x.dtype
    return x.view(torch.int32)


def same_bits(got, want):
    """True when two float32 arrays / tensors (host or device) hold the same bits: equality of
    their int32 views, no tolerance."""
    a, b = _bits(got), _bits(want)
    return a.shape == b.shape and torch.equal(a, b)


def first_difference(got, want):
    """For an assertion's message: (index, got bits, want bits) of the first differing float,
    a shape pair for unequal lengths, None for equal bits."""
    a, b = _bits(got), _bits(want)
    if a.shape != b.shape:
        return tuple(a.shape), tuple(b.shape)
    d = (a != b).nonzero()
    if d.numel() == 0:
        return None
    i = int(d[0])
    return i, hex(int(a[i]) & M32), hex(int(b[i]) & M32)
