"""tests/philox_ref.py against the published Philox4x32-10 known-answer vectors, the package's
host mirrors of Philox (data._philox, which cluster.kmeans_pp_host draws through) against
both, the shape of ``uniform_ref``'s outputs, and proof that the cases of
tests/test_noise_gpu.py tell a wrong generator from the right one."""
import functools

import numpy as np
import pytest
import torch

from tests import philox_ref as R
from tests.philox_ref import M32, philox4x32, same_bits, uniform_ref

# Random123's kat_vectors, philox4x32 at 10 rounds: (counter, key, expected)
KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_reference_gives_the_published_vectors(counter, key, want):
    assert tuple(int(w) for w in philox4x32(counter, key)) == want
    # ... and as one lane of an array
    lanes = [np.array([1, c, 2], dtype=np.uint64) for c in counter]
    got = philox4x32(lanes, key, rounds=10)
    assert tuple(int(w[1]) for w in got) == want


@pytest.mark.parametrize("counter,key,want", KAT)
def test_data_philox_gives_the_published_vectors(counter, key, want):
    from torch_scae_amd import data as D
    c = [torch.tensor([w], dtype=torch.int64) for w in counter]
    got = D._philox(c, key[0], key[1], 10)
    assert tuple(int(w[0]) for w in got) == want


@pytest.mark.parametrize("rounds", [3, 10])
def test_data_philox_agrees_with_the_reference(rounds):
    """3 rounds is the Feistel round function's setting (data._F_PHILOX_ROUNDS), 10 the key
    and shift draws' and k-means++'s; counters and keys with words >= 2^31 included."""
    from torch_scae_amd import data as D
    assert D._F_PHILOX_ROUNDS == 3 and D._KEY_PHILOX_ROUNDS == 10
    g = np.random.default_rng(rounds)
    n = 300
    words = [g.integers(0, 2 ** 32, n, dtype=np.uint64) for _ in range(4)]
    edge = [0, 1, 0x7FFFFFFF, 0x80000000, 0x80000001, M32]
    for i, w in enumerate(words):
        w[:len(edge)] = np.roll(edge, i)
    assert sum(int((w >= 2 ** 31).sum()) for w in words) > n
    keys = [(0, 0), (M32, M32), (0x80000000, 0x7FFFFFFF),
            *[tuple(int(v) for v in g.integers(0, 2 ** 32, 2, dtype=np.uint64))
              for _ in range(5)]]
    for k0, k1 in keys:
        want = philox4x32(words, (k0, k1), rounds=rounds)
        got = D._philox([torch.from_numpy(w.astype(np.int64)) for w in words], k0, k1, rounds)
        for a, b in zip(got, want):
            assert a.dtype == torch.int64
            assert np.array_equal(a.numpy().astype(np.uint64), b), (k0, k1)


def test_kmeans_pp_uniform_draws_through_the_reference():
    """cluster.pp_uniform(seed, restart, j) = the first word's 24 bits of
    philox4x32((j, 0, 0, tag), (seed, restart)) scaled by 2^-24."""
    from torch_scae_amd import cluster as C
    for seed, restart, j in [(11, 0, 0), (11, 1, 0), (M32, 7, 5), (0x80000000, 3, 1000)]:
        w0 = int(philox4x32((j, 0, 0, C._TAG_KMPP), (seed & M32, restart))[0])
        assert float(C.pp_uniform(seed, restart, j)) == (w0 >> 8) * 2.0 ** -24


def test_uniform_ref_values_and_prefixes():
    seed, launch = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    full = uniform_ref(seed, launch, 4099)
    assert full.dtype == np.float32 and full.shape == (4099,)
    k = full.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.floor(k)) and k.min() >= 0 and k.max() < 2 ** 24
    assert float(full.max()) < 1.0
    # word e of group g, by hand
    for g_, e in [(0, 0), (0, 3), (1, 2), (1024, 1)]:
        w = philox4x32((g_, 0, launch & M32, launch >> 32), (seed & M32, seed >> 32))[e]
        assert full[4 * g_ + e] == np.float32((int(w) >> 8) * 2.0 ** -24)
    for n in (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 4098):
        assert same_bits(uniform_ref(seed, launch, n), full[:n]), n
    assert not same_bits(uniform_ref(seed, launch + 1, 64), full[:64])
    assert not same_bits(uniform_ref(seed + 1, launch, 64), full[:64])


def test_same_bits_is_exact():
    a = uniform_ref(3, 4, 1025)
    assert same_bits(a, a.copy()) and same_bits(torch.from_numpy(a), a)
    assert R.first_difference(a, a.copy()) is None
    b = a.copy()
    b.view(np.int32)[1024] ^= 1                       # one ulp in the last float
    assert not same_bits(a, b) and R.first_difference(b, a)[0] == 1024
    assert not same_bits(a, a[:-1])
    z = np.zeros(4, np.float32)
    assert not same_bits(z, -z)                       # 0.0 == -0.0 as floats, not as bits


# -- the device tests' cases distinguish wrong generators ------------------------------------------
WRONG = {
    "multipliers swapped": dict(
        philox=functools.partial(philox4x32, multipliers=(R.PHILOX_M1, R.PHILOX_M0))),
    "launch high word dropped": dict(
        counter=lambda g, launch: R.counter_of(g, launch & M32)),
    "launch off by one": dict(
        counter=lambda g, launch: R.counter_of(g, launch + 1)),
    "seed high word dropped": dict(
        philox=lambda c, k, **kw: philox4x32(c, (k[0], 0), **kw)),
    "output words reversed": dict(
        philox=lambda c, k, **kw: philox4x32(c, k, **kw)[::-1]),
    "second pass repeats the first": dict(
        counter=lambda g, launch: R.counter_of(
            np.asarray(g, dtype=np.uint64) % np.uint64(R.PASS // 4), launch)),
}


def test_sizes_cover_what_the_issue_names():
    assert {1, 2, 3, 4, 5, 1023, 1024, 1025, 79872, 2097152, 2097153,
            2 * 2097152 + 4099} <= set(R.DRAW_SIZES)
    assert {128 * 24, 128 * 24 * 24, 79872} <= set(R.DRAW_SIZES)                # cfg-2
    assert {1024 * 48, 1024 * 64, 1024 * 64 * 48, 1024 * (48 + 64 + 64 * 48)} \
        <= set(R.DRAW_SIZES)                                                    # 48 / 64
    assert 4 * max(R.DRAW_SIZES) < 20e6                                         # bytes
    assert R.SEEDS == [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1]


@pytest.mark.parametrize("name", ["multipliers swapped", "launch off by one",
                                  "output words reversed"])
def test_a_wrong_generator_is_a_mismatch_at_every_size_and_seed(name):
    """Errors that change every group: the comparison reports them at each size (first launch
    of seed 1234) and, at the smallest and a mid size, for each seed, the salted seed and each
    written counter."""
    wrong = WRONG[name]
    for n in R.DRAW_SIZES:
        assert not same_bits(uniform_ref(1234, 0, n, **wrong), uniform_ref(1234, 0, n)), n
    seeds = [*R.SEEDS, R.effective_seed(1234, R.NOISE_SALT)]
    for seed in seeds:
        for launch in (0, 1, 2, *R.CARRY_LAUNCHES):
            for n in (1, 1025):
                assert not same_bits(uniform_ref(seed, launch, n, **wrong),
                                     uniform_ref(seed, launch, n)), (seed, launch, n)


def test_a_dropped_high_word_is_a_mismatch_where_that_word_is_live():
    """Dropping the launch counter's high word shows at launch 2^32 (the draw after the
    written 2^32 - 1) and nowhere below; dropping the seed's shows at seeds 2^32 and
    2^63 - 1 and under the salt: the cases that carry those words are in the lists."""
    lw, sw = WRONG["launch high word dropped"], WRONG["seed high word dropped"]
    assert R.CARRY_LAUNCHES == [2 ** 32 - 1, 2 ** 32]
    for n in (1, 5, 1025):
        for seed in R.SEEDS:
            assert same_bits(uniform_ref(seed, 2 ** 32 - 1, n, **lw),
                             uniform_ref(seed, 2 ** 32 - 1, n))
            assert not same_bits(uniform_ref(seed, 2 ** 32, n, **lw),
                                 uniform_ref(seed, 2 ** 32, n)), (seed, n)
        live = [s for s in R.SEEDS if s >> 32]
        assert live == [2 ** 32, 2 ** 63 - 1]
        for seed in [*live, R.effective_seed(1234, R.NOISE_SALT)]:
            assert not same_bits(uniform_ref(seed, 0, n, **sw), uniform_ref(seed, 0, n))
        for seed in (0, 1, 2 ** 32 - 1):
            assert same_bits(uniform_ref(seed, 0, n, **sw), uniform_ref(seed, 0, n))


def test_a_wrong_grid_stride_is_a_mismatch_past_one_pass():
    """A second pass that redraws the first one's groups: equal up to exactly one pass of the
    capped grid, a mismatch from one float more on."""
    wrong = WRONG["second pass repeats the first"]
    for n in R.DRAW_SIZES:
        same = same_bits(uniform_ref(7, 3, n, **wrong), uniform_ref(7, 3, n))
        assert same == (n <= R.PASS), n
    assert sum(n > R.PASS for n in R.DRAW_SIZES) >= 3
