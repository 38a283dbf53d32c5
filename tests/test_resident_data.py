"""CPU checks of the device-resident dataset (data.ResidentDataset / DatasetView): the
shuffled epoch order, rank shards, random_split's rows, the integer shift rule, the CPU batch
against pad_and_translate, IDX files, and the new C entry points' argument checks."""
import gzip

import numpy as np
import pytest
import torch

from torch_scae_amd import data as D


def _philox_ref(c, k0, k1, rounds):
    """Philox4x32 on Python ints (the reference for the limb arithmetic of data._philox)."""
    M = 0xFFFFFFFF
    c = list(c)
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M, (p0 >> 32) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c


def test_philox_limbs_match_python_integers():
    g = np.random.default_rng(0)
    words = [torch.tensor(g.integers(0, 2 ** 32, 257), dtype=torch.int64) for _ in range(4)]
    words[0][:3] = torch.tensor([0, 0xFFFFFFFF, 0x80000000])
    got = D._philox(words, 0xDEADBEEF, 0xFFFFFFFF, 10)
    for i in range(257):
        want = _philox_ref([int(w[i]) for w in words], 0xDEADBEEF, 0xFFFFFFFF, 10)
        assert [int(g_[i]) for g_ in got] == want


@pytest.mark.parametrize("n", [1, 2, 3, 127, 128, 1000, 55000, 60000])
def test_feistel_order_is_a_bijection(n):
    p = torch.arange(n)
    order = D.feistel_order(p, n, seed=11, epoch=0)
    assert torch.equal(order.sort().values, p)
    if n >= 127:
        assert not torch.equal(order, p)
        assert not torch.equal(order, D.feistel_order(p, n, seed=11, epoch=1))
        assert not torch.equal(order, D.feistel_order(p, n, seed=12, epoch=0))


def test_identity_order_without_shuffle():
    ds = D.ResidentDataset(torch.zeros(50, 4, 4, dtype=torch.uint8), torch.arange(50),
                           out_size=(4, 4), device="cpu")
    v = ds.view(shuffle=False, translate=False)
    rows, shifts = v.indices_and_shifts(3, 1, 16)
    assert torch.equal(rows, torch.arange(16, 32))
    assert not shifts.any()


@pytest.mark.parametrize("shuffle", [False, True])
def test_rank_shards_are_disjoint_and_cover_the_epoch(shuffle):
    n, B, world = 1003, 16, 3
    ds = D.ResidentDataset(torch.zeros(n, 2, 2, dtype=torch.uint8), torch.zeros(n, dtype=torch.long),
                           out_size=(2, 2), device="cpu")
    views = [ds.view(shuffle=shuffle, seed=4, rank=r, world=world) for r in range(world)]
    steps = views[0].steps_per_epoch(B)
    assert steps == n // (world * B)
    seen = torch.cat([v.indices_and_shifts(2, s, B)[0] for v in views for s in range(steps)])
    assert seen.numel() == world * B * steps == torch.unique(seen).numel()


def test_split_gives_random_splits_rows():
    n = 600
    ds = D.ResidentDataset(torch.zeros(n, 2, 2), torch.zeros(n, dtype=torch.long), out_size=(2, 2),
                           device="cpu")
    views = ds.split([550, 50], generator=torch.Generator().manual_seed(42))
    want = torch.utils.data.random_split(range(n), [550, 50],
                                         generator=torch.Generator().manual_seed(42))
    for v, w in zip(views, want):
        assert v.index.tolist() == list(w.indices)


def test_integer_shift_rule_matches_float64_round_and_torchvision_weights():
    g = torch.Generator().manual_seed(0)
    r = torch.randint(0, 2 ** 24, (400000,), generator=g)
    r[:4] = torch.tensor([0, 2 ** 23, 2 ** 24 - 1, 2 ** 22])
    for pad in (0, 1, 3, 6):
        got = D.shift_rule(r, pad)
        want = torch.round(-pad + 2 * pad * (r.double() / 2 ** 24)).to(torch.int64)
        assert torch.equal(got, want), pad
    # a draw of positions: torchvision's half-weight ends, equal interior weights
    s = D.translate_shifts(torch.arange(400000), 0, 9, (6, 6))
    for col in (0, 1):
        h = torch.bincount(s[:, col] + 6, minlength=13).double() / s.shape[0]
        assert torch.allclose(h[1:12], torch.full((11,), 1 / 12, dtype=torch.float64),
                              atol=3e-3)
        assert torch.allclose(h[[0, 12]], torch.full((2,), 1 / 24, dtype=torch.float64),
                              atol=2e-3)
    assert D.translate_shifts(torch.arange(8), 0, 9, (0, 0)).abs().sum() == 0


@pytest.mark.parametrize("u8", [True, False])
def test_cpu_batch_is_pad_and_translate_of_the_rows(u8):
    g = torch.Generator().manual_seed(3)
    n = 97
    imgs = torch.randint(0, 256, (n, 1, 28, 28), generator=g, dtype=torch.uint8)
    if not u8:
        imgs = imgs.float() / 255
    labels = torch.randint(0, 10, (n,), generator=g)
    ds = D.ResidentDataset(imgs, labels, out_size=(40, 40), device="cpu")
    v = ds.view(shuffle=True, seed=5)
    image, label = v.batch(1, 2, 16)
    rows, shifts = v.indices_and_shifts(1, 2, 16)
    assert shifts.abs().max() <= 6 and shifts.abs().max() > 0
    assert torch.equal(image, D.pad_and_translate(imgs[rows], (40, 40), shifts=shifts))
    assert torch.equal(label, labels[rows])


def test_take_step_wraps_and_state_round_trips():
    ds = D.ResidentDataset(torch.zeros(70, 2, 2), torch.zeros(70, dtype=torch.long), out_size=(2, 2),
                           device="cpu")
    v = ds.view(shuffle=True, seed=1)
    assert [v.take_step(16) for _ in range(5)] == [(0, 0), (0, 16), (0, 32), (0, 48), (1, 0)]
    sd = v.state_dict()
    w = ds.view(shuffle=True, seed=1)
    w.load_state_dict(sd)
    assert [w.take_step(16) for _ in range(3)] == [v.take_step(16) for _ in range(3)]


@pytest.mark.parametrize("gz", [False, True])
def test_read_idx_round_trip(tmp_path, gz):
    cases = [(np.arange(2 * 5 * 3, dtype=np.uint8).reshape(2, 5, 3), 0x08, ">u1"),
             (np.array([7, 1, 255], dtype=np.uint8), 0x08, ">u1"),
             (np.arange(6, dtype=np.int32).reshape(3, 2) - 3, 0x0C, ">i4"),
             (np.linspace(0, 1, 4).astype(np.float32), 0x0D, ">f4")]
    for i, (a, code, big) in enumerate(cases):
        raw = bytes([0, 0, code, a.ndim]) + \
            b"".join(int(d).to_bytes(4, "big") for d in a.shape) + a.astype(big).tobytes()
        path = tmp_path / (f"a{i}.idx" + (".gz" if gz else ""))
        path.write_bytes(gzip.compress(raw) if gz else raw)
        t = D.read_idx(str(path))
        assert t.shape == a.shape and np.array_equal(t.numpy(), a)
    bad = tmp_path / "bad"
    bad.write_bytes(b"\x01\x02\x03\x04")
    with pytest.raises(ValueError):
        D.read_idx(str(bad))


def test_views_reject_bad_arguments():
    ds = D.ResidentDataset(torch.zeros(10, 2, 2), torch.zeros(10, dtype=torch.long), out_size=(4, 4),
                           device="cpu")
    with pytest.raises(ValueError):
        ds.view(rank=2, world=2)
    with pytest.raises(ValueError):
        D.DatasetView(ds, torch.tensor([0, 10]))
    with pytest.raises(ValueError):
        ds.split([5, 4])
    with pytest.raises(ValueError):
        D.ResidentDataset(torch.zeros(4, 5, 2, 2), torch.zeros(4, dtype=torch.long), out_size=(2, 2),
                          device="cpu")     # C > 4
    with pytest.raises(ValueError):
        D.ResidentDataset(torch.zeros(4, 1, 6, 6), torch.zeros(4, dtype=torch.long), out_size=(4, 4),
                          device="cpu")     # smaller output


def test_source_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes
    from torch_scae_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)       # (never dereferenced: every call below is refused)

    def desc(**kw):
        d = _lib.BatchSourceDesc()
        d.images, d.labels, d.rows, d.n = 0x1000, 0x1000, 100, 100
        d.C, d.h, d.w, d.H, d.W, d.world = 1, 28, 28, 40, 40, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert lib.scae_gather_batch_f32(fake, fake, 4, None, None) == -1
    assert lib.scae_gather_batch_f32(None, fake, 4, desc(), None) == -1     # no destination
    for bad in (dict(images=None), dict(n=0), dict(n=101), dict(h=41), dict(w=0),
                dict(rank=1), dict(world=0), dict(epoch=-1), dict(position=97),
                dict(image_u8=2), dict(labels=None)):
        assert lib.scae_gather_batch_f32(fake, fake, 4, desc(**bad), None) == -1, bad
    assert lib.scae_gather_batch_f32(fake, fake, 0, desc(), None) == -1
    assert lib.scae_gather_batch_f32(fake, fake, 4, desc(C=5), None) == -2
    assert lib.scae_gather_batch_f32(fake, fake, 51, desc(rank=1, world=2), None) == -1
    assert lib.scae_step_prologue_source_f32(fake, fake, 4, None, None, 0, None, None,
                                             None, None) == -1
    assert lib.scae_step_prologue_source_f32(None, fake, 4, desc(), None, 0, None, None,
                                             None, None) == -1
    first = _lib.FirstLayerDesc()          # describes no batch of the source
    assert lib.scae_step_prologue_source_f32(fake, fake, 4, desc(), None, 0, None, None,
                                             first, None) == -1
    assert lib.scae_step_prologue_source_f32(fake, fake, 4, desc(), fake, 16, None, None,
                                             None, None) == -1          # noise w/o state
