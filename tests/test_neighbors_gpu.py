"""The k-NN kernels (csrc/knn.hip) against the numpy restatement (neighbors.*_host).  The rules
define arithmetic that float32 numpy reproduces and a total order, so every comparison is
``torch.equal``: no tolerance, nothing screened."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_neighbors import duplicated, grid, uniform
from torch_scae_amd import _lib
from torch_scae_amd import neighbors as NB

pytestmark = pytest.mark.gpu


def groups(Nq, Nb):
    return _lib.load().scae_knn_groups(Nq, Nb)


def same(dev, host):
    assert dev.idx.is_cuda and dev.idx.dtype == torch.int64 and dev.d2.dtype == torch.float32
    assert dev.idx.shape == host.idx.shape and dev.d2.shape == host.d2.shape
    assert torch.equal(dev.idx.cpu(), host.idx)
    assert torch.equal(dev.d2.cpu(), host.d2)


# (Nq, Nb, F, k, the groups the shape is here for: None = whatever scae_knn_groups says)
SHAPES = [(1, 1, 1, 1, 1), (3, 70, 1, 1, 1), (65, 257, 24, 20, 1),
          (257, 4099, 33, 64, None),              # F one above the register form
          (64, 1000, 256, 5, 1),
          (100, 2000, 24, 20, "many"),            # uneven groups: 2000 rows over 3
          (300, 511, 7, 9, 1)]


@pytest.mark.parametrize("Nq, Nb, F, k, G", SHAPES)
def test_search_against_the_host(Nq, Nb, F, k, G):
    if G == "many":
        assert groups(Nq, Nb) >= 2
    elif G is not None:
        assert groups(Nq, Nb) == G
    q, b = uniform(Nq, F, 100 + Nq), uniform(Nb, F, 200 + Nb)
    same(NB.knn(q.cuda(), k, b.cuda()), NB.knn_host(q, k, b))


@pytest.mark.parametrize("N, F, k", [(513, 24, 12), (65, 5, 64), (1100, 40, 3)])
def test_self_mode_against_the_host(N, F, k):
    x = uniform(N, F, 300 + N)
    got = NB.knn(x.cuda(), k)
    same(got, NB.knn_host(x, k))
    assert not bool((got.idx.cpu() == torch.arange(N)[:, None]).any())
    if k == N - 1:      # the whole order: every other row, once
        rows = torch.arange(N)
        want = torch.stack([rows[rows != i] for i in range(N)])
        assert torch.equal(got.idx.sort(1).values.cpu(), want)


def test_ties_take_the_lowest_indices_across_groups():
    x = grid(500)
    same(NB.knn(x.cuda(), 20), NB.knn_host(x, 20))
    b = grid(1500, seed=1)
    assert groups(40, 1500) >= 2
    same(NB.knn(x[:40].cuda(), 64, b.cuda()), NB.knn_host(x[:40], 64, b))
    # 8 distinct rows over and over, across at least two base groups
    b = duplicated(1100, 6, 4)
    q = torch.cat([b[:8], uniform(5, 6, 5)])
    assert groups(13, 1100) >= 2
    got = NB.knn(q.cuda(), 64, b.cuda())
    same(got, NB.knn_host(q, 64, b))
    for r in range(8):
        assert got.idx[r].tolist() == list(range(r, 8 * 64, 8)) and not got.d2[r].any()
    same(NB.knn(b.cuda(), 64), NB.knn_host(b, 64))


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_vote_against_the_host(weights):
    b, lab = uniform(1500, 8, 9), torch.from_numpy(np.random.default_rng(9).integers(0, 10, 1500))
    q = torch.cat([uniform(190, 8, 10), b[:10]])          # (ten queries duplicate base rows)
    assert groups(200, 1500) >= 2
    ks = (1, 5, 20)
    pred, res = NB.classify(q.cuda(), b.cuda(), lab.cuda(), ks, weights)
    hpred, hres = NB.classify_host(q, b, lab, ks, weights)
    same(res, hres)
    assert pred.is_cuda and pred.dtype == torch.int64 and torch.equal(pred.cpu(), hpred)
    # the vote alone, on the device's own lists
    assert torch.equal(NB.vote(res.idx, res.d2, lab.cuda(), ks, weights).cpu(),
                       NB.vote_host(res.idx.cpu(), res.d2.cpu(), lab, ks, weights))
    assert torch.equal(pred[190:, 0].cpu(), lab[:10])
    # leave-one-out, the labels far apart and negative: no per-class array
    wide = (lab - 5) * 1000003
    pred, res = NB.classify(b.cuda(), None, wide.cuda(), (1, 2, 64), weights)
    hpred, hres = NB.classify_host(b, None, wide, (1, 2, 64), weights)
    same(res, hres)
    assert torch.equal(pred.cpu(), hpred)


@functools.lru_cache(maxsize=None)
def _trust_case(N, F):
    return uniform(N, F, 400 + N), uniform(N, 2, 500 + N)


@pytest.mark.parametrize("N, F, k", [(513, 24, 1), (513, 24, 5), (513, 24, 12), (1100, 33, 20)])
def test_ranks_and_trustworthiness_against_the_host(N, F, k):
    x, y = _trust_case(N, F)
    assert (groups(N, N) >= 2) == (N == 1100)
    idx = NB.knn(y.cuda(), k).idx
    hidx = NB.knn_host(y, k).idx
    assert torch.equal(idx.cpu(), hidx)
    got, want = NB.ranks(x.cuda(), idx), NB.ranks_host(x, hidx)
    assert got.rank.is_cuda and got.rank.dtype == torch.int32 and got.penalty.dtype == torch.int64
    assert torch.equal(got.rank.cpu(), want.rank)
    assert torch.equal(got.penalty.cpu(), want.penalty) and int(want.penalty) > 0
    t = NB.trustworthiness(x.cuda(), y.cuda(), k)
    assert isinstance(t, float) and t == NB.trustworthiness_host(x, y, k)
    # a row's own neighbours rank 1 .. k
    own = NB.ranks(x.cuda(), NB.knn(x.cuda(), k).idx)
    assert torch.equal(own.rank.cpu(), torch.arange(1, k + 1, dtype=torch.int32).expand(N, k))
    assert int(own.penalty) == 0


def test_ranks_with_ties():
    x, y = grid(600, seed=2), uniform(600, 2, 3)
    idx = NB.knn(y.cuda(), 7).idx
    got, want = NB.ranks(x.cuda(), idx), NB.ranks_host(x, idx.cpu())
    assert torch.equal(got.rank.cpu(), want.rank) and torch.equal(got.penalty.cpu(), want.penalty)


def test_bits_repeat():
    q, b = uniform(100, 24, 1).cuda(), uniform(2000, 24, 2).cuda()
    a, c = NB.knn(q, 20, b), NB.knn(q, 20, b)
    assert torch.equal(a.idx, c.idx) and torch.equal(a.d2, c.d2)
    x, y = (t.cuda() for t in _trust_case(1100, 33))
    idx = NB.knn(y, 12).idx
    r1, r2 = NB.ranks(x, idx), NB.ranks(x, idx)
    assert torch.equal(r1.rank, r2.rank) and torch.equal(r1.penalty, r2.penalty)
    # non-contiguous input is taken by copy
    qt = q.t().contiguous().t()
    assert not qt.is_contiguous() and torch.equal(NB.knn(qt, 20, b).idx, a.idx)


def test_errors_on_the_device():
    x, b = uniform(10, 4, 17).cuda(), uniform(30, 4, 18).cuda()
    with pytest.raises(ValueError, match="both be device tensors or both CPU"):
        NB.knn(x, 2, b.cpu())
    with pytest.raises(ValueError, match="both be device tensors or both CPU"):
        NB.knn(x.cpu(), 2, b)
    with pytest.raises(ValueError, match="both be device tensors or both CPU"):
        NB.trustworthiness(x, x.cpu()[:, :2], 2)
    with pytest.raises(ValueError, match="both be device tensors or both CPU"):
        NB.ranks(x, torch.zeros(10, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="must be fp32"):
        NB.knn(x.double(), 2, b.double())
    with pytest.raises(ValueError, match="must be fp32"):
        NB.knn(x, 2, b.half())
    with pytest.raises(ValueError, match="must be fp32"):
        NB.knn(x.double(), 2)
    with pytest.raises(ValueError, match=r"k = 31, Nb = 30"):
        NB.knn(x, 31, b)
    with pytest.raises(ValueError, match=r"k = 10, N = 10"):
        NB.knn(x, 10)
    with pytest.raises(ValueError, match=r"k must be an int in 1 \.\. 64"):
        NB.knn(x, 65, uniform(100, 4, 1).cuda())
    # the library's own limits are the Python checks'
    lib = _lib.load()
    for Nq, Nb, F, k in [(1, 1, 1, 1), (5, 64, 256, 64), (5, 64, 257, 64), (5, 65, 256, 65),
                         (5, 63, 4, 64), (5, 64, 4, 0), (5, 3, 4, 3), (5, 3, 4, 4)]:
        try:
            NB._check(torch.empty(Nq, F), k, torch.empty(Nb, F))
            ok = True
        except ValueError:
            ok = False
        assert bool(lib.scae_knn_supported(Nq, Nb, F, k)) == ok, (Nq, Nb, F, k)
    assert not lib.scae_knn_supported(1 << 31, 5, 4, 1)
    assert lib.scae_knn_supported((1 << 31) - 1, 5, 4, 1)
    assert not lib.scae_knn_supported(5, 1 << 31, 4, 1) and lib.scae_knn_groups(5, 1 << 31) == 0
    d2 = torch.empty(10, 64, device="cuda")
    idx = torch.empty(10, 64, device="cuda", dtype=torch.int64)
    P = NB._P

    def search(k, self_mode):
        base = x if self_mode else b
        return lib.scae_knn_f32(P(x), 10, P(base), base.shape[0], 4, k, self_mode, None, P(d2),
                                P(idx), None)
    assert search(31, 0) == _lib.ERR_UNSUPPORTED and search(65, 0) == _lib.ERR_UNSUPPORTED
    assert search(10, 1) == _lib.ERR_UNSUPPORTED and search(0, 1) == _lib.ERR_UNSUPPORTED
    assert lib.scae_knn_f32(P(x), 10, P(b), 10, 4, 2, 1, None, P(d2), P(idx), None) == -1
    ks = (ctypes.c_int * 2)(5, 3)                     # not ascending
    lab = torch.zeros(30, device="cuda", dtype=torch.int64)
    pred = torch.empty(10, 2, device="cuda", dtype=torch.int64)
    assert lib.scae_knn_vote_f32(P(idx), P(d2), 10, 3, P(lab), 30, ks, 2, 0, P(pred), None) == -1
    torch.cuda.synchronize()


def test_knn_accuracy_and_trusted_embedding_end_to_end():
    from tests.test_eval_step_gpu import _model
    from tests.test_hip_model import full_size_params
    from torch_scae_amd import EvalStep, cluster, embed, ops
    from torch_scae_amd import data as D
    cfg, B, sd, _ = full_size_params("cfg2")
    model = _model(cfg, sd)
    imgs, labs = D.stroke_batches(4, B, cfg["image_shape"], seed=4)
    imgs, labs = imgs.flatten(0, 1).cuda(), labs.flatten().cuda()
    step = EvalStep(model, B, cfg["image_shape"])
    # (both splits leave a remainder of 4: EvalStep caches one remainder step, and rebuilding it
    # for another size draws from the noise stream, so only then do two passes see the same noise)
    fit, test = (imgs[:260], labs[:260]), (imgs[260:392], labs[260:392])
    step.encode(*fit)
    ks = (1, 5, 20)

    def fresh():
        torch.manual_seed(5)
        ops.reset_noise()

    for weights in ("uniform", "distance"):
        fresh()
        out = NB.knn_accuracy(step, fit, test, ks=ks, weights=weights)
        assert set(out) == {"fit_accuracy", "test_accuracy", "confusion", "ks"} and out["ks"] == ks
        fresh()
        xf = cluster.features(step.encode(*fit), "prior")
        xt = cluster.features(step.encode(*test), "prior")
        pred, _ = NB.classify(xt, xf, fit[1], ks, weights)
        own, _ = NB.classify(xf, None, fit[1], ks, weights)
        for col, k in enumerate(ks):
            assert out["test_accuracy"][k] == int((pred[:, col] == test[1]).sum()) / 132
            assert out["fit_accuracy"][k] == int((own[:, col] == fit[1]).sum()) / 260
        n_classes = out["confusion"].shape[0]
        assert out["confusion"].shape == (n_classes, n_classes) and out["confusion"].sum() == 132
        want = np.zeros_like(out["confusion"])
        np.add.at(want, (pred[:, -1].cpu().numpy(), test[1].cpu().numpy()), 1)
        assert np.array_equal(out["confusion"], want)
        assert np.trace(want) / 132 == out["test_accuracy"][20]
    kw = dict(perplexity=20.0, n_iter=40, exaggeration_iter=15, check_every=20)
    fresh()
    out = embed.capsule_embedding(step, fit, trustworthiness_k=5, **kw)
    fresh()
    x = cluster.features(step.encode(*fit), "prior")
    assert out["trustworthiness"] == NB.trustworthiness(x, out["y"], 5)
    assert out["trustworthiness"] == NB.trustworthiness_host(x.cpu(), out["y"].cpu(), 5)
    assert 0.0 < out["trustworthiness"] <= 1.0
    fresh()
    assert "trustworthiness" not in embed.capsule_embedding(step, fit, **kw)
