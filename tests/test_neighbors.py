"""Host side of the k-NN tools (torch_scae_amd/neighbors.py): the numpy restatement against
plainer restatements of the same rules -- a full lexicographic sort of the float32 distance
matrix, a per-class tally, a double loop over the ranks -- on random data, on inputs with massive
ties and duplicated rows, against scikit-learn where it imports, and the argument errors."""
import numpy as np
import pytest
import torch

from torch_scae_amd import neighbors as NB


def uniform(N, F, seed):
    return torch.from_numpy(np.random.default_rng(seed).random((N, F)).astype(np.float32))


def grid(N, seed=0):
    """{0, 1, 2}^3 integer features: 27 distinct rows, squared distances in 0 .. 12."""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 3, (N, 3)).astype(np.float32))


def duplicated(N, F, seed, distinct=8):
    """``distinct`` uniform rows repeated in turn up to N rows."""
    return uniform(distinct, F, seed).repeat(-(-N // distinct), 1)[:N].contiguous()


def dist32(q, b):
    """(Nq, Nb) float32 distances by the rules: f order, every operation rounded once."""
    q, b = q.numpy(), b.numpy()
    d = np.zeros((q.shape[0], b.shape[0]), dtype=np.float32)
    for f in range(q.shape[1]):
        u = q[:, None, f] - b[None, :, f]
        d = d + u * u
    assert d.dtype == np.float32
    return d


def full_sort(q, k, base=None):
    """The k least (d, j) of every row by a whole lexsort -> (idx, d2) numpy"""
    d = dist32(q, q if base is None else base)
    if base is None:
        np.fill_diagonal(d, np.inf)
    cols = np.broadcast_to(np.arange(d.shape[1]), d.shape)
    order = np.lexsort((cols, d), axis=1)[:, :k]
    return order, np.take_along_axis(d, order, 1)


def same(res, idx, d2):
    assert res.idx.dtype == torch.int64 and res.d2.dtype == torch.float32
    assert np.array_equal(res.idx.numpy(), idx)
    assert np.array_equal(res.d2.numpy(), d2)


# -- search ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq, Nb, F, k", [(1, 1, 1, 1), (37, 211, 5, 7), (70, 300, 33, 64)])
def test_search_is_the_full_lexsort_on_random_data(Nq, Nb, F, k):
    q, b = uniform(Nq, F, 1), uniform(Nb, F, 2)
    same(NB.knn_host(q, k, b), *full_sort(q, k, b))
    assert NB.knn(q, k, b).idx.equal(NB.knn_host(q, k, b).idx)     # CPU tensors take the host


def test_search_on_the_integer_grid_takes_the_lowest_indices():
    x = grid(500)
    idx, d2 = full_sort(x, 20)
    res = NB.knn_host(x, 20)
    same(res, idx, d2)
    assert set(np.unique(d2)) <= set(float(v) for v in range(13))     # exact distances
    # within a run of equal distances the base indices ascend
    tied = d2[:, 1:] == d2[:, :-1]
    assert tied.mean() > 0.5 and bool((idx[:, 1:] > idx[:, :-1])[tied].all())
    # a base row is passed over only for rows that are strictly nearer or equal with a lower index
    i = 7
    d = dist32(x[i:i + 1], x)[0]
    d[i] = np.inf
    last = (d2[i, -1], idx[i, -1])
    out = np.setdiff1d(np.arange(500), np.append(idx[i], i))
    assert all((d[j], j) > last for j in out)
    q = grid(40, seed=3)
    same(NB.knn_host(q, 9, x), *full_sort(q, 9, x))


def test_search_on_duplicated_rows():
    b = duplicated(100, 6, 4)
    q = torch.cat([b[:5], uniform(6, 6, 5)])
    res = NB.knn_host(q, 30, b)
    same(res, *full_sort(q, 30, b))
    # a query that is base row r: its 13 or 12 copies first, at distance 0, lowest index first
    for r in range(5):
        copies = np.arange(r, 100, 8)
        assert np.array_equal(res.idx[r, :len(copies)].numpy(), copies)
        assert not res.d2[r, :len(copies)].any() and float(res.d2[r, len(copies)]) > 0
    same(NB.knn_host(b, 30), *full_sort(b, 30))


def test_self_mode_with_every_other_row():
    x = uniform(65, 4, 6)
    res = NB.knn_host(x, 64)
    same(res, *full_sort(x, 64))
    want = torch.arange(65)
    for i in range(65):
        assert torch.equal(res.idx[i].sort().values, want[want != i])
    assert bool((res.d2[:, 1:] >= res.d2[:, :-1]).all())


def test_float64_restatement_and_chunks(monkeypatch):
    q, b = uniform(50, 7, 7), uniform(333, 7, 8)
    a = NB.knn_host(q, 10, b)
    monkeypatch.setattr(NB, "_ELEMS", 1000)          # three query rows per chunk
    c = NB.knn_host(q, 10, b)
    assert torch.equal(a.idx, c.idx) and torch.equal(a.d2, c.d2)
    d = NB.knn_host(q, 10, b, dtype=np.float64)
    assert d.d2.dtype == torch.float64
    D = np.zeros((50, 333))
    for f in range(7):
        D += (q.double().numpy()[:, None, f] - b.double().numpy()[None, :, f]) ** 2
    assert np.array_equal(d.idx.numpy(), np.argsort(D, 1, kind="stable")[:, :10])


# -- vote -----------------------------------------------------------------------------------------
def tally_vote(idx, d2, labels, kk, weights):
    """A per-class tally of the first kk neighbours, ties to the lowest class."""
    out = []
    for i in range(idx.shape[0]):
        if weights == "uniform":
            w = [np.float32(1)] * kk
        elif d2[i, 0] == 0:
            w = [np.float32(d2[i, m] == 0) for m in range(kk)]
        else:
            w = [np.float32(1) / np.sqrt(np.float32(d2[i, m])) for m in range(kk)]
        score = {}
        for m in range(kk):
            c = int(labels[idx[i, m]])
            score[c] = np.float32(score.get(c, np.float32(0)) + w[m])
        top = max(score.values())
        out.append(min(c for c, s in score.items() if s == top))
    return np.array(out)


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_vote_is_the_per_class_tally(weights):
    b, lab = uniform(400, 5, 9), torch.from_numpy(np.random.default_rng(9).integers(0, 10, 400))
    q = torch.cat([uniform(60, 5, 10), b[:7]])            # (seven queries duplicate base rows)
    ks = (1, 2, 5, 20)
    pred, res = NB.classify_host(q, b, lab, ks, weights)
    assert pred.shape == (67, 4) and pred.dtype == torch.int64
    same(res, *full_sort(q, 20, b))
    for col, kk in enumerate(ks):
        want = tally_vote(res.idx.numpy(), res.d2.numpy(), lab.numpy(), kk, weights)
        assert np.array_equal(pred[:, col].numpy(), want), kk
    assert torch.equal(pred[60:, 0], lab[:7])
    # self mode: leave-one-out
    pred, res = NB.classify_host(b, None, lab, (3,), weights)
    assert np.array_equal(pred[:, 0].numpy(),
                          tally_vote(res.idx.numpy(), res.d2.numpy(), lab.numpy(), 3, weights))


def test_uniform_two_way_tie_goes_to_the_lower_class():
    b = torch.tensor([[1.0], [2.0], [3.0], [4.0], [5.0]])
    lab = torch.tensor([7, 3, 3, 7, 9])
    pred, res = NB.classify_host(torch.tensor([[0.0]]), b, lab, (1, 2, 3, 4, 5))
    assert res.idx.tolist() == [[0, 1, 2, 3, 4]]
    # 7 | 7 3 -> 3 (tie, lower class) | 3 3 7 -> 3 | 2 : 2 -> 3 | 3
    assert pred.tolist() == [[7, 3, 3, 3, 3]]
    lab = torch.tensor([3, 7, 7, 3, 9])
    pred, _ = NB.classify_host(torch.tensor([[0.0]]), b, lab, (1, 2, 3, 4))
    assert pred.tolist() == [[3, 3, 7, 3]]


def test_distance_vote_of_an_exact_duplicate_counts_only_the_zero_distances():
    b = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [0.1, 0.0], [0.2, 0.0], [0.0, 0.0],
                      [0.3, 0.0]])
    lab = torch.tensor([5, 2, 2, 4, 4, 8, 4])
    q = torch.tensor([[1.0, 0.0], [0.0, 0.0], [0.05, 0.0]])
    pred, res = NB.classify_host(q, b, lab, (2, 5), "distance")
    # query 0 duplicates rows 1, 2 (class 2): the three nearer-weighted 4s do not vote
    assert res.idx[0, :2].tolist() == [1, 2] and pred[0].tolist() == [2, 2]
    # query 1 duplicates rows 0 (class 5) and 5 (class 8): one vote each, the lower class
    assert res.idx[1, :2].tolist() == [0, 5] and pred[1].tolist() == [5, 5]
    # query 2 duplicates nothing: 1 / distance, where the three 4s outweigh the nearer 5 and 8
    assert pred[2, 1].item() == 4
    # uniform votes at k = 5 for query 0: 2, 2, 4, 4, 4 -> 4
    assert NB.classify_host(q, b, lab, (2, 5))[0][0].tolist() == [2, 4]


def test_uniform_vote_is_sklearns_brute_force_classifier():
    sk = pytest.importorskip("sklearn.neighbors")
    b, lab = uniform(500, 8, 11), np.random.default_rng(11).integers(0, 10, 500)
    q = uniform(200, 8, 12)
    for col, kk in enumerate((1, 5, 20)):
        want = sk.KNeighborsClassifier(n_neighbors=kk, algorithm="brute").fit(
            b.numpy(), lab).predict(q.numpy())
        got = NB.classify_host(q, b, torch.from_numpy(lab), (1, 5, 20))[0][:, col].numpy()
        assert np.array_equal(got, want), kk


# -- ranks and trustworthiness --------------------------------------------------------------------
def loop_ranks(x, idx):
    d = dist32(x, x)
    N, k = idx.shape
    r = np.zeros((N, k), dtype=np.int32)
    for i in range(N):
        for m in range(k):
            j = int(idx[i, m])
            r[i, m] = 1 + sum(1 for l in range(N) if l != i and (d[i, l], l) < (d[i, j], j))
    return r


@pytest.mark.parametrize("kind", ["uniform", "grid"])
def test_ranks_and_trustworthiness_are_the_double_loop(kind):
    N, k = 60, 5
    x = uniform(N, 6, 13) if kind == "uniform" else grid(N, 13)
    y = uniform(N, 2, 14)
    idx = NB.knn_host(y, k).idx
    res = NB.ranks_host(x, idx)
    assert res.rank.dtype == torch.int32 and res.penalty.dtype == torch.int64
    r = loop_ranks(x, idx.numpy())
    assert np.array_equal(res.rank.numpy(), r)
    penalty = int(np.maximum(r.astype(np.int64) - k, 0).sum())
    assert int(res.penalty) == penalty and penalty > 0
    want = 1.0 - 2.0 * penalty / (N * k * (2 * N - 3 * k - 1))
    assert NB.trustworthiness_host(x, y, k) == want == NB.trustworthiness(x, y, k)
    # the ranks of a row's own neighbours are 1 .. k, and an embedding that is the features
    # is trusted fully
    own = NB.ranks_host(x, NB.knn_host(x, k).idx)
    assert torch.equal(own.rank, torch.arange(1, k + 1, dtype=torch.int32).expand(N, k))
    assert int(own.penalty) == 0 and NB.trustworthiness_host(x, x, k) == 1.0


@pytest.mark.parametrize("k", [1, 5, 12])
def test_trustworthiness_is_sklearns_on_tie_free_data(k):
    sk = pytest.importorskip("sklearn.manifold")
    x, y = uniform(300, 24, 15), uniform(300, 2, 16)
    want = sk.trustworthiness(x.numpy(), y.numpy(), n_neighbors=k)
    assert abs(NB.trustworthiness_host(x, y, k) - want) <= 1e-12


# -- errors ---------------------------------------------------------------------------------------
def test_argument_errors():
    x, b = uniform(10, 4, 17), uniform(30, 4, 18)
    lab = torch.arange(30) % 3
    for k in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError, match=r"k must be an int in 1 \.\. 64"):
            NB.knn(x, k, b)
    with pytest.raises(ValueError, match=r"k = 31, Nb = 30: needs k <= Nb"):
        NB.knn(x, 31, b)
    with pytest.raises(ValueError, match=r"k = 10, N = 10: self mode needs k <= N - 1"):
        NB.knn(x, 10)
    NB.knn(x, 9)
    NB.knn(x, 30, b)
    with pytest.raises(ValueError, match=r"F = 257: the search takes 1 <= F <= 256"):
        NB.knn(torch.zeros(4, 257), 1)
    with pytest.raises(ValueError, match=r"x must be an \(N, F\) tensor"):
        NB.knn(torch.zeros(4, 0), 1)
    with pytest.raises(ValueError, match=r"x must be an \(N, F\) tensor"):
        NB.knn(torch.zeros(4), 1)
    with pytest.raises(ValueError, match=r"base must be \(Nb, 4\)"):
        NB.knn(x, 1, torch.zeros(30, 5))
    for ks in ((5, 1), (1, 1), (0, 2), tuple(range(1, 10)), (), (1, 2.0)):
        with pytest.raises(ValueError, match="ks must"):
            NB.classify(x, b, lab, ks)
    with pytest.raises(ValueError, match=r"ks\[-1\] = 31, Nb = 30"):
        NB.classify(x, b, lab, (1, 31))
    with pytest.raises(ValueError, match=r"ks\[-1\] = 10, Nb = 10"):
        NB.classify(x, None, lab[:10], (1, 10))
    with pytest.raises(ValueError, match=r"k must be an int in 1 \.\. 64"):
        NB.classify(uniform(10, 4, 1), uniform(100, 4, 2), torch.zeros(100, dtype=torch.int64),
                    (1, 65))
    with pytest.raises(ValueError, match="weights must be 'uniform' or 'distance'"):
        NB.classify(x, b, lab, (1, 5), weights="rank")
    with pytest.raises(ValueError, match=r"base_labels must be an integer \(30,\) tensor"):
        NB.classify(x, b, lab[:29], (1, 5))
    with pytest.raises(ValueError, match=r"base_labels must be an integer"):
        NB.classify(x, b, lab.float(), (1, 5))
    y = uniform(10, 2, 19)
    for k in (5, 6):
        with pytest.raises(ValueError, match=rf"k = {k}, N = 10: trustworthiness needs k < N / 2"):
            NB.trustworthiness(x, y, k)
    NB.trustworthiness(x, y, 4)
    with pytest.raises(ValueError, match=r"y must embed the 10 rows of x"):
        NB.trustworthiness(x, uniform(9, 2, 1), 2)
    with pytest.raises(ValueError, match=r"idx must be an \(10, k\) int64 tensor"):
        NB.ranks(x, torch.zeros(10, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"k = 10, N = 10: ranks take"):
        NB.ranks(x, torch.zeros(10, 10, dtype=torch.int64))
