"""Sparse t-SNE without a GPU: the numpy restatement of the k-NN affinities (at K = N - 1 it is the
dense definition), the CSR's invariants, the CPU path of ``tsne(neighbors=...)``, argument errors
and what the library answers without a device."""
import math

import numpy as np
import pytest
import torch

from tests.test_tsne import blobs, duplicates_and_outlier, purity_1nn, uniform
from torch_scae_amd import _lib
from torch_scae_amd import embed as E


@pytest.mark.parametrize("N, F, perplexity", [(40, 5, 13.0), (64, 24, 21.0)])
def test_every_neighbour_listed_is_the_dense_definition(N, F, perplexity):
    x = uniform(N, F, N)
    indptr, indices, values, beta, plogp = E.affinities_knn_host(x, perplexity, N - 1)
    P, beta_d, plogp_d = E.affinities_host(x, perplexity)
    assert values.dtype == torch.float64 and indices.shape == (N * (N - 1),)
    assert float(np.abs(E.densify(indptr, indices, values) - P.numpy()).max()) <= 1e-12
    assert float((beta - beta_d).abs().max()) <= 1e-9 and abs(plogp - plogp_d) <= 1e-12
    # 60 iterations, 20 of them exaggerated.  The learning rate is 5, not "auto" (50 at these N):
    # at 50 the fp64 run is chaotic over 60 iterations -- a relative perturbation of 1e-16 of the
    # dense P moves the dense run's own Y by about 10 -- so no two summation orders agree there;
    # at 5 the embedding still unfolds (|Y| reaches about 6)
    kw = dict(n_iter=60, exaggeration_iter=20, learning_rate=5.0)
    a, b = E.tsne_host(x, perplexity, neighbors=N - 1, **kw), E.tsne_host(x, perplexity, **kw)
    assert float(b.y.abs().max()) > 1.0
    assert float((a.y - b.y).abs().max()) <= 1e-9 and abs(a.kl - b.kl) <= 1e-9


def check_csr(indptr, indices, values, K):
    """Columns ascend, no diagonal, the transpose has the same bits, at least K entries a row."""
    indptr, indices, values = (np.asarray(torch.as_tensor(a).cpu()) for a in
                               (indptr, indices, values))
    N = len(indptr) - 1
    assert indptr[0] == 0 and indptr[-1] == len(indices) == len(values)
    counts = np.diff(indptr)
    assert counts.min() >= K
    rows = np.repeat(np.arange(N), counts)
    assert not (rows == indices).any() and indices.min() >= 0 and indices.max() < N
    keys = rows * N + indices
    assert (np.diff(keys) > 0).all()              # rows in order, a row's columns ascending
    order = np.argsort(indices * N + rows, kind="stable")
    assert np.array_equal(keys, (indices * N + rows)[order])      # the pattern is symmetric
    assert np.array_equal(values, values[order])                  # and so are the bits


CASES = [("uniform", 12, 2, 3.0, 9), ("uniform", 65, 24, 10.0, "auto"),
         ("duplicates", 65, 24, 10.0, "auto")]


@pytest.mark.parametrize("kind, N, F, perplexity, neighbors", CASES)
def test_csr_invariants_and_the_entropy_at_beta(kind, N, F, perplexity, neighbors):
    x = uniform(N, F, N) if kind == "uniform" else duplicates_and_outlier(N, F, N)
    K = math.ceil(3 * perplexity) if neighbors == "auto" else neighbors
    indptr, indices, values, beta, plogp = E.affinities_knn_host(x, perplexity, neighbors)
    assert indptr.dtype == indices.dtype == torch.int64 and indptr.shape == (N + 1,)
    check_csr(indptr, indices, values, K)
    assert abs(float(values.double().sum()) - 1.0) <= 1e-12
    v = values.numpy()
    assert abs(plogp - float((v[v > 0] * np.log(v[v > 0])).sum())) <= 1e-12
    lists = E.neighbor_lists_host(x, K, np.float64)
    assert lists.idx.shape == (N, K) and bool((lists.d2[:, 1:] >= lists.d2[:, :-1]).all())
    cond, H = E.conditionals_knn_host(lists.d2, beta)
    assert float(np.abs(H - math.log(perplexity)).max()) <= 1e-5
    assert float(np.abs(cond.sum(1) - 1.0).max()) <= 1e-12


def test_the_wide_lists_are_the_knn_rule():
    from torch_scae_amd import neighbors
    x = duplicates_and_outlier(70, 3, 1)
    for K in (1, 64):
        a, b = E.neighbor_lists(x, K), neighbors.knn_host(x, K)
        assert torch.equal(a.idx, b.idx) and torch.equal(a.d2, b.d2)
    wide = E.neighbor_lists(x, 69)
    assert torch.equal(wide.idx[:, :64], b.idx) and torch.equal(wide.d2[:, :64], b.d2)
    assert torch.equal(wide.idx.sort(1).values,
                       torch.tensor([[j for j in range(70) if j != i] for i in range(70)]))


def test_tsne_on_a_cpu_tensor_with_neighbors_is_the_host_run():
    x, y = blobs(120, 8, 4, 0)
    kw = dict(perplexity=10.0, n_iter=250, exaggeration_iter=80, init="random", seed=1)
    got = E.tsne(x, neighbors="auto", **kw)
    host = E.tsne_host(x, neighbors="auto", **kw)
    assert torch.equal(got.y, host.y) and got.kl == host.kl
    assert torch.equal(got.history, host.history) and torch.equal(got.beta, host.beta)
    assert got.y.dtype == torch.float64 and got.history.shape == (5, 3)
    seven = E.tsne(x, neighbors=30, check_every=7, **kw)
    assert torch.equal(seven.y, got.y) and seven.history.shape == (36, 3)
    assert purity_1nn(got.y.numpy(), y) >= 0.95
    assert float(got.y.mean(0).abs().max()) <= 1e-9 * float(got.y.abs().max())


def test_argument_errors():
    x = uniform(200, 4, 5)
    with pytest.raises(ValueError, match=r"neighbors = 129, perplexity = 30.0, N = 200"):
        E.tsne(x, neighbors=129)
    with pytest.raises(ValueError, match=r"neighbors = 50, perplexity = 10.0, N = 50"):
        E.tsne(x[:50], perplexity=10.0, neighbors=50)
    with pytest.raises(ValueError, match=r"neighbors = 89, perplexity = 30.0, N = 200"):
        E.tsne(x, neighbors=89)
    with pytest.raises(ValueError, match=r"neighbors = 128, perplexity = 43.0"):
        E.affinities_knn(x, 43.0, 128)
    with pytest.raises(ValueError, match="neighbors must be None, 'auto' or an int, got 'many'"):
        E.tsne(x, neighbors="many")
    with pytest.raises(ValueError, match="neighbors must be None, 'auto' or an int, got True"):
        E.tsne_host(x, neighbors=True)
    with pytest.raises(ValueError, match=rf"N = {E.SPARSE_MAX_N + 1}, F = 1"):
        E.tsne(torch.zeros(E.SPARSE_MAX_N + 1, 1), neighbors="auto")
    with pytest.raises(ValueError, match=r"N = 200, F = 257"):
        E.affinities_knn(torch.zeros(200, 257), 30.0)
    with pytest.raises(ValueError, match="lists must be"):
        E.affinities_knn_host(x, 30.0, 90, lists=E.neighbor_lists_host(x, 89))
    with pytest.raises(ValueError, match=rf"N = {E.MAX_N + 1}, F = 1: t-SNE takes N <= {E.MAX_N}"):
        E.tsne(torch.zeros(E.MAX_N + 1, 1))          # the dense form's limit is where it was
    assert (E.MAX_NEIGHBORS, E.SPARSE_MAX_N) == \
        (_lib.TSNE_MAX_NEIGHBORS, _lib.TSNE_SPARSE_MAX_N) == (128, 262144)


def test_the_library_answers_the_sparse_limits_and_groups_without_a_gpu():
    lib = _lib.load()
    for N, F, K in ((2, 1, 1), (262144, 256, 128), (129, 24, 128), (60000, 24, 90)):
        assert lib.scae_tsne_sparse_supported(N, F, K) == 1
    for N, F, K in ((1, 1, 1), (262145, 24, 90), (100, 257, 90), (100, 0, 90), (100, 24, 0),
                    (1000, 24, 129), (90, 24, 90)):
        assert lib.scae_tsne_sparse_supported(N, F, K) == 0
    # whole 256-column tiles, about 1024 workgroups over the 512-row blocks, at most 64 groups
    assert [lib.scae_tsne_sparse_groups(n) for n in (1, 2, 256, 257, 513, 4099, 10000, 32768,
                                                      60000, 262144, 262145)] == \
        [0, 1, 1, 2, 3, 17, 40, 16, 9, 2, 0]
    d = _lib.TsneSparseDesc()
    assert lib.scae_tsne_sparse_run_f32(d, 0, 1, None) == -1    # an empty descriptor is refused
    assert lib.scae_tsne_knn_bandwidths_f32(None, 10, 3, 1.0, None, None, None) == -1
    assert lib.scae_knn_wide_f32(None, 10, 3, 3, None, None, None, None) == -1
