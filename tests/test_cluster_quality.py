"""Host side of the cluster-quality tools (torch_scae_amd/cluster_quality.py): the numpy
restatement of the silhouette against scikit-learn and against itself in the other distance
arithmetic, the distance rule pinned bit for bit on pair clusters, the label-based indices and
the Calinski-Harabasz / Davies-Bouldin indices against scikit-learn with their conventions, the
choice of k, ``unsupervised_accuracy``'s unchanged keys, and the argument errors."""
import numpy as np
import pytest
import torch

from tests.test_neighbors import dist32, uniform
from tests.test_tsne import blobs
from torch_scae_amd import cluster as C
from torch_scae_amd import cluster_quality as Q

SHAPES = [(300, 24, 10), (1000, 7, 3), (2000, 24, 10)]


def noisy_blobs(N, F, k, seed):
    """``blobs`` with a fifth of the labels re-drawn at random -> (x fp32, labels int64 tensor)"""
    x, y = blobs(N, F, k, seed)
    rng = np.random.default_rng(seed + 1000)
    redraw = rng.random(N) < 0.2
    y = np.where(redraw, rng.integers(0, k, N), y)
    return x, torch.from_numpy(y.astype(np.int64))


def separated(N, F, k, seed, spread=20.0):
    """k far-apart Gaussian clusters of equal share -> (x fp32, labels)"""
    rng = np.random.default_rng(seed)
    y = np.arange(N) % k
    x = spread * rng.standard_normal((k, F))[y] + rng.standard_normal((N, F))
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.int64))


_RESULTS = {}


def both(shape):
    """the fp32- and fp64-arithmetic restatements of a shape, computed once"""
    if shape not in _RESULTS:
        x, y = noisy_blobs(*shape, seed=3)
        _RESULTS[shape] = (x, y, Q.silhouette_host(x, y, shape[2]),
                           Q.silhouette_host(x, y, shape[2], dtype=np.float64))
    return _RESULTS[shape]


# -- silhouette -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_fp64_restatement_is_scikit_learns_silhouette(shape):
    metrics = pytest.importorskip("sklearn.metrics")
    x, y, _, r64 = both(shape)
    want = metrics.silhouette_samples(x.double().numpy(), y.numpy())
    got = r64.values.numpy()
    print("max |s - sklearn| =", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-12
    assert abs(r64.score - want.mean()) <= 1e-12
    for c in range(shape[2]):
        assert abs(r64.cluster_score[c] - want[y.numpy() == c].mean()) <= 1e-12


def test_singleton_and_duplicate_conventions_are_scikit_learns():
    metrics = pytest.importorskip("sklearn.metrics")
    x, y = noisy_blobs(200, 5, 4, 7)
    y[17] = 4                                   # a singleton cluster: s = 0
    r = Q.silhouette_host(x, y, 6, dtype=np.float64)        # (cluster 5 is empty)
    want = metrics.silhouette_samples(x.double().numpy(), y.numpy())
    assert np.abs(r.values.numpy() - want).max() <= 1e-12
    assert r.values[17] == 0 and r.a[17] == 0 and r.nearest[17] >= 0
    assert bool(torch.isfinite(r.b[17]))
    assert np.isnan(r.cluster_score[5]) and r.cluster_score[4] == 0
    # every row the same point: a = b = 0, s = 0
    same = torch.ones(12, 3)
    lab = torch.arange(12) % 3
    r = Q.silhouette_host(same, lab, 3, dtype=np.float64)
    want = metrics.silhouette_samples(same.double().numpy(), lab.numpy())
    assert np.array_equal(r.values.numpy(), want) and not want.any()
    assert not r.a.any() and not r.b.any() and r.nearest.tolist() == [1, 0, 0] * 4


def test_one_cluster_and_all_singletons():
    x = uniform(9, 4, 0)
    one = Q.silhouette_host(x, torch.zeros(9, dtype=torch.int64), 3)
    assert not one.values.any() and bool(torch.isinf(one.b).all()) and bool((one.a > 0).all())
    assert one.nearest.tolist() == [-1] * 9 and one.score == 0
    assert one.cluster_score[0] == 0 and np.isnan(one.cluster_score[1:]).all()
    each = Q.silhouette_host(x, torch.arange(9), None)
    assert not each.values.any() and not each.a.any() and bool((each.b > 0).all())
    assert bool((each.nearest != torch.arange(9)).all()) and each.cluster_score.shape == (9,)
    lone = Q.silhouette_host(x[:1], torch.zeros(1, dtype=torch.int64))
    assert lone.values.tolist() == [0] and lone.a.tolist() == [0] and lone.nearest.tolist() == [-1]


@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_and_fp64_restatements_differ_by_the_distances_rounding(shape):
    """The two differ only in the distances.  In fp32 every term (x - y)^2 carries two roundings
    and each of the F - 1 partial sums one, all relative to at most the whole sum, so d^2 is
    within (F + 1) 2^-24 relative and d = sqrt(d^2), rounded once more, within
    e = ((F + 1) / 2 + 1) 2^-24 (first order; the factor 1.01 covers the second).  a and b are
    means of such distances: the same relative bound.  s is a ratio of the two with derivative at
    most 2 in each relative error: |s32 - s64| <= 4 e."""
    x, y, r32, r64 = both(shape)
    e = 1.01 * ((shape[1] + 1) / 2 + 1) * 2.0 ** -24
    rel_a = float(((r32.a - r64.a).abs() / r64.a).max())
    rel_b = float(((r32.b - r64.b).abs() / r64.b).max())
    err_s = float((r32.values - r64.values).abs().max())
    print(f"rel a {rel_a:.3g} rel b {rel_b:.3g} abs s {err_s:.3g} (e = {e:.3g})")
    assert rel_a <= e and rel_b <= e and err_s <= 4 * e
    assert abs(r32.score - r64.score) <= 4 * e
    # nearest agrees wherever the two least cluster means are further apart than the rounding
    X, L = x.double().numpy(), y.numpy()
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    mean = np.stack([d[:, L == c].mean(1) for c in range(shape[2])], 1)
    mean[np.arange(len(L)), L] = np.inf
    two = np.sort(mean, 1)[:, :2]
    clear = two[:, 1] - two[:, 0] > 4 * e * two[:, 1]
    assert clear.mean() > 0.99
    assert torch.equal(r32.nearest[clear], r64.nearest[clear])


def test_pair_clusters_pin_the_distance_arithmetic():
    """Cluster c = {2c, 2c + 1}: a is the distance to the partner alone, so it must be the
    fp32-rule distance bit for bit (and b a mean of two of them)."""
    x = uniform(64, 5, 11)
    lab = torch.arange(64) // 2
    r = Q.silhouette_host(x, lab, 32)
    d = np.sqrt(dist32(x, x))
    assert d.dtype == np.float32
    partner = np.arange(64) ^ 1
    assert np.array_equal(r.a.numpy(), d[np.arange(64), partner].astype(np.float64))
    pair_mean = (d[:, 0::2].astype(np.float64) + d[:, 1::2].astype(np.float64)) / 2
    pair_mean[np.arange(64), np.arange(64) // 2] = np.inf
    assert np.array_equal(r.b.numpy(), pair_mean.min(1))
    assert np.array_equal(r.nearest.numpy(), pair_mean.argmin(1))
    assert Q.silhouette(x, lab, 32).values.equal(r.values)        # CPU tensors take the host


def test_ties_in_b_go_to_the_lowest_cluster_and_sums_are_sequential():
    # integer points on a line: every distance and every sum exact
    x = torch.tensor([[0.], [2.], [2.], [4.], [4.], [0.]])
    lab = torch.tensor([1, 0, 3, 3, 0, 1])
    r = Q.silhouette_host(x, lab, 5)              # clusters 2 and 4 are empty
    # rows 0 and 5 (cluster 1): clusters 0 and 3 are both at mean distance 3
    assert r.b[0] == 3 and r.nearest[0] == 0 and r.nearest[5] == 0
    assert r.a.tolist() == [0, 2, 2, 2, 2, 0]
    s = r.values.numpy()
    assert r.score == float(np.cumsum(s)[-1] / 6)
    assert np.isnan(r.cluster_score[[2, 4]]).all()


# -- label-based indices ------------------------------------------------------------------------
def _expand(table):
    rows, cols = np.nonzero(table)
    reps = table[rows, cols]
    return np.repeat(rows, reps), np.repeat(cols, reps)


def _tables():
    rng = np.random.default_rng(5)
    out = [rng.integers(0, 30, (7, 4)), rng.integers(0, 9, (3, 11)), rng.integers(1, 50, (5, 5))]
    empty = rng.integers(0, 20, (6, 4))
    empty[2] = 0                                 # an empty cluster
    out.append(empty)
    out.append(np.diag([5, 9, 2, 7]))            # a perfect labelling
    out.append(np.array([[4, 8, 1, 3]]))         # everything in one cluster
    out.append(np.array([[6], [2], [5]]))        # everything in one class
    out.append(np.array([[3, 0], [0, 0]]))       # one cluster, one class
    return out


@pytest.mark.parametrize("i", range(8))
def test_label_indices_against_scikit_learn(i):
    metrics = pytest.importorskip("sklearn.metrics")
    table = _tables()[i]
    cid, lab = _expand(table)
    got = Q.label_indices(table)
    hom, com, v = metrics.homogeneity_completeness_v_measure(lab, cid)
    want = {"ari": metrics.adjusted_rand_score(lab, cid),
            "nmi": metrics.normalized_mutual_info_score(lab, cid),
            "homogeneity": hom, "completeness": com, "v_measure": v,
            "purity": table.max(1).sum() / table.sum()}
    assert set(got) == set(want)
    for name in want:
        print(name, got[name], want[name])
        assert abs(got[name] - want[name]) <= 1e-12, name
    if i == 4:
        assert got == {n: 1.0 for n in want}


def test_label_indices_of_counts_the_table():
    rng = np.random.default_rng(2)
    cid, lab = torch.from_numpy(rng.integers(0, 6, 500)), torch.from_numpy(rng.integers(0, 4, 500))
    assert Q.label_indices_of(cid, lab, 7, 4) == Q.label_indices(C.contingency(cid, lab, 7, 4))
    for bad in (np.zeros((2, 2), dtype=np.int64), np.ones((2, 2)), np.array([1, 2]),
                np.array([[1, -1]])):
        with pytest.raises(ValueError, match="table must be"):
            Q.label_indices(bad)


# -- dispersion ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_dispersion_indices_against_scikit_learn(shape):
    metrics = pytest.importorskip("sklearn.metrics")
    x, y, _, _ = both(shape)
    r = Q.dispersion_host(x, y, shape[2] + 2)               # two empty clusters at the end
    X = x.double().numpy()
    ch, db = metrics.calinski_harabasz_score(X, y.numpy()), metrics.davies_bouldin_score(
        X, y.numpy())
    print(r.calinski_harabasz, ch, r.davies_bouldin, db)
    assert abs(r.calinski_harabasz - ch) <= 1e-10 * ch
    assert abs(r.davies_bouldin - db) <= 1e-10 * db
    assert r.count.tolist() == np.bincount(y.numpy(), minlength=shape[2] + 2).tolist()
    assert bool(torch.isnan(r.centroid[-1]).all()) and r.within[-1] == 0
    c = 1
    rows = X[y.numpy() == c]
    assert np.abs(r.centroid[c].numpy() - rows.mean(0)).max() <= 1e-12
    want_w = ((rows - rows.mean(0)) ** 2).sum()
    assert abs(float(r.within[c]) - want_w) <= 1e-10 * want_w
    assert Q.dispersion(x, y, shape[2] + 2).calinski_harabasz == r.calinski_harabasz


def test_dispersion_conventions_are_scikit_learns():
    metrics = pytest.importorskip("sklearn.metrics")
    # two clusters with one centroid (the origin): a zero centroid distance counts as +inf
    x = torch.tensor([[-1., 0.], [1., 0.], [0., -2.], [0., 2.], [5., 5.], [7., 5.]])
    y = torch.tensor([0, 0, 1, 1, 2, 2])
    r = Q.dispersion_host(x, y)
    X = x.double().numpy()
    assert r.centroid[0].tolist() == r.centroid[1].tolist() == [0, 0]
    assert abs(r.davies_bouldin - metrics.davies_bouldin_score(X, y.numpy())) <= 1e-12
    assert abs(r.calinski_harabasz - metrics.calinski_harabasz_score(X, y.numpy())) <= 1e-10
    # every centroid the same: every centroid distance 0 -> DB = 0
    r = Q.dispersion_host(x[:4], y[:4])
    assert r.davies_bouldin == 0.0 == metrics.davies_bouldin_score(X[:4], y[:4].numpy())
    # zero scatter: every S_c = 0 -> DB = 0, CH = 1
    x = torch.tensor([[1., 2.], [1., 2.], [4., 0.], [4., 0.], [4., 0.]])
    y = torch.tensor([0, 0, 3, 3, 3])
    r = Q.dispersion_host(x, y)
    assert r.davies_bouldin == 0.0 == metrics.davies_bouldin_score(x.double().numpy(), y.numpy())
    assert r.calinski_harabasz == 1.0 == metrics.calinski_harabasz_score(x.double().numpy(),
                                                                         y.numpy())
    # fewer than two non-empty clusters: no index
    r = Q.dispersion_host(x, torch.zeros(5, dtype=torch.int64), 2)
    assert np.isnan(r.calinski_harabasz) and np.isnan(r.davies_bouldin)


# -- the choice of k, the pipeline ----------------------------------------------------------------
@pytest.mark.parametrize("criterion", ["silhouette", "calinski_harabasz", "davies_bouldin"])
def test_select_k_finds_four_planted_centres_on_cpu_tensors(criterion):
    x, _ = separated(240, 6, 4, 1)
    out = Q.select_k(x, range(2, 8), criterion=criterion, n_init=3, seed=0)
    assert out.k == 4 and out.result.centroids.shape == (4, 6)
    assert out.table["k"] == list(range(2, 8)) and set(out.table) == {
        "k", "inertia", "silhouette", "calinski_harabasz", "davies_bouldin", "n_iter"}
    assert all(len(v) == 6 for v in out.table.values())
    assert out.table["inertia"][2] == out.result.inertia
    assert all(a >= b for a, b in zip(out.table["inertia"], out.table["inertia"][1:]))
    col = out.table[criterion]
    assert col[2] == (min(col) if criterion == "davies_bouldin" else max(col))


def test_select_k_ties_go_to_the_smallest_k(monkeypatch):
    x, _ = separated(60, 3, 3, 2)
    flat = Q.SilhouetteResult(None, None, None, None, 0.5, None)
    monkeypatch.setattr(Q, "quality", lambda x, labels, k: (
        flat, Q.DispersionResult(None, None, None, None, float("nan") if k == 3 else 2.0, 1.0)))
    assert Q.select_k(x, (5, 3, 4), n_init=1).k == 3
    assert Q.select_k(x, (5, 3, 4), "calinski_harabasz", n_init=1).k == 4      # NaN never wins


class _FakeStep:
    """EvalStep.encode for ``unsupervised_accuracy``: the images are the features already"""
    model = None

    def encode(self, images, labels):
        return {"prior": images, "posterior": images, "features": images[:, None],
                "label": labels}


def test_unsupervised_accuracy_keeps_todays_keys_without_metrics():
    x, y = separated(120, 5, 3, 4)
    fit, test = (x[:90], y[:90]), (x[90:], y[90:])
    out = C.unsupervised_accuracy(_FakeStep(), fit, test, k=3, n_init=2)
    assert list(out) == ["fit_accuracy", "test_accuracy", "inertia", "mapping", "n_iter"]
    more = C.unsupervised_accuracy(_FakeStep(), fit, test, k=3, n_init=2, metrics=True)
    assert set(more) - set(out) == {
        "fit_nmi", "fit_ari", "fit_purity", "test_nmi", "test_ari", "test_purity", "silhouette",
        "calinski_harabasz", "davies_bouldin"}
    for name in out:
        assert np.array_equal(more[name], out[name]), name
    assert more["fit_nmi"] == more["fit_ari"] == more["fit_purity"] == 1.0 == more["test_ari"]
    assert more["silhouette"] == Q.silhouette_host(x[:90], C.kmeans(x[:90], 3, n_init=2).labels,
                                                   3).score > 0.8


# -- arguments ----------------------------------------------------------------------------------
def test_argument_errors():
    x, y = uniform(10, 3, 0), torch.arange(10) % 2
    for fn in (Q.silhouette, Q.silhouette_host, Q.dispersion, Q.dispersion_host, Q.quality):
        with pytest.raises(ValueError, match=r"x must be an \(N, F\) tensor"):
            fn(x[0], y)
        with pytest.raises(ValueError, match="F = 257"):
            fn(torch.zeros(10, 257), y)
        with pytest.raises(ValueError, match=r"labels must be an integer \(10,\) tensor"):
            fn(x, y[:9])
        with pytest.raises(ValueError, match="labels must be an integer"):
            fn(x, y.float())
        with pytest.raises(ValueError, match="k must be an int"):
            fn(x, y, 0)
        with pytest.raises(ValueError, match="k must be an int"):
            fn(x, y, 2.0)
        with pytest.raises(ValueError, match=r"5 labels outside \[0, 1\)"):
            fn(x, y, 1)
        with pytest.raises(ValueError, match=r"1 labels outside \[0, 2\)"):
            fn(x, torch.where(torch.arange(10) == 3, -1, y), 2)
    with pytest.raises(ValueError, match="none is non-negative"):
        Q.silhouette(x, -torch.ones(10, dtype=torch.int64))
    with pytest.raises(ValueError, match="criterion must be one of"):
        Q.select_k(x, (2, 3), criterion="inertia")
    for ks in ((), (1, 2), (2, 2), (2.0, 3), 4):
        with pytest.raises(ValueError, match="ks must be"):
            Q.select_k(x, ks)
    with pytest.raises(ValueError, match="k = 11, N = 10"):
        Q.select_k(x, (2, 11))
