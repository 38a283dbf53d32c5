"""Cluster quality on the GPU: the silhouette kernels (csrc/cluster_quality.hip) against the numpy
restatement in the device's distance arithmetic (cluster_quality.silhouette_host) -- bit for bit
where every sum is exact, within the reordering bound of fp64 sums elsewhere -- the distance
arithmetic pinned on pair clusters, duplicates, singletons and empty clusters, run-to-run bits,
the dispersion tables, and the pipeline up to ``unsupervised_accuracy(metrics=True)``.

The bound: both sides add the same non-negative fp32 distances in fp64.  Any two orders of a sum
of n such terms differ by at most (n - 1) 2^-53 relative each, so a and b agree within
N 2^-51 relative with room to spare; s is a ratio of the two with derivative at most 2 in each
relative error, hence 4 N 2^-52 at most, and 8 N 2^-52 is that with a factor of 2 over."""
import numpy as np
import pytest
import torch

from tests.test_cluster_quality import noisy_blobs, separated
from tests.test_neighbors import dist32, duplicated, grid, uniform
from torch_scae_amd import cluster as C
from torch_scae_amd import cluster_quality as Q

pytestmark = pytest.mark.gpu

GENERAL = [(65, 24, 4), (257, 33, 10), (300, 256, 5), (1500, 7, 3), (5000, 24, 10)]
_HOST = {}


def general(shape):
    """a general shape's input and its host results, computed once -> (x, labels, silhouette,
    dispersion with an empty cluster k)"""
    if shape not in _HOST:
        x, y = noisy_blobs(*shape, seed=5)
        _HOST[shape] = (x, y, Q.silhouette_host(x, y, shape[2]),
                        Q.dispersion_host(x, y, shape[2] + 1))
    return _HOST[shape]


def same_bits(got, want):
    for name in ("values", "a", "b", "nearest"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g.cpu(), w), name
    assert isinstance(got.score, float) and got.score == want.score
    assert got.cluster_score.dtype == np.float64
    assert np.array_equal(got.cluster_score, want.cluster_score, equal_nan=True)


def within_bound(got, want, N):
    s, a, b = got.values.cpu(), got.a.cpu(), got.b.cpu()
    err_s = float((s - want.values).abs().max())
    rel_a = float(((a - want.a).abs() / want.a.clamp_min(1e-300)).max())
    finite = torch.isfinite(want.b)
    assert torch.equal(torch.isfinite(b), finite)
    rel_b = float(((b - want.b)[finite].abs() / want.b[finite].clamp_min(1e-300)).max()) \
        if bool(finite.any()) else 0.0
    print(f"N = {N}: |s - s_host| {err_s:.3g} (bound {8 * N * 2.0 ** -52:.3g}), "
          f"rel a {rel_a:.3g}, rel b {rel_b:.3g} (bound {N * 2.0 ** -51:.3g})")
    assert err_s <= 8 * N * 2.0 ** -52
    assert rel_a <= N * 2.0 ** -51 and rel_b <= N * 2.0 ** -51
    assert abs(got.score - want.score) <= 8 * N * 2.0 ** -52
    live = ~np.isnan(want.cluster_score)
    assert np.array_equal(np.isnan(got.cluster_score), ~live)
    assert np.abs(got.cluster_score[live] - want.cluster_score[live]).max() <= 8 * N * 2.0 ** -52


def cluster_means(x, y, k):
    """(N, k) mean fp32-rule distance of every row to every cluster (its own: +inf), fp64"""
    X, L = x.numpy(), y.numpy()
    out = np.empty((len(L), k))
    for lo in range(0, len(L), 256):
        d = Q._dist_rows(X, lo, min(lo + 256, len(L))).astype(np.float64)
        out[lo:lo + 256] = np.stack([d[:, L == c].mean(1) for c in range(k)], 1)
    out[np.arange(len(L)), L] = np.inf
    return out


# -- bit for bit: every distance an integer, every fp64 sum exact in any order ------------------
@pytest.mark.parametrize("clusters", ["one", "three", "each"])
@pytest.mark.parametrize("N", [1, 2, 65, 257, 1100])
def test_integer_line_is_the_host_bit_for_bit(N, clusters):
    rng = np.random.default_rng(N)
    x = torch.from_numpy(rng.integers(0, 8, (N, 1)).astype(np.float32))
    ids = {"one": np.zeros(N, dtype=np.int64), "three": rng.integers(0, 3, N),
           "each": rng.permutation(N)}[clusters]
    lab = torch.from_numpy(2 * ids + 1)           # the even label ids are empty clusters
    k = int(lab.max()) + 3
    want = Q.silhouette_host(x, lab, k)
    got = Q.silhouette(x.cuda(), lab.cuda(), k)
    same_bits(got, want)
    assert got.cluster_score.shape == (k,) and np.isnan(got.cluster_score[0::2]).all()
    if clusters != "three":
        assert not want.values.any()


def test_ties_in_b_go_to_the_lowest_cluster_on_the_device():
    # clusters 0 and 2 are the same multiset: every row of cluster 1 is as far from both
    x = torch.tensor([[0.], [3.], [0.], [5.], [4.], [5.]] * 40)
    lab = torch.tensor([0, 1, 2, 0, 1, 2] * 40)
    want = Q.silhouette_host(x, lab, 3)
    assert want.nearest[1::3].tolist() == [0] * 80
    same_bits(Q.silhouette(x.cuda(), lab.cuda(), 3), want)


def test_integer_grid_within_the_bound():
    x = grid(500)
    lab = torch.arange(500) % 5
    want = Q.silhouette_host(x, lab, 5)
    got = Q.silhouette(x.cuda(), lab.cuda())       # k = the largest label + 1
    within_bound(got, want, 500)
    assert got.cluster_score.shape == (5,)


# -- general data ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GENERAL)
def test_general_data_within_the_bound_and_nearest_equal(shape):
    N, F, k = shape
    x, y, want, _ = general(shape)
    # no row's two least cluster means are close enough for a reordered sum to swap them
    two = np.sort(cluster_means(x, y, k), 1)[:, :2]
    assert ((two[:, 1] - two[:, 0]) > 1e-9 * two[:, 1]).all()
    got = Q.silhouette(x.cuda(), y.cuda(), k)
    within_bound(got, want, N)
    assert torch.equal(got.nearest.cpu(), want.nearest)


@pytest.mark.parametrize("N, F", [(64, 5), (130, 40)])
def test_pair_clusters_pin_the_kernels_distance_arithmetic(N, F):
    """Cluster c = {2c, 2c + 1}: a is one distance, so the kernel's no-fma squared distance and
    its square root must be the rules' bit for bit."""
    x = uniform(N, F, 21)
    lab = torch.arange(N) // 2
    got = Q.silhouette(x.cuda(), lab.cuda(), N // 2)
    d = np.sqrt(dist32(x, x))
    assert d.dtype == np.float32
    want = d[np.arange(N), np.arange(N) ^ 1].astype(np.float64)
    assert np.array_equal(got.a.cpu().numpy(), want)
    same_bits(got, Q.silhouette_host(x, lab, N // 2))     # (b: means of two, exact to a bit)


def test_duplicates_and_singletons():
    x = duplicated(1100, 6, 4)
    lab = torch.arange(1100) % 8                   # a cluster is one point many times: a = 0
    got = Q.silhouette(x.cuda(), lab.cuda(), 8)
    within_bound(got, Q.silhouette_host(x, lab, 8), 1100)
    assert not got.a.any() and bool((got.b > 0).all()) and bool((got.values == 1).all())
    # every row the same point: a = b = 0, so s = 0 and nearest is the lowest other cluster
    x = duplicated(1100, 6, 4, distinct=1)
    lab = torch.arange(1100) % 3
    got = Q.silhouette(x.cuda(), lab.cuda(), 3)
    same_bits(got, Q.silhouette_host(x, lab, 3))
    assert not got.a.any() and not got.b.any() and not got.values.any()
    assert got.nearest.cpu().tolist() == [1, 0, 0] * 366 + [1, 0]
    # every row a cluster of its own
    x = uniform(300, 9, 2)
    got = Q.silhouette(x.cuda(), torch.arange(300).cuda(), 300)
    want = Q.silhouette_host(x, torch.arange(300), 300)
    assert not got.values.any() and not got.a.any() and got.score == 0
    assert torch.equal(got.b.cpu(), want.b) and torch.equal(got.nearest.cpu(), want.nearest)


def test_two_runs_give_the_same_bits_and_a_permutation_permutes():
    shape = (5000, 24, 10)
    x, y, want, _ = general(shape)
    xd, yd = x.cuda(), y.cuda()
    one, two = Q.silhouette(xd, yd, 10), Q.silhouette(xd, yd, 10)
    for name in ("values", "a", "b", "nearest"):
        assert torch.equal(getattr(one, name), getattr(two, name)), name
    assert one.score == two.score and np.array_equal(one.cluster_score, two.cluster_score)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(5000))
    moved = Q.silhouette(x[perm].cuda(), y[perm].cuda(), 10)
    err = float((moved.values.cpu() - one.values.cpu()[perm]).abs().max())
    print(f"permuted rows: |s - s[perm]| {err:.3g}")
    assert err <= 8 * 5000 * 2.0 ** -52
    assert torch.equal(moved.nearest.cpu(), one.nearest.cpu()[perm])


# -- dispersion ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GENERAL)
def test_dispersion_tables_and_indices(shape):
    """The blobs' centroids lie about 4 sqrt(2 F) apart with coordinates of a few units: their
    separations are far above 1e-2 of the coordinates, so 1e-10 on the tables leaves CH and DB
    within 1e-9.  Cluster k is empty."""
    N, F, k = shape
    x, y, _, want = general(shape)
    got = Q.dispersion(x.cuda(), y.cuda(), k + 1)
    assert got.count.dtype == torch.int64 and torch.equal(got.count.cpu(), want.count)
    assert got.count[k] == 0 and got.within[k] == 0
    assert bool(torch.isnan(got.centroid[k]).all()) and bool(torch.isnan(got.mean_distance[k]))
    cen, ref = got.centroid.cpu()[:k], want.centroid[:k]
    scale = ref.abs().max(1, keepdim=True).values          # a cluster's coordinate magnitude
    rel_c = float(((cen - ref).abs() / scale).max())
    rel_w = float(((got.within.cpu()[:k] - want.within[:k]).abs() / want.within[:k]).max())
    rel_s = float(((got.mean_distance.cpu()[:k] - want.mean_distance[:k]).abs()
                   / want.mean_distance[:k]).max())
    rel_ch = abs(got.calinski_harabasz - want.calinski_harabasz) / want.calinski_harabasz
    rel_db = abs(got.davies_bouldin - want.davies_bouldin) / want.davies_bouldin
    print(f"centroid {rel_c:.3g} W {rel_w:.3g} S {rel_s:.3g} CH {rel_ch:.3g} DB {rel_db:.3g}")
    assert rel_c <= 1e-10 and rel_w <= 1e-10 and rel_s <= 1e-10
    assert rel_ch <= 1e-9 and rel_db <= 1e-9
    again = Q.dispersion(x.cuda(), y.cuda(), k + 1)
    assert torch.equal(again.within, got.within)
    assert torch.equal(again.mean_distance[:k], got.mean_distance[:k])
    assert torch.equal(again.centroid[:k], got.centroid[:k])


# -- arguments, pipeline ------------------------------------------------------------------------
def test_labels_outside_the_range_are_counted_on_the_device():
    x, y = uniform(200, 4, 0).cuda(), (torch.arange(200) % 4).cuda()
    bad = y.clone()
    bad[[3, 50, 199]] = torch.tensor([-1, 4, 1 << 40]).cuda()
    for fn in (Q.silhouette, Q.dispersion, Q.quality):
        with pytest.raises(ValueError, match=r"3 labels outside \[0, 4\)"):
            fn(x, bad, 4)
        with pytest.raises(ValueError, match=r"50 labels outside \[0, 3\)"):
            fn(x, y, 3)
    with pytest.raises(ValueError, match="x must be fp32"):
        Q.silhouette(x.double(), y)
    with pytest.raises(ValueError, match="both be device tensors"):
        Q.silhouette(x, y.cpu())
    sil, disp = Q.quality(x, y.to(torch.int32))
    assert sil.values.shape == (200,) and disp.count.tolist() == [50] * 4


def test_label_indices_of_device_ids_is_the_host_tables():
    rng = np.random.default_rng(3)
    cid, lab = torch.from_numpy(rng.integers(0, 12, 3000)), torch.from_numpy(
        rng.integers(0, 10, 3000))
    assert Q.label_indices_of(cid.cuda(), lab.cuda(), 13, 10) == Q.label_indices(
        C.contingency(cid, lab, 13, 10))


@pytest.mark.parametrize("criterion", ["silhouette", "calinski_harabasz", "davies_bouldin"])
def test_select_k_picks_the_planted_k_on_the_device(criterion):
    x, _ = separated(600, 8, 5, 3)
    out = Q.select_k(x.cuda(), range(2, 9), criterion=criterion, n_init=4, seed=1)
    assert out.k == 5 and out.result.labels.is_cuda and out.table["k"] == list(range(2, 9))
    assert out.table["inertia"][3] == out.result.inertia


def test_unsupervised_accuracy_with_metrics_on_a_model():
    from tests.test_eval_step_gpu import _model
    from tests.test_hip_model import full_size_params
    from torch_scae_amd import EvalStep, ops
    cfg, B, sd, g = full_size_params("cfg2")
    model = _model(cfg, sd)
    # (both splits leave a remainder of 4: one tail step, captured by the first encode)
    images = torch.rand(2 * B + 8, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (2 * B + 8,), generator=g).cuda()
    fit, test = (images[:B + 4], labels[:B + 4]), (images[B + 4:], labels[B + 4:])
    step = EvalStep(model, B, cfg["image_shape"])
    step.encode(*fit)
    step.encode(*test)
    outs = []
    for metrics in (False, True):
        torch.manual_seed(5)
        ops.reset_noise()
        outs.append(C.unsupervised_accuracy(step, fit, test, k=4, n_init=2, seed=0,
                                            metrics=metrics))
    plain, more = outs
    assert list(plain) == ["fit_accuracy", "test_accuracy", "inertia", "mapping", "n_iter"]
    for name in plain:
        assert np.array_equal(more[name], plain[name]), name
    new = set(more) - set(plain)
    assert new == {"fit_nmi", "fit_ari", "fit_purity", "test_nmi", "test_ari", "test_purity",
                   "silhouette", "calinski_harabasz", "davies_bouldin"}
    for name in new:
        assert isinstance(more[name], float) and np.isfinite(more[name]), (name, more[name])
    assert -1 <= more["silhouette"] <= 1 and 0 < more["fit_purity"] <= 1
