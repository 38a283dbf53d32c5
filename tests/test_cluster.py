"""Host side of the unsupervised classification (torch_scae_amd/cluster.py): the Hungarian
matching against brute force and scipy, the majority rule for more clusters than classes,
the fp64 k-means restatement on separable blobs, argument checks, and EvalStep.encode on a
CPU model (rows against an eager forward, means against evaluate())."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from torch_scae_amd import cluster as C


def _best_by_permutation(T):
    k, n = T.shape
    return max(sum(T[i, p[i]] for i in range(k)) for p in itertools.permutations(range(n), k))


def test_hungarian_matches_brute_force_up_to_six_clusters():
    rng = np.random.default_rng(0)
    for _ in range(300):
        k = int(rng.integers(1, 7))
        n = int(rng.integers(k, 7))
        T = rng.integers(0, 30, (k, n))
        m = C.mapping_from_table(T)
        assert len(set(m.tolist())) == k and m.min() >= 0 and m.max() < n
        assert T[np.arange(k), m].sum() == _best_by_permutation(T)


def test_hungarian_matches_scipy_on_square_and_rectangular_tables():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(1)
    for k, n in [(10, 10)] * 20 + [(4, 9), (7, 12), (1, 5), (10, 16)] * 5:
        T = rng.integers(0, 500, (k, n))
        m = C.mapping_from_table(T)
        r, c = opt.linear_sum_assignment(-T)
        assert T[np.arange(k), m].sum() == T[r, c].sum()


def test_hungarian_on_costs_with_ties_is_optimal():
    rng = np.random.default_rng(2)
    for _ in range(100):
        T = rng.integers(0, 3, (5, 6))
        m = C.mapping_from_table(T)
        assert T[np.arange(5), m].sum() == _best_by_permutation(T)


def test_more_clusters_than_classes_take_the_majority_class():
    T = np.array([[5, 1, 0], [0, 2, 2], [0, 0, 9], [3, 3, 0], [1, 7, 0]])
    m = C.mapping_from_table(T)
    assert m.tolist() == [0, 1, 2, 0, 1]         # (ties to the lowest class)
    cid = torch.tensor(sum(([c] * int(T[c].sum()) for c in range(5)), []))
    lab = torch.tensor(sum(([l] * int(T[c, l]) for c in range(5) for l in range(3)), []))
    mapping, acc = C.match_clusters(cid, lab, 5, 3)
    assert mapping.tolist() == m.tolist()
    assert acc == (5 + 2 + 9 + 3 + 7) / T.sum()


def _blobs(n_per, k, F, seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(k, F, generator=g, dtype=torch.float64) * 20
    x = torch.cat([centres[c] + torch.randn(n_per, F, generator=g, dtype=torch.float64)
                   for c in range(k)])
    y = torch.arange(k).repeat_interleave(n_per)
    return x.float(), y, centres


def test_host_kmeans_on_blobs_recovers_a_permutation_of_the_classes():
    x, y, _ = _blobs(60, 6, 5, 3)
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    labels = perm[y]
    res = C.kmeans_host(x, 6, n_init=4, seed=7)
    assert res.converged and res.n_iter >= 2
    assert res.labels.shape == (360,) and res.labels.dtype == torch.int64
    mapping, acc = C.match_clusters(res.labels, labels, 6, 6)
    assert acc == 1.0
    # each cluster's points carry one class: the mapping is the permutation in cluster terms
    for c in range(6):
        assert set(labels[res.labels == c].tolist()) == {int(mapping[c])}
    # inertia is the fp64 sum of the points' squared distances to their centroids
    d = ((x.double() - res.centroids[res.labels]) ** 2).sum()
    assert abs(res.inertia - float(d)) <= 1e-9 * float(d)
    # CPU tensors take the host path through kmeans() too, and assign() agrees
    again = C.kmeans(x, 6, n_init=4, seed=7)
    assert torch.equal(again.labels, res.labels) and again.inertia == res.inertia
    assert torch.equal(C.assign(x, res.centroids), res.labels)


def test_host_kmeans_pp_draws_follow_the_d2_rule():
    x, _, _ = _blobs(20, 3, 2, 4)
    cent, chosen, margin = C.kmeans_pp_host(x, 3, n_init=2, seed=11)
    X = x.double().numpy()
    for r in range(2):
        w = np.ones(len(X))
        for j in range(3):
            u = float(C.pp_uniform(11, r, j))
            assert 0.0 <= u < 1.0
            cs = np.cumsum(w)
            assert chosen[r, j] == np.argmax(cs > u * cs[-1])
            d = ((X - X[chosen[r, j]]) ** 2).sum(1)
            w = d if j == 0 else np.minimum(w, d)
            assert np.array_equal(cent[r, j], X[chosen[r, j]])
    assert (margin >= 0).all()
    # different restarts draw different uniforms
    assert C.pp_uniform(11, 0, 0) != C.pp_uniform(11, 1, 0)


def test_given_init_and_empty_clusters_keep_their_centroid():
    x = torch.tensor([[0.0], [0.1], [10.0], [10.2]])
    init = torch.tensor([[0.0], [10.0], [100.0]])     # cluster 2 never wins a point
    res = C.kmeans_host(x, 3, init=init)
    assert res.labels.tolist() == [0, 0, 1, 1] and res.converged and res.n_iter == 2
    assert res.centroids[2, 0] == 100.0
    assert float(res.centroids[0, 0]) == (0.0 + float(np.float32(0.1))) / 2
    one = C.kmeans_host(x, 3, init=init, max_iter=1)  # stopped: no update after the last
    assert not one.converged and one.n_iter == 1 and torch.equal(one.centroids,
                                                                 init.double())


def test_arguments_are_checked():
    x = torch.zeros(10, 4)
    with pytest.raises(ValueError):
        C.kmeans(x, 0)
    with pytest.raises(ValueError):
        C.kmeans(x, 257)
    with pytest.raises(ValueError):
        C.kmeans(torch.zeros(10, 257), 2)
    with pytest.raises(ValueError):
        C.kmeans(torch.zeros(10, 200), 100)           # k * F > 16384
    with pytest.raises(ValueError):
        C.kmeans(torch.zeros(0, 4), 2)
    with pytest.raises(ValueError):
        C.kmeans(x, 3, init=torch.zeros(3, 5))        # bad init shape
    with pytest.raises(ValueError):
        C.kmeans(x, 3, init=torch.zeros(2, 2, 4))
    with pytest.raises(ValueError):
        C.kmeans(x, 3, init="random")
    with pytest.raises(ValueError):
        C.kmeans(x, 3, max_iter=0)
    with pytest.raises(ValueError):
        C.assign(x, torch.zeros(3, 5))
    with pytest.raises(ValueError):
        C.match_clusters(torch.tensor([0, 4]), torch.tensor([0, 1]), 3, 2)
    with pytest.raises(ValueError):
        C.features({"prior": x}, "mass")


def test_kmeans_entry_points_reject_bad_arguments_without_a_gpu():
    from torch_scae_amd import _lib
    lib = _lib.load()
    assert lib.scae_kmeans_supported(10, 24) == 1
    assert lib.scae_kmeans_supported(257, 1) == 0 and lib.scae_kmeans_supported(100, 200) == 0
    assert lib.scae_kmeans_groups(60000, 10) == 204 and lib.scae_kmeans_groups(100, 1) == 1
    assert lib.scae_kmeans_lloyd_f32(None, 1, None) == -1
    assert lib.scae_kmeans_assign_f32(None, 10, 4, 2, None, None, None) == -1
    assert lib.scae_eval_features_f32(None, None, 4, 4, 4, None, None) == -1


class StubSCAE(torch.nn.Module):
    """A CPU stand-in with the surface EvalStep.encode reads (SCAE's kernels run on the GPU
    only): object-capsule presences, a posterior mixing probability over M parts, class
    probabilities, and a loss that depends on the batch size."""

    n_classes = 3

    def __init__(self, O=4, M=5):
        super().__init__()
        self.obj_decoder = SimpleNamespace(n_obj_capsules=O)
        self.w = torch.nn.Parameter(torch.linspace(0.5, 1.5, O * M).view(O, M))
        self.O, self.M = O, M

    def forward(self, image):
        x = image.flatten(1)[:, :self.O * self.M].view(-1, self.O, self.M) * self.w
        post = torch.softmax(x, 1)
        presence = torch.sigmoid(x.mean(-1))
        return SimpleNamespace(caps_presence=presence, posterior_mixing_prob=post,
                               prior_cls_prob=torch.softmax(presence[:, :3], -1),
                               posterior_cls_prob=torch.softmax(post.sum(-1)[:, :3], -1))

    def loss(self, res, image, label):
        lp = image.mean() * image.shape[0]
        loss = lp + res.prior_cls_prob[:, 0].mean()
        return loss, dict(log_prob_loss=lp, rec_ll_loss=loss - lp,
                          cpr_dynamic_reg_loss=torch.zeros(()))


def test_encode_on_a_cpu_model_gives_the_eager_rows_and_evaluate_means():
    from torch_scae_amd import EvalStep
    model = StubSCAE()
    g = torch.Generator().manual_seed(5)
    N, B, O = 11, 4, 4
    images = torch.rand(N, 1, 5, 5, generator=g)
    labels = torch.randint(0, 3, (N,), generator=g)
    step = EvalStep(model, B, (1, 5, 5))
    enc = step.encode(images, labels)
    assert enc["prior"].shape == (N, O) and enc["posterior"].shape == (N, O)
    assert torch.equal(enc["label"], labels) and enc["rows"] == N and not enc["overflow"]
    with torch.no_grad():
        for lo in range(0, N, B):
            res = model(images[lo:lo + B])
            assert torch.equal(enc["prior"][lo:lo + B], res.caps_presence)
            assert torch.equal(enc["posterior"][lo:lo + B], res.posterior_mixing_prob.sum(-1))
    want = step.evaluate(images, labels)
    for key in ("loss", "accuracy", "prior_accuracy", "posterior_accuracy", "log_prob",
                "rec_ll"):
        assert torch.equal(enc["means"][key], want[key]), key
    assert enc["means"]["batches"] == want["batches"] == 3
    # a short output: the rows that fit, and the overflow reported
    enc2 = step.encode(images, labels, out=torch.empty(6, 2, O))
    assert enc2["rows"] == 6 and enc2["overflow"]
    assert torch.equal(enc2["prior"], enc["prior"][:6])
    # unlabelled splits encode too
    enc3 = step.encode(images)
    assert enc3["label"] is None and torch.equal(enc3["prior"], enc["prior"])
    assert torch.equal(C.features(enc, "both"), enc["features"].reshape(N, 2 * O))


def test_unsupervised_accuracy_on_a_cpu_model_is_the_host_pipeline():
    from torch_scae_amd import EvalStep
    model = StubSCAE()
    g = torch.Generator().manual_seed(6)
    images = torch.rand(40, 1, 5, 5, generator=g)
    labels = torch.randint(0, 3, (40,), generator=g)
    step = EvalStep(model, 8, (1, 5, 5))
    init = torch.rand(2, 3, 4, generator=g)
    out = C.unsupervised_accuracy(step, (images[:30], labels[:30]), (images[30:], labels[30:]),
                                  k=3, feature="prior", init=init)
    assert set(out) == {"fit_accuracy", "test_accuracy", "inertia", "mapping", "n_iter"}
    fit = step.encode(images[:30], labels[:30])
    test = step.encode(images[30:], labels[30:])
    res = C.kmeans_host(fit["prior"], 3, init=init)
    mapping, acc = C.match_clusters(res.labels, labels[:30], 3, 3)
    assert out["fit_accuracy"] == acc and out["mapping"].tolist() == mapping.tolist()
    cid = C.assign(test["prior"], res.centroids)
    assert out["test_accuracy"] == float((torch.from_numpy(mapping)[cid] == labels[30:])
                                         .double().mean())
    assert 0.0 <= out["fit_accuracy"] <= 1.0 and out["inertia"] == res.inertia
    with pytest.raises(ValueError):
        C.unsupervised_accuracy(step, (images, labels), feature="mass")
