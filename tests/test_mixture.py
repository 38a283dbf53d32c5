"""Gaussian mixtures on the host (torch_scae_amd.mixture): the numpy restatement against
scikit-learn's GaussianMixture from the same first parameters -- parameters, lower bound and
the stop rule --, its arithmetic on inputs checked by hand, the information criteria, the choice
of k and every argument error."""
import math

import numpy as np
import pytest
import torch

from torch_scae_amd import mixture as M

# Largest distances measured on the six cases below (3 shapes x 2 covariances, 7 iterations
# from the restatement's first M-step), fp64 restatement against scikit-learn 1.7 / against its
# own np.longdouble evaluation:
#   weights      1.3e-15 / 2.9e-15  absolute
#   means        2.4e-14 / 6.9e-15  absolute
#   variances    4.3e-13 / 3.3e-11  relative (E[x^2] - mu^2 cancels at variances near reg_covar)
#   lower bound  9.1e-12 / 4.4e-12  absolute
# The bound is 16 times the larger of the two: scikit-learn expands the square and sums in BLAS
# order.
TOL_WEIGHTS = 16 * 2.9e-15
TOL_MEANS = 16 * 2.4e-14
TOL_VAR_REL = 16 * 3.3e-11
TOL_BOUND = 16 * 9.1e-12
SHAPES = [(600, 5, 3), (2000, 24, 10), (257, 3, 4)]


def blobs(N, F, k, seed, sep=1.5):
    """Blobs with per-component per-feature spreads and column 0 clipped to [0, 1] -> (x (N, F)
    fp32 tensor, planted labels (N,) numpy).  ``sep`` scales the centres: small, they overlap."""
    g = np.random.default_rng(seed)
    centres = g.normal(size=(k, F)) * sep
    spread = g.uniform(0.05, 0.6, size=(k, F))
    y = g.integers(0, k, N)
    x = centres[y] + g.normal(size=(N, F)) * spread[y]
    x[:, 0] = np.clip(x[:, 0], 0.0, 1.0)
    return torch.from_numpy(x.astype(np.float32)), y


def _seeded(N, F, k, cov):
    from torch_scae_amd import cluster
    x, _ = blobs(N, F, k, N)
    lab = cluster.kmeans_host(x, k, n_init=1, seed=0).labels.numpy()
    X = x.double().numpy()
    w, mu, var = M.m_step_host(X, lab[:, None] == np.arange(k), 1e-6, cov)
    return x, X, lab, dict(weights_init=w, means_init=mu, precisions_init=1 / var)


@pytest.mark.parametrize("cov", ["diag", "spherical"])
@pytest.mark.parametrize("N,F,k", SHAPES)
def test_restatement_against_scikit_learn(N, F, k, cov):
    mixture = pytest.importorskip("sklearn.mixture")
    x, X, lab, inits = _seeded(N, F, k, cov)
    gm = mixture.GaussianMixture(k, covariance_type=cov, tol=0, max_iter=7, n_init=1,
                                 reg_covar=1e-6, **inits)
    with pytest.warns(Warning):          # (tol = 0 never converges)
        gm.fit(X)
    w, mu, var, lb, it, conv, failed = M._em_host(X, lab, k, cov, 1e-6, 0.0, 7, np.float64)
    assert (it, conv, failed) == (7, False, False)
    figures = (np.abs(w - gm.weights_).max(), np.abs(mu - gm.means_).max(),
               (np.abs(var - gm.covariances_) / gm.covariances_).max(),
               abs(lb - gm.lower_bound_))
    print("weights %.2e means %.2e variances (rel) %.2e lower bound %.2e" % figures)
    assert figures[0] <= TOL_WEIGHTS and figures[1] <= TOL_MEANS
    assert figures[2] <= TOL_VAR_REL and figures[3] <= TOL_BOUND
    # the public fit from the same labels is that restart
    res = M.fit_host(x, k, cov, init=torch.from_numpy(lab), tol=0.0, max_iter=7)
    assert np.array_equal(res.means.numpy(), mu) and res.lower_bound == lb
    assert tuple(res.variances.shape) == ((k, F) if cov == "diag" else (k,))
    # fit_predict's last E-step: the labels of the final parameters
    assert np.array_equal(res.labels.numpy(), gm.predict(X))


@pytest.mark.parametrize("cov", ["diag", "spherical"])
@pytest.mark.parametrize("N,F,k", SHAPES)
def test_stop_rule_against_scikit_learn(N, F, k, cov):
    mixture = pytest.importorskip("sklearn.mixture")
    x, X, lab, inits = _seeded(N, F, k, cov)
    gm = mixture.GaussianMixture(k, covariance_type=cov, tol=1e-3, max_iter=100, n_init=1,
                                 reg_covar=1e-6, **inits).fit(X)
    res = M.fit_host(x, k, cov, init=torch.from_numpy(lab), tol=1e-3, max_iter=100)
    assert (res.n_iter, res.converged) == (gm.n_iter_, gm.converged_)
    # a max_iter below that count stops unconverged, at that count
    if gm.n_iter_ > 1:
        short = M.fit_host(x, k, cov, init=torch.from_numpy(lab), tol=1e-3,
                           max_iter=gm.n_iter_ - 1)
        assert (short.n_iter, short.converged) == (gm.n_iter_ - 1, False)


def test_one_component_is_the_column_mean_and_variance():
    x, _ = blobs(300, 4, 2, 3)
    X = x.double().numpy()
    for cov in ("diag", "spherical"):
        res = M.fit_host(x, 1, cov, init=torch.zeros(300, dtype=torch.int64), reg_covar=0.25)
        var = (X ** 2).mean(0) - X.mean(0) ** 2 + 0.25
        assert res.converged and res.n_iter == 2          # lb_2 == lb_1
        assert float(res.weights[0]) == 1.0
        assert np.abs(res.means.numpy()[0] - X.mean(0)).max() <= 1e-14
        want = var if cov == "diag" else var.mean()
        assert np.abs(res.variances.numpy()[0] - want).max() <= 1e-13
        assert res.labels.tolist() == [0] * 300


def test_two_separated_point_masses_have_the_closed_form():
    # 3 rows at (0, 0) and 5 at (8, -8): every responsibility is exactly 0 or 1, so the
    # parameters are the groups' own and the lower bound is the closed form below
    x = torch.tensor([[0.0, 0.0]] * 3 + [[8.0, -8.0]] * 5)
    lab = torch.tensor([0] * 3 + [1] * 5)
    reg = 0.01
    res = M.fit_host(x, 2, "diag", init=lab, reg_covar=reg, tol=1e-3)
    assert res.converged and res.n_iter == 2 and res.labels.tolist() == lab.tolist()
    assert np.abs(res.weights.numpy() - [3 / 8, 5 / 8]).max() <= 1e-15
    assert np.abs(res.means.numpy() - [[0, 0], [8, -8]]).max() <= 1e-13
    # (E[x^2] - mu^2 at x = 8 cancels 64 to about 64 * 2^-52)
    assert np.abs(res.variances.numpy() - reg).max() <= 1e-13
    # each row sits on its component's mean: log pi_c - (2 log(2 pi) + 2 log reg) / 2
    lb = (3 * math.log(3 / 8) + 5 * math.log(5 / 8)) / 8 - math.log(2 * math.pi) - math.log(reg)
    assert abs(res.lower_bound - lb) <= 1e-10
    assert M.score(x, res) == pytest.approx(lb, abs=1e-10)


def test_an_empty_initial_cluster_has_the_stated_parameters():
    x, _ = blobs(50, 3, 2, 5)
    onehot = np.zeros((50, 3))
    onehot[:25, 0] = onehot[25:, 2] = 1.0
    for cov in ("diag", "spherical"):
        w, mu, var = M.m_step_host(x, onehot, 1e-6, cov)
        # nk = 10 * 2^-52, about 2e-15, of 50 rows
        assert w[1] == pytest.approx(10 * 2.0 ** -52 / 50, rel=1e-12)
        assert np.all(mu[1] == 0.0) and np.all(var[1] == 1e-6)
        assert abs(w.sum() - 1.0) <= 1e-15


def test_information_criteria_and_parameter_counts():
    assert M.n_parameters(10, 24, "diag") == 2 * 10 * 24 + 10 - 1
    assert M.n_parameters(10, 24, "spherical") == 10 * 24 + 2 * 10 - 1
    x, _ = blobs(400, 6, 3, 7)
    for cov in ("diag", "spherical"):
        res = M.fit_host(x, 3, cov, n_init=2, seed=1)
        s, p = M.score(x, res), M.n_parameters(3, 6, cov)
        assert s == float(M.score_samples(x, res).sum()) / 400
        assert M.bic(x, res) == -2 * 400 * s + p * math.log(400)
        assert M.aic(x, res) == -2 * 400 * s + 2 * p
        proba = M.predict_proba(x, res)
        assert tuple(proba.shape) == (400, 3)
        assert float((proba.sum(1) - 1).abs().max()) <= 3 * 2.0 ** -52
        assert torch.equal(M.predict(x, res), res.labels)
    sk = pytest.importorskip("sklearn.mixture")
    gm = sk.GaussianMixture(3, covariance_type="diag")
    diag = M.fit_host(x, 3, "diag", n_init=2, seed=1)
    gm.weights_, gm.means_, gm.covariances_ = (diag.weights.numpy(), diag.means.numpy(),
                                               diag.variances.numpy())
    gm.precisions_cholesky_ = 1 / np.sqrt(gm.covariances_)
    X = x.double().numpy()
    assert M.bic(x, diag) == pytest.approx(gm.bic(X), rel=1e-12)
    assert M.aic(x, diag) == pytest.approx(gm.aic(X), rel=1e-12)


def test_choose_k_ties_and_nan():
    nan = float("nan")
    table = {"k": [5, 2, 3, 4], "bic": [1.0, 1.0, nan, 2.0], "aic": [nan, 7.0, 3.0, 3.0]}
    assert M.choose_k(table, "bic") == 2          # the tie goes to the smallest k
    assert M.choose_k(table, "aic") == 3          # a NaN never wins
    with pytest.raises(ValueError):
        M.choose_k({"k": [2, 3], "bic": [nan, nan]}, "bic")
    with pytest.raises(ValueError):
        M.choose_k(table, "silhouette")


def test_select_k_on_the_host_fills_the_table_and_picks_the_planted_k():
    g = np.random.default_rng(0)
    y = g.integers(0, 3, 300)
    x = torch.from_numpy((np.array([[0.0, 0], [6, 0], [0, 6]])[y]
                          + g.normal(size=(300, 2)) * 0.3).astype(np.float32))
    out = M.select_k(x, [2, 3, 4, 5], criterion="bic", n_init=2)
    assert out.k == 3 and out.fit.means.shape[0] == 3
    assert list(out.table) == ["k", "lower_bound", "bic", "aic", "n_iter", "converged"]
    assert out.table["k"] == [2, 3, 4, 5]
    i = out.table["k"].index(3)
    assert out.table["bic"][i] == M.bic(x, out.fit) == min(out.table["bic"])
    assert out.table["lower_bound"][i] == out.fit.lower_bound
    for bad in ([], [2, 2], [0, 3], [2.0], 3):
        with pytest.raises(ValueError):
            M.select_k(x, bad)
    with pytest.raises(ValueError):
        M.select_k(x, [2, 3], criterion="silhouette")


@pytest.mark.parametrize("kwargs", [
    dict(x=torch.zeros(10)), dict(x=torch.zeros(0, 3)), dict(k=0), dict(k=2.0), dict(k=True),
    dict(covariance="full"), dict(init="random"), dict(tol=-1e-3), dict(tol=float("nan")),
    dict(reg_covar=-1e-6), dict(max_iter=0), dict(n_init=0),
    dict(init=torch.zeros(9, dtype=torch.int64)), dict(init=torch.zeros(10)),
    dict(init=torch.full((10,), 3, dtype=torch.int64)),
    dict(init=torch.full((2, 10), -1, dtype=torch.int64)),
])
def test_every_argument_error(kwargs):
    args = dict(x=torch.rand(10, 3), k=3)
    args.update(kwargs)
    x = args.pop("x")
    with pytest.raises(ValueError):
        M.fit(x, **args)
    with pytest.raises(ValueError):
        M.fit_host(x, **args)


def test_all_restarts_failing_raises():
    # duplicated rows with a constant column: its variance is exactly 0 in every component
    x = torch.tensor([[0.0, 1.0], [0.0, 2.0]] * 20)
    lab = torch.tensor([[0, 1] * 20, [1, 0] * 20])
    with pytest.raises(ValueError, match="every restart failed"):
        M.fit_host(x, 2, init=lab, reg_covar=0.0)
    assert M.fit_host(x, 2, init=lab, reg_covar=1e-6).converged
    # one restart that survives wins, whatever its lower bound
    x2 = torch.tensor([[0.0, 1.0], [1.0, 2.0], [0.5, 1.0], [1.5, 2.5]] * 10)
    lab2 = torch.tensor([[0, 0, 0, 0] * 10,         # component 1 empty: variance 0
                         [0, 1, 0, 1] * 10])
    res = M.fit_host(x2, 2, init=lab2, reg_covar=0.0)
    assert res.restart == 1 and math.isnan(float(res.lower_bounds[0]))


class _Step:
    """An EvalStep stand-in: ``encode`` returns the split's rows as capsule features."""
    class model:
        n_classes = 3

    def encode(self, images, labels):
        return {"prior": images, "posterior": images, "label": labels,
                "features": torch.stack([images, images], 1)}


def test_unsupervised_accuracy_on_planted_clusters():
    from torch_scae_amd import cluster as C
    g = np.random.default_rng(3)
    centres = np.array([[0.0, 0, 0, 0], [5.0, 0, 0, 0], [0, 5.0, 0, 0]])
    sigma = np.array([0.1, 1.5, 0.1])

    def split(n):
        y = g.integers(0, 3, n)
        x = centres[y] + g.normal(size=(n, 4)) * sigma[y, None]
        return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y)
    fit, test = split(600), split(200)
    out = M.unsupervised_accuracy(_Step(), fit, test, k=3, n_init=3, seed=0, metrics=True)
    for key in ("fit_accuracy", "test_accuracy", "lower_bound", "bic", "test_score", "mapping",
                "n_iter", "fit_nmi", "test_ari", "test_purity", "silhouette"):
        assert key in out, key
    assert "inertia" not in out
    res = M.fit(fit[0], 3, n_init=3, seed=0)
    mapping, acc = C.match_clusters(res.labels, fit[1], 3, 3)
    assert out["fit_accuracy"] == acc >= 0.99 and out["mapping"].tolist() == mapping.tolist()
    cid = M.predict(test[0], res)
    assert out["test_accuracy"] == C.mapped_accuracy(cid, test[1], mapping, 3)
    assert out["bic"] == M.bic(fit[0], res) and out["test_score"] == M.score(test[0], res)
    # k-means mislabels the wide cluster's fringe; the mixture does not
    km = C.match_clusters(C.kmeans(fit[0], 3, seed=0).labels, fit[1], 3, 3)[1]
    assert km < acc
