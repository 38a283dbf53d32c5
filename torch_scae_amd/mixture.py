"""Gaussian mixtures on SCAE's capsule features: EM with diagonal or spherical covariance, soft
responsibilities, a likelihood and therefore BIC / AIC to choose ``k`` without labels, and
unsupervised accuracy from mixture components instead of k-means' Voronoi cells.

Everything here runs in numpy on the host (``fit_host`` / ``e_step_host`` / ``m_step_host``,
fp64, or ``np.longdouble`` for the tests); tensors are brought to the CPU first.  There are no
device kernels yet: this is the statement of the rules they will be checked against, all in fp64
on x (N, F) read exactly:

- M-step from responsibilities r: nk_c = sum_n r_nc + 10 * 2^-52, mu_cf = sum_n r_nc x_nf / nk_c,
  var_cf = sum_n r_nc x_nf^2 / nk_c - mu_cf^2 + reg_covar (spherical: var_c the mean of these
  over f), pi_c = nk_c / sum_c nk_c;
- E-step: lw_nc = log pi_c - (F log(2 pi) + sum_f log var_cf + sum_f (x_nf - mu_cf)^2 / var_cf)
  / 2 (the quadratic form taken directly), lse_n = m + log sum_c exp(lw_nc - m) with m = max_c
  lw_nc, r_nc = exp(lw_nc - lse_n); the lower bound is sum_n lse_n / N; the hard label is the
  first largest lw_nc;
- every restart starts from hard labels: its first parameters are the M-step of their one-hot
  responsibilities (an empty cluster: mean 0, variance reg_covar, weight about 1e-15);
- iteration it = 1, 2, ... is an E-step under the current parameters (lb_it), then an M-step;
  the restart stops converged when |lb_it - lb_(it-1)| < tol (lb_0 = -inf), unconverged after
  ``max_iter`` iterations; its result is the parameters after its last M-step and the lower
  bound of its last E-step (scikit-learn's ``GaussianMixture.fit`` loop);
- a restart whose lower bound or parameters are not finite, or with a variance <= 0, stops as
  failed and cannot win (possible only with reg_covar = 0);
- the result is the restart of greatest lower bound, ties to the lowest restart index; labels,
  responsibilities and row log-likelihoods come from one more E-step under the final parameters.
"""
import math
from typing import Any, NamedTuple

import numpy as np
import torch

from . import cluster as _cluster

_COVARIANCES = ("diag", "spherical")
_NK_EPS = 10 * 2.0 ** -52


class GmmResult(NamedTuple):
    weights: torch.Tensor        # (k,) fp64
    means: torch.Tensor          # (k, F) fp64
    variances: torch.Tensor      # (k, F) fp64 diag, (k,) spherical
    labels: torch.Tensor         # (N,) int64: the first largest log-weight of each row
    lower_bound: float           # mean row log-likelihood of the chosen restart's last E-step
    n_iter: int                  # its EM iterations
    converged: bool
    restart: int                 # the chosen restart
    lower_bounds: torch.Tensor   # (n_init,) fp64 CPU; a failed restart's is NaN
    covariance: str
    reg_covar: float


class SelectKResult(NamedTuple):
    table: dict
    k: int
    fit: Any


# -- arguments --------------------------------------------------------------------------------
def _check_k(k):
    if not isinstance(k, int) or isinstance(k, bool) or k <= 0:
        raise ValueError(f"k must be a positive int, got {k!r}")


def _check_cov(covariance):
    if covariance not in _COVARIANCES:
        raise ValueError(f"covariance must be 'diag' or 'spherical', got {covariance!r}")


def _args(x, k, covariance, n_init, max_iter, tol, reg_covar, init):
    """-> (restarts, labels (R, N) int64 tensor or None for a named init)"""
    _cluster._check_x(x)
    N = x.shape[0]
    _check_k(k)
    _check_cov(covariance)
    if not isinstance(max_iter, int) or isinstance(max_iter, bool) or max_iter <= 0:
        raise ValueError(f"max_iter must be a positive int, got {max_iter!r}")
    if not tol >= 0:
        raise ValueError(f"tol must be >= 0, got {tol!r}")
    if not reg_covar >= 0:
        raise ValueError(f"reg_covar must be >= 0, got {reg_covar!r}")
    if isinstance(init, str):
        if init not in ("k-means++", "kmeans"):
            raise ValueError("init must be 'k-means++', 'kmeans' or an int64 tensor of labels, "
                             f"got {init!r}")
        if not isinstance(n_init, int) or isinstance(n_init, bool) or n_init <= 0:
            raise ValueError(f"n_init must be a positive int, got {n_init!r}")
        return n_init, None
    lab = torch.as_tensor(init)
    if lab.dtype != torch.int64:
        raise ValueError(f"init labels must be int64, got {lab.dtype}")
    if lab.dim() == 1:
        lab = lab[None]
    if lab.dim() != 2 or lab.shape[0] == 0 or lab.shape[1] != N:
        raise ValueError(f"init labels must be (N,) = ({N},) or (n_init, {N}), got "
                         f"{tuple(torch.as_tensor(init).shape)}")
    if int(lab.min()) < 0 or int(lab.max()) >= k:
        raise ValueError(f"init labels must lie in [0, {k})")
    return lab.shape[0], lab


def _init_labels(x, k, R, init, seed):
    """The (R, N) int64 start labels of a named init (x on the CPU)."""
    if init == "kmeans":
        return torch.stack([_cluster.kmeans(x, k, n_init=1, seed=seed + r).labels
                            for r in range(R)])
    cent = torch.from_numpy(_cluster.kmeans_pp_host(x, k, R, seed)[0])
    return torch.stack([_cluster.assign(x, cent[r]) for r in range(R)])


# -- the host restatement (numpy) ---------------------------------------------------------------
def _np(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(dtype)


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def m_step_host(x, resp, reg_covar=1e-6, covariance="diag", dtype=np.float64):
    """-> (weights (k,), means (k, F), variances (k, F) or (k,)) of responsibilities (N, k)."""
    _check_cov(covariance)
    X, r = _np(x, dtype), _np(resp, dtype)
    with np.errstate(all="ignore"):
        nk = r.sum(0) + dtype(_NK_EPS)
        mu = (r.T @ X) / nk[:, None]
        var = (r.T @ (X * X)) / nk[:, None] - mu * mu + dtype(reg_covar)
        if covariance == "spherical":
            var = var.sum(1) / dtype(X.shape[1])
        return nk / nk.sum(), mu, var


def e_step_host(x, weights, means, variances, dtype=np.float64):
    """-> (lw (N, k), lse (N,), resp (N, k), lower bound) under the given parameters;
    ``variances`` (k, F) or (k,)."""
    X, w, mu, var = _np(x, dtype), _np(weights, dtype), _np(means, dtype), _np(variances, dtype)
    N, F = X.shape
    if var.ndim == 1:
        var = np.repeat(var[:, None], F, 1)
    with np.errstate(all="ignore"):
        lw = np.empty((N, w.shape[0]), dtype)
        const = dtype(F) * np.log(2 * _pi(dtype))
        for c in range(w.shape[0]):
            u = X - mu[c]
            lw[:, c] = np.log(w[c]) - (const + np.log(var[c]).sum() + (u * u / var[c]).sum(1)) / 2
        m = lw.max(1)
        lse = m + np.log(np.exp(lw - m[:, None]).sum(1))
        return lw, lse, np.exp(lw - lse[:, None]), lse.sum() / dtype(N)


def _params_ok(w, mu, var):
    return bool(np.isfinite(w).all() and np.isfinite(mu).all() and np.isfinite(var).all()
                and (var > 0).all())


def _em_host(X, lab, k, covariance, reg_covar, tol, max_iter, dtype):
    """One restart -> (weights, means, variances, lower bound, iterations, converged, failed)"""
    onehot = (lab[:, None] == np.arange(k)[None]).astype(dtype)
    w, mu, var = m_step_host(X, onehot, reg_covar, covariance, dtype)
    if not _params_ok(w, mu, var):
        return w, mu, var, -np.inf, 0, False, True
    prev, it = -np.inf, 0
    while True:
        it += 1
        _, _, resp, lb = e_step_host(X, w, mu, var, dtype)
        if not np.isfinite(lb):
            return w, mu, var, lb, it, False, True
        w, mu, var = m_step_host(X, resp, reg_covar, covariance, dtype)
        if not _params_ok(w, mu, var):
            return w, mu, var, lb, it, False, True
        if abs(lb - prev) < tol:
            return w, mu, var, lb, it, True, False
        if it >= max_iter:
            return w, mu, var, lb, it, False, False
        prev = lb


def _choose_restart(lbs, failed):
    """Greatest lower bound among the restarts that did not fail, ties to the lowest index."""
    best = None
    for r, (lb, bad) in enumerate(zip(lbs, failed)):
        if not bad and (best is None or lb > lbs[best]):
            best = r
    if best is None:
        raise ValueError("every restart failed (a variance <= 0 or a non-finite value): "
                         "raise reg_covar")
    return best


def fit_host(x, k, covariance="diag", n_init=10, max_iter=100, tol=1e-3, reg_covar=1e-6,
             init="k-means++", seed=0, dtype=np.float64):
    """``fit`` in numpy (the kernels' check; CPU tensors take it).  -> GmmResult with fp64 CPU
    tensors."""
    R, lab = _args(x, k, covariance, n_init, max_iter, tol, reg_covar, init)
    if lab is None:
        lab = _init_labels(x.detach().cpu(), k, R, init, seed)
    X, lab = _np(x, dtype), lab.cpu().numpy()
    runs = [_em_host(X, lab[r], k, covariance, reg_covar, tol, max_iter, dtype)
            for r in range(R)]
    best = _choose_restart([u[3] for u in runs], [u[6] for u in runs])
    w, mu, var, lb, it, conv, _ = runs[best]
    lw = e_step_host(X, w, mu, var, dtype)[0]
    lbs = np.array([np.nan if u[6] else float(u[3]) for u in runs])
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
    return GmmResult(t(w), t(mu), t(var), torch.from_numpy(np.argmax(lw, 1).astype(np.int64)),
                     float(lb), int(it), bool(conv), int(best), t(lbs), covariance,
                     float(reg_covar))


def fit(x, k, covariance="diag", n_init=10, max_iter=100, tol=1e-3, reg_covar=1e-6,
        init="k-means++", seed=0):
    """EM for a mixture of ``k`` Gaussians with ``covariance`` "diag" or "spherical" on the rows
    of ``x`` (N, F).  ``init``: "k-means++" (restart r: the k-means++ centres of (seed, r), every
    row assigned to its nearest), "kmeans" (the labels of ``cluster.kmeans(x, k, n_init=1,
    seed=seed + r)``) or an int64 tensor of labels (N,) / (n_init, N).  -> GmmResult of the
    restart with the greatest lower bound (``fit_host``: there is no device path)."""
    return fit_host(x, k, covariance, n_init, max_iter, tol, reg_covar, init, seed)


# -- scoring --------------------------------------------------------------------------------------
def _e_pass(x, model, resp):
    """-> (labels (N,), row log-likelihood (N,), resp (N, k) or None), CPU tensors"""
    _cluster._check_x(x)
    if x.shape[1] != model.means.shape[1]:
        raise ValueError(f"x must be (N, {model.means.shape[1]}), got {tuple(x.shape)}")
    lw, lse, rs, _ = e_step_host(x, model.weights, model.means, model.variances)
    return (torch.from_numpy(np.argmax(lw, 1).astype(np.int64)), torch.from_numpy(lse),
            torch.from_numpy(rs) if resp else None)


def score_samples(x, model):
    """(N,) fp64 log-likelihood of each row of ``x`` under ``model`` (a GmmResult)."""
    return _e_pass(x, model, False)[1]


def score(x, model):
    """The mean row log-likelihood."""
    return float(score_samples(x, model).sum()) / x.shape[0]


def predict(x, model):
    """(N,) int64 component of each row: the first largest weighted log-density."""
    return _e_pass(x, model, False)[0]


def predict_proba(x, model):
    """(N, k) fp64 responsibilities."""
    return _e_pass(x, model, True)[2]


def n_parameters(k, F, covariance="diag"):
    """Free parameters: 2 k F + k - 1 (diag), k F + 2 k - 1 (spherical)."""
    _check_cov(covariance)
    return 2 * k * F + k - 1 if covariance == "diag" else k * F + 2 * k - 1


def _criteria(N, F, k, covariance, mean_ll):
    p = n_parameters(k, F, covariance)
    return -2 * N * mean_ll + p * math.log(N), -2 * N * mean_ll + 2 * p


def bic(x, model):
    """-2 N score + p log N."""
    k, F = model.means.shape
    return _criteria(x.shape[0], F, k, model.covariance, score(x, model))[0]


def aic(x, model):
    """-2 N score + 2 p."""
    k, F = model.means.shape
    return _criteria(x.shape[0], F, k, model.covariance, score(x, model))[1]


# -- model selection --------------------------------------------------------------------------------
_COLUMNS = ("k", "lower_bound", "bic", "aic", "n_iter", "converged")


def choose_k(table, criterion="bic"):
    """The k of the least ``criterion`` in a ``select_k`` table, ties to the smallest k; a NaN
    never wins."""
    if criterion not in ("bic", "aic"):
        raise ValueError(f"criterion must be 'bic' or 'aic', got {criterion!r}")
    best = None
    for k, v in zip(table["k"], table[criterion]):
        if v == v and (best is None or (v, k) < (best[1], best[0])):
            best = (k, v)
    if best is None:
        raise ValueError(f"{criterion} is NaN for every k in {tuple(table['k'])!r}")
    return best[0]


def select_k(x, ks, criterion="bic", **fit_args):
    """``fit`` (with ``fit_args``) for every k in ``ks``, each fit's lower bound, BIC and AIC on
    ``x``, and the k of the least ``criterion``.  -> SelectKResult(table {"k", "lower_bound",
    "bic", "aic", "n_iter", "converged"} of lists, k, its GmmResult)."""
    if criterion not in ("bic", "aic"):
        raise ValueError(f"criterion must be 'bic' or 'aic', got {criterion!r}")
    try:
        ks = tuple(ks)
    except TypeError:
        raise ValueError(f"ks must be a sequence of ints, got {ks!r}") from None
    if not ks or any(not isinstance(v, int) or isinstance(v, bool) or v < 1 for v in ks) or \
            len(set(ks)) != len(ks):
        raise ValueError(f"ks must be distinct positive ints, got {ks!r}")
    _cluster._check_x(x)
    table = {c: [] for c in _COLUMNS}
    fits = {}
    for k in ks:
        res = fits[k] = fit(x, k, **fit_args)
        b, a = _criteria(x.shape[0], x.shape[1], k, res.covariance, score(x, res))
        for c, v in zip(_COLUMNS, (k, res.lower_bound, b, a, res.n_iter, res.converged)):
            table[c].append(v)
    best = choose_k(table, criterion)
    return SelectKResult(table, best, fits[best])


# -- the whole measurement ---------------------------------------------------------------------
def unsupervised_accuracy(step, fit_split, *others, k=10, feature="prior", names=None,
                          n_classes=None, metrics=False, **fit_args):
    """``cluster.unsupervised_accuracy`` with mixture components as clusters: ``fit`` on the
    object-capsule features of ``fit_split`` (encoded by the EvalStep ``step``), components
    matched to classes on its contingency table, and that mapping applied to ``others``
    labelled by ``predict`` under the fitted model.  -> {"fit_accuracy", "<name>_accuracy"...,
    "lower_bound", "bic", "<name>_score"..., "mapping", "n_iter"}; ``metrics=True`` adds the
    figures of ``cluster.unsupervised_accuracy``."""
    C = _cluster
    if names is None:
        names = ["test"] if len(others) == 1 else [f"split{i + 1}" for i in range(len(others))]
    if len(names) != len(others):
        raise ValueError("one name per split")
    if n_classes is None:
        n_classes = getattr(step.model, "n_classes", None)
    enc = C._encode(step, fit_split)
    if n_classes is None:
        n_classes = int(enc["label"].max()) + 1
    xf = C.features(enc, feature)
    res = fit(xf, k, **fit_args)
    res = res._replace(labels=res.labels.to(xf.device))
    mapping, acc = C.match_clusters(res.labels, enc["label"], k, n_classes)
    out = {"fit_accuracy": acc}
    if metrics:
        from . import cluster_quality as Q

        def label_figures(name, cid, lab):
            ind = Q.label_indices_of(cid, lab, k, n_classes)
            out.update({f"{name}_{m}": ind[m] for m in ("nmi", "ari", "purity")})

        label_figures("fit", res.labels, enc["label"])
    for name, split in zip(names, others):
        e = C._encode(step, split)
        cid, ll, _ = _e_pass(C.features(e, feature), res, False)
        cid = cid.to(xf.device)
        out[f"{name}_accuracy"] = C.mapped_accuracy(cid, e["label"], mapping, n_classes)
        out[f"{name}_score"] = float(ll.sum()) / ll.shape[0]
        if metrics:
            label_figures(name, cid, e["label"])
    if metrics:
        sil, disp = Q.quality(xf, res.labels, k)
        out.update(silhouette=sil.score, calinski_harabasz=disp.calinski_harabasz,
                   davies_bouldin=disp.davies_bouldin)
    out.update(lower_bound=res.lower_bound, bic=bic(xf, res), mapping=mapping,
               n_iter=res.n_iter)
    return out
