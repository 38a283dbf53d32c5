"""k nearest neighbours on the capsule features: the exact search, the k-NN classifier on the
frozen features (the third standard figure for an unsupervised encoder, beside the cluster
matching of ``cluster`` and the linear probe of ``probe``; the only one with no fit) and the
trustworthiness of an embedding (the quality figure of ``embed``'s t-SNE that can be compared
across perplexities, which its KL cannot).

``knn`` / ``classify`` / ``ranks`` / ``trustworthiness`` run on the library's kernels
(csrc/knn.hip) for device tensors; ``knn_host`` / ``classify_host`` / ``ranks_host`` /
``trustworthiness_host`` are the same rules in numpy, used for CPU tensors and to check the
kernels.  The rules define arithmetic that numpy's float32 reproduces exactly and a total order,
so the device's bits are the host's bits: nothing is screened, nothing has a tolerance.

- inputs: queries q (Nq, F) fp32 and a base b (Nb, F) fp32, 1 <= F <= 256, 1 <= k <= 64,
  k <= Nb, Nq and Nb < 2^31.  In self mode (``base=None``) the base is q itself and row i is not
  its own neighbour, so k <= N - 1.  Inputs are finite; anything else is the caller's error and
  is not checked (a check would cost a host read);
- distance: d_ij = sum_f (q_if - b_jf)^2, accumulated in f order from 0; the difference, the
  product and the sum are each rounded to fp32, there is no fused multiply-add (``cluster``'s
  k-means fuses and is checked against fp64 through a margin; here the bits are the contract);
- order: neighbours ascend by the pair (d_ij, j) -- equal distances go to the lower base index.
  The result, idx (Nq, k) int64 and d2 (Nq, k) fp32, does not depend on how the base is split
  over workgroups;
- vote: ``ks`` is an ascending tuple of at most 8 list lengths, the search runs at k = ks[-1];
  ``weights`` is "uniform" or "distance".  Walking the neighbour list m = 0, 1, ...: uniform
  w_m = 1; distance w_m = 1 / sqrt(d2_m), the root and the quotient each correctly rounded in
  fp32 -- unless d2_0 == 0, then w_m = 1 where d2_m == 0 and 0 elsewhere (the zeros are a prefix
  of the list, so the rule does not depend on k).  The tally of neighbour m is the fp32 sum, in
  list order, of w_n over n <= m with label_n == label_m; the running best becomes
  (tally, label_m) when the tally is greater, or equal with a lower label; the prediction for
  ks[i] is the best after neighbour ks[i] - 1.  This is scikit-learn's KNeighborsClassifier with
  ties to the lowest class; it needs no per-class array, so labels are any int64 values;
- rank (self mode): r(i, j) = 1 + #{ l != i : (d_il, l) < (d_ij, j) };
- trustworthiness of an embedding y (N, E), E <= 256, of features x (N, F), for k < N / 2:
  idx_y = the k neighbours of every row of y (self mode); penalty = sum_i sum_{j in idx_y[i]}
  max(0, r_x(i, j) - k), an exact int64; T = 1 - 2 * penalty / (N k (2 N - 3 k - 1)) in fp64 on
  the host.  On tie-free data this is ``sklearn.manifold.trustworthiness``.
"""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .cluster import _P, _encode, _stream, contingency, features

MAX_K, MAX_F, MAX_KS = _lib.KNN_MAX_K, _lib.KNN_MAX_F, _lib.KNN_MAX_KS   # SCAE_KNN_MAX_*
_ELEMS = 1 << 22        # the host restatement's (rows, Nb) chunk (memory, not arithmetic)


class KnnResult(NamedTuple):
    idx: torch.Tensor            # (Nq, k) int64 base rows, ascending by (d2, idx)
    d2: torch.Tensor             # (Nq, k) squared distances


class RankResult(NamedTuple):
    rank: torch.Tensor           # (N, k) int32
    penalty: torch.Tensor        # (1,) int64: sum max(0, rank - k)


# -- arguments --------------------------------------------------------------------------------
def _matrix(name, x):
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError(f"{name} must be an (N, F) tensor with N, F > 0")
    if x.shape[0] >= 1 << 31:
        raise ValueError(f"{name} has {x.shape[0]} rows: at most 2^31 - 1")


def _check(x, k, base):
    """-> True on the device path"""
    _matrix("x", x)
    F = x.shape[1]
    if base is not None:
        _matrix("base", base)
        if base.shape[1] != F:
            raise ValueError(f"base must be (Nb, {F}), got {tuple(base.shape)}")
        if base.is_cuda != x.is_cuda:
            raise ValueError("x and base must both be device tensors or both CPU tensors")
    if F > MAX_F:
        raise ValueError(f"F = {F}: the search takes 1 <= F <= {MAX_F}")
    if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k > MAX_K:
        raise ValueError(f"k must be an int in 1 .. {MAX_K}, got {k!r}")
    if base is None and k > x.shape[0] - 1:
        raise ValueError(f"k = {k}, N = {x.shape[0]}: self mode needs k <= N - 1")
    if base is not None and k > base.shape[0]:
        raise ValueError(f"k = {k}, Nb = {base.shape[0]}: needs k <= Nb")
    if x.is_cuda and (x.dtype != torch.float32 or
                      (base is not None and base.dtype != torch.float32)):
        raise ValueError("x and base must be fp32")
    return x.is_cuda


def _check_ks(ks, weights):
    """-> ks as a tuple"""
    try:
        ks = tuple(ks)
    except TypeError:
        raise ValueError(f"ks must be a tuple of ints, got {ks!r}") from None
    if not 1 <= len(ks) <= MAX_KS:
        raise ValueError(f"ks must hold 1 .. {MAX_KS} list lengths, got {len(ks)}")
    if any(not isinstance(v, int) or isinstance(v, bool) or v < 1 for v in ks) or \
            any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks must be ascending positive ints, got {ks!r}")
    if weights not in ("uniform", "distance"):
        raise ValueError(f"weights must be 'uniform' or 'distance', got {weights!r}")
    return ks


def _check_labels(base_labels, Nb):
    if not isinstance(base_labels, torch.Tensor) or base_labels.dim() != 1 or \
            base_labels.shape[0] != Nb or base_labels.dtype.is_floating_point:
        raise ValueError(f"base_labels must be an integer ({Nb},) tensor")


def _check_idx(x, idx):
    _matrix("x", x)
    N, F = x.shape
    if F > MAX_F:
        raise ValueError(f"F = {F}: the search takes 1 <= F <= {MAX_F}")
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.shape[0] != N or \
            idx.dtype != torch.int64:
        raise ValueError(f"idx must be an ({N}, k) int64 tensor")
    k = idx.shape[1]
    if k < 1 or k > MAX_K or k > N - 1:
        raise ValueError(f"k = {k}, N = {N}: ranks take 1 <= k <= min({MAX_K}, N - 1)")
    if idx.is_cuda != x.is_cuda:
        raise ValueError("x and idx must both be device tensors or both CPU tensors")
    if x.is_cuda and x.dtype != torch.float32:
        raise ValueError("x must be fp32")
    return x.is_cuda


def _np(x, dtype):
    return np.ascontiguousarray(np.asarray(torch.as_tensor(x).detach().cpu()).astype(dtype))


# -- the host restatement (numpy; float32 unless dtype says otherwise) ------------------------
def _dist_rows(Q, B, lo, hi):
    """(hi - lo, Nb) squared distances of queries lo .. hi - 1 in Q's dtype, f order; each
    numpy operation rounds once, as the rules ask"""
    d = np.zeros((hi - lo, B.shape[0]), dtype=Q.dtype)
    for f in range(Q.shape[1]):
        u = Q[lo:hi, None, f] - B[None, :, f]
        d += u * u
    return d


def _chunks(Nq, Nb):
    rows = max(1, min(256, _ELEMS // Nb))
    return [(lo, min(lo + rows, Nq)) for lo in range(0, Nq, rows)]


def _least(d, k):
    """The k least entries of every row of d by (value, column) -> (columns (rows, k), values):
    everything below the row's k-th least value, then the first columns that equal it; a stable
    sort of those k (their columns ascend) orders them."""
    rows = d.shape[0]
    kth = np.partition(d, k - 1, axis=1)[:, k - 1:k]
    below, equal = d < kth, d == kth
    room = k - below.sum(1, keepdims=True)
    take = below | (equal & (np.cumsum(equal, axis=1) <= room))
    cols = np.nonzero(take)[1].reshape(rows, k)
    vals = np.take_along_axis(d, cols, 1)
    order = np.argsort(vals, axis=1, kind="stable")
    return np.take_along_axis(cols, order, 1), np.take_along_axis(vals, order, 1)


def knn_host(x, k, base=None, dtype=np.float32):
    """``knn`` in numpy (the kernels' check; CPU tensors take it): the rules' arithmetic in
    ``dtype``, rows in chunks.  -> KnnResult with CPU tensors (d2 in ``dtype``)."""
    _check(x.cpu() if isinstance(x, torch.Tensor) else x, k,
           base.cpu() if isinstance(base, torch.Tensor) else base)
    Q = _np(x, dtype)
    B = Q if base is None else _np(base, dtype)
    Nq = Q.shape[0]
    idx, d2 = np.empty((Nq, k), dtype=np.int64), np.empty((Nq, k), dtype=dtype)
    for lo, hi in _chunks(Nq, B.shape[0]):
        d = _dist_rows(Q, B, lo, hi)
        if base is None:
            d[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        idx[lo:hi], d2[lo:hi] = _least(d, k)
    return KnnResult(torch.from_numpy(idx), torch.from_numpy(d2))


def vote_host(idx, d2, base_labels, ks=(1, 5, 20), weights="uniform"):
    """The rules' vote on neighbour lists, every query at once -> pred (Nq, len(ks)) int64."""
    ks = _check_ks(ks, weights)
    idx, d2 = _np(idx, np.int64), _np(d2, np.float32)
    if idx.ndim != 2 or idx.shape != d2.shape or idx.shape[1] != ks[-1]:
        raise ValueError(f"idx and d2 must be (Nq, {ks[-1]}), the lists of k = ks[-1]")
    L = _np(base_labels, np.int64)[idx]
    Nq, k = idx.shape
    if weights == "uniform":
        w = np.ones((Nq, k), dtype=np.float32)
    else:
        with np.errstate(divide="ignore"):
            w = np.float32(1) / np.sqrt(d2)
        zeros = d2[:, :1] == 0
        w = np.where(zeros, (d2 == 0).astype(np.float32), w).astype(np.float32)
    pred = np.empty((Nq, len(ks)), dtype=np.int64)
    best_t, best_l = np.zeros(Nq, dtype=np.float32), np.zeros(Nq, dtype=np.int64)
    for m in range(k):
        tally = np.zeros(Nq, dtype=np.float32)
        for n in range(m + 1):
            tally = tally + np.where(L[:, n] == L[:, m], w[:, n], np.float32(0))
        upd = (tally > best_t) | ((tally == best_t) & (L[:, m] < best_l)) if m else \
            np.ones(Nq, dtype=bool)
        best_t, best_l = np.where(upd, tally, best_t), np.where(upd, L[:, m], best_l)
        for i, kk in enumerate(ks):
            if kk == m + 1:
                pred[:, i] = best_l
    return torch.from_numpy(pred)


def classify_host(x, base, base_labels, ks=(1, 5, 20), weights="uniform"):
    """``classify`` in numpy -> (pred (Nq, len(ks)) int64, KnnResult), CPU tensors."""
    ks = _check_ks(ks, weights)
    _check_labels(base_labels, (x if base is None else base).shape[0])
    res = knn_host(x, ks[-1], base)
    return vote_host(res.idx, res.d2, base_labels, ks, weights), res


def ranks_host(x, idx, dtype=np.float32):
    """``ranks`` in numpy -> RankResult with CPU tensors."""
    _check_idx(x.cpu(), idx.cpu())
    X, J = _np(x, dtype), _np(idx, np.int64)
    N, k = J.shape
    rank = np.empty((N, k), dtype=np.int32)
    cols = np.arange(N)[None, :]
    for lo, hi in _chunks(N, N):
        d = _dist_rows(X, X, lo, hi)
        j = J[lo:hi]
        dt = np.take_along_axis(d, j, 1)
        d[np.arange(hi - lo), np.arange(lo, hi)] = np.inf       # l != i
        for m in range(k):
            t, jm = dt[:, m:m + 1], j[:, m:m + 1]
            rank[lo:hi, m] = 1 + ((d < t) | ((d == t) & (cols < jm))).sum(1)
    penalty = np.maximum(rank.astype(np.int64) - k, 0).sum()
    return RankResult(torch.from_numpy(rank), torch.tensor([int(penalty)], dtype=torch.int64))


def _check_trust(x, y, k):
    _matrix("x", x)
    _matrix("y", y)
    if y.shape[0] != x.shape[0]:
        raise ValueError(f"y must embed the {x.shape[0]} rows of x, got {tuple(y.shape)}")
    if y.is_cuda != x.is_cuda:
        raise ValueError("x and y must both be device tensors or both CPU tensors")
    if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k > MAX_K:
        raise ValueError(f"k must be an int in 1 .. {MAX_K}, got {k!r}")
    if 2 * k >= x.shape[0]:
        raise ValueError(f"k = {k}, N = {x.shape[0]}: trustworthiness needs k < N / 2")


def _trust(penalty, N, k):
    return 1.0 - 2.0 * int(penalty) / (N * k * (2 * N - 3 * k - 1))


def trustworthiness_host(x, y, k=12):
    """``trustworthiness`` in numpy (float32 distances, the rules' order) -> float."""
    _check_trust(x, y, k)
    res = ranks_host(x, knn_host(y, k).idx)
    return _trust(res.penalty, x.shape[0], k)


# -- the device path --------------------------------------------------------------------------
def _knn_device(x, k, base):
    x = x.contiguous()
    b = x if base is None else base.contiguous()
    (Nq, F), Nb, dev = x.shape, b.shape[0], x.device
    G = _lib.load().scae_knn_groups(Nq, Nb)
    part = torch.empty(Nq * G * k, device=dev, dtype=torch.int64) if G > 1 else None
    d2 = torch.empty(Nq, k, device=dev)
    idx = torch.empty(Nq, k, device=dev, dtype=torch.int64)
    _lib.call("scae_knn_f32", _P(x), Nq, _P(b), Nb, F, k, int(base is None), _P(part), _P(d2),
              _P(idx), _stream(x))
    return KnnResult(idx, d2)


def knn(x, k, base=None):
    """The k nearest rows of ``base`` (Nb, F) for every row of ``x`` (Nq, F), or with
    ``base=None`` the k nearest other rows of ``x`` itself.  Device tensors (fp32) run on the
    kernels, CPU tensors take ``knn_host``.  -> KnnResult(idx (Nq, k) int64, d2 (Nq, k))."""
    if not _check(x, k, base):
        return knn_host(x, k, base)
    return _knn_device(x, k, base)


def vote(idx, d2, base_labels, ks=(1, 5, 20), weights="uniform"):
    """The rules' vote on the neighbour lists ``idx`` / ``d2`` (Nq, ks[-1]) of a base with labels
    ``base_labels`` -> pred (Nq, len(ks)) int64, on the lists' device."""
    ks = _check_ks(ks, weights)
    if not idx.is_cuda:
        return vote_host(idx, d2, base_labels, ks, weights)
    if idx.dim() != 2 or idx.shape != d2.shape or idx.shape[1] != ks[-1] or \
            idx.dtype != torch.int64 or d2.dtype != torch.float32:
        raise ValueError(f"idx (int64) and d2 (fp32) must be (Nq, {ks[-1]}), the lists of "
                         f"k = ks[-1]")
    idx, d2 = idx.contiguous(), d2.contiguous()
    labels = base_labels.to(idx.device, torch.int64).contiguous()
    pred = torch.empty(idx.shape[0], len(ks), device=idx.device, dtype=torch.int64)
    _lib.call("scae_knn_vote_f32", _P(idx), _P(d2), idx.shape[0], ks[-1], _P(labels),
              labels.shape[0], (ctypes.c_int * len(ks))(*ks), len(ks),
              int(weights == "distance"), _P(pred), _stream(idx))
    return pred


def classify(x, base, base_labels, ks=(1, 5, 20), weights="uniform"):
    """The k-NN classifier: the rows of ``x`` (Nq, F) labelled by their neighbours in ``base``
    (Nb, F) with labels ``base_labels`` (Nb,), for every list length in ``ks`` from one search at
    k = ks[-1].  ``base=None``: leave-one-out on ``x`` itself (self mode).  -> (pred
    (Nq, len(ks)) int64, KnnResult)."""
    ks = _check_ks(ks, weights)
    _matrix("x", x)
    if base is not None:
        _matrix("base", base)
    Nb = (x if base is None else base).shape[0]
    if ks[-1] > (Nb - 1 if base is None else Nb):
        raise ValueError(f"ks[-1] = {ks[-1]}, Nb = {Nb}: needs ks[-1] <= "
                         f"{'N - 1' if base is None else 'Nb'}")
    _check_labels(base_labels, Nb)
    if not _check(x, ks[-1], base):
        return classify_host(x, base, base_labels.cpu(), ks, weights)
    res = _knn_device(x, ks[-1], base)
    return vote(res.idx, res.d2, base_labels, ks, weights), res


def ranks(x, idx):
    """The self-mode ranks of the listed neighbours ``idx`` (N, k) int64 (rows j != i of ``x``,
    not checked) among the rows of ``x`` (N, F), and their penalty sum max(0, rank - k).
    -> RankResult(rank (N, k) int32, penalty (1,) int64)."""
    if not _check_idx(x, idx):
        return ranks_host(x, idx)
    x, idx = x.contiguous(), idx.contiguous()
    (N, F), k, dev = x.shape, idx.shape[1], x.device
    G = _lib.load().scae_knn_groups(N, N)
    rank = torch.empty(N, k, device=dev, dtype=torch.int32)
    part_count = torch.empty(N * G * k, device=dev, dtype=torch.int32)
    part = torch.empty((N + 255) // 256, device=dev, dtype=torch.int64)
    penalty = torch.empty(1, device=dev, dtype=torch.int64)
    _lib.call("scae_knn_ranks_f32", _P(x), N, F, _P(idx), k, _P(rank), _P(part_count), _P(part),
              _P(penalty), _stream(x))
    return RankResult(rank, penalty)


def trustworthiness(x, y, k=12):
    """How far the embedding ``y`` (N, E) keeps the neighbourhoods of the features ``x`` (N, F):
    1 when every one of a point's k neighbours in ``y`` is among its k neighbours in ``x``, less
    by the ranks of those that are not.  Device tensors run on the kernels (one read: the
    penalty), CPU tensors take ``trustworthiness_host``.  -> float."""
    _check_trust(x, y, k)
    if not x.is_cuda:
        return trustworthiness_host(x, y, k)
    res = ranks(x, knn(y, k).idx)
    return _trust(res.penalty, x.shape[0], k)


# -- the whole measurement ------------------------------------------------------------------------
def _accuracies(pred, labels, ks):
    labels = labels.to(pred.device)
    hits = (pred == labels[:, None]).sum(0).tolist()
    return {k: h / pred.shape[0] for k, h in zip(ks, hits)}


def knn_accuracy(step, fit_split, *others, ks=(1, 5, 20), feature="prior", weights="uniform",
                 names=None, n_classes=None):
    """The k-NN classifier on the object-capsule features of ``fit_split`` (encoded by the
    EvalStep ``step``) applied to ``others``.  Splits are (images, labels) pairs or
    data.DatasetView objects, each encoded once; ``names`` names ``others`` (default "test" for
    one, else "split1", "split2", ...).  -> {"fit_accuracy": {k: accuracy} (leave-one-out: self
    mode on the fit split), "<name>_accuracy": {k: accuracy}..., "confusion" (the first other
    split's (predicted, label) table at the largest k, None without one), "ks"}."""
    ks = _check_ks(ks, weights)
    if names is None:
        names = ["test"] if len(others) == 1 else [f"split{i + 1}" for i in range(len(others))]
    if len(names) != len(others):
        raise ValueError("one name per split")
    if n_classes is None:
        n_classes = getattr(step.model, "n_classes", None)
    encoded = []                                   # (split, features, labels): each split once

    def enc_of(split):
        for s, xs, ys in encoded:
            if s is split:
                return xs, ys
        e = _encode(step, split)
        encoded.append((split, features(e, feature), e["label"]))
        return encoded[-1][1:]

    xf, yf = enc_of(fit_split)
    if n_classes is None:
        n_classes = int(yf.max()) + 1
    pred, _ = classify(xf, None, yf, ks, weights)
    out = {"fit_accuracy": _accuracies(pred, yf, ks)}
    confusion = None
    for i, (name, split) in enumerate(zip(names, others)):
        xo, yo = enc_of(split)
        pred, _ = classify(xo, xf, yf, ks, weights)
        out[f"{name}_accuracy"] = _accuracies(pred, yo, ks)
        if i == 0:
            confusion = contingency(pred[:, -1].contiguous(), yo.to(pred.device), n_classes,
                                    n_classes)
    out.update(confusion=confusion, ks=ks)
    return out
