"""How good a clustering is, with and without labels: the exact silhouette, the Calinski-Harabasz
and Davies-Bouldin indices, the label-based indices (ARI, NMI, homogeneity / completeness /
V-measure, purity) and a choice of k for ``cluster.kmeans`` from them.

``silhouette`` / ``dispersion`` run on the library's kernels (csrc/cluster_quality.hip) for device
tensors; ``silhouette_host`` / ``dispersion_host`` are the same rules in numpy, used for CPU
tensors and to check the kernels.  The label-based indices are functions of the integer
contingency table (``cluster.contingency``) alone and are computed on the host in fp64.

Rules, for x (N, F) fp32 with 1 <= F <= 256 and labels (N,) integers in [0, k).  Clusters may be
empty and are then ignored; a label outside [0, k) raises ValueError (counted on the device, as
``cluster.contingency`` counts them).  n_c is the size of cluster c, c(i) the cluster of row i.

- distance: d_ij = sqrt(sum_f (x_if - x_jf)^2) in fp32.  The squared distance follows
  ``neighbors``' rule exactly (f order from 0; the difference, the product and the sum each
  rounded to fp32, no fused multiply-add); the root is the correctly rounded fp32 one; d_ij is
  widened to fp64 before any sum;
- D_i(c) = the fp64 sum of d_ij over the rows j != i of cluster c in ascending j, whatever the
  launch geometry (the kernel never splits the base).  The self pair is skipped by row index, not
  by d = 0: duplicated rows are legitimate zero distances;
- a_i = D_i(c(i)) / (n_c(i) - 1); b_i = min over non-empty c != c(i) of D_i(c) / n_c; nearest_i is
  the c that attains the minimum, ties to the lowest c; s_i = (b_i - a_i) / max(a_i, b_i);
- s_i = 0 when n_c(i) = 1, when there is no other non-empty cluster, or when max(a_i, b_i) = 0.
  A singleton has a_i = 0 (its b_i and nearest_i are the rule's); with no other non-empty cluster
  b_i = +inf and nearest_i = -1 (a_i is the rule's);
- ``score`` = the fp64 sum of s_i in row order (from 0, one value after the other) over N;
  ``cluster_score[c]`` the same over cluster c's rows, NaN for an empty cluster.  Both are summed
  on the device and come back as host numbers in one small read (with the count of labels
  outside the range);
- dispersion, from centroids, fp64 sums over each cluster's rows in a fixed order: n_c, the mean
  m_c, W_c = sum |x_i - m_c|^2 and S_c = (1 / n_c) sum |x_i - m_c|.  An empty cluster has
  n_c = 0, W_c = 0 and NaN for m_c and S_c.  The host finishes in fp64 numpy from these (k, .)
  tables, with k' the number of non-empty clusters and m = sum n_c m_c / N:
  Calinski-Harabasz = [sum n_c |m_c - m|^2 / (k' - 1)] / [sum W_c / (N - k')], 1.0 when
  sum W_c = 0, NaN for k' < 2;
  Davies-Bouldin = the mean over non-empty c of max over c' != c of (S_c + S_c') / |m_c - m_c'|,
  scikit-learn's conventions: a zero centroid distance counts as +inf, the result is 0 when
  every S_c or every centroid distance is 0; NaN for k' < 2;
- label-based indices of a (clusters, classes) contingency table n with N = sum n, in fp64 with
  natural logarithms: ARI = (sum C(n_ij, 2) - E) / ((A + B) / 2 - E) with A, B the row / column
  sums' pairs and E = A B / C(N, 2), 1.0 when the denominator is 0; MI = sum n_ij / N
  log(N n_ij / (a_i b_j)); NMI = MI / ((H(clusters) + H(classes)) / 2), 1.0 when both entropies
  are 0; homogeneity = MI / H(classes), completeness = MI / H(clusters) (1.0 where the entropy is
  0), V-measure their harmonic mean; purity = sum_c max_j n_cj / N.  AMI is left out.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import cluster as _cluster
from .cluster import _P, _check_x, _stream, contingency

MAX_F = _lib.CLUSTER_QUALITY_MAX_F      # SCAE_CLUSTER_QUALITY_MAX_F
_ELEMS = 1 << 22        # the host restatement's (rows, N) chunk (memory, not arithmetic)
_CRITERIA = {"silhouette": 1.0, "calinski_harabasz": 1.0, "davies_bouldin": -1.0}


class SilhouetteResult(NamedTuple):
    values: torch.Tensor         # (N,) fp64 s_i
    a: torch.Tensor              # (N,) fp64 mean distance to the own cluster's other rows
    b: torch.Tensor              # (N,) fp64 least mean distance to another cluster (+inf: none)
    nearest: torch.Tensor        # (N,) int64 the cluster that attains b (-1: none)
    score: float                 # the mean of values
    cluster_score: np.ndarray    # (k,) fp64 the mean of each cluster's values (NaN: empty)


class DispersionResult(NamedTuple):
    count: torch.Tensor          # (k,) int64 n_c
    centroid: torch.Tensor       # (k, F) fp64 m_c (NaN: empty)
    within: torch.Tensor         # (k,) fp64 W_c
    mean_distance: torch.Tensor  # (k,) fp64 S_c (NaN: empty)
    calinski_harabasz: float
    davies_bouldin: float


class SelectKResult(NamedTuple):
    table: dict                  # column -> list, one entry per k in ks: k, inertia,
    #                              silhouette, calinski_harabasz, davies_bouldin, n_iter
    k: int                       # the chosen k
    result: _cluster.KMeansResult   # its fit


# -- arguments --------------------------------------------------------------------------------
def _check(x, labels, k):
    """-> (True on the device path, k)"""
    _check_x(x)
    N, F = x.shape
    if F > MAX_F:
        raise ValueError(f"F = {F}: cluster quality takes 1 <= F <= {MAX_F}")
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.shape[0] != N or \
            labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"labels must be an integer ({N},) tensor")
    if labels.is_cuda != x.is_cuda:
        raise ValueError("x and labels must both be device tensors or both CPU tensors")
    if k is None:
        k = int(labels.max()) + 1        # (a read; pass k to avoid it)
        if k < 1:
            raise ValueError(f"{N} labels outside [0, k): none is non-negative")
    if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k >= (1 << 31) - 1:
        raise ValueError(f"k must be an int in 1 .. 2^31 - 2 or None, got {k!r}")
    if x.is_cuda and x.dtype != torch.float32:
        raise ValueError("x must be fp32")
    return x.is_cuda, k


def _np(x, dtype):
    return np.ascontiguousarray(np.asarray(torch.as_tensor(x).detach().cpu()).astype(dtype))


def _host_labels(labels, k):
    L = _np(labels, np.int64)
    outside = int(((L < 0) | (L >= k)).sum())
    if outside:
        raise ValueError(f"{outside} labels outside [0, {k})")
    return L


def _sequential_sum(v, axis=-1):
    """The sum of v along ``axis`` from 0, one value after the other (numpy's own sum is
    pairwise); 0 for no values."""
    v = np.asarray(v, dtype=np.float64)
    if v.shape[axis] == 0:
        return np.zeros(np.delete(v.shape, axis))
    return np.take(np.cumsum(v, axis=axis), -1, axis=axis)


# -- the host restatement (numpy) -------------------------------------------------------------
def _dist_rows(X, lo, hi):
    """(hi - lo, N) distances of rows lo .. hi - 1 in X's dtype: f order, each numpy operation
    rounds once, as the rules ask"""
    d = np.zeros((hi - lo, X.shape[0]), dtype=X.dtype)
    for f in range(X.shape[1]):
        u = X[lo:hi, None, f] - X[None, :, f]
        d += u * u
    return np.sqrt(d)


def _scores(s, L, k):
    members = [np.nonzero(L == c)[0] for c in range(k)]
    cs = np.array([_sequential_sum(s[m]) / len(m) if len(m) else np.nan for m in members])
    return float(_sequential_sum(s) / len(s)), cs


def silhouette_host(x, labels, k=None, dtype=np.float32):
    """``silhouette`` in numpy (the kernels' check; CPU tensors take it), rows in chunks.
    ``dtype=np.float32``: the device's distance arithmetic; ``np.float64``: exact fp64 distances.
    -> SilhouetteResult with CPU tensors."""
    _, k = _check(x.cpu() if isinstance(x, torch.Tensor) else x,
                  labels.cpu() if isinstance(labels, torch.Tensor) else labels, k)
    X, L = _np(x, dtype), _host_labels(labels, k)
    N = X.shape[0]
    members = [(c, np.nonzero(L == c)[0]) for c in range(k)]
    members = [(c, m) for c, m in members if len(m)]
    ids = np.array([c for c, _ in members])
    sizes = np.array([len(m) for _, m in members], dtype=np.float64)
    own = np.searchsorted(ids, L)                      # the row's cluster among the non-empty
    a, b = np.zeros(N), np.full(N, np.inf)
    nearest = np.full(N, -1, dtype=np.int64)
    rows = max(1, min(256, _ELEMS // N))
    for lo in range(0, N, rows):
        hi = min(lo + rows, N)
        d = _dist_rows(X, lo, hi).astype(np.float64)
        d[np.arange(hi - lo), np.arange(lo, hi)] = 0.0       # j != i: +0 leaves a sum as it is
        D = np.stack([_sequential_sum(d[:, m]) for _, m in members], axis=1)
        r, o = np.arange(hi - lo), own[lo:hi]
        n_own = sizes[o]
        a[lo:hi] = np.where(n_own > 1, D[r, o] / np.maximum(n_own - 1, 1), 0.0)
        if len(members) > 1:
            mean = D / sizes[None, :]
            mean[r, o] = np.inf
            best = np.argmin(mean, axis=1)                   # (the first of equal minima)
            b[lo:hi], nearest[lo:hi] = mean[r, best], ids[best]
    mx = np.maximum(a, b)
    ok = (sizes[own] > 1) & (nearest >= 0) & (mx > 0)
    s = np.zeros(N)
    s[ok] = (b[ok] - a[ok]) / mx[ok]
    score, cs = _scores(s, L, k)
    return SilhouetteResult(torch.from_numpy(s), torch.from_numpy(a), torch.from_numpy(b),
                            torch.from_numpy(nearest), score, cs)


def _indices_from_tables(count, centroid, within, mean_distance):
    """Calinski-Harabasz and Davies-Bouldin from the (k, .) tables, fp64 numpy."""
    n = np.asarray(count, dtype=np.float64)
    live = n > 0
    kk, N = int(live.sum()), n.sum()
    if kk < 2:
        return float("nan"), float("nan")
    n, m = n[live], np.asarray(centroid, dtype=np.float64)[live]
    W, S = np.asarray(within, dtype=np.float64)[live], \
        np.asarray(mean_distance, dtype=np.float64)[live]
    centre = (n[:, None] * m).sum(0) / N
    between, inside = float((n * ((m - centre) ** 2).sum(1)).sum()), float(W.sum())
    ch = 1.0 if inside == 0.0 else (between / (kk - 1)) / (inside / (N - kk))
    gap = np.sqrt(((m[:, None, :] - m[None, :, :]) ** 2).sum(-1))
    if not S.any() or not gap.any():
        return float(ch), 0.0
    gap[gap == 0.0] = np.inf
    db = float(np.mean(np.max((S[:, None] + S[None, :]) / gap, axis=1)))
    return float(ch), db


def dispersion_host(x, labels, k=None):
    """``dispersion`` in fp64 numpy -> DispersionResult with CPU tensors."""
    _, k = _check(x.cpu() if isinstance(x, torch.Tensor) else x,
                  labels.cpu() if isinstance(labels, torch.Tensor) else labels, k)
    X, L = _np(x, np.float64), _host_labels(labels, k)
    F = X.shape[1]
    count = np.bincount(L, minlength=k).astype(np.int64)
    centroid = np.full((k, F), np.nan)
    within, mean_distance = np.zeros(k), np.full(k, np.nan)
    for c in np.nonzero(count)[0]:
        rows = X[L == c]
        centroid[c] = rows.sum(0) / count[c]
        d2 = ((rows - centroid[c]) ** 2).sum(1)
        within[c], mean_distance[c] = d2.sum(), np.sqrt(d2).sum() / count[c]
    ch, db = _indices_from_tables(count, centroid, within, mean_distance)
    return DispersionResult(torch.from_numpy(count), torch.from_numpy(centroid),
                            torch.from_numpy(within), torch.from_numpy(mean_distance), ch, db)


# -- the device path --------------------------------------------------------------------------
class _Sorted(NamedTuple):
    xs: torch.Tensor             # (N, F) the rows sorted by (label, row)
    ls: torch.Tensor             # (N,) int32 their clusters
    order: torch.Tensor          # (N,) int64 their original rows
    off: torch.Tensor            # (k + 1,) int64 the clusters' first positions
    outside: torch.Tensor        # (1,) int32 labels outside [0, k) (clamped into it in ls)


def _sort(x, labels, k):
    """The rows by (label, row): a stable integer sort and the clusters' offsets, on the device
    with no read.  Labels outside [0, k) are clamped (the kernels stay in bounds) and counted;
    the caller raises once it has read the count."""
    x = x.contiguous()
    N, dev = x.shape[0], x.device
    labels = labels.to(torch.int64).contiguous()
    lab32 = torch.empty(N, device=dev, dtype=torch.int32)
    outside = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("scae_cluster_quality_labels", _P(labels), N, k, _P(lab32), _P(outside),
              _stream(x))
    ls, order = torch.sort(lab32, stable=True)
    off = torch.searchsorted(ls, torch.arange(k + 1, device=dev, dtype=torch.int32)).contiguous()
    return _Sorted(x.index_select(0, order), ls.contiguous(), order.contiguous(), off, outside)


def _raise_outside(outside, k):
    if outside:
        raise ValueError(f"{int(outside)} labels outside [0, {k})")


def _silhouette_device(x, k, srt):
    (N, F), dev = x.shape, x.device
    out = torch.empty(4, N, device=dev, dtype=torch.float64)     # values, a, b, sorted values
    nearest = torch.empty(N, device=dev, dtype=torch.int64)
    tail = torch.empty(k + 2, device=dev, dtype=torch.float64)   # scores, then the outside count
    _lib.call("scae_cluster_quality_silhouette_f32", _P(srt.xs), _P(srt.ls), _P(srt.off),
              _P(srt.order), N, F, k, _P(out[0]), _P(out[1]), _P(out[2]), _P(nearest),
              _P(out[3]), _P(tail), _stream(x))
    tail[k + 1] = srt.outside[0]
    host = tail.cpu().numpy()                                    # the one read
    _raise_outside(int(host[k + 1]), k)
    return SilhouetteResult(out[0], out[1], out[2], nearest, float(host[k]), host[:k].copy())


def _dispersion_device(x, k, srt):
    (N, F), dev = x.shape, x.device
    table = torch.empty(k + 1, F + 3, device=dev, dtype=torch.float64)
    _lib.call("scae_cluster_quality_dispersion_f32", _P(srt.xs), _P(srt.off), N, F, k, _P(table),
              _stream(x))
    table[k] = srt.outside[0].double()
    host = table.cpu().numpy()                                   # the one read
    _raise_outside(int(host[k, 0]), k)
    ch, db = _indices_from_tables(host[:k, 0], host[:k, 1:F + 1], host[:k, F + 1], host[:k, F + 2])
    return DispersionResult(table[:k, 0].to(torch.int64), table[:k, 1:F + 1], table[:k, F + 1],
                            table[:k, F + 2], ch, db)


def silhouette(x, labels, k=None):
    """The silhouette of every row of ``x`` (N, F) under the clustering ``labels`` (N,) integers
    in [0, k) (``k=None``: the largest label + 1, which costs a read) -- exact, over every pair.
    Device tensors (fp32) run on the kernels, CPU tensors take ``silhouette_host``.
    -> SilhouetteResult(values, a, b (N,) fp64, nearest (N,) int64, score, cluster_score)."""
    device, k = _check(x, labels, k)
    if not device:
        return silhouette_host(x, labels, k)
    return _silhouette_device(x, k, _sort(x, labels, k))


def dispersion(x, labels, k=None):
    """The clusters' sizes, centroids and scatter, and the Calinski-Harabasz (higher is better)
    and Davies-Bouldin (lower is better) indices from them.  Device tensors (fp32) run on the
    kernels, CPU tensors take ``dispersion_host``.  -> DispersionResult(count (k,) int64,
    centroid (k, F), within (k,), mean_distance (k,) fp64, calinski_harabasz, davies_bouldin)."""
    device, k = _check(x, labels, k)
    if not device:
        return dispersion_host(x, labels, k)
    return _dispersion_device(x, k, _sort(x, labels, k))


def quality(x, labels, k=None):
    """``silhouette`` and ``dispersion`` of one labelling, from one sort of the rows
    -> (SilhouetteResult, DispersionResult)."""
    device, k = _check(x, labels, k)
    if not device:
        return silhouette_host(x, labels, k), dispersion_host(x, labels, k)
    srt = _sort(x, labels, k)
    return _silhouette_device(x, k, srt), _dispersion_device(x, k, srt)


# -- label-based indices ------------------------------------------------------------------------
def _entropy(counts, N):
    p = counts[counts > 0] / N
    return float(-(p * np.log(p)).sum())


def label_indices(table):
    """ARI, NMI (arithmetic-mean normaliser), homogeneity, completeness, V-measure and purity of
    a (clusters, classes) contingency table of integer counts, in fp64 with natural logarithms
    -> dict.  Empty rows and columns change nothing."""
    t = np.asarray(table)
    if t.ndim != 2 or t.size == 0 or (t < 0).any() or t.sum() <= 0 or \
            not np.issubdtype(t.dtype, np.integer):
        raise ValueError("table must be a (clusters, classes) array of non-negative integer "
                         "counts with a positive sum")
    t = t.astype(np.float64)
    N = t.sum()
    rows, cols = t.sum(1), t.sum(0)

    def pairs(v):
        return float((v * (v - 1.0) / 2.0).sum())

    same, in_rows, in_cols = pairs(t), pairs(rows), pairs(cols)
    total = N * (N - 1.0) / 2.0
    expected = in_rows * in_cols / total if total else 0.0
    spread = (in_rows + in_cols) / 2.0 - expected
    ari = 1.0 if spread == 0.0 else (same - expected) / spread
    h_rows, h_cols = _entropy(rows, N), _entropy(cols, N)
    i, j = np.nonzero(t)
    nij = t[i, j]
    mi = max(float((nij / N * (np.log(nij) + np.log(N) - np.log(rows[i]) - np.log(cols[j])))
                   .sum()), 0.0)
    norm = (h_rows + h_cols) / 2.0
    nmi = 1.0 if h_rows == 0.0 and h_cols == 0.0 else (0.0 if norm == 0.0 else mi / norm)
    hom = 1.0 if h_cols == 0.0 else mi / h_cols
    com = 1.0 if h_rows == 0.0 else mi / h_rows
    v = 0.0 if hom + com == 0.0 else 2.0 * hom * com / (hom + com)
    return {"ari": float(ari), "nmi": float(nmi), "homogeneity": float(hom),
            "completeness": float(com), "v_measure": float(v),
            "purity": float(t.max(1).sum() / N)}


def label_indices_of(cluster_ids, labels, k, n_classes):
    """``label_indices`` of the contingency table of ``cluster_ids`` and ``labels`` (N,), counted
    on the device for device tensors (``cluster.contingency``)."""
    return label_indices(contingency(cluster_ids, labels, k, n_classes))


# -- the choice of k ----------------------------------------------------------------------------
def select_k(x, ks, criterion="silhouette", **kmeans_args):
    """``cluster.kmeans`` (with ``kmeans_args``) for every k in ``ks``, each fit's silhouette and
    dispersion indices, and the k that is best under ``criterion``: the greatest "silhouette" or
    "calinski_harabasz" or the least "davies_bouldin", ties to the smallest k (a NaN never wins).
    -> SelectKResult(table {"k", "inertia", "silhouette", "calinski_harabasz", "davies_bouldin",
    "n_iter"} of lists, k, its KMeansResult)."""
    if criterion not in _CRITERIA:
        raise ValueError(f"criterion must be one of {sorted(_CRITERIA)}, got {criterion!r}")
    try:
        ks = tuple(ks)
    except TypeError:
        raise ValueError(f"ks must be a sequence of ints, got {ks!r}") from None
    if not ks or any(not isinstance(v, int) or isinstance(v, bool) or v < 2 for v in ks) or \
            len(set(ks)) != len(ks):
        raise ValueError(f"ks must be distinct ints >= 2, got {ks!r}")
    _check_x(x)
    if max(ks) > x.shape[0]:
        raise ValueError(f"k = {max(ks)}, N = {x.shape[0]}: needs k <= N")
    table = {c: [] for c in ("k", "inertia", "silhouette", "calinski_harabasz", "davies_bouldin",
                             "n_iter")}
    fits = {}
    for k in ks:
        res = _cluster.kmeans(x, k, **kmeans_args)
        sil, disp = quality(x, res.labels.to(x.device), k)
        fits[k] = res
        for c, v in zip(table, (k, res.inertia, sil.score, disp.calinski_harabasz,
                                disp.davies_bouldin, res.n_iter)):
            table[c].append(v)
    sign = _CRITERIA[criterion]
    best = None
    for k, v in zip(table["k"], table[criterion]):
        if v == v and (best is None or (sign * v, -k) > (sign * best[1], -best[0])):
            best = (k, v)
    if best is None:
        raise ValueError(f"{criterion} is NaN for every k in {ks!r}")
    return SelectKResult(table, best[0], fits[best[0]])
