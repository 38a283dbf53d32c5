"""Unsupervised classification from SCAE's object-capsule activations: k-means on each
image's capsule features, then clusters matched to classes -- the evaluation the SCAE paper
reports next to its supervised heads.

``kmeans`` / ``assign`` / the contingency table of ``match_clusters`` run on the library's
kernels (csrc/kmeans.hip) for device tensors; ``kmeans_host`` is the same algorithm in fp64
numpy, used for CPU tensors and to check the kernels.  Both follow one set of rules:

- distance: sum_f (x_f - c_f)^2 in f order; a tie goes to the lowest cluster index;
- update: the mean of the assigned points; an empty cluster keeps its centroid;
- a restart stops when no assignment changed (no float tolerance) or after ``max_iter``
  assignments, and the update of that last assignment is skipped: centroids, labels and
  inertia (an fp64 sum) belong to one assignment;
- k-means++: D^2 sampling, centre j of restart r drawn with the uniform of Philox4x32-10
  keyed (seed, r) at counter (j, 0, 0, 0x4B4D5050) (``pp_uniform``; the device generator's
  rounds, noise_dev.h), the first point whose running D^2 sum exceeds u * total (centre 0:
  every weight 1);
- the result is the restart of least inertia, ties to the lowest restart index.
"""
import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .data import _M32, _philox
from .ops import _p as _P, _stream   # (probe.py takes them from here too)

MAX_K, MAX_F, MAX_KF = 256, 256, 16384   # SCAE_KMEANS_MAX_K / _F / _KF
_TAG_KMPP = 0x4B4D5050


class KMeansResult(NamedTuple):
    centroids: torch.Tensor      # (k, F)
    labels: torch.Tensor         # (N,) int64
    inertia: float               # fp64 sum of the points' squared distances
    n_iter: int                  # assignments of the chosen restart
    converged: bool              # its last assignment changed nothing
    restart: int                 # the chosen restart
    init_index: Optional[torch.Tensor] = None  # (n_init, k) k-means++ rows (None: given init)


# -- arguments --------------------------------------------------------------------------------
def _check_x(x):
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError("x must be an (N, F) tensor with N, F > 0")
    if x.shape[0] >= 1 << 31:
        raise ValueError(f"N = {x.shape[0]} points: at most 2^31 - 1")


def _check_kf(k, F):
    if not isinstance(k, int) or isinstance(k, bool) or k <= 0:
        raise ValueError(f"k must be a positive int, got {k!r}")
    if k > MAX_K or F > MAX_F or k * F > MAX_KF:
        raise ValueError(f"k = {k}, F = {F}: the kernels take k <= {MAX_K}, F <= {MAX_F}, "
                         f"k * F <= {MAX_KF}")


def _args(x, k, n_init, max_iter, init):
    """-> (restarts, init tensor (R, k, F) or None for k-means++)"""
    _check_x(x)
    F = x.shape[1]
    _check_kf(k, F)
    if not isinstance(max_iter, int) or max_iter <= 0:
        raise ValueError(f"max_iter must be a positive int, got {max_iter!r}")
    if isinstance(init, str):
        if init != "k-means++":
            raise ValueError(f"init must be 'k-means++' or a tensor, got {init!r}")
        if not isinstance(n_init, int) or n_init <= 0:
            raise ValueError(f"n_init must be a positive int, got {n_init!r}")
        return n_init, None
    init = torch.as_tensor(init)
    if init.dim() == 2 and tuple(init.shape) == (k, F):
        init = init[None]
    if init.dim() != 3 or tuple(init.shape[1:]) != (k, F):
        raise ValueError(f"init must be (k, F) = ({k}, {F}) or (n_init, {k}, {F}), got "
                         f"{tuple(init.shape)}")
    return init.shape[0], init


def pp_uniform(seed, restart, j):
    """The k-means++ uniform of centre ``j`` of ``restart`` (a float32 value in [0, 1))."""
    c = _philox([j & _M32, 0, 0, _TAG_KMPP], seed & _M32, restart & _M32, 10)
    return np.float32((c[0] >> 8) * (1.0 / 16777216.0))


# -- the host restatement (fp64 numpy) ----------------------------------------------------------
def _dist_host(X, C):
    d = np.zeros((X.shape[0], C.shape[0]))
    for f in range(X.shape[1]):
        d += (X[:, None, f] - C[None, :, f]) ** 2
    return d


def kmeans_pp_host(x, k, n_init=1, seed=0):
    """k-means++ of ``n_init`` restarts in fp64 -> (centroids (n_init, k, F) fp64, chosen rows
    (n_init, k) int64, margin (n_init, k)): each draw's distance from u * total to the nearest
    running-sum boundary, over the total (a draw closer than float rounding can reach may
    pick a neighbour on the device)."""
    X = np.asarray(torch.as_tensor(x).detach().cpu(), dtype=np.float64)
    N, F = X.shape
    cent = np.zeros((n_init, k, F))
    chosen = np.zeros((n_init, k), dtype=np.int64)
    margin = np.zeros((n_init, k))
    for r in range(n_init):
        w = np.ones(N)
        for j in range(k):
            cs = np.cumsum(w)
            total = cs[-1]
            target = float(pp_uniform(seed, r, j)) * total
            idx = int(np.searchsorted(cs, target, side="right"))
            if idx >= N:
                pos = np.nonzero(w > 0)[0]
                idx = int(pos[-1]) if pos.size else N - 1
            lo = cs[idx - 1] if idx > 0 else 0.0
            margin[r, j] = min(cs[idx] - target, target - lo) / total if total > 0 else 0.0
            chosen[r, j] = idx
            cent[r, j] = X[idx]
            d = _dist_host(X, X[idx:idx + 1])[:, 0]
            w = d if j == 0 else np.minimum(w, d)
    return cent, chosen, margin


def _lloyd_host(X, C, max_iter):
    C = C.copy()
    prev = np.full(X.shape[0], -1)
    it = 0
    while True:
        d = _dist_host(X, C)
        lab = np.argmin(d, 1)
        inertia = float(d[np.arange(X.shape[0]), lab].sum())
        it += 1
        changed = int((lab != prev).sum())
        if changed == 0 or it >= max_iter:
            return C, lab, inertia, it, changed == 0
        for c in range(C.shape[0]):
            m = lab == c
            if m.any():
                C[c] = X[m].mean(0)
        prev = lab


def kmeans_host(x, k, n_init=10, max_iter=300, seed=0, init="k-means++", check_every=8):
    """``kmeans`` in fp64 numpy (the kernels' check; CPU tensors take it).  -> KMeansResult with
    fp64 CPU centroids."""
    R, init_t = _args(x, k, n_init, max_iter, init)
    X = np.asarray(x.detach().cpu(), dtype=np.float64)
    chosen = None
    if init_t is None:
        inits, chosen, _ = kmeans_pp_host(X, k, R, seed)
    else:
        inits = np.asarray(init_t.detach().cpu(), dtype=np.float64)
    best = None
    for r in range(R):
        out = _lloyd_host(X, inits[r], max_iter)
        if best is None or out[2] < best[1][2]:
            best = (r, out)
    r, (C, lab, inertia, it, conv) = best
    return KMeansResult(torch.from_numpy(C), torch.from_numpy(lab.astype(np.int64)),
                        float(inertia), int(it), bool(conv), int(r),
                        None if chosen is None else torch.from_numpy(chosen))


# -- the device path ------------------------------------------------------------------------------
def kmeans(x, k, n_init=10, max_iter=300, seed=0, init="k-means++", check_every=8):
    """Lloyd's k-means of ``n_init`` restarts of the rows of ``x`` (N, F) fp32.  ``init``:
    "k-means++" (seeded by ``seed``) or a (k, F) / (n_init, k, F) tensor (its first dimension
    sets the restarts).  On the device all restarts run in one grid, ``check_every``
    iterations enqueued at a time with one read of the stopped-restart count per chunk.
    -> KMeansResult of the restart with the least inertia."""
    R, init_t = _args(x, k, n_init, max_iter, init)
    if not x.is_cuda:
        return kmeans_host(x, k, n_init, max_iter, seed, init)
    if x.dtype != torch.float32:
        raise ValueError("x must be fp32")
    if not isinstance(check_every, int) or check_every <= 0:
        raise ValueError(f"check_every must be a positive int, got {check_every!r}")
    x = x.contiguous()
    N, F = x.shape
    dev = x.device
    lib = _lib.load()
    cent = torch.empty(R, k, F, device=dev)
    chosen = None
    if init_t is None:
        d2 = torch.empty(R, N, device=dev)
        chosen = torch.empty(R, k, device=dev, dtype=torch.int64)
        _lib.call("scae_kmeans_pp_f32", _P(x), N, F, k, R, int(seed) & _M32, _P(cent), _P(d2),
                  _P(chosen), _stream(x))
    else:
        cent.copy_(init_t.to(dev, torch.float32))
    G = lib.scae_kmeans_groups(N, R)
    labels = torch.full((R, N), -1, device=dev, dtype=torch.int64)
    part_sum = torch.empty(R * G * k * F, device=dev)
    part_count = torch.empty(R * G * k, device=dev, dtype=torch.int32)
    part_changed = torch.empty(R * G, device=dev, dtype=torch.int32)
    part_inertia = torch.empty(R * G, device=dev, dtype=torch.float64)
    state = torch.zeros(R * _lib.KMEANS_STATE_INTS + 1, device=dev, dtype=torch.int32)
    inertia = torch.zeros(R, device=dev, dtype=torch.float64)
    d = _lib.KmeansDesc()
    d.x, d.N, d.F, d.k, d.R, d.G, d.max_iter = x.data_ptr(), N, F, k, R, G, max_iter
    d.centroids, d.labels = cent.data_ptr(), labels.data_ptr()
    d.part_sum, d.part_count = part_sum.data_ptr(), part_count.data_ptr()
    d.part_changed, d.part_inertia = part_changed.data_ptr(), part_inertia.data_ptr()
    d.state, d.inertia = state.data_ptr(), inertia.data_ptr()
    enqueued = 0
    while enqueued < max_iter:
        n = min(check_every, max_iter - enqueued)
        _lib.call("scae_kmeans_lloyd_f32", ctypes.byref(d), n, _stream(x))
        enqueued += n
        if int(state[-1]) >= R:        # every restart has stopped
            break
    st = state[:-1].view(R, _lib.KMEANS_STATE_INTS).cpu()
    inn = inertia.cpu().numpy()
    best = int(np.argmin(inn))
    return KMeansResult(cent[best].clone(), labels[best].clone(), float(inn[best]),
                        int(st[best, 1]), bool(st[best, 2]), best,
                        None if chosen is None else chosen.cpu())


def assign(x, centroids):
    """Nearest-centroid labels (N,) int64 of the rows of ``x`` (N, F) under ``centroids``
    (k, F) -- e.g. a test split under the centroids fitted on the training split."""
    _check_x(x)
    if centroids.dim() != 2 or centroids.shape[1] != x.shape[1]:
        raise ValueError(f"centroids must be (k, {x.shape[1]}), got {tuple(centroids.shape)}")
    k, F = centroids.shape
    _check_kf(k, F)
    if not x.is_cuda:
        d = _dist_host(np.asarray(x.detach().cpu(), dtype=np.float64),
                       np.asarray(centroids.detach().cpu(), dtype=np.float64))
        return torch.from_numpy(np.argmin(d, 1).astype(np.int64))
    x = x.contiguous()
    c = centroids.to(x.device, torch.float32).contiguous()
    labels = torch.empty(x.shape[0], device=x.device, dtype=torch.int64)
    _lib.call("scae_kmeans_assign_f32", _P(x), x.shape[0], F, k, _P(c), _P(labels), _stream(x))
    return labels


# -- clusters to classes ---------------------------------------------------------------------------
def contingency(cluster_ids, labels, k, n_classes):
    """(k, n_classes) int64 numpy table of (cluster, class) counts; on the device with integer
    counts, read in one transfer."""
    if cluster_ids.shape != labels.shape or cluster_ids.dim() != 1:
        raise ValueError("cluster_ids and labels must be (N,) tensors of one shape")
    if k <= 0 or n_classes <= 0:
        raise ValueError("k and n_classes must be positive")
    N = cluster_ids.shape[0]
    if N == 0:
        return np.zeros((k, n_classes), dtype=np.int64)
    if cluster_ids.is_cuda:
        cid = cluster_ids.to(torch.int64).contiguous()
        lab = labels.to(cid.device, torch.int64).contiguous()
        buf = torch.zeros(k * n_classes + 1, device=cid.device, dtype=torch.int32)
        _lib.call("scae_kmeans_contingency", _P(cid), _P(lab), N, k, n_classes, _P(buf),
                  ctypes.c_void_p(buf.data_ptr() + 4 * k * n_classes), _stream(cid))
        host = buf.cpu().numpy().astype(np.int64)
        table, outside = host[:-1].reshape(k, n_classes), int(host[-1])
    else:
        c = np.asarray(cluster_ids, dtype=np.int64)
        lab = np.asarray(labels.cpu(), dtype=np.int64)
        ok = (c >= 0) & (c < k) & (lab >= 0) & (lab < n_classes)
        table = np.zeros((k, n_classes), dtype=np.int64)
        np.add.at(table, (c[ok], lab[ok]), 1)
        outside = int((~ok).sum())
    if outside:
        raise ValueError(f"{outside} (cluster, label) pairs outside [0, {k}) x "
                         f"[0, {n_classes})")
    return table


def hungarian(cost):
    """Rows-to-columns assignment of least total cost for an (n, m) matrix with n <= m (the
    shortest-augmenting-path method with potentials, O(n^2 m)).  -> (n,) column per row."""
    cost = np.asarray(cost, dtype=np.float64)
    n, m = cost.shape
    if n > m:
        raise ValueError("hungarian takes n <= m rows")
    u, v = np.zeros(n + 1), np.zeros(m + 1)
    p = np.zeros(m + 1, dtype=np.int64)      # p[j]: the row matched to column j (1-based)
    way = np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv = np.full(m + 1, np.inf)
        used = np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used[1:]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    out = np.full(n, -1, dtype=np.int64)
    for j in range(1, m + 1):
        if p[j]:
            out[p[j] - 1] = j - 1
    return out


def mapping_from_table(table):
    """Cluster -> class of a (k, n_classes) contingency table: k <= n_classes one-to-one,
    maximising the correct count (Hungarian); k > n_classes each cluster's majority class
    (ties to the lowest class)."""
    table = np.asarray(table)
    k, n = table.shape
    if k <= n:
        return hungarian(-table.astype(np.float64))
    return np.argmax(table, 1).astype(np.int64)


def match_clusters(cluster_ids, labels, k, n_classes):
    """-> (mapping (k,) int64 numpy, accuracy): clusters matched to classes from the
    contingency table of ``cluster_ids`` and ``labels`` (``mapping_from_table``), and the
    fraction of images whose cluster maps to their class."""
    table = contingency(cluster_ids, labels, k, n_classes)
    mapping = mapping_from_table(table)
    N = int(table.sum())
    return mapping, float(table[np.arange(k), mapping].sum()) / N if N else float("nan")


def mapped_accuracy(cluster_ids, labels, mapping, n_classes):
    """Accuracy of a fixed cluster -> class ``mapping`` (e.g. the training split's)."""
    mapping = np.asarray(mapping)
    table = contingency(cluster_ids, labels, len(mapping), n_classes)
    N = int(table.sum())
    return float(table[np.arange(len(mapping)), mapping].sum()) / N if N else float("nan")


# -- the whole measurement ---------------------------------------------------------------------
def features(enc, feature):
    """The (N, F) k-means input of an ``EvalStep.encode`` result: "prior" (capsule
    presences), "posterior" (posterior masses) or "both" (the two side by side)."""
    if feature == "prior":
        return enc["prior"].contiguous()
    if feature == "posterior":
        return enc["posterior"].contiguous()
    if feature == "both":
        f = enc["features"]
        return f.reshape(f.shape[0], -1)
    raise ValueError(f"feature must be 'prior', 'posterior' or 'both', got {feature!r}")


def _encode(step, split):
    from .data import DatasetView
    if isinstance(split, DatasetView):
        enc = step.encode(split)
    else:
        images, labels = split
        enc = step.encode(images, labels)
    if enc["label"] is None:
        raise ValueError("unsupervised accuracy needs the splits' labels")
    return enc


def unsupervised_accuracy(step, fit, *others, k=10, feature="prior", names=None,
                          n_classes=None, metrics=False, **kmeans_args):
    """k-means on the object-capsule features of split ``fit`` (encoded by the EvalStep
    ``step``), clusters matched to classes on ``fit``'s contingency table, and that mapping
    applied to ``others`` under the fitted centroids.  Splits are (images, labels) pairs or
    data.DatasetView objects; ``names`` names ``others`` (default "test" for one, else
    "split1", "split2", ...).  -> {"fit_accuracy", "<name>_accuracy"..., "inertia",
    "mapping", "n_iter"}.  ``metrics=True`` adds the figures that need no matching
    (``cluster_quality``): "fit_nmi", "fit_ari", "fit_purity", "<name>_nmi", "<name>_ari",
    "<name>_purity", and of the fit split's clustering "silhouette", "calinski_harabasz",
    "davies_bouldin"."""
    if names is None:
        names = ["test"] if len(others) == 1 else [f"split{i + 1}" for i in range(len(others))]
    if len(names) != len(others):
        raise ValueError("one name per split")
    if n_classes is None:
        n_classes = getattr(step.model, "n_classes", None)
    enc = _encode(step, fit)
    if n_classes is None:
        n_classes = int(enc["label"].max()) + 1
    xf = features(enc, feature)
    res = kmeans(xf, k, **kmeans_args)
    mapping, acc = match_clusters(res.labels, enc["label"], k, n_classes)
    out = {"fit_accuracy": acc}
    if metrics:
        from . import cluster_quality as Q       # (it imports this module)

        def label_figures(name, cid, lab):
            ind = Q.label_indices_of(cid, lab, k, n_classes)
            out.update({f"{name}_{m}": ind[m] for m in ("nmi", "ari", "purity")})

        label_figures("fit", res.labels, enc["label"])
    for name, split in zip(names, others):
        e = _encode(step, split)
        cid = assign(features(e, feature), res.centroids)
        out[f"{name}_accuracy"] = mapped_accuracy(cid, e["label"], mapping, n_classes)
        if metrics:
            label_figures(name, cid, e["label"])
    if metrics:
        sil, disp = Q.quality(xf, res.labels, k)
        out.update(silhouette=sil.score, calinski_harabasz=disp.calinski_harabasz,
                   davies_bouldin=disp.davies_bouldin)
    out.update(inertia=res.inertia, mapping=mapping, n_iter=res.n_iter)
    return out
