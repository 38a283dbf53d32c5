"""t-SNE of the capsule features: the 2-D embedding coloured by class that the SCAE paper shows
for a trained encoder, next to the k-means figure of ``cluster`` and the linear probe of ``probe``.

``affinities`` / ``tsne`` run on the library's kernels (csrc/tsne.hip) for device tensors;
``affinities_host`` / ``tsne_host`` are the same algorithm in fp64 numpy (or, with
``dtype=np.float32``, the same arithmetic in fp32: the tests' yardstick), used for CPU tensors and
to check the kernels.  Exact t-SNE, every pair, no approximation.  Both follow one set of rules:

- input: x (N, F) fp32 and a perplexity with 3 * perplexity <= N - 1, F <= 256, N <= 32768
  (``MAX_N``: one row of N fp32 squared distances, 128 KiB, is staged in a CU's 160 KiB LDS for
  the bandwidth search);
- distances: d_ij = sum_f (x_if - x_jf)^2, accumulated in f order;
- conditional affinities: for j != i  p_{j|i} = e_j / S,  e_j = exp(-beta_i (d_ij - min_{k != i}
  d_ik)),  S = sum_j e_j.  beta_i by bisection on the entropy H = log S + beta * sum_j (d e) / S
  (d the shifted distance): from beta = 1 with both bounds open, H > log(perplexity) raises the
  lower bound to beta and doubles beta while the upper side is open, else moves it to the
  midpoint; H below it does the same downwards with halving; the search ends at the first beta
  whose |H - log(perplexity)| <= 1e-5, or with the 100th evaluated beta;
- joint affinities: P_ij = (p_{j|i} + p_{i|j}) / (2 N), P_ii = 0, dense (N, N) fp32 on the device,
  symmetric bit for bit (both orders add the same two numbers);
- embedding Y (N, 2): q_ij = 1 / (1 + |y_i - y_j|^2), q_ii = 0; the rows' sums over j of
  P q (y_i - y_j), q^2 (y_i - y_j), q and P log1p(|y_i - y_j|^2) are taken in the working
  precision, Z = sum_ij q_ij is the fp64 sum of the rows' sums, and
  g_i = 4 * (exaggeration * sum_j P_ij q_ij (y_i - y_j) - (1/Z) * sum_j q_ij^2 (y_i - y_j))
  with 1/Z rounded once to the working precision;
- update, per coordinate: gain = max(gain + 0.2 where g * velocity < 0 else gain * 0.8, 0.01);
  velocity = momentum * velocity - (learning_rate * gain) * g;  y += velocity; then Y loses its
  column means (fp64 sums, the mean rounded once).  Gains start at 1, velocities at 0;
- schedule: exactly ``n_iter`` iterations, no early stop; iteration it < ``exaggeration_iter`` runs
  with exaggeration ``early_exaggeration`` and momentum 0.5, a later one with 1 and 0.8;
  ``learning_rate="auto"`` is max(N / early_exaggeration / 4, 50);
- initialisation, built on the host in fp64 for both paths, rounded to fp32 once (the device path
  copies x to the host for it: the two paths start from the same bits):  "random": y_nk = 1e-4 *
  sqrt(-2 ln u1) cos(2 pi u2) with (u1, u2) = ((w + 1) / 2^24, w' / 2^24) from the top 24 bits
  of words (2k, 2k + 1) of Philox4x32-10 keyed (seed, seed >> 32) at counter (n, 0, 0,
  0x54534E45);  "pca": the projection on the top two eigenvectors of the fp64 covariance
  (``numpy.linalg.eigh``), each with the sign that makes its largest-magnitude entry positive,
  scaled so that the first column's standard deviation is 1e-4 (a second column of zeros for
  F = 1);
- KL = sum P log P + sum_ij P_ij log1p(|y_i - y_j|^2) + log Z: the first term once, in fp64, over
  the entries with P > 0; the second the fp64 sum of the rows' sums.  A history row (it, KL, the
  gradient's 2-norm as the fp64 root of the sum of squares) belongs to the Y that iteration it
  starts from and is recorded for it = check_every, 2 check_every, ... < n_iter, and for the
  result (it = n_iter, no update, the exaggeration iteration n_iter would have); on the device
  the rows land in a buffer that is read once at the end;
- every sum that crosses a lane, a workgroup or a column group is taken in a fixed order and there
  are no floating-point atomics: two runs give the same bits, whatever ``check_every`` is.

The sparse form (``neighbors="auto"`` or an int K; ``affinities_knn`` / ``affinities_knn_host``;
csrc/tsne_sparse.hip) keeps P on each row's K nearest neighbours and the repulsion exact over every
pair: no (N, N) array, no Barnes-Hut, no FFT.  It follows the rules above with these differences:

- input: 3 * perplexity <= K <= min(N - 1, ``MAX_NEIGHBORS`` = 128), F <= 256, 2 <= N <=
  ``SPARSE_MAX_N`` = 262144; "auto" is K = ceil(3 * perplexity);
- neighbour lists: ``neighbors.knn``'s rule in self mode -- d_ij = sum_f (x_if - x_jf)^2 in f
  order, the difference, the product and the sum each rounded (no fused multiply-add), the
  neighbours ascending by (d_ij, j) -- so the device's lists are ``neighbors.knn_host``'s bit for
  bit (the host restatement takes them in its own ``dtype``, or the device's through ``lists``);
- bandwidth: the same bisection over the row's K listed distances, shifted by the first (the
  smallest); p_{j|i} = e_j / S for j in the list and 0 elsewhere;
- joint affinities: P_ij = (p_{j|i} + p_{i|j}) / (2 N) on the union of the directed edges, as CSR
  with a row's columns ascending and no diagonal: a stable sort of the integer keys i N + j over
  the forward and the mirrored edges, then the sum of a key's one or two values -- symmetric bit
  for bit.  sum P log P is taken once in fp64 over the stored entries;
- iteration: the sums of P q (y_i - y_j) and P log1p(|y_i - y_j|^2) run over row i's stored
  entries in column order, those of q^2 (y_i - y_j) and q over every j != i; everything after
  the rows' sums is the dense form's.
"""
import ctypes
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import neighbors as _nb
from .cluster import _P, _encode, _stream, features
from .data import _M32, _philox

MAX_N, MAX_F = _lib.TSNE_MAX_N, _lib.TSNE_MAX_F   # SCAE_TSNE_MAX_N / _F
MAX_NEIGHBORS, SPARSE_MAX_N = _lib.TSNE_MAX_NEIGHBORS, _lib.TSNE_SPARSE_MAX_N
_TAG_TSNE = 0x54534E45
_ROWS = 256        # the host restatement's row chunk (memory, not arithmetic)


class Csr(NamedTuple):
    """The sparse joint affinities: row i holds columns indices[indptr[i]:indptr[i + 1]]."""
    indptr: object               # (N + 1,) int64
    indices: object              # (nnz,) int64, a row's columns ascending, no diagonal
    values: object               # (nnz,)


class TsneResult(NamedTuple):
    y: torch.Tensor              # (N, 2)
    kl: float                    # of y
    history: torch.Tensor        # (ceil(n_iter / check_every), 3) fp64: iteration, KL, |g|
    beta: torch.Tensor           # (N,)
    n_iter: int


# -- arguments --------------------------------------------------------------------------------
def _check_x(x, perplexity):
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError("x must be an (N, F) tensor with N, F > 0")
    N, F = x.shape
    if N > MAX_N or F > MAX_F:
        raise ValueError(f"N = {N}, F = {F}: t-SNE takes N <= {MAX_N}, F <= {MAX_F}")
    if isinstance(perplexity, bool) or not isinstance(perplexity, (int, float)) or \
            not (perplexity > 0 and math.isfinite(perplexity)):
        raise ValueError(f"perplexity must be a positive float, got {perplexity!r}")
    if 3 * perplexity > N - 1:
        raise ValueError(f"perplexity = {perplexity}, N = {N}: needs 3 * perplexity <= N - 1")


def _check_sparse(x, perplexity, neighbors):
    """The sparse form's arguments -> K"""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError("x must be an (N, F) tensor with N, F > 0")
    N, F = x.shape
    if N < 2 or N > SPARSE_MAX_N or F > MAX_F:
        raise ValueError(f"N = {N}, F = {F}: sparse t-SNE takes 2 <= N <= {SPARSE_MAX_N}, "
                         f"F <= {MAX_F}")
    if isinstance(perplexity, bool) or not isinstance(perplexity, (int, float)) or \
            not (perplexity > 0 and math.isfinite(perplexity)):
        raise ValueError(f"perplexity must be a positive float, got {perplexity!r}")
    if isinstance(neighbors, str) and neighbors == "auto":
        K = math.ceil(3 * perplexity)
    elif isinstance(neighbors, int) and not isinstance(neighbors, bool):
        K = neighbors
    else:
        raise ValueError(f"neighbors must be None, 'auto' or an int, got {neighbors!r}")
    if not 3 * perplexity <= K <= min(N - 1, MAX_NEIGHBORS):
        raise ValueError(f"neighbors = {K}, perplexity = {perplexity}, N = {N}: needs "
                         f"3 * perplexity <= neighbors <= min(N - 1, {MAX_NEIGHBORS})")
    return K


def _pos_int(name, v, least=1):
    if not isinstance(v, int) or isinstance(v, bool) or v < least:
        raise ValueError(f"{name} must be an int >= {least}, got {v!r}")


def _args(x, perplexity, n_iter, early_exaggeration, exaggeration_iter, learning_rate, init,
          check_every, neighbors=None):
    """-> the learning rate as a float"""
    if neighbors is None:
        _check_x(x, perplexity)
    else:
        _check_sparse(x, perplexity, neighbors)
    _pos_int("n_iter", n_iter)
    _pos_int("check_every", check_every)
    _pos_int("exaggeration_iter", exaggeration_iter, 0)
    if not (isinstance(early_exaggeration, (int, float)) and early_exaggeration > 0):
        raise ValueError(f"early_exaggeration must be > 0, got {early_exaggeration!r}")
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError(f"learning_rate must be 'auto' or > 0, got {learning_rate!r}")
        learning_rate = max(x.shape[0] / early_exaggeration / 4.0, 50.0)
    if not (isinstance(learning_rate, (int, float)) and learning_rate > 0):
        raise ValueError(f"learning_rate must be 'auto' or > 0, got {learning_rate!r}")
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise ValueError(f"init must be 'pca', 'random' or an (N, 2) tensor, got {init!r}")
    elif not isinstance(init, torch.Tensor) or tuple(init.shape) != (x.shape[0], 2):
        raise ValueError(f"init must be 'pca', 'random' or an (N, 2) = ({x.shape[0]}, 2) tensor")
    return float(learning_rate)


def _np(x, dtype=np.float64):
    return np.asarray(torch.as_tensor(x).detach().cpu()).astype(dtype)


# -- initialisation (fp64 on the host, rounded once) ------------------------------------------
def init_random(N, seed):
    """(N, 2) fp32 ~ N(0, 1e-4^2), Box-Muller on Philox uniforms."""
    n = torch.arange(N, dtype=torch.int64)
    zero = torch.zeros_like(n)
    w = _philox([n, zero, zero, torch.full_like(n, _TAG_TSNE)], seed & _M32,
                (seed >> 32) & _M32, 10)
    cols = []
    for k in range(2):
        u1 = ((w[2 * k] >> 8).double() + 1.0) / 16777216.0
        u2 = (w[2 * k + 1] >> 8).double() / 16777216.0
        cols.append(1e-4 * torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(2.0 * math.pi * u2))
    return torch.stack(cols, 1).float()


def init_pca(x):
    """(N, 2) fp32: the projection on the top two principal axes, first column's deviation 1e-4."""
    X = _np(x)
    Xc = X - X.mean(0)
    w, V = np.linalg.eigh(Xc.T @ Xc / X.shape[0])        # (ascending eigenvalues)
    V = V[:, ::-1][:, :2]
    for k in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, k])), k] < 0:
            V[:, k] = -V[:, k]
    proj = Xc @ V
    if proj.shape[1] < 2:
        proj = np.concatenate([proj, np.zeros((X.shape[0], 1))], 1)
    sd = proj[:, 0].std()
    return torch.from_numpy((proj * (1e-4 / sd if sd > 0 else 0.0)).astype(np.float32))


def _init(x, init, seed):
    if isinstance(init, str):
        return init_random(x.shape[0], int(seed)) if init == "random" else init_pca(x)
    return init.detach().cpu().float()


# -- the host restatement (numpy; fp64 unless dtype says otherwise) ---------------------------------
def distances_host(x, dtype=np.float64):
    """(N, N) squared distances in ``dtype``, f order."""
    X = _np(x, dtype)
    N, F = X.shape
    D = np.empty((N, N), dtype=dtype)
    for lo in range(0, N, _ROWS):
        d = np.zeros((min(_ROWS, N - lo), N), dtype=dtype)
        for f in range(F):
            u = X[lo:lo + _ROWS, None, f] - X[None, :, f]
            d += u * u
        D[lo:lo + _ROWS] = d
    return D


def _shifted(D):
    """d_ij - min_{k != i} d_ik, the diagonal at +inf (e = 0 there)."""
    D = D.copy()
    np.fill_diagonal(D, np.inf)
    return D - D.min(1, keepdims=True)


def _entropy(Ds, beta):
    """-> (H, e, S) of shifted rows Ds at beta (rows,), all in Ds' dtype"""
    e = np.exp(-beta[:, None] * Ds)
    S = e.sum(1)
    de = np.where(np.isinf(Ds), 0, Ds).astype(Ds.dtype) * e
    return np.log(S) + beta * de.sum(1) / S, e, S


def entropy_host(x, beta, dtype=np.float64):
    """The rows' entropies H (N,) at the given ``beta`` (N,), arithmetic in ``dtype``."""
    Ds = _shifted(distances_host(x, dtype))
    beta = _np(beta, dtype)
    return np.concatenate([_entropy(Ds[lo:lo + _ROWS], beta[lo:lo + _ROWS])[0]
                           for lo in range(0, len(beta), _ROWS)])


def bandwidths_host(Ds, perplexity, dtype=np.float64):
    """beta (N,) in ``dtype`` by the bisection of the rules, every row at once with a per-row
    stop mask."""
    N = Ds.shape[0]
    target = dtype(math.log(perplexity))
    beta = np.ones(N, dtype=dtype)
    lo, hi = np.full(N, -np.inf, dtype=dtype), np.full(N, np.inf, dtype=dtype)
    run = np.ones(N, dtype=bool)
    for step in range(100):
        idx = np.nonzero(run)[0]
        if idx.size == 0 or step == 99:
            break
        H = _entropy(Ds[idx], beta[idx])[0]
        diff = H - target
        ok = np.abs(diff) <= dtype(1e-5)
        run[idx[ok]] = False
        up, dn = idx[~ok & (diff > 0)], idx[~ok & ~(diff > 0)]
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * dtype(2), (beta[up] + hi[up]) * dtype(0.5))
        hi[dn] = beta[dn]
        beta[dn] = np.where(np.isinf(lo[dn]), beta[dn] * dtype(0.5),
                            (beta[dn] + lo[dn]) * dtype(0.5))
    return beta


def joint_host(x, beta, dtype=np.float64):
    """-> (P (N, N) in ``dtype``, sum P log P (fp64)) of the given ``beta``: the conditional rows
    e / S, then (p_{j|i} + p_{i|j}) / (2 N)."""
    Ds = _shifted(distances_host(x, dtype))
    beta = _np(beta, dtype)
    N = len(beta)
    C = np.empty((N, N), dtype=dtype)
    for lo in range(0, N, _ROWS):
        _, e, S = _entropy(Ds[lo:lo + _ROWS], beta[lo:lo + _ROWS])
        C[lo:lo + _ROWS] = e / S[:, None]
    P = (C + C.T) / dtype(2 * N)
    pos = P[P > 0].astype(np.float64)
    return P, float((pos * np.log(pos)).sum())


def affinities_host(x, perplexity=30.0, dtype=np.float64):
    """``affinities`` in numpy -> (P (N, N), beta (N,), sum P log P) with CPU tensors of
    ``dtype``."""
    _check_x(x, perplexity)
    beta = bandwidths_host(_shifted(distances_host(x, dtype)), perplexity, dtype)
    P, plogp = joint_host(x, beta, dtype)
    return torch.from_numpy(P), torch.from_numpy(beta), plogp


def neighbor_lists_host(x, K, dtype=np.float32):
    """The self-mode lists of ``neighbors.knn_host`` for K up to ``MAX_NEIGHBORS``, arithmetic in
    ``dtype`` -> KnnResult(idx (N, K) int64, d2 (N, K)) with CPU tensors."""
    X = _nb._np(x, dtype)
    N = X.shape[0]
    idx, d2 = np.empty((N, K), dtype=np.int64), np.empty((N, K), dtype=dtype)
    for lo, hi in _nb._chunks(N, N):
        d = _nb._dist_rows(X, X, lo, hi)
        d[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        idx[lo:hi], d2[lo:hi] = _nb._least(d, K)
    return _nb.KnnResult(torch.from_numpy(idx), torch.from_numpy(d2))


def conditionals_knn_host(d2, beta, dtype=np.float64):
    """-> (p_{j|i} of the listed neighbours (N, K), the rows' entropies H (N,)) at the given
    ``beta``, from the lists' distances ``d2`` (N, K); arithmetic in ``dtype``."""
    d2 = _np(d2, dtype)
    H, e, S = _entropy(d2 - d2[:, :1], _np(beta, dtype))
    return e / S[:, None], H


def joint_knn_host(idx, cond, dtype=np.float64):
    """The lists ``idx`` (N, K) and their conditional rows ``cond`` (N, K) -> (Csr of numpy arrays,
    sum P log P (fp64)): the stable sort of the keys i N + j over the forward, then the mirrored
    edges, a key's one or two values added in that order, / (2 N)."""
    idx, c = _np(idx, np.int64), _np(cond, dtype).reshape(-1)
    N, K = idx.shape
    i, j = np.repeat(np.arange(N, dtype=np.int64), K), idx.reshape(-1)
    keys, v = np.concatenate([i * N + j, j * N + i]), np.concatenate([c, c])
    order = np.argsort(keys, kind="stable")
    keys, v = keys[order], v[order]
    first = np.ones(len(keys), dtype=bool)
    first[1:] = keys[1:] != keys[:-1]
    pos = np.nonzero(first)[0]
    nxt = np.minimum(pos + 1, len(keys) - 1)
    twice = (pos + 1 < len(keys)) & ~first[nxt]
    values = ((v[pos] + np.where(twice, v[nxt], dtype(0))) / dtype(2 * N)).astype(dtype)
    indptr = np.searchsorted(keys[pos], np.arange(N + 1, dtype=np.int64) * N).astype(np.int64)
    p = values[values > 0].astype(np.float64)
    return Csr(indptr, keys[pos] % N, values), float((p * np.log(p)).sum())


def affinities_knn_host(x, perplexity=30.0, neighbors="auto", dtype=np.float64, lists=None):
    """``affinities_knn`` in numpy -> (indptr, indices, values, beta, sum P log P) with CPU tensors,
    values and beta in ``dtype``.  ``lists`` = (idx, d2): neighbour lists to use instead of the
    host's own (the tests hand it the device's)."""
    K = _check_sparse(x, perplexity, neighbors)
    idx, d2 = neighbor_lists_host(x, K, dtype) if lists is None else lists
    if tuple(idx.shape) != (x.shape[0], K) or tuple(d2.shape) != (x.shape[0], K):
        raise ValueError(f"lists must be (idx, d2), each ({x.shape[0]}, {K})")
    d2 = _np(d2, dtype)
    beta = bandwidths_host(d2 - d2[:, :1], perplexity, dtype)
    csr, plogp = joint_knn_host(idx, conditionals_knn_host(d2, beta, dtype)[0], dtype)
    return tuple(torch.from_numpy(a) for a in csr) + (torch.from_numpy(beta), plogp)


def densify(indptr, indices, values):
    """The CSR as a dense (N, N) numpy array of the values' dtype (tests, small N)."""
    indptr, indices, values = (np.asarray(torch.as_tensor(a).cpu()) for a in
                               (indptr, indices, values))
    N = len(indptr) - 1
    P = np.zeros((N, N), dtype=values.dtype)
    P[np.repeat(np.arange(N), np.diff(indptr)), indices] = values
    return P


def pair_sums_host(Y, dtype=np.float64, rows=None):
    """The repulsion's sums over every j != i for the given ``rows`` (all by default), in
    ``dtype`` -> dict(rep (R, 2), z (R,))."""
    Y = _np(Y, dtype)
    rows = np.arange(Y.shape[0]) if rows is None else np.asarray(rows)
    rep, z = np.empty((len(rows), 2), dtype=dtype), np.empty(len(rows), dtype=dtype)
    for lo in range(0, len(rows), _ROWS):
        r = rows[lo:lo + _ROWS]
        dy0 = Y[r, None, 0] - Y[None, :, 0]
        dy1 = Y[r, None, 1] - Y[None, :, 1]
        q = dtype(1) / (dtype(1) + (dy0 * dy0 + dy1 * dy1))
        q[np.arange(len(r)), r] = 0
        q2 = q * q
        rep[lo:lo + _ROWS, 0], rep[lo:lo + _ROWS, 1] = (q2 * dy0).sum(1), (q2 * dy1).sum(1)
        z[lo:lo + _ROWS] = q.sum(1)
    return dict(rep=rep, z=z)


def edge_sums_host(P, Y, dtype=np.float64):
    """The attraction's and the KL's sums over the stored entries of the Csr ``P`` (every row
    has some), in ``dtype`` -> dict(att (N, 2), kl (N,))."""
    indptr, cols = (np.asarray(torch.as_tensor(a).cpu()) for a in P[:2])
    v, Y = _np(P[2], dtype), _np(Y, dtype)
    i = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    dy0, dy1 = Y[i, 0] - Y[cols, 0], Y[i, 1] - Y[cols, 1]
    d = dy0 * dy0 + dy1 * dy1
    pq = v * (dtype(1) / (dtype(1) + d))
    at = indptr[:-1]
    att = np.stack([np.add.reduceat(pq * dy0, at), np.add.reduceat(pq * dy1, at)], 1)
    return dict(att=att.astype(dtype), kl=np.add.reduceat(v * np.log1p(d), at).astype(dtype))


def row_sums_host(P, Y, dtype=np.float64):
    """The rows' sums over j in ``dtype`` -> dict(att (N, 2), rep (N, 2), z (N,), kl (N,)).
    ``P``: the dense (N, N) matrix, or the sparse form's ``Csr``."""
    if isinstance(P, Csr):
        return {**edge_sums_host(P, Y, dtype), **pair_sums_host(Y, dtype)}
    P, Y = _np(P, dtype), _np(Y, dtype)
    N = Y.shape[0]
    att, rep = np.empty((N, 2), dtype=dtype), np.empty((N, 2), dtype=dtype)
    z, kl = np.empty(N, dtype=dtype), np.empty(N, dtype=dtype)
    for lo in range(0, N, _ROWS):
        hi = min(lo + _ROWS, N)
        dy0 = Y[lo:hi, None, 0] - Y[None, :, 0]
        dy1 = Y[lo:hi, None, 1] - Y[None, :, 1]
        d = dy0 * dy0 + dy1 * dy1
        q = dtype(1) / (dtype(1) + d)
        q[np.arange(hi - lo), np.arange(lo, hi)] = 0
        pq, q2 = P[lo:hi] * q, q * q
        att[lo:hi, 0], att[lo:hi, 1] = (pq * dy0).sum(1), (pq * dy1).sum(1)
        rep[lo:hi, 0], rep[lo:hi, 1] = (q2 * dy0).sum(1), (q2 * dy1).sum(1)
        z[lo:hi] = q.sum(1)
        kl[lo:hi] = (P[lo:hi] * np.log1p(d)).sum(1)
    return dict(att=att, rep=rep, z=z, kl=kl)


def kl_host(P, Y, plogp, dtype=np.float64):
    """KL of the embedding ``Y`` under ``P`` (``plogp`` = sum P log P)."""
    s = row_sums_host(P, Y, dtype)
    return float(plogp) + float(s["kl"].astype(np.float64).sum()) + \
        math.log(float(s["z"].astype(np.float64).sum()))


def step_host(P, Y, velocity, gains, exaggeration, momentum, learning_rate, plogp=0.0,
              dtype=np.float64):
    """One iteration from the state (Y, velocity, gains) -> dict(Y, velocity, gains, grad, gv
    (= grad * the incoming velocity: the gain rule's test), kl and grad_norm of the incoming Y)."""
    Y, velocity, gains = _np(Y, dtype), _np(velocity, dtype), _np(gains, dtype)
    s = row_sums_host(P, Y, dtype)
    Z = float(s["z"].astype(np.float64).sum())
    zinv = dtype(1.0 / Z)
    g = dtype(4) * (dtype(exaggeration) * s["att"] - s["rep"] * zinv)
    gv = g * velocity
    gains_n = np.maximum(np.where(gv < 0, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
    vel_n = dtype(momentum) * velocity - (dtype(learning_rate) * gains_n) * g
    Yn = Y + vel_n
    Yn = Yn - (Yn.astype(np.float64).sum(0) / Y.shape[0]).astype(dtype)
    return dict(Y=Yn, velocity=vel_n, gains=gains_n, grad=g, gv=gv,
                kl=float(plogp) + float(s["kl"].astype(np.float64).sum()) + math.log(Z),
                grad_norm=math.sqrt(float((g.astype(np.float64) ** 2).sum())))


def _schedule(it, exaggeration_iter, early_exaggeration):
    """-> (exaggeration, momentum) of iteration ``it``"""
    return (early_exaggeration, 0.5) if it < exaggeration_iter else (1.0, 0.8)


def tsne_host(x, perplexity=30.0, n_iter=1000, early_exaggeration=12.0, exaggeration_iter=250,
              learning_rate="auto", init="pca", seed=0, check_every=50, dtype=np.float64,
              neighbors=None):
    """``tsne`` in numpy (the kernels' check; CPU tensors take it), fp64 or, with
    ``dtype=np.float32``, the same arithmetic in fp32.  -> TsneResult with CPU tensors."""
    lr = _args(x, perplexity, n_iter, early_exaggeration, exaggeration_iter, learning_rate, init,
               check_every, neighbors)
    if neighbors is None:
        P, beta, plogp = affinities_host(x, perplexity, dtype)
        P = P.numpy()
    else:
        *csr, beta, plogp = affinities_knn_host(x, perplexity, neighbors, dtype)
        P = Csr(*(a.numpy() for a in csr))
    Y = _init(x, init, seed).numpy().astype(dtype)
    vel, gains = np.zeros_like(Y), np.ones_like(Y)
    hist = []
    for it in range(n_iter):
        ex, mom = _schedule(it, exaggeration_iter, early_exaggeration)
        s = step_host(P, Y, vel, gains, ex, mom, lr, plogp, dtype)
        if it > 0 and it % check_every == 0:
            hist.append((float(it), s["kl"], s["grad_norm"]))
        Y, vel, gains = s["Y"], s["velocity"], s["gains"]
    ex, mom = _schedule(n_iter, exaggeration_iter, early_exaggeration)
    s = step_host(P, Y, vel, gains, ex, mom, lr, plogp, dtype)
    hist.append((float(n_iter), s["kl"], s["grad_norm"]))
    return TsneResult(torch.from_numpy(Y), s["kl"], torch.tensor(hist, dtype=torch.float64),
                      beta, n_iter)


# -- the device path ------------------------------------------------------------------------------
def _device_x(x):
    if x.dtype != torch.float32:
        raise ValueError("x must be fp32")
    return x.contiguous()


def _affinities_device(x, perplexity):
    """-> (P (N, N), beta (N,), sum P log P as a (1,) fp64 device tensor)"""
    N, F = x.shape
    T = (N + 31) // 32
    P = torch.empty(N, N, device=x.device)
    beta = torch.empty(N, device=x.device)
    part = torch.empty(T * (T + 1) // 2, device=x.device, dtype=torch.float64)
    plogp = torch.zeros(1, device=x.device, dtype=torch.float64)
    _lib.call("scae_tsne_affinities_f32", _P(x), N, F, float(perplexity), _P(P), _P(beta),
              _P(part), _P(plogp), _stream(x))
    return P, beta, plogp


def affinities(x, perplexity=30.0):
    """The joint affinities of the rows of ``x`` (N, F): -> (P (N, N), beta (N,), sum P log P).
    Device tensors (fp32) run on the kernels, CPU tensors take ``affinities_host`` (fp64)."""
    _check_x(x, perplexity)
    if not x.is_cuda:
        return affinities_host(x, perplexity)
    P, beta, plogp = _affinities_device(_device_x(x), perplexity)
    return P, beta, float(plogp)


def neighbor_lists(x, K):
    """The K nearest other rows of every row of ``x`` (N, F), ``neighbors.knn``'s self mode for
    1 <= K <= min(N - 1, ``MAX_NEIGHBORS``): the lists the sparse affinities are built on.
    -> KnnResult(idx (N, K) int64, d2 (N, K)); CPU tensors take ``neighbor_lists_host``."""
    _check_sparse(x, 1.0 / 3.0, K)       # (the perplexity that admits every K >= 1)
    if not x.is_cuda:
        return neighbor_lists_host(x, K)
    x = _device_x(x)
    (N, F), dev = x.shape, x.device
    G = _lib.load().scae_knn_groups(N, N)
    part = torch.empty(N * G * K, device=dev, dtype=torch.int64) if G > 1 else None
    d2 = torch.empty(N, K, device=dev)
    idx = torch.empty(N, K, device=dev, dtype=torch.int64)
    _lib.call("scae_knn_wide_f32", _P(x), N, F, K, _P(part), _P(d2), _P(idx), _stream(x))
    return _nb.KnnResult(idx, d2)


def _joint_knn_device(idx, cond):
    """``joint_knn_host`` in torch ops on the lists' device (integer sorts: deterministic)
    -> (Csr, sum P log P as a (1,) fp64 tensor)"""
    (N, K), dev = idx.shape, idx.device
    i = torch.arange(N, device=dev).repeat_interleave(K)
    j, c = idx.reshape(-1), cond.reshape(-1)
    keys, order = torch.sort(torch.cat([i * N + j, j * N + i]), stable=True)
    v = torch.cat([c, c])[order]
    first = torch.ones_like(keys, dtype=torch.bool)
    first[1:] = keys[1:] != keys[:-1]
    pos = first.nonzero().squeeze(1)
    nxt = (pos + 1).clamp_(max=keys.numel() - 1)
    twice = (pos + 1 < keys.numel()) & ~first[nxt]
    # (a tensor divisor: a Python scalar would be turned into a multiplication by 1 / (2 N))
    values = (v[pos] + torch.where(twice, v[nxt], torch.zeros_like(c[:1]))) / \
        torch.full((1,), float(2 * N), device=dev)
    ukeys = keys[pos]
    indptr = torch.searchsorted(ukeys, torch.arange(N + 1, device=dev) * N)
    p = values.double()
    plogp = torch.where(p > 0, p * torch.log(p), torch.zeros_like(p)).sum().reshape(1)
    return Csr(indptr, ukeys % N, values), plogp


def _affinities_knn_device(x, perplexity, K):
    """-> (Csr, beta (N,), sum P log P as a (1,) fp64 device tensor)"""
    idx, d2 = neighbor_lists(x, K)
    N = x.shape[0]
    cond, beta = torch.empty(N, K, device=x.device), torch.empty(N, device=x.device)
    _lib.call("scae_tsne_knn_bandwidths_f32", _P(d2), N, K, float(perplexity), _P(cond),
              _P(beta), _stream(x))
    csr, plogp = _joint_knn_device(idx, cond)
    return csr, beta, plogp


def affinities_knn(x, perplexity=30.0, neighbors="auto"):
    """The sparse joint affinities of the rows of ``x`` (N, F) on their K nearest neighbours
    (``neighbors``: "auto" = ceil(3 * perplexity), or K): -> (indptr (N + 1,) int64, indices
    (nnz,) int64, values (nnz,), beta (N,), sum P log P), a row's columns ascending, no diagonal.
    Device tensors (fp32) run on the kernels, CPU tensors take ``affinities_knn_host`` (fp64)."""
    K = _check_sparse(x, perplexity, neighbors)
    if not x.is_cuda:
        return affinities_knn_host(x, perplexity, K)
    csr, beta, plogp = _affinities_knn_device(_device_x(x), perplexity, K)
    return csr + (beta, float(plogp))


class _Problem:
    """The device state of one run that both forms share -- Y, velocity, gains, the rows' sums,
    the partials, the history -- and their fields of the descriptor.  A form names its
    descriptor type, its ``groups`` function, the ``part`` rows per group, its ``block`` size and
    whether ``rows`` starts as zeros."""
    DESC = GROUPS = PART_ROWS = BLOCK_DOUBLES = ZERO_ROWS = None

    def _setup(self, N, dev, plogp, Y0, n_iter, early_exaggeration, exaggeration_iter,
               learning_rate, check_every):
        G = getattr(_lib.load(), self.GROUPS)(N)
        self.plogp = torch.as_tensor(plogp, dtype=torch.float64).reshape(1).to(dev)
        self.Y = torch.as_tensor(Y0).to(dev, torch.float32).contiguous().clone()
        self.velocity = torch.zeros(N, 2, device=dev)
        self.gains = torch.ones(N, 2, device=dev)
        self.part = torch.empty(self.PART_ROWS * G * N, device=dev)
        self.rows = (torch.zeros if self.ZERO_ROWS else torch.empty)(6 * N, device=dev)
        self.block = torch.zeros(self.BLOCK_DOUBLES, device=dev, dtype=torch.float64)
        self.history = torch.zeros(-(-n_iter // check_every), _lib.TSNE_HISTORY_COLS, device=dev,
                                   dtype=torch.float64)
        d = self.desc = self.DESC()
        d.N, d.G, d.n_iter, d.exaggeration_iter, d.check_every = \
            N, G, n_iter, exaggeration_iter, check_every
        d.early_exaggeration, d.learning_rate = early_exaggeration, learning_rate
        d.Y, d.velocity, d.gains = (self.Y.data_ptr(), self.velocity.data_ptr(),
                                    self.gains.data_ptr())
        d.part, d.rows, d.block = self.part.data_ptr(), self.rows.data_ptr(), self.block.data_ptr()
        d.plogp, d.history = self.plogp.data_ptr(), self.history.data_ptr()
        return d

    def load_state(self, Y, velocity, gains):
        self.Y.copy_(torch.as_tensor(Y).to(self.Y))
        self.velocity.copy_(torch.as_tensor(velocity).to(self.Y))
        self.gains.copy_(torch.as_tensor(gains).to(self.Y))


class _SparseProblem(_Problem):
    """``_TsneProblem`` for the sparse form: the device state of one run over a Csr."""
    DESC, GROUPS, PART_ROWS = _lib.TsneSparseDesc, "scae_tsne_sparse_groups", 3
    BLOCK_DOUBLES, ZERO_ROWS = _lib.TSNE_SPARSE_BLOCK_DOUBLES, True

    def __init__(self, csr, plogp, Y0, n_iter, early_exaggeration, exaggeration_iter,
                 learning_rate, check_every):
        self.indptr = csr.indptr.contiguous()
        self.cols = csr.indices.to(torch.int32).contiguous()
        self.vals = csr.values.contiguous()
        d = self._setup(csr.indptr.numel() - 1, csr.values.device, plogp, Y0, n_iter,
                        early_exaggeration, exaggeration_iter, learning_rate, check_every)
        d.indptr, d.cols, d.vals, d.nnz = (self.indptr.data_ptr(), self.cols.data_ptr(),
                                           self.vals.data_ptr(), self.vals.numel())

    def run(self, first_iter, n):
        _lib.call("scae_tsne_sparse_run_f32", ctypes.byref(self.desc), first_iter, n,
                  _stream(self.Y))


class _TsneProblem(_Problem):
    """The device state of one run over a given P: Y, velocity, gains, the partials, the history
    and the descriptor; ``run(first_iter, n)`` enqueues iterations.  ``tsne`` drives it; the tests
    also load a state of their own (``load_state``) and read the raw buffers."""
    DESC, GROUPS, PART_ROWS = _lib.TsneDesc, "scae_tsne_groups", 6
    BLOCK_DOUBLES, ZERO_ROWS = _lib.TSNE_BLOCK_DOUBLES, False

    def __init__(self, P, plogp, Y0, n_iter, early_exaggeration, exaggeration_iter,
                 learning_rate, check_every):
        self.P = P
        d = self._setup(P.shape[0], P.device, plogp, Y0, n_iter, early_exaggeration,
                        exaggeration_iter, learning_rate, check_every)
        d.P = P.data_ptr()

    def run(self, first_iter, n):
        _lib.call("scae_tsne_run_f32", ctypes.byref(self.desc), first_iter, n, _stream(self.P))


def tsne(x, perplexity=30.0, n_iter=1000, early_exaggeration=12.0, exaggeration_iter=250,
         learning_rate="auto", init="pca", seed=0, check_every=50, neighbors=None):
    """Exact t-SNE of the rows of ``x`` (N, F) into two dimensions.  ``init``: "pca", "random"
    (seeded by ``seed``) or an (N, 2) tensor.  ``neighbors``: None for the dense (N, N) affinities
    (N <= ``MAX_N``), "auto" or an int K for the sparse form on each row's K nearest neighbours
    (N <= ``SPARSE_MAX_N``; the repulsion stays exact).  On the device the affinities and all
    ``n_iter`` iterations are enqueued with no read until the end; CPU tensors take
    ``tsne_host``.  -> TsneResult."""
    lr = _args(x, perplexity, n_iter, early_exaggeration, exaggeration_iter, learning_rate, init,
               check_every, neighbors)
    if not x.is_cuda:
        return tsne_host(x, perplexity, n_iter, early_exaggeration, exaggeration_iter,
                         learning_rate, init, seed, check_every, neighbors=neighbors)
    x = _device_x(x)
    if neighbors is None:
        P, beta, plogp = _affinities_device(x, perplexity)
        p = _TsneProblem(P, plogp, _init(x, init, seed), n_iter, float(early_exaggeration),
                         exaggeration_iter, lr, check_every)
    else:
        csr, beta, plogp = _affinities_knn_device(x, perplexity,
                                                  _check_sparse(x, perplexity, neighbors))
        p = _SparseProblem(csr, plogp, _init(x, init, seed), n_iter, float(early_exaggeration),
                           exaggeration_iter, lr, check_every)
    p.run(0, n_iter)
    hist = p.history.cpu()
    return TsneResult(p.Y, float(hist[-1, 1]), hist, beta, n_iter)


# -- the whole figure ----------------------------------------------------------------------------
def capsule_embedding(step, split, feature="prior", trustworthiness_k=None, **tsne_args):
    """The t-SNE embedding of the object-capsule features of ``split`` (an (images, labels) pair
    or a data.DatasetView), encoded by the EvalStep ``step``.  -> {"y" (N, 2), "label" (N,) in
    encode order, "kl", "history"}, and with ``trustworthiness_k`` also "trustworthiness": how
    far y keeps the features' neighbourhoods at that k (``neighbors.trustworthiness``)."""
    enc = _encode(step, split)
    x = features(enc, feature)
    res = tsne(x, **tsne_args)
    out = {"y": res.y, "label": enc["label"], "kl": res.kl, "history": res.history}
    if trustworthiness_k is not None:
        from .neighbors import trustworthiness
        out["trustworthiness"] = trustworthiness(x, res.y, trustworthiness_k)
    return out
