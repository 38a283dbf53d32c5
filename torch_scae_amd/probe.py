"""Linear probe: the accuracy of a linear classifier fitted on frozen capsule features -- the
second figure the SCAE paper reports for a trained encoder, next to the k-means one of
``cluster``.

``fit`` / ``predict`` run on the library's kernels (csrc/linear_probe.hip) for device tensors;
``fit_host`` is the same algorithm in fp64 numpy, used for CPU tensors and to check the kernels.
Both follow one set of rules -- multinomial logistic regression with L2 on the weights, not on
the bias, on standardised features:

- moments: G = [x 1]^T [x 1] (F + 1, F + 1) in fp64; from it, in fp64 on the host, the column
  mean m_f, the population standard deviation s_f and the scale d_f = 1 / s_f, or d_f = 0 where
  s_f <= 1e-6 * max(1, |m_f|): a constant column (a dead capsule) takes no part and gets weight
  exactly 0.  z = (x - m) * d with a trailing 1 for the bias;
- step size: L = 0.5 * lambda_max(Z^T Z / N) + l2, Z^T Z derived from G, m and d in fp64
  (``numpy.linalg.eigvalsh``; no second pass over the data); the step is 1 / L;
- objective: J(V) = (1/N) sum_n [logsumexp_c(V_c . z_n) - V_{y_n} . z_n]
  + (l2 / 2) sum_{c, f < F} V_{c,f}^2, the softmax max-subtracted;
- iteration: FISTA with gradient restart from W = V = 0, t = 1:  g = grad J(V);
  W' = V - g / L;  if sum g . (W' - W) > 0 (an fp64 sum) t = 1;  t' = (1 + sqrt(1 + 4 t^2)) / 2;
  V = W' + ((t - 1) / t') (W' - W);  W = W', t = t'.  t, L, J and the restart sum are fp64
  everywhere; the tensors are fp32 on the device and ``dtype`` in ``fit_host``;
- stopping: the iteration that measures max |g| <= tol ends its problem as converged, and the
  point the gradient was measured at is the result (W = V, no step taken: weights, gradient
  norm and history row belong together, as k-means skips the update of its last assignment); a
  problem also ends, not converged, after ``max_iter`` iterations;
- result in raw-feature coordinates: weight[c, f] = W[c, f] * d_f, bias[c] = W[c, F]
  - sum_f weight[c, f] * m_f; prediction is the arg max of weight . x + bias, ties to the lowest
  class;
- several l2 values are independent problems over the same data, solved side by side in one
  grid, each with its own L, state and stop flag; a problem's bits do not depend on the others.
"""
import ctypes
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .cluster import _P, _encode, _stream, contingency, features

MAX_F, MAX_C, MAX_CF, MAX_R = 256, 256, 16384, 16   # SCAE_PROBE_MAX_F / _C / _CF / _R


class ProbeResult(NamedTuple):
    weight: torch.Tensor         # (C, F), raw-feature coordinates
    bias: torch.Tensor           # (C,)
    loss: float                  # fp64 mean cross-entropy on the fit data, without the penalty
    n_iter: int
    converged: bool              # max |g| <= tol was reached (else: max_iter)
    grad_norm: float             # max |g| of the last iteration
    l2: float
    history: torch.Tensor        # (n_iter, 3) fp64: J(V), max |g|, restarted


# -- arguments --------------------------------------------------------------------------------
def _check_x(x):
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError("x must be an (N, F) tensor with N, F > 0")
    if x.shape[0] >= 1 << 31:
        raise ValueError(f"N = {x.shape[0]} rows: at most 2^31 - 1")


def _check_cf(n_classes, F, R=1):
    if not isinstance(n_classes, int) or isinstance(n_classes, bool) or n_classes <= 0:
        raise ValueError(f"n_classes must be a positive int, got {n_classes!r}")
    if F > MAX_F or n_classes > MAX_C or n_classes * (F + 1) > MAX_CF or R > MAX_R:
        raise ValueError(f"F = {F}, n_classes = {n_classes}, {R} l2 values: the probe takes "
                         f"F <= {MAX_F}, n_classes <= {MAX_C}, n_classes * (F + 1) <= {MAX_CF} "
                         f"and at most {MAX_R} l2 values")


def _args(x, y, n_classes, l2, max_iter, tol):
    """-> (l2 list, tol list, whether l2 was a single value)"""
    _check_x(x)
    if not isinstance(y, torch.Tensor) or y.dim() != 1 or y.shape[0] != x.shape[0] or \
            y.dtype.is_floating_point or y.dtype == torch.bool:
        raise ValueError(f"y must be an (N,) = ({x.shape[0]},) integer tensor")
    single = isinstance(l2, (int, float))
    l2s = [float(l2)] if single else [float(v) for v in l2]
    if not l2s:
        raise ValueError("l2 must be a float or a non-empty sequence of floats")
    _check_cf(n_classes, x.shape[1], len(l2s))
    for v in l2s:
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError(f"l2 must be finite and >= 0, got {v!r}")
    if not isinstance(max_iter, int) or isinstance(max_iter, bool) or max_iter <= 0:
        raise ValueError(f"max_iter must be a positive int, got {max_iter!r}")
    tols = [float(tol)] * len(l2s) if isinstance(tol, (int, float)) else [float(v) for v in tol]
    if len(tols) != len(l2s) or not all(v >= 0.0 for v in tols):
        raise ValueError(f"tol must be a float >= 0 (or one per l2 value), got {tol!r}")
    return l2s, tols, single


def _outside(count, n_classes):
    if count:
        raise ValueError(f"{count} labels outside [0, {n_classes})")


# -- the host restatement (numpy; fp64 unless dtype says otherwise) ---------------------------------
def moments_host(x):
    """G = [x 1]^T [x 1], (F + 1, F + 1) fp64."""
    X = np.asarray(torch.as_tensor(x).detach().cpu(), dtype=np.float64)
    X1 = np.concatenate([X, np.ones((X.shape[0], 1))], 1)
    return X1.T @ X1


def standardisation(G):
    """-> (mean (F,), scale (F,)) fp64 from the moments: scale 1 / population standard
    deviation, 0 for a constant column."""
    G = np.asarray(G, dtype=np.float64)
    F = G.shape[0] - 1
    N = G[F, F]
    mean = G[:F, F] / N
    var = np.maximum(np.diagonal(G)[:F] / N - mean * mean, 0.0)
    sd = np.sqrt(var)
    live = sd > 1e-6 * np.maximum(1.0, np.abs(mean))
    scale = np.where(live, 1.0 / np.where(live, sd, 1.0), 0.0)
    return mean, scale


def lipschitz(G, mean, scale, l2):
    """L = 0.5 * lambda_max(Z^T Z / N) + l2, Z^T Z from the moments."""
    G = np.asarray(G, dtype=np.float64)
    F = G.shape[0] - 1
    N = G[F, F]
    A = np.zeros((F + 1, F + 1))
    A[:F, :F] = (G[:F, :F] / N - np.outer(mean, mean)) * np.outer(scale, scale)
    zbar = (G[:F, F] / N - mean) * scale           # (the standardised columns' means: 0)
    A[:F, F] = A[F, :F] = zbar
    A[F, F] = 1.0
    return 0.5 * float(np.linalg.eigvalsh(A)[-1]) + float(l2)


def standardise(x, mean, scale, dtype=np.float64):
    """Z (N, F + 1) = [(x - mean) * scale, 1] in ``dtype``."""
    X = np.asarray(torch.as_tensor(x).detach().cpu()).astype(dtype)
    Z = (X - mean.astype(dtype)) * scale.astype(dtype)
    return np.concatenate([Z, np.ones((Z.shape[0], 1), dtype=dtype)], 1)


def objective_host(Z, y, V, l2, dtype=np.float64):
    """-> (J(V) fp64, grad J(V) (C, F + 1) in ``dtype``) on standardised rows Z."""
    N, F = Z.shape[0], Z.shape[1] - 1
    rows = np.arange(N)
    logits = Z @ V.T
    mx = logits.max(1, keepdims=True)
    e = np.exp(logits - mx)
    s = e.sum(1, keepdims=True, dtype=dtype)
    loss = ((mx[:, 0] + np.log(s[:, 0])) - logits[rows, y]).astype(np.float64).sum() / N
    D = e / s
    D[rows, y] -= dtype(1)
    g = ((D.T @ Z).astype(np.float64) / N).astype(dtype)
    g[:, :F] += dtype(l2) * V[:, :F]
    pen = 0.5 * float(l2) * float((V[:, :F].astype(np.float64) ** 2).sum())
    return float(loss) + pen, g


def step_host(Z, y, W, V, t, l2, L, tol=0.0, dtype=np.float64):
    """One iteration from the state (W, V, t) -> dict(W, V, t, J, grad, grad_norm, restart,
    dot, converged)."""
    J, g = objective_host(Z, y, V, l2, dtype)
    gmax = float(np.abs(g).max())
    if gmax <= tol:
        return dict(W=V.copy(), V=V.copy(), t=t, J=J, grad=g, grad_norm=gmax, restart=False,
                    dot=0.0, converged=True)
    Wn = V - dtype(1.0 / L) * g
    dot = float((g.astype(np.float64) * (Wn - W).astype(np.float64)).sum())
    restart = dot > 0.0
    tt = 1.0 if restart else float(t)
    tn = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * tt * tt))
    Vn = Wn + dtype((tt - 1.0) / tn) * (Wn - W)
    return dict(W=Wn, V=Vn, t=tn, J=J, grad=g, grad_norm=gmax, restart=restart, dot=dot,
                converged=False)


def raw_coordinates(W, mean, scale):
    """(weight (C, F), bias (C,)) fp64 of a standardised-coordinate W (C, F + 1)."""
    W = np.asarray(W, dtype=np.float64)
    weight = W[:, :-1] * scale
    return weight, W[:, -1] - weight @ mean


def _logits_host(x, weight, bias, dtype=np.float64):
    X = np.asarray(torch.as_tensor(x).detach().cpu()).astype(dtype)
    return X @ np.asarray(weight).astype(dtype).T + np.asarray(bias).astype(dtype)


def _lse_rows(logits):
    mx = logits.max(1)
    return mx + np.log(np.exp(logits - mx[:, None]).sum(1))


def fit_host(x, y, n_classes, l2=1e-3, max_iter=2000, tol=1e-5, dtype=np.float64):
    """``fit`` in numpy (the kernels' check; CPU tensors take it), fp64 or, with
    ``dtype=np.float32``, the same arithmetic in fp32 (the tests' yardstick).  -> ProbeResult
    with fp64 CPU tensors, or a list of them for a sequence ``l2``."""
    l2s, tols, single = _args(x, y, n_classes, l2, max_iter, tol)
    yn = np.asarray(y.detach().cpu(), dtype=np.int64)
    _outside(int(((yn < 0) | (yn >= n_classes)).sum()), n_classes)
    G = moments_host(x)
    mean, scale = standardisation(G)
    Z = standardise(x, mean, scale, dtype)
    F = Z.shape[1] - 1
    m_used, d_used = mean.astype(dtype).astype(np.float64), scale.astype(dtype).astype(np.float64)
    out = []
    for l2v, tolv in zip(l2s, tols):
        L = lipschitz(G, mean, scale, l2v)
        W = np.zeros((n_classes, F + 1), dtype=dtype)
        V, t, hist, conv = W.copy(), 1.0, [], False
        for _ in range(max_iter):
            s = step_host(Z, yn, W, V, t, l2v, L, tolv, dtype)
            W, V, t, conv = s["W"], s["V"], s["t"], s["converged"]
            hist.append((s["J"], s["grad_norm"], float(s["restart"])))
            if conv:
                break
        weight, bias = raw_coordinates(W, m_used, d_used)
        logits = _logits_host(x, weight, bias, dtype)
        loss = float((_lse_rows(logits) - logits[np.arange(len(yn)), yn])
                     .astype(np.float64).mean())
        out.append(ProbeResult(torch.from_numpy(weight), torch.from_numpy(bias), loss,
                               len(hist), bool(conv), hist[-1][1], l2v,
                               torch.tensor(hist, dtype=torch.float64).reshape(-1, 3)))
    return out[0] if single else out


# -- the device path ------------------------------------------------------------------------------
def _moments_device(x, y, n_classes):
    """-> (G (F + 1, F + 1) fp64 numpy, labels outside [0, n_classes))"""
    N, F = x.shape
    groups = _lib.load().scae_probe_groups(N, F)
    n = (F + 1) * (F + 1)
    part = torch.empty(groups * n, device=x.device, dtype=torch.float64)
    out = torch.zeros(n + 1, device=x.device, dtype=torch.float64)   # (+ the count's 8 bytes)
    _lib.call("scae_probe_moments_f64", _P(x), _P(y), N, F, n_classes, _P(part), _P(out),
              ctypes.c_void_p(out.data_ptr() + 8 * n), _stream(x))
    host = out.cpu()
    return host[:n].view(F + 1, F + 1).numpy(), int(host[n:].view(torch.int32)[0])


class DeviceProblems:
    """The device state of R problems over one (x, y): moments, standardisation and step
    sizes at construction, then ``run(n)`` enqueues n iterations.  ``fit`` drives it; the tests
    also load a state of their own (``load_state``) and read the raw buffers."""

    def __init__(self, x, y, n_classes, l2s, tols, max_iter):
        N, F = x.shape
        R, CF = len(l2s), n_classes * (F + 1)
        dev = x.device
        self.x, self.y, self.n_classes, self.l2s, self.max_iter = x, y, n_classes, l2s, max_iter
        self.moments, outside = _moments_device(x, y, n_classes)
        _outside(outside, n_classes)
        self.mean, self.scale = standardisation(self.moments)
        self.L = [lipschitz(self.moments, self.mean, self.scale, v) for v in l2s]
        f64 = dict(device=dev, dtype=torch.float64)
        self.mean_d = torch.tensor(self.mean, device=dev, dtype=torch.float32)
        self.scale_d = torch.tensor(self.scale, device=dev, dtype=torch.float32)
        self.l2_d = torch.tensor(l2s, **f64)
        self.step_d = torch.tensor([1.0 / v for v in self.L], **f64)
        self.tol_d = torch.tensor(tols, **f64)
        self.W = torch.zeros(R, n_classes, F + 1, device=dev)
        self.V = torch.zeros(R, n_classes, F + 1, device=dev)
        self.grad = torch.zeros(R, n_classes, F + 1, device=dev)
        self.t = torch.ones(R, **f64)
        G = _lib.load().scae_probe_groups(N, F)
        self.part_grad = torch.empty(R * G * CF, device=dev)
        self.part_loss = torch.empty(R * G, **f64)
        self.history = torch.zeros(R, max_iter, 3, **f64)
        self.state = torch.zeros(R * _lib.PROBE_STATE_INTS + 1, device=dev, dtype=torch.int32)
        d = self.desc = _lib.ProbeDesc()
        d.x, d.y, d.N, d.F, d.C, d.R, d.G, d.max_iter = \
            x.data_ptr(), y.data_ptr(), N, F, n_classes, R, G, max_iter
        d.mean, d.scale = self.mean_d.data_ptr(), self.scale_d.data_ptr()
        d.l2, d.step, d.tol = self.l2_d.data_ptr(), self.step_d.data_ptr(), self.tol_d.data_ptr()
        d.W, d.V, d.grad, d.t = (self.W.data_ptr(), self.V.data_ptr(), self.grad.data_ptr(),
                                 self.t.data_ptr())
        d.part_grad, d.part_loss = self.part_grad.data_ptr(), self.part_loss.data_ptr()
        d.history, d.state = self.history.data_ptr(), self.state.data_ptr()

    def load_state(self, W, V, t):
        self.W.copy_(torch.as_tensor(W).to(self.W))
        self.V.copy_(torch.as_tensor(V).to(self.V))
        self.t.copy_(torch.as_tensor(t).to(self.t))

    def run(self, n_iters):
        _lib.call("scae_probe_fit_f32", ctypes.byref(self.desc), n_iters, _stream(self.x))

    def stopped(self):
        return int(self.state[-1])

    def results(self):
        R = len(self.l2s)
        st = self.state[:-1].view(R, _lib.PROBE_STATE_INTS).cpu()
        hist = self.history.cpu()
        W = self.W.cpu().double().numpy()
        m_used = self.mean_d.cpu().double().numpy()
        d_used = self.scale_d.cpu().double().numpy()
        out = []
        for r in range(R):
            weight, bias = raw_coordinates(W[r], m_used, d_used)
            weight = torch.from_numpy(weight).to(self.x)
            bias = torch.from_numpy(bias).to(self.x)
            n_iter = int(st[r, 1])
            _, _, loss = _predict_device(self.x, weight, bias, self.y)
            out.append(ProbeResult(weight, bias, loss, n_iter, bool(st[r, 2]),
                                   float(hist[r, n_iter - 1, 1]) if n_iter else float("nan"),
                                   self.l2s[r], hist[r, :n_iter].clone()))
        return out


def _predict_device(x, weight, bias, y=None):
    """-> (labels (N,) int64, log_prob (N,), mean cross-entropy against ``y`` or None)"""
    N, F = x.shape
    C = weight.shape[0]
    pred = torch.empty(N, device=x.device, dtype=torch.int64)
    logp = torch.empty(N, device=x.device)
    ce = None
    if y is not None:
        blocks = _lib.load().scae_probe_predict_blocks(N)
        ce = torch.zeros(blocks + 1, device=x.device, dtype=torch.float64)
    _lib.call("scae_probe_predict_f32", _P(x), N, F, C, _P(weight), _P(bias), _P(y), _P(pred),
              _P(logp), _P(ce), ctypes.c_void_p(0 if ce is None else ce.data_ptr() + 8 * blocks),
              _stream(x))
    return pred, logp, None if ce is None else float(ce[-1])


def _device_inputs(x, y=None):
    if x.dtype != torch.float32:
        raise ValueError("x must be fp32")
    x = x.contiguous()
    if y is not None:
        y = y.to(x.device, torch.int64).contiguous()
    return x, y


def fit(x, y, n_classes, l2=1e-3, max_iter=2000, tol=1e-5, check_every=50):
    """Fit the probe on the rows of ``x`` (N, F) with labels ``y`` (N,) in [0, n_classes).
    ``l2``: a float, or a sequence of up to 16 floats solved side by side (``tol`` may then be
    a sequence too, one per problem).  Device tensors (fp32) run on the kernels,
    ``check_every`` iterations enqueued at a time with one read of the stopped-problem count
    per chunk; CPU tensors take ``fit_host``.  -> ProbeResult, or a list for a sequence."""
    l2s, tols, single = _args(x, y, n_classes, l2, max_iter, tol)
    if not x.is_cuda:
        return fit_host(x, y, n_classes, l2, max_iter, tol)
    if not isinstance(check_every, int) or isinstance(check_every, bool) or check_every <= 0:
        raise ValueError(f"check_every must be a positive int, got {check_every!r}")
    x, y = _device_inputs(x, y)
    p = DeviceProblems(x, y, n_classes, l2s, tols, max_iter)
    enqueued = 0
    while enqueued < max_iter:
        n = min(check_every, max_iter - enqueued)
        p.run(n)
        enqueued += n
        if p.stopped() >= len(l2s):
            break
    out = p.results()
    return out[0] if single else out


def _check_result(x, result):
    _check_x(x)
    w, b = result.weight, result.bias
    if w.dim() != 2 or w.shape[1] != x.shape[1] or b.shape != (w.shape[0],):
        raise ValueError(f"result must hold weight (C, {x.shape[1]}) and bias (C,), got "
                         f"{tuple(w.shape)} and {tuple(b.shape)}")
    _check_cf(int(w.shape[0]), x.shape[1])


def predict(x, result):
    """-> (labels (N,) int64, log_prob (N,)): the arg max of weight . x + bias for each row of
    ``x`` (ties to the lowest class) and the row's log-probability of it.  fp64 on the host."""
    _check_result(x, result)
    if not x.is_cuda:
        logits = _logits_host(x, result.weight, result.bias)
        lab = np.argmax(logits, 1)
        logp = logits[np.arange(len(lab)), lab] - _lse_rows(logits)
        return torch.from_numpy(lab.astype(np.int64)), torch.from_numpy(logp)
    x, _ = _device_inputs(x)
    pred, logp, _ = _predict_device(x, result.weight.to(x).contiguous(),
                                    result.bias.to(x).contiguous())
    return pred, logp


def mean_cross_entropy(x, y, result):
    """The fp64 mean cross-entropy of ``result`` on rows ``x`` with labels ``y``."""
    _check_result(x, result)
    C = result.weight.shape[0]
    if not x.is_cuda:
        yn = np.asarray(y.detach().cpu(), dtype=np.int64)
        _outside(int(((yn < 0) | (yn >= C)).sum()), C)
        logits = _logits_host(x, result.weight, result.bias)
        return float((_lse_rows(logits) - logits[np.arange(len(yn)), yn]).mean())
    x, y = _device_inputs(x, y)
    _outside(int(((y < 0) | (y >= C)).sum()), C)
    return _predict_device(x, result.weight.to(x).contiguous(), result.bias.to(x).contiguous(),
                           y)[2]


# -- the whole measurement ---------------------------------------------------------------------
def _accuracy(x, labels, result, n_classes):
    """-> (accuracy, (predicted, label) table (C, C) int64 numpy)"""
    pred, _ = predict(x, result)
    table = contingency(pred, labels.to(pred.device), n_classes, n_classes)
    return float(np.trace(table)) / int(table.sum()), table


def linear_probe_accuracy(step, fit_split, *others, feature="prior", names=None,
                          n_classes=None, l2=1e-3, select=None, **fit_args):
    """The probe fitted on the object-capsule features of ``fit_split`` (encoded by the
    EvalStep ``step``) and applied to ``others``.  Splits are (images, labels) pairs or
    data.DatasetView objects; ``names`` names ``others`` (default "test" for one, else
    "split1", "split2", ...).  With a sequence ``l2`` the problem with the highest accuracy on
    the split ``select`` is kept, ties to the largest l2 (``select`` may be one of the other
    arguments: it is then encoded once).  -> {"fit_accuracy", "<name>_accuracy"..., "loss",
    "l2", "n_iter", "converged", "confusion" (the first other split's (predicted, label)
    table, None without one), "result"}."""
    if names is None:
        names = ["test"] if len(others) == 1 else [f"split{i + 1}" for i in range(len(others))]
    if len(names) != len(others):
        raise ValueError("one name per split")
    many = not isinstance(l2, (int, float))
    if many and select is None:
        raise ValueError("a sequence of l2 values needs the split `select` to choose on")
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
    res = fit(xf, yf, n_classes, l2=l2, **fit_args)
    if many:
        xs, ys = enc_of(select)
        accs = [_accuracy(xs, ys, r, n_classes)[0] for r in res]
        res = max(zip(accs, res), key=lambda ar: (ar[0], ar[1].l2))[1]
    out = {"fit_accuracy": _accuracy(xf, yf, res, n_classes)[0]}
    confusion = None
    for i, (name, split) in enumerate(zip(names, others)):
        xo, yo = enc_of(split)
        out[f"{name}_accuracy"], table = _accuracy(xo, yo, res, n_classes)
        if i == 0:
            confusion = table
    out.update(loss=res.loss, l2=res.l2, n_iter=res.n_iter, converged=res.converged,
               confusion=confusion, result=res)
    return out
