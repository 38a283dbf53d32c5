"""Test infrastructure: fp64 references that round where the bf16 matrix-core kernels round.

Inside ``ops.mfma_bf16()`` (BASELINE.json configs[2]) a product on the bf16 matrix cores
rounds each fp32 operand to bf16 with round-to-nearest-even and accumulates in fp32:

- ``pack_bf16`` (v_cvt_pk_bf16_f32) in csrc/mfma_tile.h: the batched GEMM's 128 x 128
  tiles (scae_gemm_bf16, _pair_bf16, _multi_bf16) round BOTH operands as they are
  deposited in LDS.  The bias, the ReLU, the mask gate and ``asum`` stay fp32; ``asum``
  sums the operand before it is rounded.
- ``to_bf16x4`` (wave_mfma.h ``mma16p``) in csrc/seed_attention_wave.hip: the output
  attention rounds both operands of the logits S = qk h^T, of T = P h, and of the three
  backward products dP = dT h^T, d(qk) = dS h, dh = P^T dT + dS^T qk (``seed_attention``).
  qk = q wk, dT = gout wv, out = T wv^T + bv, dwv, dbv and the reduction to gq, gwk are
  fp32 products.  scae_seed_attention_mfma_bwd_gemm_bf16 runs the same backward.
- ``f2bf`` in csrc/set_attention.hip: scae_qkv_attention_fwd_bf16 takes q, k, v as bf16
  (nothing left to round), keeps the fp32 softmax ``probs`` for the backward pass and
  rounds them as the A operand of P V; the output is rounded to bf16.  The backward is
  the fp32 kernel on upcast operands and the saved fp32 probabilities; its gradients are
  rounded to bf16 (torch, RNE) at the end.

A product of two bf16 values is exact in fp32, so an fp64 reference that applies ``rne``
at the same points predicts such a kernel to its fp32 accumulation error, which
``accumulation_bound`` bounds.  Where the kernel writes out the fp32 value it then
rounds (the saved ``probs``), the reference rounds the kernel's own value ("imposed
rounding"): both sides round identically by construction.

Bound constant.  A K-term dot product of exact products summed in fp32 in any order has
|fl(s) - s| <= gamma_K * sum |a_i b_i| with gamma_K = K u / (1 - K u) (Higham, eq. 3.4)
for u = 2^-24 under round-to-nearest.  We take u = 2^-23: the matrix core's internal
additions are not documented as round-to-nearest, and one ulp per addition (any
faithful rounding) is what the bound then still covers.  A bf16 rounding moves a value by
up to 2^-9 of itself, six orders of magnitude above these bounds at the sizes tested.
"""
import torch

U = 2.0 ** -23          # per-addition error of the fp32 accumulation (see above)
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
_BF16_MIN_NORMAL = 2.0 ** -126
_BF16_SUB_QUANTUM = 2.0 ** -133


def rne(x):
    """fp64 tensor -> the bf16 value nearest to it (ties to even), as fp64.  Exact for every
    fp64 input (no detour through fp32, which would round twice); values at or past the
    midpoint above the largest finite bf16 go to +-inf, like the hardware conversion."""
    x = x.double()
    m, e = torch.frexp(x)                     # x = m 2^e, 0.5 <= |m| < 1
    # 8 significant bits: quantum 2^(e - 8); below the normal range the subnormal quantum
    q = torch.where(x.abs() >= _BF16_MIN_NORMAL, torch.ldexp(torch.ones_like(x), e - 8),
                    torch.full_like(x, _BF16_SUB_QUANTUM))
    r = torch.round(x / q) * q                # torch.round: half to even; x / q is exact
    r = torch.where(r.abs() > BF16_MAX, torch.copysign(torch.full_like(r, float("inf")), r), r)
    return torch.where(torch.isfinite(x), r, x)


def near_midpoint(x, err):
    """Mask of the entries whose interval [x - err, x + err] holds a bf16 rounding midpoint:
    a value there that is off by up to ``err`` may round to either neighbour."""
    x = x.double()
    err = torch.as_tensor(err, dtype=torch.float64, device=x.device).expand_as(x)
    return rne(x - err) != rne(x + err)


def gamma(K):
    """gamma_K = K u / (1 - K u), u = U: the relative bound of a K-term fp32 sum."""
    return K * U / (1.0 - K * U)


def accumulation_bound(absA, absB, K, extra=0):
    """Entry-wise bound of an fp32-accumulated product: gamma_(K + extra) * (|A| @ |B|).
    ``extra``: further fp32 additions into the same value (a bias, ...)."""
    return gamma(K + extra) * (absA.double() @ absB.double())


def identity(x):
    return x


# ---------------------------------------------------------------------------- K7 GEMM
def gemm(A, B, bias=None, relu=False, mask=None, round=identity):
    """C[g] = epi(round(A[g]) round(B[g])^T) in fp64 -> (C, C before the mask gate,
    entry-wise bound of C's fp32 evaluation).  A (G, M, K), B (G, N, K), bias (G, N)."""
    A, B = A.double(), B.double()
    Ar, Br = round(A), round(B)
    c = Ar @ Br.transpose(1, 2)
    err = accumulation_bound(Ar.abs(), Br.abs().transpose(1, 2), A.shape[2], extra=1)
    if bias is not None:
        c = c + bias.double()[:, None, :]
        err = err + gamma(1) * bias.double().abs()[:, None, :]
    if relu:
        c = torch.relu(c)                     # 1-Lipschitz: the bound carries
    raw = c
    if mask is not None:
        c = torch.where(mask > 0, c, torch.zeros_like(c))
    return c, raw, err


# ----------------------------------------------------------------------- K2 attention
def qkv_attention_fwd(q, k, v, presence=None, probs=None, round=identity, sqrt_dk=None):
    """set_transformer.py:24-47 in fp64 -> (out, probs, bound of out, bound of probs).
    ``probs``: the kernel's fp32 probabilities, imposed (rounded by ``round``) as the A
    operand of P V; None: the reference's own.  q, k, v (HB, N|M, d); presence (HB, M).
    ``sqrt_dk``: the divisor of the logits (None: the fp32 value the kernels are handed)."""
    q, k, v = q.double(), k.double(), v.double()
    dk = q.shape[2]
    if sqrt_dk is None:
        sqrt_dk = float(torch.tensor(dk, dtype=torch.float32).sqrt())
    qr, kr = round(q), round(k)
    s = qr @ kr.transpose(1, 2)
    s_err = accumulation_bound(qr.abs(), kr.abs().transpose(1, 2), dk, extra=2)  # mask, scale
    if presence is not None:
        s = s - (1.0 - presence.double())[:, None, :] * 1e32
    s = s / sqrt_dk
    p_ref = torch.softmax(s, -1)
    # logits moved by at most m move p_i by a factor within exp(+-2m); fp32 exp / sum /
    # divide: a few ulps relative, written as 2^-18
    row = (s_err / sqrt_dk).amax(-1, keepdim=True)
    p_err = p_ref * (torch.expm1(2.0 * row) + 2.0 ** -18) + 2.0 ** -40
    P = p_ref if probs is None else probs.double()
    Pr, vr = round(P), round(v)
    out = Pr @ vr
    out_err = accumulation_bound(Pr.abs(), vr.abs(), P.shape[2])
    return out, p_ref, out_err, p_err


def qkv_attention_bwd(q, k, v, probs, gout, sqrt_dk, round=identity):
    """The backward of ``qkv_attention_fwd`` given the saved probabilities (softmax over
    the keys; the presence term has no gradient path into q, k, v) -> ((gq, gk, gv),
    (their entry-wise bounds of an fp32 evaluation, whose products round: ``extra=1``)).
    ``round``: at the operands of the four products dP = gout v^T, gv = P^T gout,
    gq = dS k, gk = dS^T q."""
    q, k, v, P, go = (t.double() for t in (q, k, v, probs, gout))
    M, dv, dk = v.shape[1], v.shape[2], q.shape[2]
    gor, vr, Pr = round(go), round(v), round(P)
    dP = gor @ vr.transpose(1, 2)
    dP_err = accumulation_bound(gor.abs(), vr.abs().transpose(1, 2), dv, extra=1)
    gv = Pr.transpose(1, 2) @ gor
    gv_err = accumulation_bound(Pr.abs().transpose(1, 2), gor.abs(), P.shape[1], extra=1)
    rs = (P * dP).sum(-1, keepdim=True)
    rs_err = (P * dP_err).sum(-1, keepdim=True) + gamma(M + 1) * (P * dP).abs().sum(-1, keepdim=True)
    dS = P * (dP - rs) / sqrt_dk
    dS_err = (P * (dP_err + rs_err) + gamma(4) * (P * (dP - rs)).abs()) / sqrt_dk
    dSr, kr, qr = round(dS), round(k), round(q)
    gq = dSr @ kr
    gq_err = dS_err @ kr.abs() + accumulation_bound(dSr.abs(), kr.abs(), M, extra=1)
    gk = dSr.transpose(1, 2) @ qr
    gk_err = dS_err.transpose(1, 2) @ qr.abs() + \
        accumulation_bound(dSr.abs().transpose(1, 2), qr.abs(), P.shape[1], extra=1)
    return (gq, gk, gv), (gq_err, gk_err, gv_err)


# ------------------------------------------------------------- K2c output attention
# Values the kernel rounds but never writes out (qk, P, dT, dS inside the output attention)
# cannot be imposed.  Each such value is rounded in the reference as rne(x); where x's
# interval [x - err, x + err] holds a rounding midpoint ("tainted", ``near_midpoint``) the
# kernel's rounded value may be the other neighbour, so the reference carries that
# rounding step, rne(x + err) - rne(x - err), as an absolute uncertainty of the rounded
# operand into every product that reads it.  Untainted operands carry none: their entries
# keep the fp32 accumulation bound, and an output is loose only where a tainted operand
# reaches it -- the taint propagates through the products' sparsity and row-wide through
# the softmax, with its size.
def round_iv(x, err, round=rne):
    """-> (round(x), uncertainty of the kernel's rounded value, taint mask)."""
    if round is identity:
        return x, err, torch.zeros_like(x, dtype=torch.bool)
    taint = near_midpoint(x, err)
    step = torch.where(taint, rne(x + err) - rne(x - err), torch.zeros_like(x))
    return rne(x), step, taint


def product(A, dA, B, dB, K, extra=0):
    """A @ B in fp64 and the entry-wise bound of the kernel's value: operands known to
    dA, dB (absolute), products accumulated in fp32 (K terms + ``extra``)."""
    aA, aB = A.abs() + dA, B.abs() + dB
    return A @ B, dA @ B.abs() + A.abs() @ dB + dA @ dB + gamma(K + extra) * (aA @ aB)


def seed_attention(h, q, wk, wv, bv, presence, gout, inv_sqrt_c, round=identity,
                   exact_folds=False):
    """The output attention of csrc/seed_attention_wave.hip (its folding: qk = q wk,
    S = qk h^T, P = softmax, T = P h, out = T wv^T + bv; bk drops out of the softmax)
    forward and backward in fp64 -> dict of values and dict of their entry-wise bounds.
    ``round`` at the operands of the bf16 products: S (qk, h), T (P, h), dP (dT, h),
    d(qk) (dS, h), dh (P, dT and dS, qk).  qk, dT, the dwv / dbv sums, out and the
    reduction to gq, gwk stay fp32.  ``exact_folds``: q, wk, gout, wv are chosen so that
    qk and dT are exact in fp32 and in bf16 (asserted): their bound is zero."""
    h, q, wk, wv, bv, gout = (t.double() for t in (h, q, wk, wv, bv, gout))
    B, N, D = h.shape
    O, C = q.shape
    z = torch.zeros_like
    hr, dh_, _ = round_iv(h, z(h), round)                       # inputs: exact
    qk, e_qk = product(q, z(q), wk, z(wk), C, 1)
    if exact_folds:
        e_qk = z(qk)
        assert bool((rne(qk) == qk).all())
    qkr, d_qk, t_qk = round_iv(qk, e_qk, round)
    S, e_S = product(qkr.expand(B, O, D), d_qk.expand(B, O, D), hr.transpose(1, 2),
                     dh_.transpose(1, 2), D)
    logits = S
    if presence is not None:
        logits = S - (1.0 - presence.double())[:, None, :] * 1e32
    P = torch.softmax(logits * inv_sqrt_c, -1)
    # logits moved by at most m move p_i by a factor within exp(+-2m); the fp32 softmax
    # (__expf, reciprocal) adds a few ulps relative, written as 2^-16
    e_P = P * (torch.expm1(2.0 * (e_S * inv_sqrt_c).amax(-1, keepdim=True)) + 2.0 ** -16)
    Pr, d_P, t_P = round_iv(P, e_P, round)
    T, e_T = product(Pr, d_P, hr, dh_, N)
    wvT = wv.transpose(0, 1)
    out, e_out = product(T, e_T, wvT, z(wvT), D, 2)            # + bv, fp32 products
    out = out + bv
    e_out = e_out + gamma(D + 2) * bv.abs()
    # backward
    dT, e_dT = product(gout, z(gout), wv, z(wv), C, 1)
    if exact_folds:
        e_dT = z(dT)
        assert bool((rne(dT) == dT).all())
    dTr, d_dT, t_dT = round_iv(dT, e_dT, round)
    ds, e_ds = product(dTr, d_dT, hr.transpose(1, 2), dh_.transpose(1, 2), D)
    dot = (P * ds).sum(-1, keepdim=True)
    e_dot = (e_P * ds.abs() + P * e_ds).sum(-1, keepdim=True) + \
        gamma(N) * (P * ds).abs().sum(-1, keepdim=True)
    dS = P * (ds - dot) * inv_sqrt_c
    e_dS = (e_P * (ds - dot).abs() + P * (e_ds + e_dot) +
            gamma(3) * (P * (ds - dot)).abs()) * inv_sqrt_c
    dSr, d_dS, t_dS = round_iv(dS, e_dS, round)
    dqk, e_dqk = product(dSr, d_dS, hr, dh_, N)
    g1, e1 = product(Pr.transpose(1, 2), d_P.transpose(1, 2), dTr, d_dT, O)
    g2, e2 = product(dSr.transpose(1, 2), d_dS.transpose(1, 2), qkr.expand(B, O, D),
                     d_qk.expand(B, O, D), O)
    gh, e_gh = g1 + g2, e1 + e2 + gamma(2 * O) * (g1.abs() + g2.abs())
    rows = B * O + 2 * B                                        # fp32 batch sums
    dq = dqk.sum(0)
    e_dq = e_dqk.sum(0) + gamma(rows) * dqk.abs().sum(0)
    gq, e_gq = product(dq, e_dq, wk.transpose(0, 1), z(wk).transpose(0, 1), D, 1)
    gwk, e_gwk = product(q.transpose(0, 1), z(q).transpose(0, 1), dq, e_dq, O, 1)
    gwv_b, e_gwv_b = product(gout.transpose(1, 2), z(gout).transpose(1, 2), T, e_T, O, 1)
    gwv = gwv_b.sum(0)
    e_gwv = e_gwv_b.sum(0) + gamma(rows) * gwv_b.abs().sum(0)
    gbv = gout.sum((0, 1))
    e_gbv = gamma(rows) * gout.abs().sum((0, 1))
    vals = dict(out=out, gh=gh, gq=gq, gwk=gwk, gwv=gwv, gbv=gbv)
    errs = dict(out=e_out, gh=e_gh, gq=e_gq, gwk=e_gwk, gwv=e_gwv, gbv=e_gbv)
    taints = dict(qk=t_qk, P=t_P, dT=t_dT, dS=t_dS)
    return vals, errs, taints
