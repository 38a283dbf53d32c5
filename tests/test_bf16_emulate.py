"""The fp64 bf16 emulator of tests/bf16_emulate.py checked on the CPU: ``rne`` against torch's
fp32 -> bf16 conversion bit for bit, ``near_midpoint`` on constructed cases, and each
restatement, at identity rounding, against the oracle in fp64."""
import numpy as np
import torch

from oracle import scae_oracle as O
from tests import bf16_emulate as E


def _torch_bf16(x32):
    return x32.to(torch.bfloat16).double()


def _same_bits(a, b):
    """fp64 tensors equal entry for entry, signed zeros and infinities included."""
    return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


def test_rne_matches_torch_on_random_fp32_bit_patterns():
    g = np.random.default_rng(0)
    bits = g.integers(0, 2 ** 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    x = torch.from_numpy(bits.view(np.float32).copy())
    x = x[torch.isfinite(x)]
    assert _same_bits(E.rne(x.double()), _torch_bf16(x))


def test_rne_matches_torch_on_ties_subnormals_and_the_top_of_the_range():
    # every exponent, mantissas whose low 16 bits are the tie 0x8000 (even and odd kept
    # part), one below and one above it; fp32 subnormals (bf16 subnormals and ties between
    # them); values around the largest finite bf16 and the overflow midpoint
    hi = torch.arange(0, 1 << 16, 37, dtype=torch.int64)
    low = torch.tensor([0x7FFF, 0x8000, 0x8001, 0x0000, 0xFFFF], dtype=torch.int64)
    pat = (hi[:, None] << 16 | low[None, :]).flatten()
    sub = torch.arange(1, 1 << 23, 4099, dtype=torch.int64)
    top = 0x7F7F0000 + torch.arange(-3 << 16, 1 << 16, 0x1000, dtype=torch.int64)
    pat = torch.cat([pat, sub, sub | 0x8000, top, top | (1 << 31)])
    x = pat.to(torch.int32).view(torch.float32)
    x = x[torch.isfinite(x)]
    assert (x.view(torch.int32) & 0xFFFF == 0x8000).sum() > 1000      # ties are in
    assert ((x.abs() < 2.0 ** -126) & (x != 0)).sum() > 1000          # subnormals are in
    got, want = E.rne(x.double()), _torch_bf16(x)
    assert _same_bits(got, want)
    assert bool(torch.isinf(want).any()) and bool((want.abs() == E.BF16_MAX).any())


def test_rne_is_exact_on_fp64_values_between_fp32_neighbours():
    # an fp64 value just above a tie (not an fp32 value): fp32 first would round it onto
    # the tie and then to even -- rne must round it up
    tie = 1.0 + 2.0 ** -8
    x = torch.tensor([tie + 2.0 ** -40, tie - 2.0 ** -40, tie], dtype=torch.float64)
    assert E.rne(x).tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0]


def test_near_midpoint():
    ulp = 2.0 ** -7                     # bf16 spacing in [1, 2)
    mid = 1.0 + ulp / 2
    x = torch.tensor([mid - 1e-6, mid + 1e-6, 1.0, 1.0 + ulp, mid - 1e-3], dtype=torch.float64)
    assert E.near_midpoint(x, 2e-6).tolist() == [True, True, False, False, False]
    # (below 1.0 the spacing halves: the midpoint under 1.0 is 1 - 2^-9)
    assert E.near_midpoint(x, 2e-3).tolist() == [True, True, True, False, True]
    # an entry-wise err
    err = torch.tensor([1e-7, 2e-6, 1e-3, 1e-3, 2e-3], dtype=torch.float64)
    assert E.near_midpoint(x, err).tolist() == [False, True, False, False, True]


def test_gamma_and_accumulation_bound():
    assert E.gamma(1) == 2.0 ** -23 / (1 - 2.0 ** -23)
    assert 1024 * 2.0 ** -23 < E.gamma(1024) < 1024 * 2.0 ** -23 * (1 + 2.0 ** -12)
    # holds for a worst-case fp32 sum: a large K of same-signed terms in sequence
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(1, 4096, generator=g), torch.rand(4096, 1, generator=g)
    s32 = torch.zeros(1)
    for t in (a[0] * b[:, 0]):          # products of fp32 values, fp32 sum in order
        s32 = s32 + t
    exact = a.double() @ b.double()
    bound = E.accumulation_bound(a.abs(), b.abs(), 4096, extra=1)
    assert float((s32.double() - exact).abs()) <= float(bound)


def test_gemm_restatement_vs_einsum():
    g = torch.Generator().manual_seed(1)
    A, B = torch.randn(3, 17, 40, generator=g), torch.randn(3, 9, 40, generator=g)
    bias, mask = torch.randn(3, 9, generator=g), torch.randn(3, 17, 9, generator=g)
    want = torch.einsum("gmk,gnk->gmn", A.double(), B.double()) + bias.double()[:, None]
    c, raw, err = E.gemm(A, B, bias, relu=True, mask=mask)
    assert float((raw - want.relu()).abs().max()) <= 1e-12
    assert float((c - want.relu() * (mask > 0)).abs().max()) <= 1e-12
    assert bool((err > 0).all())
    cr, _, _ = E.gemm(A, B, round=E.rne)
    assert float((cr - torch.einsum("gmk,gnk->gmn", E.rne(A.double()),
                                    E.rne(B.double()))).abs().max()) <= 1e-12


def test_qkv_attention_restatement_vs_oracle():
    g = torch.Generator().manual_seed(2)
    HB, N, M, dk, dv = 4, 7, 11, 24, 13
    q, k = torch.randn(HB, N, dk, generator=g), torch.randn(HB, M, dk, generator=g)
    v, gout = torch.randn(HB, M, dv, generator=g), torch.randn(HB, N, dv, generator=g)
    p = torch.ones(HB, M)
    p[:, ::3] = torch.rand(HB, len(range(0, M, 3)), generator=g)
    ins = [t.double().requires_grad_() for t in (q, k, v)]
    want = O.qkv_attention(*ins, p.double())
    (want * gout.double()).sum().backward()
    out, probs, out_err, p_err = E.qkv_attention_fwd(q, k, v, p, sqrt_dk=np.sqrt(dk))
    assert float((out - want.detach()).abs().max()) <= 1e-12
    assert bool((out_err > 0).all()) and bool((p_err > 0).all())
    grads, errs = E.qkv_attention_bwd(q, k, v, probs, gout, np.sqrt(dk))
    for name, got, t in zip(("gq", "gk", "gv"), grads, ins):
        assert float((got - t.grad).abs().max()) <= 1e-12, name
    assert all(bool((e >= 0).all()) for e in errs)


def test_seed_attention_restatement_vs_oracle():
    """The folded output attention at identity rounding against the oracle's qkv_attention
    on the unfolded keys / values (K' = h wk^T + bk, V' = h wv^T + bv, q for every set),
    forward and every gradient through autograd, in fp64."""
    g = torch.Generator().manual_seed(3)
    B, N, NQ, C, D = 3, 10, 7, 64, 16
    h = torch.randn(B, N, D, generator=g)
    q = torch.randn(NQ, C, generator=g) * 0.3
    wk, wv = torch.randn(C, D, generator=g) * 0.3, torch.randn(C, D, generator=g) * 0.3
    bk, bv = torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.3
    p = torch.ones(B, N)
    p[:, ::3] = torch.rand(B, len(range(0, N, 3)), generator=g)
    gout = torch.randn(B, NQ, C, generator=g)
    ins = [t.double().requires_grad_() for t in (h, q, wk, bk, wv, bv)]
    hd, qd, wkd, bkd, wvd, bvd = ins
    want = O.qkv_attention(qd.expand(B, NQ, C), hd @ wkd.T + bkd, hd @ wvd.T + bvd, p.double())
    (want * gout.double()).sum().backward()
    vals, errs, taints = E.seed_attention(h, q, wk, wv, bv, p, gout, 1.0 / np.sqrt(C))
    assert float((vals["out"] - want.detach()).abs().max()) <= 1e-12
    for name, t in zip(("gh", "gq", "gwk", "gwv", "gbv"), (hd, qd, wkd, wvd, bvd)):
        assert float((vals[name] - t.grad).abs().max()) <= 1e-12, name
    assert float(bkd.grad.abs().max()) <= 1e-12          # the kernels' exact zero
    assert all(bool((e >= 0).all() and torch.isfinite(e).all()) for e in errs.values())
    assert not any(bool(t.any()) for t in taints.values())
