"""configs[2]'s bf16 matrix-core kernels against fp64 references that round where they round
(tests/bf16_emulate.py).  Every operand a kernel rounds is rounded the same way in the
reference, so what is left is fp32 accumulation error, held entry by entry to the derived
bound ``bf16_emulate.accumulation_bound`` -- four orders of magnitude below the 2^-7 bars of
the statistical bf16 tests in test_hip_ops.py, tight enough that a mis-rounded operand, a
dropped K chunk or a wrong fragment fails.  bf16-typed outputs must equal the rounded
reference bit for bit wherever the reference is not within its bound of a rounding midpoint.
Each test checks which C entry point ran."""
import contextlib

import numpy as np
import pytest
import torch

from tests import bf16_emulate as E

pytestmark = pytest.mark.gpu

MIN_CLEAN = 0.5       # bf16 outputs: least fraction of entries that must be compared bitwise
# ... for gq and gk, whose bound carries the worst case of dP = gout v^T (dv terms) through
# the softmax backward and a second product: at dk = dv = 256 it leaves 15 % of gq clear of
# a midpoint (measured), 54 .. 92 % at the smaller shapes
MIN_CLEAN_DS = 0.1


@contextlib.contextmanager
def _spy():
    """-> the list of C entry points ``_lib.call`` launches inside the block."""
    from torch_scae_amd import _lib
    calls, real = [], _lib.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    _lib.call = spy
    try:
        yield calls
    finally:
        _lib.call = real


# --------------------------------------------------------------------------------------
# K7 batched GEMM: scae_gemm_bf16, scae_gemm_multi_bf16, scae_gemm_pair_bf16
# --------------------------------------------------------------------------------------
def _strided(X, kc, pad, gap):
    """Logical (G, R, K) operand -> NaN-padded device buffer laid out as the kernels read
    it: kc: X[g][r][k] at g*batch + r*ld + k (ld = K + pad); else at g*batch + k*ld + r
    (ld = R + pad); batch = rows * ld + gap.  -> (buffer, ld, batch)."""
    G, R, K = X.shape
    ld = (K if kc else R) + pad
    rows = R if kc else K
    batch = rows * ld + gap
    buf = torch.full((G * batch,), float("nan"))
    view = buf.as_strided((G, rows, ld), (batch, ld, 1))
    if kc:
        view[:, :, :K] = X
    else:
        view[:, :, :R] = X.transpose(1, 2)
    return buf.cuda(), ld, batch


class _Gemm:
    """One GEMM problem of the kernels' general form with random operands, its device
    buffers (padding and gaps NaN) and its scae_gemm_desc."""

    def __init__(self, seed, G, M, N, K, ak, bk, bias=False, relu=False, mask=False,
                 asum=False, craw=False, pad=(3, 5, 2), gap=(7, 1, 2)):
        from torch_scae_amd import ops
        g = torch.Generator().manual_seed(seed)
        self.G, self.M, self.N, self.K, self.relu = G, M, N, K, relu
        self.A = torch.randn(G, M, K, generator=g)
        self.B = torch.randn(G, N, K, generator=g) * 0.5
        self.bias = torch.randn(G, N, generator=g) if bias else None
        self.mask = torch.randn(G, M, N, generator=g) if mask else None
        self.a, lda, a_b = _strided(self.A, ak, pad[0], gap[0])
        self.b, ldb, b_b = _strided(self.B, bk, pad[1], gap[1])
        ldc = N + pad[2]
        c_b = M * ldc + gap[2]
        self.c = torch.full((G * c_b,), float("nan"), device="cuda")
        self.cview = lambda t: t.as_strided((G, M, N), (c_b, ldc, 1))
        kw = {}
        if bias:
            self.bias_d = self.bias.cuda()
            kw.update(bias=ops._p(self.bias_d), bias_ld=1, bias_b=N)
        if mask:
            self.mask_d = self.mask.cuda()
            kw.update(mask=ops._p(self.mask_d), ldmask=N, mask_b=M * N)
        self.asum = None
        if asum:                                  # a column of a wider matrix
            self.asum = torch.full((G, M, 3), float("nan"), device="cuda")
            kw.update(asum=ops._off(self.asum, 1), asum_b=3 * M, asum_ld=3)
        self.kw = kw
        self.args = (ops._p(self.a), ops._p(self.b), ops._p(self.c), G, M, N, K, ak, lda, a_b,
                     bk, ldb, b_b, ldc, c_b)
        self.desc = ops._gemm_desc(*self.args, relu=relu, **kw)
        self.craw = None
        if craw:
            self.craw = torch.full_like(self.c, float("nan"))
            self.desc.c_nomask = self.craw.data_ptr()

    def launch_single(self):
        from torch_scae_amd import ops
        ops._gemm(*self.args, relu=self.relu, ref=self.c, **self.kw)

    def check(self, bf16, what):
        """Rounded operands (bf16 tiles): every entry within the fp32 accumulation bound of
        the reference on rne(A), rne(B).  Otherwise (a side < 32: the fp32 tiles) the fp32
        bar against the reference on the unrounded operands."""
        ref, raw, err = E.gemm(self.A, self.B, self.bias, self.relu, self.mask,
                               round=E.rne if bf16 else E.identity)
        if not bf16:
            # fp32 products round too, and the pair's fallback sums six bf16 partial
            # products per pair (bf16x6.h): 6 K terms
            err = E.accumulation_bound(self.A.abs(), self.B.abs().transpose(1, 2),
                                       6 * self.K, extra=2)
        c = self.c.cpu()
        got = self.cview(c).double()
        d = (got - ref).abs()
        print(f"{what}: max |err| / bound {float((d / err).max()):.3g}, "
              f"max |err| / max |ref| {float(d.max()) / float(ref.abs().max()):.2e}")
        assert bool((d <= err).all()), (what, float((d - err).max()),
                                        int((d > err).sum()), d.numel())
        assert float(d.max()) <= 2e-6 * float(ref.abs().max()), what    # the practical bar
        # nothing written outside C (padding, gaps)
        inside = torch.zeros_like(c, dtype=torch.bool)
        self.cview(inside).fill_(True)
        assert bool(torch.isnan(c[~inside]).all()), what
        if bf16:
            # the operands really were rounded: the unrounded product is off somewhere
            plain, _, _ = E.gemm(self.A, self.B, self.bias, self.relu, self.mask)
            assert bool(((got - plain).abs() > err).any()), what
        if self.craw is not None:
            r = self.cview(self.craw.cpu()).double()
            assert bool(((r - raw).abs() <= err).all()), what + " c_nomask"
        if self.asum is not None:
            s = self.asum.cpu().double()
            want = self.A.double().sum(2)
            bound = E.gamma(self.K) * self.A.double().abs().sum(2)   # unrounded fp32 sum
            assert bool(((s[:, :, 1] - want).abs() <= bound).all()), what + " asum"
            assert bool(torch.isnan(s[:, :, 0]).all() and torch.isnan(s[:, :, 2]).all())


LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize("ak,bk", LAYOUTS)
@pytest.mark.parametrize("G,M,N,K", [
    (3, 150, 131, 100),      # ragged tiles, K not a multiple of the 32-wide chunk
    (2, 32, 32, 64),         # the smallest sides the bf16 tiles take
    (2, 31, 64, 40),         # one side below 32: the fp32 tiles
    (2, 64, 31, 33),
])
def test_gemm_bf16_vs_rounded_fp64(G, M, N, K, ak, bk):
    from torch_scae_amd import ops
    bf16 = M >= 32 and N >= 32
    # leading dimensions and batch strides that forbid 16-byte accesses, then ones that
    # allow them where the sizes do
    for pad, gap in (((3, 5, 2), (7, 1, 2)), ((4, 8, 4), (4, 8, 4))):
        p = _Gemm(G * M + N + K, G, M, N, K, ak, bk, pad=pad, gap=gap)
        with _spy() as calls, ops.mfma_bf16():
            p.launch_single()
        assert calls == ["scae_gemm_bf16"], calls
        p.check(bf16, f"plain {pad} {gap}")
    # every epilogue: bias, ReLU, mask gate; asum (k-strided A only)
    p = _Gemm(K, G, M, N, K, ak, bk, bias=True, relu=True, mask=True, asum=not ak)
    with _spy() as calls, ops.mfma_bf16():
        p.launch_single()
    assert calls == ["scae_gemm_bf16"], calls
    p.check(bf16, "bias+relu+mask+asum")


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_gemm_multi_bf16_vs_rounded_fp64(n):
    from torch_scae_amd import ops
    shapes = [(3, 150, 131, 100, False, False, dict(bias=True, asum=True)),
              (2, 64, 96, 77, True, True, dict(relu=True, mask=True, craw=True)),
              (4, 40, 128, 130, True, False, dict(bias=True, relu=True)),
              (1, 256, 33, 64, False, True, dict(mask=True))]
    probs = [_Gemm(17 * i + n, *s[:6], **s[6]) for i, s in enumerate(shapes[:n])]
    descs = (ops._lib.GemmDesc * n)(*[p.desc for p in probs])
    with _spy() as calls, ops.mfma_bf16():
        ops._lib.call(ops._prec("scae_gemm_multi_f32"), descs, n, ops._stream(probs[0].c))
    assert calls == ["scae_gemm_multi_bf16"], calls
    for i, p in enumerate(probs):
        p.check(True, f"multi {n}: problem {i}")
    # one problem with a side below 32: the whole list takes the fp32 tiles
    small = _Gemm(5, 2, 31, 70, 50, False, True, bias=True)
    descs = (ops._lib.GemmDesc * 2)(probs[0].desc, small.desc)
    probs[0].c.fill_(float("nan"))
    probs[0].asum.fill_(float("nan"))
    with _spy() as calls, ops.mfma_bf16():
        ops._lib.call(ops._prec("scae_gemm_multi_f32"), descs, 2, ops._stream(small.c))
    assert calls == ["scae_gemm_multi_bf16"], calls
    probs[0].check(False, "multi fallback: problem 0")
    small.check(False, "multi fallback: problem 1")


@pytest.mark.parametrize("second", [(2, 96, 40, 70, True, False),      # bf16 tiles
                                    (2, 96, 31, 70, True, False)])     # fp32 fallback
def test_gemm_pair_bf16_vs_rounded_fp64(second):
    from torch_scae_amd import ops
    first = _Gemm(1, 2, 40, 70, 96, False, False, asum=True, bias=True)     # weight gradient
    other = _Gemm(2, *second, relu=True, mask=True, craw=True)              # data gradient
    with _spy() as calls, ops.mfma_bf16():
        ops._gemm_pair(first.desc, other.desc, first.c)
    assert calls == ["scae_gemm_pair_bf16"], calls
    bf16 = second[2] >= 32
    first.check(bf16, "pair: first")
    other.check(bf16, "pair: second")


def test_gemm_bf16_at_configs2_mlp_sizes():
    """configs[2] (B = 1024): a capsule MLP layer 256 -> 128 as the forward
    (x W^T), the data gradient (g W) and the weight gradient with its bias sum (g^T x)
    take them -- K up to 1024.  8 groups rather than the 64 object capsules: the per-group
    M, N and K, and so the tiles, are configs[2]'s; the group count only repeats them."""
    from torch_scae_amd import ops
    G, B, Kin, N = 8, 1024, 256, 128
    dense = dict(pad=(0, 0, 0), gap=(0, 0, 0))
    fwd = _Gemm(1, G, B, N, Kin, True, True, bias=True, relu=True, **dense)
    dgrad = _Gemm(2, G, B, Kin, N, True, False, mask=True, **dense)
    wgrad = _Gemm(3, G, N, Kin, B, False, False, asum=True, **dense)
    with _spy() as calls, ops.mfma_bf16():
        fwd.launch_single()
        ops._gemm_pair(wgrad.desc, dgrad.desc, fwd.c)
    assert calls == ["scae_gemm_bf16", "scae_gemm_pair_bf16"], calls
    fwd.check(True, "cfg2 forward")
    dgrad.check(True, "cfg2 data gradient")
    wgrad.check(True, "cfg2 weight gradient")


# --------------------------------------------------------------------------------------
# K2 QKV attention: scae_qkv_attention_fwd_bf16 + its (fp32) backward
# --------------------------------------------------------------------------------------
def _bitwise_where_clean(got, ref, err, what, min_clean=MIN_CLEAN):
    """bf16 ``got`` equals rne(ref) wherever ref is not within ``err`` of a bf16 rounding
    midpoint (at least ``min_clean`` of the entries), and lies between rne(ref - err) and
    rne(ref + err) everywhere (rounding is monotone)."""
    clean = ~E.near_midpoint(ref, err)
    frac = float(clean.double().mean())
    print(f"{what}: {frac:.4f} of {clean.numel()} entries compared bitwise")
    assert frac >= min_clean, (what, frac)
    g = got.double().cpu()
    bad = clean & (g != E.rne(ref))
    assert not bool(bad.any()), (what, int(bad.sum()), float((g - ref)[bad].abs().max()))
    assert bool(((E.rne(ref - err) <= g) & (g <= E.rne(ref + err))).all()), what


@pytest.mark.parametrize("HB,N,M,dk,dv,pres", [
    (64, 64, 48, 256, 256, "mixed"),     # output attention of cfg-3 (O=64, M=48)
    (64, 48, 48, 16, 16, "mixed"),       # SAB of cfg-3
    (5, 33, 17, 70, 130, "mixed"),       # ragged, multi-chunk
    (7, 1, 1, 3, 5, None),               # degenerate
])
def test_qkv_attention_bf16_vs_rounded_fp64(HB, N, M, dk, dv, pres):
    """Forward: the logits of exact bf16 operands accumulate in fp32; the fp32 softmax
    ``probs`` (saved for the backward) within their derived bound; out = rne(probs) V
    (imposed rounding of the kernel's own probabilities), rounded to bf16.  Backward: the
    fp32 kernel on the upcast operands and the saved probabilities; gq, gk, gv rounded to
    bf16.  Every bf16 output equals the rounded reference bitwise where it is clear of a
    rounding midpoint."""
    from torch_scae_amd import ops
    g = torch.Generator().manual_seed(HB * 1000 + N)
    bf = torch.bfloat16
    q = torch.randn(HB, N, dk, generator=g).to(bf)
    k = torch.randn(HB, M, dk, generator=g).to(bf)
    v = torch.randn(HB, M, dv, generator=g).to(bf)
    gout = torch.randn(HB, N, dv, generator=g).to(bf)
    p = None
    if pres == "mixed":
        p = torch.ones(HB, M)
        p[:, ::3] = torch.rand(HB, len(range(0, M, 3)), generator=g)
        p[0] = 1.0
    qg, kg, vg = (t.cuda().requires_grad_(True) for t in (q, k, v))
    with _spy() as calls:
        og = ops.qkv_attention(qg, kg, vg, None if p is None else p.cuda())
        probs = og.grad_fn.saved_tensors[3].cpu()       # (freed by the backward)
        og.backward(gout.cuda())
    assert calls == ["scae_qkv_attention_fwd_bf16", "scae_qkv_attention_bwd_f32"], calls
    assert og.dtype == bf and probs.dtype == torch.float32
    sqrt_dk = float(np.float32(np.sqrt(dk)))

    out, p_ref, out_err, p_err = E.qkv_attention_fwd(q, k, v, p, probs=probs,
                                                     round=E.rne, sqrt_dk=sqrt_dk)
    dp = (probs.double() - p_ref).abs()
    assert bool((dp <= p_err).all()), ("probs", float((dp - p_err).max()))
    _bitwise_where_clean(og.detach(), out, out_err, "out")
    grads, errs = E.qkv_attention_bwd(q, k, v, probs, gout, sqrt_dk)
    for name, got, ref, err in zip(("gq", "gk", "gv"), (qg.grad, kg.grad, vg.grad), grads, errs):
        assert got.dtype == bf
        # (one key: dS = P (dP - P dP) is exactly zero, gq and gk are round-off around 0)
        floor = MIN_CLEAN if name == "gv" else 0.0 if M == 1 else MIN_CLEAN_DS
        _bitwise_where_clean(got, ref, err, name, floor)


# --------------------------------------------------------------------------------------
# K2c output attention: scae_seed_attention_mfma_fwd/bwd_bf16, ..._bwd_gemm_bf16
# --------------------------------------------------------------------------------------
TIGHT = 1e-5          # an entry is held tightly when its bound is <= TIGHT x its tensor's max
# out and gh: least share of entries held tightly.  One tainted probability loosens its
# whole query row of out, one tainted dS its whole key row of gh (0.4 % of P and 3.5 % of
# dS tainted leave 48 % of out and 33 % of gh tight at configs[2]'s 48 x 64, measured)
MIN_TIGHT_SEED = 0.3


def _seed_inputs(B, N, O, C, pres, seed):
    """h, bk, bv and the presence random; q, wk, wv and gout in {-1/4, 0, 1/4}.  The two
    C-long fp32 products the kernel rounds without writing out, qk = q wk and dT = gout wv,
    are then multiples of 1/16 far below 16 in magnitude: exact in fp32 in any order and
    exact in bf16, so no rounding of theirs is ambiguous (a C-long fp32 sum of random
    operands lies near a bf16 midpoint in a third of its entries, and qk is shared by every
    set).  What the kernel rounds of its own -- h, P, dS -- stays arbitrary."""
    D = 16
    g = torch.Generator().manual_seed(seed)
    tern = lambda *shape: torch.randint(-1, 2, shape, generator=g).float() / 4  # noqa: E731
    h = torch.randn(B, N, D, generator=g)
    q = tern(O, C)
    wk, wv = tern(C, D), tern(C, D)
    bk, bv = torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.3
    p = None
    if pres == "rand":
        p = torch.rand(B, N, generator=g)
    elif pres == "mixed":
        p = torch.ones(B, N)
        p[:, ::3] = torch.rand(B, len(range(0, N, 3)), generator=g)
    gout = tern(B, O, C)
    return h, q, wk, bk, wv, bv, p, gout


def _within(got, ref, err, what, floor):
    """Every entry within its bound; prints and floors the share of entries held tightly."""
    d = (got.double().cpu() - ref).abs()
    scale = float(ref.abs().max())
    tight = float((err <= TIGHT * scale).double().mean())
    print(f"{what}: {tight:.4f} of {d.numel()} entries held to <= {TIGHT:g} of max; "
          f"max |err| / bound {float((d / err.clamp_min(1e-300)).max()):.3g}")
    assert bool((d <= err).all()), (what, int((d > err).sum()), float((d - err).max()))
    assert tight >= floor, (what, tight)


@pytest.mark.parametrize("B,N,O,C,pres", [
    (128, 24, 24, 256, "mixed"),    # cfg-2
    (1024, 48, 64, 256, "mixed"),   # configs[2]: 48 keys, 64 queries, B = 1024
    (130, 48, 64, 256, "rand"),     # ragged B (the workgroups loop over sets)
    (4, 40, 24, 256, "mixed"),      # three key tiles
    (5, 1, 3, 64, None),            # one key
])
def test_seed_attention_bf16_vs_rounded_fp64(B, N, O, C, pres):
    """Forward and backward of the output attention with bf16 products against
    ``bf16_emulate.seed_attention``: h is rounded exactly as the kernel rounds it; qk, P,
    dT and dS carry their rounding step where they are tainted (near a midpoint).  Every
    entry of out, gh, gq, gwk, gwv, gbv within its bound, gbk exactly zero."""
    from torch_scae_amd import ops
    h, q, wk, bk, wv, bv, p, gout = _seed_inputs(B, N, O, C, pres, B * 7 + N)
    ins = [t.cuda().requires_grad_() for t in (h, q, wk, bk, wv, bv)]
    with _spy() as calls, ops.mfma_bf16():
        out = ops.seed_attention(*ins, None if p is None else p.cuda())
        out.backward(gout.cuda())
    assert calls == ["scae_seed_attention_mfma_fwd_bf16", "scae_seed_attention_mfma_bwd_bf16",
                     "scae_seed_attention_mfma_reduce_f32"], calls
    inv = float(np.float32(1.0) / np.sqrt(np.float32(C)))
    vals, errs, taints = E.seed_attention(h, q, wk, wv, bv, p, gout, inv, round=E.rne,
                                          exact_folds=True)
    print(", ".join(f"{k} tainted {float(t.double().mean()):.4f}" for k, t in taints.items()))
    assert not taints["qk"].any() and not taints["dT"].any()     # (exact by construction)
    got = dict(out=out.detach(), gh=ins[0].grad, gq=ins[1].grad, gwk=ins[2].grad,
               gwv=ins[4].grad, gbv=ins[5].grad)
    # (gq, gwk, gwv, gbv: sums over the batch in fp32, whose bound grows with B * O: held to
    # it entry by entry, without a floor)
    for name in ("out", "gh", "gq", "gwk", "gwv", "gbv"):
        _within(got[name], vals[name], errs[name], name,
                MIN_TIGHT_SEED if name in ("out", "gh") else 0.0)
    assert not bool(ins[3].grad.any())
    # the bf16 products really ran: the fp32 reference is off somewhere
    plain, _, _ = E.seed_attention(h, q, wk, wv, bv, p, gout, inv)
    assert bool(((got["out"].double().cpu() - plain["out"]).abs() > errs["out"]).any())


def test_seed_attention_bwd_gemm_bf16_vs_rounded_fp64():
    """scae_seed_attention_mfma_bwd_gemm_bf16: the output attention's backward with the
    capsule MLPs' weight-gradient GEMMs (32 x 32 fp32 tiles) as its tail.  Its attention
    part must equal scae_seed_attention_mfma_bwd_bf16 bit for bit (held to the rounded
    reference above, and checked against it here too); its GEMMs meet the fp32 bar."""
    from torch_scae_amd import _lib, ops
    B, N, O, C = 128, 24, 24, 256
    h, q, wk, bk, wv, bv, p, gout = _seed_inputs(B, N, O, C, "mixed", 5)
    dev = [t.cuda() for t in (h, q, wk, wv, p, gout)]
    rows = _lib.load().scae_seed_attention_mfma_rows(B)
    res = []
    for merged in (True, False):
        gh = torch.full((B, N, 16), float("nan"), device="cuda")
        part = torch.full((rows, O * 16 + C * 16 + C), float("nan"), device="cuda")
        args = [ops._p(t) for t in dev] + [ops._p(gh), ops._p(part), B, N, O, C]
        gemms = [_Gemm(11, 3, 24, 70, 96, False, False, asum=True),
                 _Gemm(12, 2, 40, 16, 50, False, True, bias=True)]
        descs = (_lib.GemmDesc * 2)(*[g.desc for g in gemms])
        with _spy() as calls:
            if merged:
                _lib.call("scae_seed_attention_mfma_bwd_gemm_bf16", *args, descs, 2,
                          ops._stream(gh))
            else:
                _lib.call("scae_seed_attention_mfma_bwd_bf16", *args, ops._stream(gh))
        torch.cuda.synchronize()
        if merged:
            for i, g in enumerate(gemms):
                g.check(False, f"bwd_gemm: GEMM {i}")
        res.append((gh.cpu(), part.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    inv = float(np.float32(1.0) / np.sqrt(np.float32(C)))
    vals, errs, _ = E.seed_attention(h, q, wk, wv, bv, p, gout, inv, round=E.rne,
                                     exact_folds=True)
    _within(res[0][0], vals["gh"], errs["gh"], "bwd_gemm: gh", MIN_TIGHT_SEED)
