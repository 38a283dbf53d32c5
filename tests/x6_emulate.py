"""Test infrastructure: fp64 references for the exact-split fp32 kernels (csrc/bf16x6.h).

The K8 convolutions (conv_fwd_pipe_kernel, K8r, the PipeW / PipeW16 weight-gradient tiles,
the DMODE 4 / 5 data-gradient tiles) and gemm_ksplit.hip multiply fp32 operands on the bf16
matrix cores.  Each operand x is cut into three bf16 planes by the kernel's own arithmetic

    hi = x & 0xffff0000,  r = x - hi (exact),  mid = r & 0xffff0000,  lo = r - mid (exact),

and a product a b is taken as the six partial products of weight >= 2^-16, in kind order

    KINDS = hi hi | hi mid, mid hi | hi lo, mid mid, lo hi.

Each partial product is a product of two 8-bit values: exact in fp32 and in fp64.  ``hi hi``
goes into the tile's accumulator; the five small kinds go into an accumulator of their own;
the two meet in one fp32 addition at the end of the K loop.

Kernel-model reference.  ``ref = sum over the six kinds`` of the exact partial products,
summed in fp64 (few nonzero terms per entry in the operand families of the tests: exact).
What the kernels drop (mid lo, lo mid, lo lo) is below 2^-23 of |a b| and is NOT in the
reference, so the bound need not carry it.

Bound (u = 2^-23, as in bf16_emulate: one ulp per fp32 addition, any faithful rounding).
For one output entry with n nonzero products a_k b_k, each issued by a different MFMA
(the operand families place an entry's terms in different 32-deep K chunks, asserted by
the tests), let S_hh = sum |hi_a hi_b| and S_sm = sum over the five small kinds of |p|.
  * the tile accumulator adds n exact products in sequence: gamma(n) S_hh;
  * the small accumulator adds 5 n exact products (K8r: into NS accumulators summed at the
    end, NS - 1 more additions of partial sums): gamma(5 n + 2) S_sm;
  * ``acc + accl``: one rounding, u (S_hh + S_sm);
  * x further sums of partial results: the KS wave groups of PipeC2 through LDS (1), the
    four wave-private pipelines of DMODE 5 / gemm_ksplit / K8r (3), the split-K partials
    summed by the reduce kernel (splits - 1): each partial is bounded by its own S, so
    these add gamma(x) (S_hh + S_sm);
  * an epilogue bias b: u (|value| + |b|), per bias added (``extra``).
By (1 + theta_j)(1 + theta_k) = 1 + theta_(j + k) (Higham, lemma 3.3) this is at most

    gamma(n + 1 + x + extra) S_hh + gamma(5 n + 3 + x + extra) S_sm + gamma(extra) |b|.

ReLU and the gate are 1-Lipschitz and select: the bound carries.

A missing kind moves an entry by |that kind's products|: hi mid / mid hi about 2^-8 |a b|,
hi lo / mid mid / lo hi about 2^-16 |a b| -- against a single-term entry's bound of about
(2 + x) 2^-23 |a b| that is a factor of 2^7 / (2 + x) or more (``test_x6_emulate``).

Forms on fp32 MFMAs (v_mfma_f32_16x16x4_f32: the first-generation data-gradient tiles
DMODE 0 - 2 of conv_mfma.hip, gemm_mfma.hip's tiles) and the image layer's fmaf loops take
the exact fp64 product a b as the reference and the plain bound gamma(2 n + extra) sum |a b|:
one rounding for each product and one for each addition.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -23
KINDS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))   # (plane of a, plane of b)
KIND_NAMES = ("hi.hi", "hi.mid", "mid.hi", "hi.lo", "mid.mid", "lo.hi")
SMALL_ORDER = (3, 5, 4, 1, 2)   # issue order into the small accumulator: hi lo, lo hi, mid mid,
                                # hi mid, mid hi (mfma_pipe.h, bf16x6.h)


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------- the split
def split3(x):
    """fp32 tensor -> (hi, mid, lo) fp32 tensors, by bf16x6.h's arithmetic: mask, exact
    difference, mask, exact difference (not bit fields: a value whose middle mantissa bits
    are zero has a mid that holds what bit fields would call lo)."""
    x = x.float().contiguous()
    mask = torch.tensor(-65536, dtype=torch.int32)            # 0xffff0000
    hi = (x.view(torch.int32) & mask).view(torch.float32)
    r1 = x - hi
    mid = (r1.view(torch.int32) & mask).view(torch.float32)
    lo = r1 - mid
    return hi, mid, lo


def bf16_bits(p):
    """fp32 plane (exact in bf16) -> its bf16 bit patterns as int32 (the high half)."""
    return (p.float().contiguous().view(torch.int32) >> 16) & 0xFFFF


def significant_bits(x):
    """number of significant bits of each fp32 value (0 for zero), exactly."""
    x = x.double().abs()
    m, e = torch.frexp(x)
    out = torch.zeros(x.shape, dtype=torch.int64)
    for b in range(25):   # smallest b with m 2^b an integer
        exact = (torch.ldexp(m, torch.full_like(e, b)).frac() == 0) & (out == 0) & (x > 0)
        out[exact] = b
    return out


# ---------------------------------------------------------------- kind-by-kind products
def planes3(x):
    """-> (3, ...) fp64 stack of the planes of fp32 x."""
    return torch.stack([p.double() for p in split3(x)])


def kind_terms(op, a, b, fp32=False):
    """op(A, B): a bilinear map of fp64 tensors that takes stacked planes (leading dim 3 on
    each side) to all nine plane products, leading dims (3, 3).  -> dict with
      P:   (6, ...) the kinds' sums (KINDS order),
      S:   (6, ...) the kinds' sums of |products|,
      n:   (...)    the number of nonzero products,
      ab:  (...)    sum |a b| on the unsplit operands (fp32-MFMA forms' bound),
      ex:  (...)    the exact fp64 product of the unsplit operands.
    fp32: only n, ab and ex (the fp32-MFMA forms)."""
    one = lambda t: (t != 0).double()[None]
    n = op(one(a), one(b))[0, 0]
    ex = op(a.double()[None], b.double()[None])[0, 0]
    ab = op(a.double().abs()[None], b.double().abs()[None])[0, 0]
    if fp32:
        return dict(n=n, ex=ex, ab=ab)
    pa, pb = planes3(a), planes3(b)
    full = op(pa, pb)
    absf = op(pa.abs(), pb.abs())
    P = torch.stack([full[i, j] for i, j in KINDS])
    S = torch.stack([absf[i, j] for i, j in KINDS])
    return dict(P=P, S=S, n=n, ex=ex, ab=ab)


def x6_ref(t, x=0, extra=0, bias=None):
    """The kernel-model value (the six kinds, + bias) and its bound (module docstring)."""
    ref = t["P"].sum(0)
    n = t["n"]
    bound = gamma(n + 1 + x + extra) * t["S"][0] + gamma(5 * n + 3 + x + extra) * t["S"][1:].sum(0)
    if bias is not None:
        ref = ref + bias
        bound = bound + gamma(extra) * bias.abs()
    return ref, bound


def fp32_ref(t, extra=0, bias=None):
    """The fp32-MFMA / fmaf forms: exact product, gamma(2 n + extra) sum |a b|."""
    ref, bound = t["ex"], gamma(2 * t["n"] + extra) * t["ab"]
    if bias is not None:
        ref = ref + bias
        bound = bound + gamma(extra) * bias.abs()
    return ref, bound


# ------------------------------------------- the convolutions / GEMMs as all-plane maps
# NHWC fp32 tensors as the kernels hold them; planes stacked in a leading dim of 3.
def op_fwd(stride):
    """out[b, oh, ow, co] = sum x[b, .., ci] w[co, ci, kh, kw]  (a = x (3, B, H, W, Ci),
    b = w (3, Co, Ci, 3, 3)) -> (3, 3, B, OH, OW, Co)."""
    def op(x3, w3):
        p, B, H, W, C = x3.shape
        q, Co = w3.shape[:2]
        xx = x3.reshape(p * B, H, W, C).permute(0, 3, 1, 2)
        ww = w3.reshape(q * Co, C, 3, 3)
        o = F.conv2d(xx, ww, stride=stride)                    # (pB, qCo, OH, OW)
        o = o.view(p, B, q, Co, *o.shape[2:]).permute(0, 2, 1, 4, 5, 3)
        return o
    return op


def op_dgrad(stride, in_hw):
    """din[b, ih, iw, ci] = sum dpre[b, oh, ow, co] w[co, ci, kh, kw]  (a = dpre
    (3, B, OH, OW, Co), b = w (3, Co, Ci, 3, 3)) -> (3, 3, B, IH, IW, Ci)."""
    def op(d3, w3):
        p, B, OH, OW, Co = d3.shape
        q, _, Ci = w3.shape[:3]
        dd = d3.reshape(p * B, OH, OW, Co).permute(0, 3, 1, 2)
        ww = w3.permute(1, 0, 2, 3, 4).reshape(Co, q * Ci, 3, 3)
        o = torch.nn.grad.conv2d_input((p * B, q * Ci, *in_hw), ww, dd, stride=stride)
        return o.view(p, B, q, Ci, *in_hw).permute(0, 2, 1, 4, 5, 3)
    return op


def op_wgrad(stride):
    """dW[co, ci, kh, kw] = sum dpre[b, oh, ow, co] x[b, .., ci]  (a = dpre (3, B, OH, OW, Co),
    b = x (3, B, H, W, Ci)) -> (3, 3, Co, Ci, 3, 3)."""
    def op(d3, x3):
        p, B, OH, OW, Co = d3.shape
        q, _, H, W, Ci = x3.shape
        dd = d3.permute(1, 0, 4, 2, 3).reshape(B, p * Co, OH, OW)
        xx = x3.permute(1, 0, 4, 2, 3).reshape(B, q * Ci, H, W)
        o = torch.nn.grad.conv2d_weight(xx, (p * Co, q * Ci, 3, 3), dd, stride=stride)
        return o.view(p, Co, q, Ci, 3, 3).permute(0, 2, 1, 3, 4, 5)
    return op


def op_gemm(a3, b3):
    """C[g, m, n] = sum_k A[g, m, k] B[g, n, k]  (a (3, G, M, K), b (3, G, N, K))."""
    return torch.einsum("pgmk,qgnk->pqgmn", a3, b3)


# ------------------------------------------------------------------- operand families
def full_mantissa(g, shape, span=8, lo_zero=0.0):
    """fp32 values with a full 24-bit mantissa (all three planes nonzero), random signs,
    magnitudes 2^[-span, span).  lo_zero: fraction whose lo (or mid) plane is exactly zero."""
    e = torch.randint(-span, span, shape, generator=g).double()
    m = 1.0 + torch.rand(shape, generator=g, dtype=torch.float64)
    x = (m * torch.ldexp(torch.ones(shape, dtype=torch.float64), e.long())).float()
    bits = x.view(torch.int32)
    bits |= 1 | (1 << 8) | (1 << 15)          # a set bit in each plane's part of the mantissa
    if lo_zero > 0:
        pick = torch.rand(shape, generator=g) < lo_zero
        which = torch.rand(shape, generator=g) < 0.5
        bits = torch.where(pick & which, bits & ~0xFF, bits)                 # lo = 0
        bits = torch.where(pick & ~which, bits & ~0xFF00 | (1 << 7), bits)   # middle byte 0
    x = bits.view(torch.float32)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return x * sign


def sparse_rows(g, R, K, chunk=32, max_terms=4, span=8, lo_zero=0.0):
    """(R, K) fp32 matrix: row r has 1 .. max_terms nonzeros, at most one per `chunk`-wide
    block of K, in blocks and positions that differ from row to row (every block and every
    position inside a block is used across the rows)."""
    nb = K // chunk
    assert nb >= 1
    out = torch.zeros(R, K)
    vals = full_mantissa(g, (R, max_terms), span, lo_zero)
    for r in range(R):
        cnt = 1 + (r * 7 + int(torch.randint(0, 4, (1,), generator=g))) % min(max_terms, nb)
        blocks = torch.randperm(nb, generator=g)[:cnt]
        for j, b in enumerate(blocks.tolist()):
            pos = (r * 5 + 11 * j + b) % chunk
            out[r, b * chunk + pos] = vals[r, j]
    return out


def max_per_chunk(X, chunk=32):
    """largest number of nonzeros of X (.., K) in one aligned `chunk` block of its last dim."""
    K = X.shape[-1]
    Kp = (K + chunk - 1) // chunk * chunk
    Xp = torch.zeros(*X.shape[:-1], Kp)
    Xp[..., :K] = (X != 0).float()
    return int(Xp.view(*X.shape[:-1], Kp // chunk, chunk).sum(-1).max())


# ------------------------------------------------------ float32 emulation of the K loop
def emulate_gemm(A, B, kinds=KINDS, tile_kinds=(0,), zero=(), chunk=16, splits=1):
    """float32 emulation of one exact-split tile: C = A B^T for A (M, K), B (N, K) fp32.
    Per 16-deep MFMA group (in K order) each kind's group product (fp64 sum of exact partial
    products -- at most one nonzero per entry in the tests' operand families -- rounded once,
    as an MFMA adds into its accumulator) goes into the tile accumulator if its index is in
    ``tile_kinds``, else into the small accumulator, in the loops' issue order; at the end
    acc + accl, one rounding.  ``splits`` > 1: K cut into that many contiguous parts, each its
    own pair of accumulators, the parts' results summed in fp32 in order.
    Mutations: ``kinds`` (a list of (plane a, plane b); drop one, or name the wrong plane),
    ``zero`` ({'a.lo', 'b.mid', ..}: a plane lost), ``tile_kinds`` (a kind moved)."""
    pa, pb = [p.double() for p in split3(A)], [p.double() for p in split3(B)]
    names = ("hi", "mid", "lo")
    for z in zero:
        side, plane = z.split(".")
        lst = pa if side == "a" else pb
        lst[names.index(plane)] = torch.zeros_like(lst[0])
    M, K = A.shape
    N = B.shape[0]
    order = [i for i in SMALL_ORDER if i < len(kinds)] + [i for i in range(len(kinds))
                                                            if i not in SMALL_ORDER]
    per = (K + splits - 1) // splits
    total = torch.zeros(M, N, dtype=torch.float32)
    for s in range(splits):
        acc = torch.zeros(M, N, dtype=torch.float32)
        accl = torch.zeros(M, N, dtype=torch.float32)
        for k0 in range(s * per, min(K, (s + 1) * per), chunk):
            k1 = min(k0 + chunk, (s + 1) * per, K)
            for idx in order:
                i, j = kinds[idx]
                p = pa[i][:, k0:k1] @ pb[j][:, k0:k1].T
                if idx in tile_kinds:
                    acc = (acc.double() + p).float()
                else:
                    accl = (accl.double() + p).float()
        part = (acc.double() + accl.double()).float()
        total = part if s == 0 else (total.double() + part.double()).float()
    return total


def im2col(x, stride):
    """NHWC x (B, H, W, C) -> (B*OH*OW, 9*C) in the forward's K order (tap-major, ci inner)."""
    B, H, W, C = x.shape
    OH, OW = (H - 3) // stride + 1, (W - 3) // stride + 1
    cols = [x[:, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride, :]
            for kh in range(3) for kw in range(3)]
    return torch.stack(cols, 3).reshape(B * OH * OW, 9 * C)


def filter_rows(w):
    """(Co, Ci, 3, 3) -> Wf (Co, 9*Ci): the forward's B operand, tap-major."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)



# ------------------------------------------------- sparse convolution operands (NHWC)
def sparse_pixels(g, B, H, W, C, per_block=32, p=0.35, span=8, lo_zero=0.0):
    """(B, H, W, C): each pixel holds one nonzero channel with probability p -- at most one
    nonzero per pixel and K chunk of a forward / data gradient whatever the taps."""
    x = torch.zeros(B * H * W, C)
    on = torch.rand(B * H * W, generator=g) < p
    ch = torch.randint(0, C, (B * H * W,), generator=g)
    v = full_mantissa(g, (B * H * W,), span, lo_zero)
    x[on, ch[on]] = v[on]
    return x.view(B, H, W, C)


def sparse_dpre(g, B, OH, OW, Co, max_terms=4, span=8, lo_zero=0.0):
    """(B, OH, OW, Co) pre-activation gradient for a weight gradient AND a data gradient at
    once: channel co has 1 .. max_terms nonzero pixels, in different 32-pixel blocks of the
    flattened (b, oh, ow) index (the weight gradient's K chunks), and no pixel holds more than
    one nonzero (so a data-gradient chunk of 32 channels sees at most one)."""
    M = B * OH * OW
    nb = M // 32
    assert nb >= 1
    d = torch.zeros(M, Co)
    free = [list(torch.randperm(32, generator=g).tolist()) for _ in range(nb)]
    vals = full_mantissa(g, (Co, max_terms), span, lo_zero)
    for co in torch.randperm(Co, generator=g).tolist():
        cnt = 1 + (co * 3 + int(torch.randint(0, 4, (1,), generator=g))) % max_terms
        for j, b in enumerate(torch.randperm(nb, generator=g).tolist()):
            if j >= cnt:
                break
            if free[b]:
                d[b * 32 + free[b].pop(), co] = vals[co, j]
    return d.view(B, OH, OW, Co)


def sparse_input(g, B, H, W, Ci, stride, max_terms=4, span=8, lo_zero=0.0):
    """(B, H, W, Ci) input for a weight gradient AND a forward at once: channel ci has
    1 .. max_terms nonzero pixels, no pixel more than one, and for every tap no 32-pixel
    block of output pixels reads two of the same channel (each dW entry's terms are in
    different K chunks)."""
    OH, OW = (H - 3) // stride + 1, (W - 3) // stride + 1
    x = torch.zeros(B, H, W, Ci)
    used, slots = set(), set()
    vals = full_mantissa(g, (Ci, max_terms), span, lo_zero)
    for ci in torch.randperm(Ci, generator=g).tolist():
        cnt = 1 + (ci * 3 + int(torch.randint(0, 4, (1,), generator=g))) % max_terms
        got = 0
        for flat in torch.randperm(B * H * W, generator=g)[:64].tolist():
            if got == cnt:
                break
            b, r = divmod(flat, H * W)
            ih, iw = divmod(r, W)
            if (b, ih, iw) in used:
                continue
            new = []
            for kh in range(3):
                for kw in range(3):
                    dh, dw = ih - kh, iw - kw
                    if dh < 0 or dw < 0 or dh % stride or dw % stride:
                        continue
                    oh, ow = dh // stride, dw // stride
                    if oh >= OH or ow >= OW:
                        continue
                    new.append((kh * 3 + kw, ci, ((b * OH + oh) * OW + ow) // 32))
            if not new or any(s in slots for s in new):
                continue
            slots.update(new)
            used.add((b, ih, iw))
            x[b, ih, iw, ci] = vals[ci, got]
            got += 1
    return x


def sparse_filter(g, Co, Ci, side, max_terms=4, span=8, lo_zero=0.0):
    """(Co, Ci, 3, 3) filter with 1 .. max_terms nonzeros per row of the operand a pass
    reads, one per 32-deep K chunk: side 'fwd': rows Wf[co] = (tap, ci); 'dgrad': rows
    Wd[ci] = (tap, co)."""
    if side == "fwd":
        r = sparse_rows(g, Co, 9 * Ci, 32, max_terms, span, lo_zero)
        return r.view(Co, 3, 3, Ci).permute(0, 3, 1, 2).contiguous()
    r = sparse_rows(g, Ci, 9 * Co, 32, max_terms, span, lo_zero)
    return r.view(Ci, 3, 3, Co).permute(3, 0, 1, 2).contiguous()


def chunk_counts_ok(x_nhwc, w, dpre, stride):
    """The families' premise, checked on the operands: every output entry of the forward,
    data gradient and weight gradient has at most one nonzero product per 32-deep K chunk.
    (x, w, dpre: any may be dense; a pass is checked if one of its operands is sparse
    enough -- returns the passes for which the premise holds.)"""
    ok = set()
    Co, Ci = w.shape[:2]
    wf = filter_rows(w)                                   # (Co, 9 Ci)
    wd = w.permute(1, 2, 3, 0).reshape(Ci, 9 * Co)        # (Ci, 9 Co)
    if max_per_chunk(wf) <= 1 or (x_nhwc is not None and max_per_chunk(x_nhwc) <= 1):
        ok.add("fwd")
    if max_per_chunk(wd) <= 1 or (dpre is not None and max_per_chunk(dpre) <= 1):
        ok.add("dgrad")
    if dpre is not None and x_nhwc is not None:
        M = dpre.shape[0] * dpre.shape[1] * dpre.shape[2]
        if max_per_chunk(dpre.reshape(M, -1).T.contiguous()) <= 1:
            ok.add("wgrad")
        else:
            cols = im2col(x_nhwc, stride).view(M, 9, Ci)
            if all(max_per_chunk(cols[:, t].T.contiguous()) <= 1 for t in range(9)):
                ok.add("wgrad")
    return ok


NO_TILE, NO_KSPLIT, TILE = 1, 2, 4      # scae_hip.h's SCAE_DGRAD_* bits


def dgrad_mode(B, IH, IW, Ci, Co, stride, pair, forms=0):
    """conv_mfma.hip's plan_dgrad restated (the tap-class tables of dgrad_axis and the
    tile-count thresholds SCAE_DGX_MIN_TILES = 500, SCAE_DGK_DEFAULT, SCAE_SMALL_TILES =
    SCAE_PAIR_SMALL_TILES = 1024, SCAE_PAIR_WIDE_MIN = 600): the data-gradient form a layer
    takes.  forms: the dgrad_forms argument (a set of the bits above, 0 = by shape)."""
    OH, OW = (IH - 3) // stride + 1, (IW - 3) // stride + 1
    dgx = 0 if forms & NO_TILE else 1 if forms & TILE else 500
    dgk = not forms & NO_KSPLIT

    def classes(I, O):
        def taps(i):
            return sum(1 << k for k in range(3)
                       if i - k >= 0 and (i - k) % stride == 0 and (i - k) // stride < O)
        key = (lambda i: taps(i)) if stride == 1 else (lambda i: i % stride)
        cnt = {}
        for i in range(I):
            cnt[key(i)] = cnt.get(key(i), 0) + 1
        return list(cnt.values())
    rc, cc = classes(IH, OH), classes(IW, OW)

    def tiles(T):
        return sum((B * a * b + T - 1) // T for a in rc for b in cc)
    if Ci % 128 == 0 and Co % 32 == 0 and dgx > 0 and (Ci // 128) * tiles(64) >= dgx:
        return 4
    if Ci % 64 == 0 and Co % 32 == 0 and dgk:
        return 5
    t64, t32 = (Ci // 64) * tiles(64), (Ci // 64) * tiles(32)
    if pair:
        return 0 if t64 >= 1024 else (2 if t32 >= 600 else 1)
    return 0 if t64 >= 1024 else (2 if t32 >= 600 else 1)
