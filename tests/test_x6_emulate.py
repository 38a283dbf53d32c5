"""tests/x6_emulate.py checked on the CPU: the split, the operand families, and the teeth of
the bound -- a float32 emulation of the exact-split K loop passes it, and each way of losing a
product kind fails it by a factor of 4 or more on the operand draws the GPU tests use."""
import pytest
import torch

from tests import x6_emulate as E


def _draws():
    g = torch.Generator().manual_seed(11)
    yield "full", E.full_mantissa(g, (1 << 16,))
    yield "zero planes", E.full_mantissa(g, (1 << 16,), lo_zero=0.5)
    bits = torch.randint(-(1 << 31), (1 << 31) - 1, (1 << 16,), generator=g, dtype=torch.int64)
    x = bits.to(torch.int32).view(torch.float32)
    yield "random bits", x[torch.isfinite(x) & ((x == 0) | (x.abs() >= 2.0 ** -100))]


@pytest.mark.parametrize("what,x", list(_draws()))
def test_split3_is_exact_and_each_plane_fits_bf16(what, x):
    hi, mid, lo = E.split3(x)
    # hi + mid + lo == x, bit for bit (the sums are exact: no rounding anywhere)
    assert torch.equal(((hi + mid) + lo).view(torch.int32), x.view(torch.int32)), what
    assert torch.equal((hi.double() + mid.double() + lo.double()).float(), x)
    for p in (hi, mid, lo):
        assert int(E.significant_bits(p).max()) <= 8, what
        assert torch.equal(p.to(torch.bfloat16).float(), p), what      # exact in bf16
        # the bf16 pattern the kernel keeps (the high half of the fp32 pattern) is the value
        back = (E.bf16_bits(p) << 16).to(torch.int32).view(torch.float32)
        assert torch.equal(back, p), what
    # the planes are ordered: |mid| < ulp(hi), |lo| < ulp-range of mid (2^-16 of |x|, about)
    nz = x != 0
    assert bool((mid.abs() <= x.abs() * 2.0 ** -7)[nz].all())
    assert bool((lo.abs() <= x.abs() * 2.0 ** -15)[nz].all())


def test_split3_is_arithmetic_not_bit_fields():
    # 1 + 2^-20: middle mantissa byte zero -> mid takes the bit bit-fields would put in lo
    x = torch.tensor([1.0 + 2.0 ** -20, 1.0 + 2.0 ** -9 + 2.0 ** -23], dtype=torch.float32)
    hi, mid, lo = E.split3(x)
    assert hi.tolist() == [1.0, 1.0]
    assert mid.tolist() == [2.0 ** -20, 2.0 ** -9]
    assert lo.tolist() == [0.0, 2.0 ** -23]


def test_full_mantissa_family():
    g = torch.Generator().manual_seed(1)
    x = E.full_mantissa(g, (4096,))
    hi, mid, lo = E.split3(x)
    assert bool((hi != 0).all() and (mid != 0).all() and (lo != 0).all())
    assert float(x.abs().min()) >= 2.0 ** -20 and float(x.abs().max()) <= 2.0 ** 20
    assert int(E.significant_bits(x).min()) == 24
    y = E.full_mantissa(g, (4096,), lo_zero=0.5)
    _, m2, l2 = E.split3(y)
    # half of them: lo = 0, either from a zero low byte or because mid took the low byte
    assert 1600 < int((l2 == 0).sum()) < 2500 and int((m2 == 0).sum()) == 0
    assert int((m2.abs() < y.abs() * 2.0 ** -15).sum()) > 600


def test_sparse_families_keep_one_term_per_chunk():
    g = torch.Generator().manual_seed(2)
    B, H, W, Ci, Co, s = 8, 9, 9, 128, 64, 1
    x = E.sparse_input(g, B, H, W, Ci, s)
    d = E.sparse_dpre(g, B, 7, 7, Co)
    wf, wd = E.sparse_filter(g, Co, Ci, "fwd"), E.sparse_filter(g, Co, Ci, "dgrad")
    dense = lambda *sh: E.full_mantissa(g, sh)
    assert E.chunk_counts_ok(x, dense(Co, Ci, 3, 3), dense(B, 7, 7, Co), s) >= {"fwd", "wgrad"}
    assert E.chunk_counts_ok(dense(B, H, W, Ci), dense(Co, Ci, 3, 3), d, s) >= {"dgrad", "wgrad"}
    assert "fwd" in E.chunk_counts_ok(None, wf, None, s)
    assert "dgrad" in E.chunk_counts_ok(None, wd, None, s)
    # every channel has 1 .. 4 terms where capacity allows, each nonzero a full mantissa
    per_ci = (x != 0).sum((0, 1, 2))
    assert int(per_ci.min()) >= 1 and int(per_ci.max()) <= 4
    per_co = (d != 0).sum((0, 1, 2))
    assert int(per_co.min()) >= 1 and int(per_co.max()) <= 4
    assert int((wf != 0).view(Co, -1).sum(1).max()) <= 4


def _gemm_cases():
    """The forward of test_x6_kernels_vs_fp64's first case as the GEMM the tile computes
    (im2col rows x filter rows), with the filter sparse and with the input sparse."""
    g = torch.Generator().manual_seed(3)
    B, H, W, Ci, Co, s = 3, 9, 9, 128, 64, 1
    x, w = E.full_mantissa(g, (B, H, W, Ci)), E.sparse_filter(g, Co, Ci, "fwd")
    yield "sparse filter", E.im2col(x, s), E.filter_rows(w)
    x, w = E.sparse_input(g, B, H, W, Ci, s), E.full_mantissa(g, (Co, Ci, 3, 3))
    yield "sparse input", E.im2col(x, s), E.filter_rows(w)
    x, w = E.full_mantissa(g, (B, H, W, Ci)), E.sparse_filter(g, Co, Ci, "fwd", lo_zero=0.5)
    yield "sparse filter, zero planes", E.im2col(x, s), E.filter_rows(w)


@pytest.mark.parametrize("what,A,Bm", list(_gemm_cases()))
def test_bound_has_teeth(what, A, Bm):
    """The emulated kernel passes the bound; every mutation that loses or misplaces a
    product kind exceeds it by >= 4 on its worst entry.  A kind moved from the small to
    the tile accumulator only changes which fp32 sum rounds it -- the same u per addition
    the bound already grants -- so no bound can see it; its ratio is printed and held
    below 1 (it is not a lost product)."""
    t = E.kind_terms(E.op_gemm, A[None], Bm[None])
    t = {k: v[:, 0] if k in ("P", "S") else v[0] for k, v in t.items()}
    ref, bound = E.x6_ref(t, x=1)             # PipeC2: the two wave groups meet in LDS
    ratio = lambda got: float(((got.double() - ref).abs() / bound).max())
    assert ratio(E.emulate_gemm(A, Bm)) <= 1.0
    assert ratio(E.emulate_gemm(A, Bm, splits=2)) <= 1.0
    muts = {}
    for k, name in enumerate(E.KIND_NAMES):
        kinds = [kd for j, kd in enumerate(E.KINDS) if j != k]
        tile = (0,) if k != 0 else ()
        muts[f"drop {name}"] = E.emulate_gemm(A, Bm, kinds=kinds, tile_kinds=tile)
    for z in ("a.lo", "a.mid", "b.lo", "b.mid"):
        muts[f"zero {z}"] = E.emulate_gemm(A, Bm, zero=(z,))
    # the operands' plane arrays confused: a kind read from the other operand's plane choice
    muts["hi.lo read as lo.hi"] = E.emulate_gemm(A, Bm, kinds=[E.KINDS[j] if j != 3 else (2, 0)
                                                              for j in range(6)])
    muts["hi.mid read as mid.hi"] = E.emulate_gemm(A, Bm, kinds=[E.KINDS[j] if j != 1 else (1, 0)
                                                                for j in range(6)])
    muts["mid.mid read as hi.mid"] = E.emulate_gemm(A, Bm, kinds=[E.KINDS[j] if j != 4 else (0, 1)
                                                                 for j in range(6)])
    # a kind in both accumulators (added to the tile's and kept in the small one)
    muts["hi.lo in both accumulators"] = E.emulate_gemm(
        A, Bm, kinds=list(E.KINDS) + [E.KINDS[3]], tile_kinds=(0, 6))
    print(f"\n{what}: kernel model {ratio(E.emulate_gemm(A, Bm)):.3f}")
    for name, got in muts.items():
        r = ratio(got)
        print(f"  {name:28s} worst |err| / bound {r:10.1f}")
        assert r >= 4.0, (what, name, r)
    for k in range(1, 6):
        r = ratio(E.emulate_gemm(A, Bm, tile_kinds=(0, k)))
        print(f"  {E.KIND_NAMES[k] + ' moved to the tile acc':28s} worst |err| / bound {r:10.3f}")
        assert r <= 1.0
