"""tests/tail_ref.py proven on the CPU: the fp64 reference is the oracle composition that
``test_loss_tail_vs_oracle`` uses, its hand-written restatement and backward are autograd's,
the constants of the bars come from the fp32 composition, the cases take every form and loop
edge of the kernels and satisfy the condition the comparison rests on, and the bars with these
cases see each of the mistakes this kernel's arithmetic invites (``tail_ref.MUTANTS``).
Run with -s for the measured ratios."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import scae_oracle as O
from tests import tail_ref as R

CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]
BY_ID = dict(zip(IDS, CASES))


@functools.lru_cache(maxsize=None)
def case(cid):
    ins, cfg = R.checked_case(BY_ID[cid])
    return ins, cfg, R.forward(ins, cfg)


# ----------------------------------------------------------------------- the reference is right
@pytest.mark.parametrize("prior,post,use_label,const", [
    ("l2", "entropy", True, None), ("entropy", "l2", True, 1.5), ("kl", "kl", False, None),
    ("l2", "l2", True, None)])
def test_forward_equals_the_composition_of_test_loss_tail_vs_oracle(prior, post, use_label, const):
    """tests/test_hip_ops.py::test_loss_tail_vs_oracle's own inputs and its own ``ref``, in fp64"""
    g = torch.Generator().manual_seed(3)
    B, Oc, M, ncls = 128, 24, 24, 10
    lpp = torch.randn(B, M, generator=g)
    post_full = torch.softmax(torch.randn(B, Oc + 1, M, generator=g), 1)
    cp = torch.rand(B, Oc, generator=g)
    cp[0, 0] = 0.0
    W = torch.randn(ncls, Oc, generator=g) * 0.3
    bb = torch.randn(ncls, generator=g) * 0.1
    label = torch.randint(0, ncls, (B,), generator=g)
    weights = [1.0, 2.0, 0.35, 0.7, 0.2]

    def ref(lpp, post_full, cp, W, bb):
        log_prob = lpp.sum() / B
        pw, pb = O.sparsity_loss(prior, cp, n_classes=ncls, within_example_constant=const)
        mass = post_full[:, :-1].sum(-1)
        qw, qb = O.sparsity_loss(post, mass / M, n_classes=ncls)
        tot = -weights[0] * log_prob + weights[1] * pw + weights[2] * pb \
            + weights[3] * qw + weights[4] * qb
        xe1 = xe2 = torch.zeros((), dtype=lpp.dtype)
        if use_label:
            p1 = torch.softmax(F.linear(cp.detach(), W, bb), -1)
            p2 = torch.softmax(F.linear(mass.detach(), W, bb), -1)
            xe1, xe2 = F.cross_entropy(p1, label), F.cross_entropy(p2, label)
            tot = tot + xe1 + xe2
        return torch.stack([tot, log_prob, pw, pb, qw, qb, xe1, xe2])

    lv = [t.double().requires_grad_(True) for t in (lpp, post_full, cp, W, bb)]
    want = ref(*lv)
    want[0].backward()
    ins = dict(lpp=lpp, posterior=post_full, caps_presence=cp, cls_w=W if use_label else None,
               cls_b=bb if use_label else None, label=label if use_label else None,
               rec_sums=None, reg=None)
    cfg = dict(prior=prior, post=post, weights=weights, within_const=const, n_classes_cfg=ncls,
               sparsity_on=True, w_reg=0.0)
    got = R.forward(ins, cfg)
    h = R.hand(ins, cfg, None, torch.tensor([1.0]))
    assert R.ratio(got[:8], want.detach(), h["m_out"][:8], 1e-12 / R.U) <= 1.0
    assert float(got[8]) == 0.0 and float(got[10]) == -float(got[1]) and float(got[11]) == 0.0
    gr = R.backward(ins, cfg, None, torch.tensor([1.0]))
    names = ("lpp", "posterior", "caps_presence") + (("cls_w", "cls_b") if use_label else ())
    for k, leaf in zip(names, lv):
        assert R.ratio(gr[k], leaf.grad, h["m_grads"][k], 1e-11 / R.U) <= 1.0, k
    # rec_sums, reg and w_reg as the ABI takes them
    rec, reg = torch.randn(B, 7, generator=g).flatten(), torch.rand(1, generator=g)
    got2 = R.forward(dict(ins, rec_sums=rec, reg=reg), dict(cfg, w_reg=0.37))
    rec_ll = rec.double().sum() / B
    assert abs(float(got2[0] - (got[0] - rec_ll + 0.37 * reg.double()[0]))) <= 1e-12 * 100
    assert float(got2[8]) == float(rec_ll) and float(got2[9]) == -float(rec_ll)
    assert float(got2[11]) == float(reg.double()[0])


@pytest.mark.parametrize("cid", IDS)
def test_hand_written_tail_and_backward_equal_the_oracle_and_autograd(cid):
    ins, cfg, ref = case(cid)
    h = R.hand(ins, cfg)
    assert R.ratio(h["out"], ref, h["m_out"], 1e-12 / R.U) <= 1.0
    assert bool((h["m_out"] >= h["out"].abs() * (1 - 1e-12)).all())
    worst = 0.0
    for name, go, gl in R.make_gouts(BY_ID[cid]):
        hb = R.hand(ins, cfg, go, gl)
        ag = R.backward(ins, cfg, go, gl)
        for k in R.GRAD_NAMES:
            if ag[k] is None:
                assert hb["grads"][k] is None, (name, k)
                continue
            r = R.ratio(hb["grads"][k], ag[k], hb["m_grads"][k], 1e-11 / R.U)
            worst = max(worst, r)
            assert r <= 1.0, (name, k, r)
            assert bool((hb["m_grads"][k] >= hb["grads"][k].abs() * (1 - 1e-12)).all()), (name, k)
    print(f"{cid}: worst |hand - autograd| / (1e-11 magnitude) {worst:.3g}")


# ------------------------------------------------------------------------------ the constants
def test_constants_come_from_the_fp32_oracle():
    """worst |fp32 composition - fp64| / (2^-24 magnitude) per kind over every case and every
    incoming gradient of the GPU module; ``tail_ref.C`` is 4 x the worst (rounded up to one
    digit) and the fp32 composition stays within it"""
    worst = {k: (0.0, "") for k in R.MEASURED}
    for cid in IDS:
        ins, cfg, ref = case(cid)
        m_out = R.hand(ins, cfg)["m_out"]
        o32 = R.compose(R.leaves(ins, torch.float32), cfg)
        for i, r in enumerate(R.out_ratios(o32, ref, m_out, unit=True)):
            if r > worst[R.OUT_KIND[i]][0]:
                worst[R.OUT_KIND[i]] = (r, f"{cid} {R.OUT_NAMES[i]}")
        for name, go, gl in R.make_gouts(BY_ID[cid]):
            want = R.backward(ins, cfg, go, gl)
            m = R.hand(ins, cfg, go, gl)["m_grads"]
            g32 = R.autograd(ins, cfg, go, gl, torch.float32)
            for k, r in R.grad_ratios(g32, want, m, unit=True).items():
                if r > worst[R.GRAD_KIND[k]][0]:
                    worst[R.GRAD_KIND[k]] = (r, f"{cid} {name} {k}")
    print("fp32 composition, worst |err| / (2^-24 magnitude):")
    for k, (v, where) in worst.items():
        print(f"  {k:12s} {v:.3f}  c = {R.C[k]:g}  ({where})")
    for k, (v, _) in worst.items():
        assert v <= R.C[k], (k, v)
        assert v <= 1.25 * R.MEASURED[k] + 0.05, (k, v, "re-measure MEASURED")
        # (rounding up to one digit adds less than one unit of that digit)
        assert 4 * R.MEASURED[k] <= R.C[k] < 4 * R.MEASURED[k] * 2, k
    assert set(R.OUT_KIND) | set(R.GRAD_KIND.values()) == set(R.C)


# ---------------------------------------------------------------------- the bars see mistakes
MUTANT_CASES = ["small-5x3x5x2-entropy-kl-benign-nrecB+5",
                "small-67x24x24x10-kl-kl-sparse-nrecB-3",
                "small-128x24x24x10-l2-l2-benign-nrec7B-wc",
                "small-128x24x24x10-entropy-entropy-sparse-nrec7B",
                "small-33x65x70x32-kl-l2-benign-nrecB-3",
                "large-210x24x24x10-l2-entropy-benign-nrecB+5",
                "large-131x70x5x10-entropy-entropy-cancelling-nrecB+5",
                "large-1030x3x5x2-l2-kl-benign-nrec7B"]


def _mutant_excess(mutant, cid):
    ins, cfg, ref = case(cid)
    mut = frozenset([mutant])
    good = R.hand(ins, cfg)
    worst, where = 0.0, ""
    bad = R.hand(ins, cfg, mut=mut)
    for i, r in enumerate(R.out_ratios(bad["out"], ref, good["m_out"])):
        if r > worst:
            worst, where = r, R.OUT_NAMES[i]
    for name, go, gl in R.make_gouts(BY_ID[cid]):
        want = R.backward(ins, cfg, go, gl)
        m = R.hand(ins, cfg, go, gl)["m_grads"]
        badg = R.hand(ins, cfg, go, gl, mut=mut)["grads"]
        for k, r in R.grad_ratios(badg, want, m).items():
            if r > worst:
                worst, where = r, f"grad {k} ({name})"
    return worst, where


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_bar_sees_the_mutant(mutant):
    best = (0.0, "", "")
    for cid in MUTANT_CASES:
        r, where = _mutant_excess(mutant, cid)
        if r > best[0]:
            best = (r, cid, where)
    print(f"mutant {mutant:24s} exceeds the bar {best[0]:.3g} x on {best[1]}: {best[2]}")
    assert best[0] >= 4.0, best


def test_the_reference_itself_is_no_mutant():
    assert set(MUTANT_CASES) <= set(IDS)
    for cid in MUTANT_CASES[:3]:
        ins, cfg, ref = case(cid)
        name, go, gl = R.make_gouts(BY_ID[cid])[-1]
        a, b = R.hand(ins, cfg, go, gl), R.hand(ins, cfg, go, gl, mut=frozenset())
        assert torch.equal(a["out"], b["out"])
        assert max(R.out_ratios(a["out"], ref, a["m_out"])) <= 1e-3


# ------------------------------------------------------------------------------------ coverage
def test_both_forms_meet_every_sparsity_type_and_all_nine_pairs_appear():
    on = [c for c in CASES if c["sparsity_on"]]
    for f in ("small", "large"):
        assert {c["prior"] for c in on if R.form(c) == f} == set(R.TYPES), f
        assert {c["post"] for c in on if R.form(c) == f} == set(R.TYPES), f
    assert {(c["prior"], c["post"]) for c in on} == {(p, q) for p in R.TYPES for q in R.TYPES}
    assert {c["regime"] for c in CASES} == set(R.REGIMES)
    assert {c["n_rec"] for c in CASES} == set(R.N_REC)
    assert any(not c["sparsity_on"] for c in CASES if R.form(c) == "small")
    assert any(not c["sparsity_on"] for c in CASES if R.form(c) == "large")
    # an explicit within_const together with an l2 posterior call, which must ignore it
    assert any(c["within_const"] is not None and c["post"] == "l2" and c["sparsity_on"]
               for c in CASES)
    assert any(c["within_const"] is not None and c["prior"] == "l2" for c in CASES)
    assert len(set(IDS)) == len(IDS) and 25 <= len(IDS) <= 35


def test_the_form_of_a_case_is_the_formula_of_the_library():
    # scae_loss_tail_defer_preferred: B B 2 O 4 <= 8 MiB; at O = 24 that is B <= 209
    assert R.defer_preferred(209, 24) and not R.defer_preferred(210, 24)
    for c, cid in zip(CASES, IDS):
        small = c["B"] * c["B"] * 2 * c["O"] * 4 <= 8 * 1024 * 1024
        assert cid.startswith("small-" if small else "large-")


def test_every_loop_edge_is_taken_by_a_case():
    def some(pred, f=None):
        return [R.case_id(c) for c in CASES if pred(c) and (f is None or R.form(c) == f)]
    B, Oc, M, K = (lambda c: c["B"]), (lambda c: c["O"]), (lambda c: c["M"]), (lambda c: c["ncls"])
    nt = lambda c: R.NT_SMALL if R.form(c) == "small" else R.NTC_LARGE    # noqa: E731
    edges = {
        # column_sums: lanes that never enter the unrolled loop, the boundary b + 48 < B from
        # both sides, a tail behind full passes; rounds of the 2 O 16 entries; both forms
        "colsum B < 16": some(lambda c: B(c) < 16),
        "colsum B = 63": some(lambda c: B(c) == 63),
        "colsum B = 64": some(lambda c: B(c) == 64),
        "colsum B = 67": some(lambda c: B(c) == 67),
        "colsum tail behind two passes": some(lambda c: B(c) > 128 and B(c) % 64 != 0),
        "colsum rounds, small": some(lambda c: 2 * Oc(c) * 16 > R.NT_SMALL, "small"),
        "colsum one round, small": some(lambda c: 2 * Oc(c) * 16 <= R.NT_SMALL, "small"),
        "colsum rounds, large combine": some(lambda c: 2 * Oc(c) * 16 > R.NTC_LARGE, "large"),
        "colsum rounds, large backward": some(lambda c: 2 * Oc(c) * 16 > R.NTB_LARGE, "large"),
        # tail_image_kernel
        "float4 rows": some(lambda c: M(c) % 4 == 0),
        "scalar rows": some(lambda c: M(c) % 4 != 0),
        "O > 64 lanes, small": some(lambda c: Oc(c) > 64, "small"),
        "O > 64 lanes, large": some(lambda c: Oc(c) > 64, "large"),
        "M > 64": some(lambda c: M(c) > 64),
        # cls_xe
        "dot tail (O % 4 != 0)": some(lambda c: Oc(c) % 4 != 0 and K(c) > 0),
        "dot without tail": some(lambda c: Oc(c) % 4 == 0 and K(c) > 0),
        "dot of the tail only (O < 4)": some(lambda c: Oc(c) < 4 and K(c) > 0),
        "ncls = 1": some(lambda c: K(c) == 1),
        "ncls = MAXCLS": some(lambda c: K(c) == R.MAXCLS),
        "no label": some(lambda c: K(c) == 0 and c["n_classes_cfg"] == 10, "small"),
        "no label, large": some(lambda c: K(c) == 0 and c["n_classes_cfg"] == 10, "large"),
        # tail_bwd_body: the classifier-gradient unroll (b + 12 < B) and its tail, several
        # classifier workgroups of 128 (small) and of 64 (large) outputs
        "cls grad B < 13": some(lambda c: B(c) < 13 and K(c) > 0),
        "cls grad unroll + tail": some(lambda c: B(c) > 16 and B(c) % 16 != 0 and K(c) > 0),
        "cls grad unroll, no tail": some(lambda c: B(c) % 16 == 0 and K(c) > 0),
        "cls blocks of 128": some(lambda c: K(c) * (Oc(c) + 1) > R.NT_SMALL // 4, "small"),
        "cls blocks of 64": some(lambda c: K(c) * (Oc(c) + 1) > R.NTB_LARGE // 4, "large"),
        # g_rec_sums: per = ceil(n_rec / B)
        "n_rec < B": some(lambda c: 1 < R.n_rec_of(c) < B(c)),
        "n_rec = 1": some(lambda c: R.n_rec_of(c) == 1 and B(c) > 1),
        "n_rec no multiple of B": some(lambda c: R.n_rec_of(c) > B(c) and R.n_rec_of(c) % B(c)),
        "n_rec = 7 B": some(lambda c: R.n_rec_of(c) == 7 * B(c) and B(c) > 1),
        "n_rec beyond the combine's stride": some(lambda c: R.n_rec_of(c) > nt(c)),
        # stride loops of the combine
        "B > 512, small": some(lambda c: B(c) > R.NT_SMALL, "small"),
        "B > 1024, large": some(lambda c: B(c) > R.NTC_LARGE, "large"),
        "B = 1": some(lambda c: B(c) == 1),
        "O = 1": some(lambda c: Oc(c) == 1),
        "first large B at O = 24": some(lambda c: B(c) == 210 and Oc(c) == 24, "large"),
    }
    for name, ids in edges.items():
        print(f"{name}: {ids[0] if ids else '-'}" + (f" (+{len(ids) - 1})" if len(ids) > 1 else ""))
    missing = [name for name, ids in edges.items() if not ids]
    assert not missing, missing


# ---------------------------------------------------------- the conditions hold for the cases
@pytest.mark.parametrize("cid", IDS)
def test_no_log_safe_argument_is_near_the_threshold(cid):
    ins, cfg, _ = case(cid)
    c = BY_ID[cid]
    q = R.log_safe_args(ins, cfg)
    assert bool(((q / R.EPS - 1).abs() > 2.0 ** -16).all())
    assert bool((ins["caps_presence"] >= 0).all()) and bool((ins["posterior"] >= 0).all())
    if c["ncls"] > 0:
        lab = ins["label"]
        assert int(lab.min()) == 0 and int(lab.max()) == c["ncls"] - 1
        assert int(lab[0]) == (0 if c["B"] > 1 else c["ncls"] - 1) and int(lab[-1]) == c["ncls"] - 1
    else:
        assert ins["label"] is None and ins["cls_w"] is None and c["n_classes_cfg"] == 10
    assert ins["rec_sums"].numel() == R.n_rec_of(c)


def test_the_regimes_are_what_they_say():
    sparse = [cid for cid in IDS if BY_ID[cid]["regime"] == "sparse"]
    assert len(sparse) >= 6
    floored = 0
    for cid in sparse:
        ins, cfg, _ = case(cid)
        c = BY_ID[cid]
        cp = ins["caps_presence"]
        mass = ins["posterior"][:, :c["O"]].double().sum(-1)
        assert bool((cp == 0).any()) and bool(((cp > 0) & (cp <= 1e-20)).any())
        assert bool((cp == 0).all(1).any())                           # a zero row: r = 0
        if c["O"] > 1:
            assert bool((cp == 0).all(0).any())                       # a zero column
        if c["O"] > 2:
            assert bool((mass == 0).all(0).any())                     # ... of the mass, too
        assert bool(((mass > 0) & (mass < 1e-18)).any())              # dummy-dominated: mass ~ 0
        if c["B"] > 3:
            assert bool((mass == 0).all(1).any())                     # an image without mass
        assert bool((mass.max(1)[0] >= 1.0).any())                    # one-hot posteriors
        q = R.log_safe_args(ins, cfg)
        floored += int((q < R.EPS).sum())
        assert bool((q < R.EPS).any()) and bool((q == 0).any())
    assert floored > 100
    # kl's k = O decides the floor for some entry: p < 1e-16 <= p O
    hit = False
    for cid in sparse:
        c = BY_ID[cid]
        if "kl" in (c["prior"], c["post"]):
            ins, cfg, _ = case(cid)
            a = R.hand(ins, cfg)["out"]
            b = R.hand(ins, cfg, mut=frozenset(["kl_k1"]))["out"]
            hit = hit or not torch.equal(a, b)
    assert hit
    for cid in IDS:
        c = BY_ID[cid]
        ins, cfg, ref = case(cid)
        if c["regime"] == "saturated":
            z = ins["caps_presence"].double() @ ins["cls_w"].double().t() + ins["cls_b"].double()
            assert 15 < float(z.abs().mean()) < 60
        if c["regime"] == "cancelling":
            assert float(ins["lpp"].mean()) < -9e3
            r = ins["rec_sums"]
            assert bool((r > 0).any()) and bool((r < 0).any())
            assert float(r.double().sum().abs()) < 0.5 * float(r.double().abs().sum())
