"""tests/k1_ref.py, the fp64 reference of the part decoder (K1), held against the oracle run in
fp64 and against fp64 autograd; the constants C_OUT / C_GRAD measured from the fp32 oracle's
own distance to it; and the case list held against the forms the library's dispatch can take.
CPU only (the dispatch query launches nothing).  Run with -s for the measured figures."""
import ctypes
import functools

import pytest
import torch

from oracle import scae_oracle as O
from tests import k1_ref as R

CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]
GRAD_CASES = [c for c in CASES if "B" in c["checks"]]
GRAD_IDS = [R.case_id(c) for c in GRAD_CASES]
SCALARS = ("bg_value", "bg_mixing_logit", "temperature_logit", "scale")


@functools.lru_cache(maxsize=4)
def _case(name):
    c = next(c for c in CASES if c["name"] == name)
    ins, HW = R.checked_case(c)
    return c, ins, HW


def _oracle(c, ins, HW, dtype, grads=None):
    """O.image_decoder + O.gmm_log_prob in ``dtype`` -> outputs, and with ``grads`` the
    gradients of sum(g_logprob log_prob) or of sum(g_tt tt) + sum(g_ml ml) by autograd"""
    B, M, C = c["B"], c["M"], c["C"]
    th, tw = c["ts"]
    need = grads is not None
    cv = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(need)  # noqa: E731
    lv = {k: cv(ins[k]) for k in ("templates", "pose", "presence", "bg_image", "alpha") + SCALARS}
    P = {"d." + k: lv[k] for k in SCALARS if lv[k] is not None}
    if lv["alpha"] is not None:
        P["d.templates_alpha"] = lv["alpha"].view(1, M, 1, th, tw)
    templates = lv["templates"]
    if c["repeat"] > 1:
        templates = templates.repeat_interleave(c["repeat"], 0)
    cfg = dict(output_size=HW, learn_output_scale=c["scale"], use_alpha_channel=c["alpha"])
    r = O.image_decoder(P, "d", templates, lv["pose"], lv["presence"], lv["bg_image"], cfg)
    x = ins["x"].to(dtype)
    sigma = r.scale.to(dtype)
    lp = O.gmm_log_prob(r.transformed_templates, sigma, r.mixing_logits, x)
    out = dict(tt=r.transformed_templates.flatten(3), ml=r.mixing_logits.flatten(3),
               log_prob=lp.flatten(2), mean=O.gmm_mean(r.transformed_templates,
                                                        r.mixing_logits).flatten(2))
    if not need:
        return {k: v.detach() for k, v in out.items()}, None
    if grads.get("g_logprob") is not None:
        tot = (lp * grads["g_logprob"].to(dtype)).sum()
    else:
        tot = 0.0
        if grads.get("g_tt") is not None:
            tot = tot + (r.transformed_templates * grads["g_tt"].to(dtype)).sum()
        if grads.get("g_ml") is not None:
            tot = tot + (r.mixing_logits * grads["g_ml"].to(dtype)).sum()
    names = [k for k, v in lv.items() if v is not None]
    gs = torch.autograd.grad(tot, [lv[k] for k in names], allow_unused=True)
    g = {k: (torch.zeros_like(lv[k]) if v is None else v).detach() for k, v in zip(names, gs)}
    return {k: v.detach() for k, v in out.items()}, g


def _summed(ref, mag, c):
    """the reference's per-(image, component) partials summed the way autograd of the shared
    parameters sums them -> {oracle leaf name: (gradient, companion)}"""
    out = dict(templates=(ref["templates"], mag["templates"]), pose=(ref["pose"], mag["pose"]))
    if "alpha_partial" in ref:
        out["alpha"] = (ref["alpha_partial"].sum(0), mag["alpha_partial"].sum(0))
    for k in ("presence", "bg_image"):
        if k in ref:
            out[k] = (ref[k], mag[k])
    for i, k in enumerate(SCALARS):
        out[k] = (ref["scalar_partial"][:, :, i].sum().reshape(1),
                  mag["scalar_partial"][:, :, i].sum().reshape(1))
    return out


def _grad_sets(c):
    g = R.make_grads(c)
    sets = [("g_logprob", dict(g_logprob=g["g_logprob"]))]
    if "U" in c["checks"]:
        sets += [("g_tt", dict(g_tt=g["g_tt"])), ("g_ml", dict(g_ml=g["g_ml"])),
                 ("g_tt+g_ml", dict(g_tt=g["g_tt"], g_ml=g["g_ml"]))]
    return sets


@pytest.mark.parametrize("name", IDS)
def test_forward_equals_the_oracle_in_fp64(name):
    c, ins, HW = _case(name)
    want = ("tt", "ml", "log_prob", "mean") if c["B"] * c["M"] < 3000 else ("log_prob",)
    ref = R.forward(ins, HW, want=want)
    out, _ = _oracle(c, ins, HW, torch.float64)
    for k in want:
        r = R.ratio(out[k], ref[k], ref["m_" + k], 1.0) * R.U     # in units of the companion
        assert r <= 1e-12, (k, r)


@pytest.mark.parametrize("name", GRAD_IDS)
def test_closed_form_gradients_equal_fp64_autograd_and_the_oracle(name):
    c, ins, HW = _case(name)
    for what, gs in _grad_sets(c):
        ref, mag = R.backward(ins, HW, gs)
        auto = R.autograd_backward(ins, HW, gs)
        assert set(auto) == set(ref)
        for k in ref:
            r = R.ratio(auto[k], ref[k], mag[k], 1.0) * R.U
            assert r <= 1e-12, (what, k, r)
        _, g = _oracle(c, ins, HW, torch.float64, gs)
        for k, (val, m) in _summed(ref, mag, c).items():
            if k not in g:
                assert float(val.abs().max()) == 0.0, (what, k)
                continue
            r = R.ratio(g[k], val, m, 1.0) * R.U
            assert r <= 1e-12, (what, "oracle", k, r)


@pytest.mark.parametrize("name", ["wave-ragged-C3", "classic-ks4-pad"])
def test_tile_sums_equal_the_per_pixel_sums(name):
    c, ins, HW = _case(name)
    ref = R.forward(ins, HW, want=("log_prob",))
    P = HW[0] * HW[1]
    for ppb in (64, 192, P):
        tiles = -(-P // ppb)
        s, m = R.tile_sums(ref["log_prob"], ref["m_log_prob"], tiles, ppb)
        for t in range(tiles):
            direct = ref["log_prob"][:, :, t * ppb:(t + 1) * ppb].sum((1, 2))
            assert float((s[:, t] - direct).abs().max()) <= 1e-12 * float(m[:, t].max())
        g_tile = torch.randn(c["B"], tiles)
        g = R.spread_tiles(g_tile, ppb, c["C"], P)
        assert float(((g * ref["log_prob"]).sum((1, 2)) - (g_tile.double() * s).sum(1)).abs().max()) \
            <= 1e-10 * float(m.sum(1).max())


def test_constants_come_from_the_fp32_oracle():
    """the fp32 oracle's worst distance to the reference, per kind, over every case; the
    constants of k1_ref.py are 4 x the worst (rounded up) and the oracle stays within them"""
    worst_out = {k: 0.0 for k in R.MEASURED_OUT}
    worst_grad = {k: 0.0 for k in R.MEASURED_GRAD}
    for c in CASES:
        _, ins, HW = _case(c["name"])
        big = c["B"] * c["M"] >= 3000
        want = ("log_prob",) if big else ("tt", "ml", "log_prob", "mean")
        ref = R.forward(ins, HW, want=want)
        out, _ = _oracle(c, ins, HW, torch.float32)
        for k in want:
            worst_out[k] = max(worst_out[k], R.ratio(out[k], ref[k], ref["m_" + k], 1.0))
        P = HW[0] * HW[1]
        s, m = R.tile_sums(ref["log_prob"], ref["m_log_prob"], -(-P // 64), 64)
        s32 = torch.nn.functional.pad(out["log_prob"], (0, s.shape[1] * 64 - P)) \
            .reshape(c["B"], c["C"], -1, 64).sum((1, 3))
        worst_out["tile_sums"] = max(worst_out["tile_sums"], R.ratio(s32, s, m, 1.0))
        if "B" not in c["checks"]:
            continue
        for what, gs in _grad_sets(c):
            refg, mag = R.backward(ins, HW, gs)
            _, g = _oracle(c, ins, HW, torch.float32, gs)
            for k, (val, mm) in _summed(refg, mag, c).items():
                if k not in g:
                    continue
                kind = "scalars" if k in SCALARS else k
                worst_grad[kind] = max(worst_grad[kind], R.ratio(g[k], val, mm, 1.0))
    print("fp32 oracle, worst |err| / (2^-24 magnitude):")
    print("  outputs  ", {k: round(v, 2) for k, v in worst_out.items()})
    print("  gradients", {k: round(v, 2) for k, v in worst_grad.items()})
    for k, v in worst_out.items():
        assert v <= R.C_OUT[k], (k, v)
        assert v <= 1.25 * R.MEASURED_OUT[k] + 0.05, (k, v, "re-measure MEASURED_OUT")
        # (rounding up to one digit adds less than one unit of that digit)
        assert 4 * R.MEASURED_OUT[k] <= R.C_OUT[k] < 4 * R.MEASURED_OUT[k] * 2
    for k, v in worst_grad.items():
        assert v <= R.C_GRAD[k], (k, v)
        assert v <= 1.25 * R.MEASURED_GRAD[k] + 0.05, (k, v, "re-measure MEASURED_GRAD")
        assert 4 * R.MEASURED_GRAD[k] <= R.C_GRAD[k] < 4 * R.MEASURED_GRAD[k] * 2


def test_cell_gather_moment_terms_of_the_companion():
    """``backward(..., moments=True)``: the same gradients; the texel companions grow by exactly
    sum_pixels |g| {1 + fx + fy + fx fy, fx + fx fy, fy + fx fy, fx fy} per corner (restated
    here pixel by pixel), nothing else changes"""
    c, ins, HW = _case("wave-ragged-C3")
    g = dict(g_tt=R.make_grads(c)["g_tt"])        # (the incoming gradient is the pixel's g itself)
    ref, mag = R.backward(ins, HW, g)
    ref2, mag2 = R.backward(ins, HW, g, moments=True)
    for k in ref:
        assert torch.equal(ref[k], ref2[k])
        if k not in ("templates", "alpha_partial"):
            assert torch.equal(mag[k], mag2[k])
    B, M, C = c["B"], c["M"], c["C"]
    th, tw = c["ts"]
    H, W = HW
    extra = torch.zeros(B, M, C, th, tw, dtype=torch.float64)
    gt = g["g_tt"].double()
    pose = ins["pose"].double()
    for b in range(B):
        for m in range(M):
            a = pose[b, m]
            for i in range(H):
                for j in range(W):
                    xn, yn = (2 * j + 1) / W - 1, (2 * i + 1) / H - 1
                    ix = float(((a[0] * xn + a[1] * yn + a[2] + 1) * tw - 1) / 2)
                    iy = float(((a[3] * xn + a[4] * yn + a[5] + 1) * th - 1) / 2)
                    x0, y0 = int(ix // 1), int(iy // 1)
                    fx, fy = ix - x0, iy - y0
                    terms = ((0, 0, 1 + fx + fy + fx * fy), (1, 0, fx + fx * fy),
                             (0, 1, fy + fx * fy), (1, 1, fx * fy))
                    for dx, dy, t in terms:
                        if 0 <= x0 + dx < tw and 0 <= y0 + dy < th:
                            extra[b, m, :, y0 + dy, x0 + dx] += gt[b, m, :, i, j].abs() * t
    got = mag2["templates"] - mag["templates"]
    assert float((got - extra).abs().max()) <= 1e-12 * float(extra.max())
    assert float(extra.max()) > 0


# ------------------------------------------------------------------------------------- forms
def forms(c, fused, tt_offset=0, base=4096):
    """scae_render_gmm_forms for a case's shape (host only: the addresses only say which
    optional inputs exist and how the render's outputs are aligned)"""
    from torch_scae_amd import _lib
    P = ctypes.c_void_p
    d = _lib.DecoderDesc(P(base), P(base) if c["alpha"] else None, P(base),
                         P(base) if c["presence"] is not None else None,
                         P(base) if c["bg_image"] else None, P(base), P(base), P(base),
                         P(base) if c["scale"] else None, c["B"], c["M"], c["C"], c["ts"][0],
                         c["ts"][1], c["HW"][0], c["HW"][1], c["repeat"])
    out = (ctypes.c_int * 12)()
    rc = _lib.load().scae_render_gmm_forms(ctypes.byref(d), fused, P(base + tt_offset), P(base),
                                           out)
    assert rc == 0, rc
    return dict(fwd=(out[0], out[1], out[2]), render=out[3], bwd=out[4], gather_rows=out[5],
                chunk_rows=out[6], ppb=out[7], item_budget=out[8], max_items=out[9])


def assert_forms(c):
    """the forms a case names are the ones the library takes for its shape"""
    f, u = forms(c, 1), forms(c, 0)
    assert f["fwd"] == c["fwd"] and f["render"] == c["render"], (c["name"], f)
    if c["bwd"] is not None:
        assert f["bwd"] == c["bwd"] and u["bwd"] == c["bwd_unfused"], (c["name"], f, u)
    for k in ("ppb", "chunk_rows", "gather_rows"):
        if k in c:
            assert f[k] == c[k], (c["name"], k, f)


@pytest.mark.parametrize("name", IDS)
def test_every_case_takes_the_forms_it_names(name):
    assert_forms(next(c for c in CASES if c["name"] == name))


def test_the_case_list_covers_every_form_the_dispatch_can_report():
    fwd = {c["fwd"] for c in CASES if "F" in c["checks"]}
    assert fwd == {(R.WAVE, 1, 0)} | {(R.CLASSIC, ks, pad) for ks in (1, 2, 4) for pad in (0, 1)}
    render = {c["render"] for c in CASES if "R" in c["checks"]}
    assert render == {R.WAVE, R.CLASSIC}
    fused = {c["bwd"] for c in CASES if "B" in c["checks"]}
    unfused = {c["bwd_unfused"] for c in CASES if "U" in c["checks"]}
    assert fused == {R.CELL, R.SCATTER, R.GATHER}
    assert unfused == {R.SCATTER, R.GATHER}       # (the cell-gather form is fused only)
    # the sub-forms: one and two row chunks of the cell-gather, one and two passes of the gather,
    # both sides of the 4-wave-workgroup rule, the misaligned render
    chunks = {forms(c, 1)["chunk_rows"] < c["HW"][0] for c in CASES if c["bwd"] == R.CELL}
    passes = {forms(c, 1)["gather_rows"] < c["HW"][0] for c in CASES if c["bwd"] == R.GATHER}
    assert chunks == {False, True} and passes == {False, True}
    c = next(c for c in CASES if c["name"] == "wave-1wave-tiles")
    assert forms(c, 1, tt_offset=4)["render"] == R.CLASSIC
    # the template's cells, (th + 1)(tw + 1), below and above the cell-gather's item budget
    by = {c["name"]: c for c in CASES}
    f = forms(by["cell-5x6-template"], 1)
    assert 6 * 7 < f["item_budget"] == f["max_items"]
    f = forms(by["cell-17x17-template"], 1)
    assert 18 * 18 == f["max_items"] > f["item_budget"]


def test_collapsed_poses_split_a_cell_over_more_than_six_lanes():
    """A host restatement of the cell-gather's split of a cell over P = S x G lanes
    (render_gmm_wave_dev.h, phase 2: L = item budget / cells reached, S = min(L, rows of a cell,
    64) row slices): in ``cell-collapsed`` every capsule that reaches the template puts a chunk's
    pixels into at most four cells, each spanning at least seven of the chunk's rows, so S alone
    exceeds the 6 parts beyond which the four-to-one part folding runs."""
    c = next(c for c in CASES if c["name"] == "cell-collapsed")
    ins, HW = R.checked_case(c)
    f = forms(c, 1)
    H, W = HW
    th, tw = c["ts"]
    geo = R._geometry(ins["pose"].double(), HW, c["ts"])
    cx, cy = torch.floor(geo["ix"]), torch.floor(geo["iy"])            # (B,M,P)
    inside = (cx >= -1) & (cx < tw) & (cy >= -1) & (cy < th)
    folded = total = 0
    for r0 in range(0, H, f["chunk_rows"]):
        sl = slice(r0 * W, min(H, r0 + f["chunk_rows"]) * W)
        for b in range(c["B"]):
            for m in range(c["M"]):
                ok = inside[b, m, sl]
                if not bool(ok.any()):
                    continue
                ids = (cy[b, m, sl] * 1000 + cx[b, m, sl])[ok]
                rows = (torch.arange(sl.start, sl.stop) // W)[ok]
                cells = ids.unique()
                L = max(f["item_budget"] // len(cells), 1)
                rows_cell = max(len(rows[ids == k].unique()) for k in cells)
                total += 1
                folded += min(L, rows_cell, 64) > 6
                assert len(cells) <= 4
    assert total >= 16 and folded == total, (folded, total)
    assert {c.get("ppb") for c in CASES if c["name"].startswith("wave-B")} == {256, 448}
