"""Part segmentation on the GPU: the fused E-step kernel (csrc/render_gmm_parts.hip) against
``segment_host`` in fp64 over the materialised mixture, prior ownership against the fused mode
kernel bit for bit, planted ties, reproducibility (runs, slices, streams), and the model-level
surface: ``segment``, ``part_owner``, ``EvalStep.segmentation_images``, ``part_usage``.

Measured on MI355X (test_parts_against_fp64, worst over each shape's 8 variants; e is the bar,
the other figures are distances from ``segment_host`` in fp64):

    shape        K   fp32 numpy   e (bar)   |conf - R64|   R64 max - R64[owner]   owners differing
    small        6   1.8e-7       1.67e-6   1.8e-7         0                      0 of 442
    tiles        6   1.8e-7       1.67e-6   1.8e-7         0                      0 of 3200
    chunked     25   3.2e-7       3.93e-6   3.2e-7         0                      0 of 800
    temperature  4   1.3e-7       1.43e-6   1.3e-7         0                      0 of 336

(mass: at most 0.007 of its bar.)
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, FIRST, COUNT = 4, 1, 2
SHAPES = {
    # 221 pixels: one partial round, dead lanes; odd sizes: the four-weighted-taps arithmetic
    "small": dict(M=5, C=1, th=11, tw=11, H=13, W=17, alpha=True),
    # 1600 pixels: 6.25 rounds over several tiles (the tile sum of mass); whole quads: the
    # quad-store render's arithmetic
    "tiles": dict(M=5, C=1, th=11, tw=11, H=40, W=40, alpha=True),
    # 24 templates of 3 + 1 padded planes: more than the staging budget holds at a time
    "chunked": dict(M=24, C=3, th=11, tw=11, H=20, W=20, alpha=True),
    # temperature mode: one logit per channel (Cm = C)
    "temperature": dict(M=3, C=2, th=6, tw=6, H=12, W=14, alpha=False),
}
VARIANTS = [(bg, pr, wx) for bg in (True, False) for pr in (True, False)
            for wx in (True, False)]
PALETTE_ROWS = 4                # fewer than the parts and capsules: ids wrap round
N_GROUPS = 7


def _inputs(name, bg_image, presence, dup=None):
    """Random compact decoder inputs on the device (poses at the scale at which a template
    covers a good part of the image, so that every component owns pixels), an observed image
    and an owner table.  ``dup`` = (i, j): template j is template i again, both favoured."""
    from torch_scae_amd import ops
    s = SHAPES[name]
    M, C, th, tw, H, W, alpha = (s[k] for k in ("M", "C", "th", "tw", "H", "W", "alpha"))
    g = torch.Generator().manual_seed(sorted(SHAPES).index(name) * 4 + 2 * bg_image + presence)
    r = lambda *sh: torch.rand(*sh, generator=g)          # noqa: E731
    rn = lambda *sh: torch.randn(*sh, generator=g)        # noqa: E731
    t = dict(templates=r(B, M, C, th, tw),
             templates_alpha=rn(1, M, 1, th, tw) * 2 if alpha else None,
             pose=torch.tensor([1.6, 0.0, 0.0, 0.0, 1.6, 0.0]) +
             rn(B, M, 6) * torch.tensor([0.4, 0.3, 0.5, 0.3, 0.4, 0.5]),
             presence=0.7 + 0.3 * r(B, M) if presence else None,
             bg_image=0.3 * r(B, C, H, W) if bg_image else None,
             bg_value=None if bg_image else rn(1) - 1.5,
             bg_mixing_logit=rn(1),
             temperature_logit=None if alpha else 0.3 * rn(1) - 1.5,
             out_scale=rn(1) if bg_image else None)        # (sigma != 1 in half the variants)
    x = r(B, C, H, W)
    table = torch.randint(0, N_GROUPS, (B, M), generator=g, dtype=torch.int32)
    if dup is not None:
        i, j = dup
        t["templates"][:, j] = t["templates"][:, i]
        t["pose"][:, j] = t["pose"][:, i]
        if alpha:
            t["templates_alpha"][0, i] += 3
            t["templates_alpha"][0, j] = t["templates_alpha"][0, i]
        if presence:
            t["presence"][:, j] = t["presence"][:, i]
    inputs = ops.DecoderInputs((H, W), **{k: None if v is None else v.cuda()
                                          for k, v in t.items()})
    return inputs, x.cuda(), table.cuda()


def _sigma(inputs):
    """The Normal scale the decoder gives its mixture (part_decoder.py:220-223), in fp64."""
    if inputs.out_scale is None:
        return 1.0
    return float(np.logaddexp(0.0, np.float64(inputs.out_scale.item()))) + 1e-4


@functools.lru_cache(maxsize=None)
def _case(name, bg_image, presence):
    """Inputs, the materialised mixture of the slice's images and the palette: made once and
    shared by the tests below, which leave them unchanged."""
    from torch_scae_amd import ops, segment
    inputs, x, table = _inputs(name, bg_image, presence)
    with torch.no_grad():
        tt, ml = ops.render_templates(inputs)
    sl = slice(FIRST, FIRST + COUNT)
    return dict(inputs=inputs, x=x, table=table, pal=segment.palette(PALETTE_ROWS).cuda(),
                loc=tt[sl].cpu().numpy(), ml=ml[sl].cpu().numpy(), sigma=_sigma(inputs))


@functools.lru_cache(maxsize=None)
def _host(name, bg_image, presence, with_x):
    """Per image of the slice: R in fp64 and in fp32 numpy, mass in fp64."""
    from torch_scae_amd.segment import segment_host
    c = _case(name, bg_image, presence)
    out = []
    for i in range(COUNT):
        x = c["x"][FIRST + i].cpu().numpy() if with_x else None
        s64, R64 = segment_host(c["loc"][i], c["ml"][i], c["sigma"], x=x)
        _, R32 = segment_host(c["loc"][i], c["ml"][i], c["sigma"], x=x, dtype=np.float32)
        out.append((R64, R32, s64))
    return out


def _run(c, with_x, first=FIRST, count=COUNT):
    from torch_scae_amd import ops
    return ops.render_gmm_parts(c["inputs"], x=c["x"] if with_x else None,
                                part_group=c["table"], palette=c["pal"], first=first,
                                count=count)


def test_the_chunked_shape_is_chunked_and_the_tiled_one_tiled():
    """From the launcher's own arithmetic (scae_render_gmm_parts_geometry): the chunked shape
    cannot pass on the one-stage path, the 40 x 40 one sums several tiles."""
    from torch_scae_amd import ops
    geo = {n: ops.render_gmm_parts_geometry(_case(n, False, True)["inputs"], COUNT)
           for n in SHAPES}
    print(geo)
    tiles, ppb, kchunk = geo["chunked"]
    assert kchunk < SHAPES["chunked"]["M"] and ppb == 256 and tiles == 2
    tiles, ppb, kchunk = geo["tiles"]
    assert kchunk == SHAPES["tiles"]["M"] and tiles == 7 and ppb == 256
    assert geo["small"] == (1, 256, 5)
    assert geo["temperature"][2] == 3


@pytest.mark.parametrize("bg_image,presence,with_x", VARIANTS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_parts_against_fp64(name, bg_image, presence, with_x):
    """conf, the owner and mass against ``segment_host`` in fp64 over the materialised
    mixture.  The bar e is the fp32 numpy restatement's own worst distance from fp64 on the
    same inputs times 4 (another summation order), at least (K + 8) 2^-23.  group and both
    coloured images follow exactly from the kernel's own ``part``.

    The module's docstring and DESIGN.md section 7 record the figures measured on MI355X;
    each case prints its own."""
    c = _case(name, bg_image, presence)
    s = SHAPES[name]
    M, C, H, W = s["M"], s["C"], s["H"], s["W"]
    K, HW = M + 1, H * W
    host = _host(name, bg_image, presence, with_x)
    out = _run(c, with_x)
    torch.cuda.synchronize()
    part, conf, mass = out.part.cpu().numpy(), out.conf.cpu().numpy(), out.mass.cpu().numpy()
    assert part.shape == (COUNT, H, W) and part.dtype == np.int32
    assert conf.shape == (COUNT, H, W) and mass.shape == (COUNT, K)
    assert part.min() >= 0 and part.max() <= M
    err32 = max(float(np.abs(R32.astype(np.float64) - R64).max()) for R64, R32, _ in host)
    e = max(4 * err32, (K + 8) * 2.0 ** -23)
    worst = dict(conf=0.0, owner=0.0, mass=0.0, differ=0)
    for i, (R64, _, s64) in enumerate(host):
        own = np.take_along_axis(R64, part[i][None].astype(np.int64), 0)[0]
        d_conf = np.abs(conf[i].astype(np.float64) - own)
        d_own = R64.max(0) - own
        d_mass = np.abs(mass[i].astype(np.float64) - s64.mass)
        worst["conf"] = max(worst["conf"], float(d_conf.max()))
        worst["owner"] = max(worst["owner"], float(d_own.max()))
        worst["mass"] = max(worst["mass"], float((d_mass / (HW * e + HW * 2.0 ** -24
                                                            * s64.mass)).max()))
        worst["differ"] += int((part[i] != s64.part).sum())
    print(f"{name} bg_image={bg_image} presence={presence} x={with_x}: K={K} "
          f"fp32 restatement err {err32:.3e}  e {e:.3e}  |conf-R64| {worst['conf']:.3e}  "
          f"R64max-R64[owner] {worst['owner']:.3e}  mass err / bar {worst['mass']:.3f}  "
          f"owners differing {worst['differ']} of {COUNT * HW}")
    for i, (R64, _, s64) in enumerate(host):
        own = np.take_along_axis(R64, part[i][None].astype(np.int64), 0)[0]
        assert np.abs(conf[i].astype(np.float64) - own).max() <= e
        # the kernel's owner is the fp64 owner, or as good as it within the bar: every pixel
        assert (R64.max(0) - own).max() <= e
        assert (np.abs(mass[i].astype(np.float64) - s64.mass)
                <= HW * e + HW * 2.0 ** -24 * s64.mass).all()
        assert len(np.unique(s64.part)) >= 3            # (the inputs exercise the arg-max)

    # group and the colours follow from the kernel's own part, exactly
    table, pal = c["table"].cpu().numpy(), c["pal"].cpu().numpy()
    group = out.group.cpu().numpy()
    for i in range(COUNT):
        bg = part[i] == M
        want_group = np.where(bg, -1, table[FIRST + i][np.minimum(part[i], M - 1)])
        assert np.array_equal(group[i], want_group)
        loc = c["loc"][i]                                   # (K, C, H, W) fp32
        at = np.take_along_axis(loc, part[i][None, None].astype(np.int64), 0)[0]
        tone = np.zeros((H, W), np.float32)
        for ch in range(C):
            tone = tone + at[ch]
        tone = tone * (np.float32(1) / np.float32(C))
        for rgb, ids in ((out.rgb_part, part[i]), (out.rgb_group, group[i])):
            got = rgb[i].cpu().numpy()
            want = np.where(bg[None], tone[None],
                            tone[None] * np.moveaxis(pal[ids % PALETTE_ROWS], -1, 0))
            assert got.shape == (3, H, W)
            assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()


@pytest.mark.parametrize("bg_image,presence", [(b, p) for b in (True, False)
                                               for p in (True, False)])
@pytest.mark.parametrize("name", ["small", "tiles", "chunked"])
def test_prior_ownership_is_the_modes_component(name, bg_image, presence):
    """Alpha mode, x=None: the responsibilities are the softmax of the mixing logits, so the
    owner is the component ``mode()`` picks -- both kernels take the first largest logit from
    the same arithmetic.  The materialised values gathered at ``part`` are the fused mode's
    image, bit for bit."""
    from torch_scae_amd import ops
    c = _case(name, bg_image, presence)
    part = _run(c, False).part.cpu().numpy().astype(np.int64)         # (COUNT, H, W)
    gathered = np.take_along_axis(c["loc"], part[:, None, None], 1)[:, 0]
    mode = ops.render_gmm_mode(c["inputs"], first=FIRST, count=COUNT).cpu().numpy()
    assert gathered.shape == mode.shape
    assert np.array_equal(gathered, mode)


@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("name,dup", [("tiles", (1, 2)), ("chunked", (1, 20)),
                                      ("temperature", (0, 2))])
def test_planted_ties_go_to_the_lower_index(name, dup, with_x):
    """Two identical templates with identical poses and presences have identical
    responsibilities: the lower index owns every pixel where they win, and their masses are
    equal bit for bit (on the chunked shape the twins are staged in different chunks)."""
    from torch_scae_amd import ops
    inputs, x, table = _inputs(name, False, True, dup=dup)
    out = ops.render_gmm_parts(inputs, x=x if with_x else None, part_group=table,
                               first=FIRST, count=COUNT)
    i, j = dup
    n_i, n_j = int((out.part == i).sum()), int((out.part == j).sum())
    print(f"{name}: template {i} owns {n_i} pixels, its twin {j} owns {n_j}")
    assert n_j == 0 and n_i >= 20
    assert torch.equal(out.mass[:, i], out.mass[:, j])
    assert float(out.mass[:, i].min()) > 0


@pytest.mark.parametrize("name", ["tiles", "chunked"])
def test_runs_slices_and_streams_give_the_same_bits(name):
    c = _case(name, True, True)
    a = _run(c, True)
    b = _run(c, True)
    for f, u, v in zip(a._fields, a, b):
        assert torch.equal(u, v), f
    # the whole batch against two half slices (another grid, another tile split at most)
    whole = _run(c, True, first=0, count=B)
    halves = [_run(c, True, first=0, count=B // 2), _run(c, True, first=B // 2, count=B // 2)]
    for f, u, v, w in zip(whole._fields, whole, *halves):
        assert torch.equal(u, torch.cat([v, w], 0)), f
    for f, u, v in zip(a._fields, a, whole):
        assert torch.equal(u, v[FIRST:FIRST + COUNT]), f
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = _run(c, True)
    side.synchronize()
    for f, u, v in zip(a._fields, a, s):
        assert torch.equal(u, v), f
    # mass is what the (count, tiles, K) partials say it is: about one per pixel in all
    HW = SHAPES[name]["H"] * SHAPES[name]["W"]
    assert abs(float(a.mass.double().sum(1).max()) - HW) <= 1e-4 * HW


def test_without_a_table_there_is_no_group_and_x_matters():
    from torch_scae_amd import ops
    c = _case("small", False, True)
    plain = ops.render_gmm_parts(c["inputs"], x=c["x"], first=FIRST, count=COUNT)
    assert plain.group is None and plain.rgb_group is None
    full = _run(c, True)
    assert torch.equal(plain.part, full.part) and torch.equal(plain.mass, full.mass)
    # (the default palette has M rows: another colouring of the same owners)
    assert tuple(plain.rgb_part.shape) == tuple(full.rgb_part.shape)
    prior = _run(c, False)
    assert not torch.equal(prior.conf, full.conf)


def _model(cfg, sd):
    from torch_scae_amd import factory
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(cfg)
    model.load_state_dict(sd)
    return model.cuda().train()


def test_model_level_segment_sheets_and_usage():
    from tests.test_hip_model import full_size_params
    from torch_scae_amd import EvalStep, _lib, ops, segment
    cfg, _, sd, g = full_size_params("cfg2")
    model = _model(cfg, sd)
    with torch.no_grad():
        # (at its initialisation the background owns every pixel: spread the alpha logits and
        # lower the background's, so that parts own pixels and the sheets have colours)
        model.part_decoder.templates_alpha.mul_(60.0)
        model.part_decoder.bg_mixing_logit.fill_(-6.0)
    C, H, W = cfg["image_shape"]
    M, O = cfg["n_part_caps"], cfg["n_obj_caps"]
    Bm, n = 6, 4
    image = torch.rand(Bm, C, H, W, generator=g).cuda()
    label = torch.randint(0, cfg["n_classes"], (Bm,), generator=g).cuda()
    step = EvalStep(model, Bm, cfg["image_shape"], use_graph=False)
    step(image, label)
    res = step._eager_result()

    # segment and part_owner
    owner = segment.part_owner(res)
    assert owner.dtype == torch.int32 and tuple(owner.shape) == (Bm, M)
    post = res.posterior_mixing_prob
    assert torch.equal(post.gather(1, owner.long()[:, None])[:, 0], post.amax(1))
    assert torch.equal(owner.long(), post.argmax(1))
    seg = segment.segment(res, image, first=1, count=3)
    assert tuple(seg.part.shape) == (3, H, W) and tuple(seg.rgb_group.shape) == (3, 3, H, W)
    assert int(seg.part.min()) >= 0 and int(seg.part.max()) <= M
    assert int(seg.group.min()) >= -1 and int(seg.group.max()) < O
    assert torch.equal(seg.group == -1, seg.part == M)
    assert abs(float(seg.mass.sum(1).mean()) - H * W) <= 1e-4 * H * W
    assert not dict.__contains__(res["rec"], "transformed_templates")     # still unrendered
    print(f"model: {int((seg.part < M).sum())} of {seg.part.numel()} pixels owned by a part, "
          f"{seg.part.unique().numel()} different owners")
    assert seg.part.unique().numel() >= 3

    # the two sheets: rows one and two are those of validation_images()['recons']
    with _lib.recorder() as launches:
        sheets = step.segmentation_images(res, n=n)
    names = [fn.__name__ for fn, _a, _k in launches]
    assert names.count("scae_render_gmm_parts_f32") == 1
    assert "scae_template_render_fwd_f32" not in names
    recons = step.validation_images(res, n=n)["recons"]
    assert sorted(sheets) == ["capsules", "parts"]
    rows2 = 2 * (H + 1) + 1
    for key, painted in (("parts", "rgb_part"), ("capsules", "rgb_group")):
        sheet = sheets[key]
        assert tuple(sheet.shape) == (3, 3 * (H + 1) + 1, n * (W + 1) + 1)
        assert sheet.is_cuda and sheet.dtype == torch.float32
        assert torch.equal(sheet[:, :rows2], recons[:, :rows2]), key
        want = getattr(segment.segment(res, image, first=0, count=n), painted)
        for k in range(n):
            y, x0 = 2 * (H + 1) + 1, k * (W + 1) + 1
            assert torch.equal(sheet[:, y:y + H, x0:x0 + W], want[k]), (key, k)
    again = step.segmentation_images(n=n)       # the default result: one eager forward
    assert torch.equal(again["parts"], sheets["parts"])
    with pytest.raises(ValueError):
        step.segmentation_images(res, n=0)

    # part_usage: 3 batches, the last one short
    N = 14
    images = torch.rand(N, C, H, W, generator=g)
    labels = torch.randint(0, 4, (N,), generator=g)        # (classes 4..9 are absent)
    use = segment.part_usage(model, images, labels, batch_size=6)
    assert model.training
    assert use.part_share.shape == (M + 1,) and use.capsule_share.shape == (O + 1,)
    assert abs(use.part_share.sum() - 1) <= 1e-5 and abs(use.capsule_share.sum() - 1) <= 1e-5
    assert abs(use.part_share[M] - use.capsule_share[O]) <= 1e-12      # the background
    nc = cfg["n_classes"]
    assert use.class_part_share.shape == (nc, M + 1)
    assert use.class_capsule_share.shape == (nc, O + 1)
    assert np.array_equal(use.class_count, np.bincount(labels.numpy(), minlength=nc))
    present = use.class_count > 0
    assert present.sum() >= 2 and not present.all()
    assert np.abs(use.class_part_share[present].sum(1) - 1).max() <= 1e-5
    assert np.abs(use.class_capsule_share[present].sum(1) - 1).max() <= 1e-5
    assert not use.class_part_share[~present].any()
    # the class tables average to the overall shares
    w = use.class_count / N
    assert np.abs(w @ use.class_part_share - use.part_share).max() <= 1e-9
    plain = segment.part_usage(model, images.cuda(), batch_size=14)
    assert plain.class_part_share is None
    assert np.abs(plain.part_share - use.part_share).max() <= 1e-5


def test_the_abi_lists_the_new_entry_points():
    import os
    import re
    from torch_scae_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "scae_hip.h")).read()
    declared = set(re.findall(r"\b(scae_[a-z0-9_]+)\s*\(", header)) - {"scae_decoder_desc"}
    assert {"scae_render_gmm_parts_f32", "scae_render_gmm_parts_geometry"} <= declared
    assert declared == set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
