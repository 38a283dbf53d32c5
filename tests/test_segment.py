"""Part segmentation on the host: ``segment_host`` against a loop-by-loop fp64 restatement of
the definitions in torch_scae_amd/segment.py, the properties those definitions imply, the
palette, the part-to-capsule owner table, and the argument checks of ``ops.render_gmm_parts``
and ``segment`` (which need no GPU: they come before any launch)."""
import math

import numpy as np
import pytest
import torch


def _loops(loc, ml, sigma, x):
    """R[k, p], part, conf, mass -- one scalar at a time, in Python floats (fp64)."""
    K, C, P = loc.shape
    Cm = ml.shape[1]
    R = np.zeros((K, P))
    for p in range(P):
        for c in range(C):
            j = []
            for k in range(K):
                v = float(ml[k, c if Cm == C else 0, p])
                if x is not None:
                    v -= 0.5 * (float(x[c, p]) - float(loc[k, c, p])) ** 2 / sigma ** 2
                j.append(v)
            m = -math.inf
            for k in range(K):
                m = max(m, j[k])
            s = 0.0
            for k in range(K):
                s += math.exp(j[k] - m)
            for k in range(K):
                R[k, p] += math.exp(j[k] - m) / s
        for k in range(K):
            R[k, p] *= 1.0 / C
    part = np.zeros(P, np.int32)
    conf = np.zeros(P)
    for p in range(P):
        best = 0
        for k in range(1, K):
            if R[k, p] > R[best, p]:
                best = k
        part[p], conf[p] = best, R[best, p]
    mass = np.array([sum(R[k, p] for p in range(P)) for k in range(K)])
    return R, part, conf, mass


def _tiny(C, Cm, seed):
    g = np.random.default_rng(seed)
    K, P = 3, 7
    return (g.random((K, C, P)), 2 * g.standard_normal((K, Cm, P)), 0.6, g.random((C, P)))


@pytest.mark.parametrize("C,Cm", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("with_x", [True, False])
def test_segment_host_is_the_definitions_loop_by_loop(C, Cm, with_x):
    from torch_scae_amd.segment import segment_host
    loc, ml, sigma, x = _tiny(C, Cm, seed=10 * C + Cm + with_x)
    x = x if with_x else None
    seg, R = segment_host(loc, ml, sigma, x=x)
    R0, part0, conf0, mass0 = _loops(loc, ml, sigma, x)
    assert R.shape == (3, 7) and R.dtype == np.float64
    # (numpy's exp and the math module's may differ in the last bit: a few ulps of values <= 1)
    assert np.abs(R - R0).max() <= 8 * 2.0 ** -53
    assert np.array_equal(seg.part, part0)
    assert np.abs(seg.conf - conf0).max() <= 8 * 2.0 ** -53
    assert np.abs(seg.mass - mass0).max() <= 7 * 16 * 2.0 ** -53
    if with_x:        # the observation matters: the posterior is not the prior
        assert np.abs(R - segment_host(loc, ml, sigma)[1]).max() > 1e-3


@pytest.mark.parametrize("C,Cm", [(1, 1), (3, 1), (2, 2)])
def test_segment_host_properties(C, Cm):
    from torch_scae_amd.segment import palette, segment_host
    g = np.random.default_rng(C + Cm)
    K, H, W = 5, 6, 9
    M = K - 1
    loc, ml = g.random((K, C, H, W)), 2 * g.standard_normal((K, Cm, H, W))
    x = g.random((C, H, W))
    table = np.array([2, 0, 2, 1])
    pal = palette(3)
    seg, R = segment_host(loc, ml, 0.8, x=x, part_group=table, palette=pal)
    assert seg.part.shape == (H, W) and seg.part.dtype == np.int32
    assert seg.part.min() >= 0 and seg.part.max() <= M
    assert len(np.unique(seg.part)) >= 3          # (not one constant owner)
    assert np.array_equal(seg.conf, R.max(0))
    assert np.array_equal(seg.part, R.argmax(0))
    assert abs(seg.mass.sum() - H * W) <= 1e-12 * H * W
    assert np.abs(R.sum(0) - 1).max() <= 1e-12
    # group: the table's entry, -1 exactly on the background
    bg = seg.part == M
    assert bg.any() and not bg.all()
    assert np.array_equal(seg.group == -1, bg)
    assert np.array_equal(seg.group[~bg], table[seg.part[~bg]])
    # colours: t * palette[id mod P]; t itself on the background
    tone = np.take_along_axis(loc, seg.part[None, None].astype(np.int64), 0)[0].mean(0)
    pal64 = pal.numpy().astype(np.float64)
    for rgb, ids in ((seg.rgb_part, seg.part), (seg.rgb_group, seg.group)):
        assert rgb.shape == (3, H, W)
        want = np.where(bg[None], tone[None], tone[None] * np.moveaxis(pal64[ids % 3], -1, 0))
        assert np.abs(rgb - want).max() <= 4 * 2.0 ** -53
    # without a table: no group, no capsule colouring; the default palette has M rows
    seg2, _ = segment_host(loc, ml, 0.8, x=x)
    assert seg2.group is None and seg2.rgb_group is None
    assert np.array_equal(seg2.part, seg.part)
    assert np.array_equal(seg2.rgb_part[:, bg], seg.rgb_part[:, bg])


def test_an_exact_tie_goes_to_the_lowest_component():
    from torch_scae_amd.segment import segment_host
    g = np.random.default_rng(3)
    K, C, P = 4, 2, 11
    loc, ml = g.random((K, C, P)), g.standard_normal((K, 1, P))
    loc[2], ml[2] = loc[1], ml[1]                 # components 1 and 2 are the same
    ml[1:3] += 3                                  # ... and win most pixels
    seg, R = segment_host(loc, ml, 1.0, x=g.random((C, P)))
    assert np.array_equal(R[1], R[2])
    assert (seg.part == 1).sum() >= P // 2 and not (seg.part == 2).any()
    assert seg.mass[1] == seg.mass[2]
    # all components equal: component 0 owns everything
    seg, _ = segment_host(np.ones((3, 1, 5)), np.zeros((3, 1, 5)), 1.0)
    assert not seg.part.any() and np.array_equal(seg.conf, np.full(5, 1 / 3))


def test_palette_is_deterministic_with_distinct_rows():
    from torch_scae_amd.segment import palette
    a, b = palette(64), palette(64)
    assert a.dtype == torch.float32 and tuple(a.shape) == (64, 3)
    assert torch.equal(a, b)
    assert torch.equal(palette(5), a[:5])         # a prefix: ids keep their colour
    assert len({tuple(r) for r in a.tolist()}) == 64
    assert float(a.min()) >= 0.25 - 1e-7 and float(a.max()) == 1.0
    # golden-angle hues: neighbours in id are far apart in colour
    assert float((a[1:] - a[:-1]).abs().amax(1).min()) > 0.3
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            palette(bad)


def test_part_owner_is_the_first_largest_posterior():
    from torch_scae_amd.segment import part_owner
    post = torch.tensor([[[0.1, 0.5, 0.2, 0.0],      # image 0: (O=3, M=4)
                          [0.7, 0.5, 0.2, 0.0],
                          [0.2, 0.0, 0.6, 0.0]],
                         [[0.3, 0.1, 0.4, 0.9],
                          [0.3, 0.2, 0.4, 0.1],
                          [0.3, 0.7, 0.1, 0.0]]])
    own = part_owner(dict(posterior_mixing_prob=post))
    assert own.dtype == torch.int32 and tuple(own.shape) == (2, 4)
    # ties: part 1 of image 0 (capsules 0, 1), part 3 (all zero), image 1's parts 0 and 2
    assert own.tolist() == [[1, 0, 2, 0], [0, 2, 0, 0]]
    with pytest.raises(ValueError):
        part_owner(dict(posterior_mixing_prob=post[0]))


def _cpu_inputs(B=4, M=3, C=2, th=5, tw=5, H=6, W=7, alpha=True):
    from torch_scae_amd import ops
    g = torch.Generator().manual_seed(0)
    return ops.DecoderInputs(
        (H, W), templates=torch.rand(B, M, C, th, tw, generator=g),
        templates_alpha=torch.randn(1, M, 1, th, tw, generator=g) if alpha else None,
        pose=torch.randn(B, M, 6, generator=g), presence=torch.rand(B, M, generator=g),
        bg_value=torch.zeros(1), bg_mixing_logit=torch.zeros(1),
        temperature_logit=None if alpha else torch.zeros(1))


def test_render_gmm_parts_checks_its_arguments_before_any_launch():
    from torch_scae_amd import ops
    inputs = _cpu_inputs()
    B, M, C, H, W = 4, 3, 2, 6, 7
    for first, count in ((B, 1), (0, B + 1), (-1, 1), (0, 0), (1.0, 1), (2, 3)):
        with pytest.raises(ValueError, match="slice"):
            ops.render_gmm_parts(inputs, first=first, count=count)
    with pytest.raises(ValueError, match="observed image"):
        ops.render_gmm_parts(inputs, x=torch.zeros(B, C, H, W + 1))
    with pytest.raises(ValueError, match="observed image"):
        ops.render_gmm_parts(inputs, x=torch.zeros(2, C, H, W), first=1, count=2)
    for bad in (torch.zeros(B, M, dtype=torch.int64), torch.zeros(B, M + 1, dtype=torch.int32),
                torch.zeros(M, dtype=torch.int32)):
        with pytest.raises(ValueError, match="part_group"):
            ops.render_gmm_parts(inputs, part_group=bad)
    for bad in (torch.zeros(3), torch.zeros(4, 4), torch.zeros(0, 3),
                torch.zeros(4, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="palette"):
            ops.render_gmm_parts(inputs, palette=bad)
    # well-formed arguments on the CPU: there is no CPU path
    with pytest.raises(ops.ScaeHipError):
        ops.render_gmm_parts(inputs, x=torch.zeros(B, C, H, W),
                             part_group=torch.zeros(B, M, dtype=torch.int32))


def test_segment_needs_a_result_of_the_library_decoder():
    from torch_scae_amd import ops
    from torch_scae_amd.segment import segment

    class Pdf:
        _decoder_inputs = None
    res = dict(rec=type("Rec", (), {"pdf": Pdf()})(),
               posterior_mixing_prob=torch.rand(4, 2, 3))
    with pytest.raises(ops.ScaeHipError, match="segment_host"):
        segment(res)
    Pdf._decoder_inputs = _cpu_inputs()
    with pytest.raises(ValueError, match="slice"):
        segment(res, first=3, count=2)
    with pytest.raises(ops.ScaeHipError):
        segment(res, image=torch.zeros(4, 2, 6, 7))


def test_parts_geometry_follows_the_staging_budget():
    """The launch geometry is host arithmetic: 64 KB of padded planes (+ 7 floats per template
    for pose and presence) are staged at a time."""
    from torch_scae_amd import ops
    tiles, ppb, kchunk = ops.render_gmm_parts_geometry(_cpu_inputs(), 2)
    assert (tiles, ppb, kchunk) == (1, 256, 3)                   # 42 pixels, all 3 templates
    big = _cpu_inputs(B=2, M=24, C=3, th=11, tw=11, H=40, W=40)
    tiles, ppb, kchunk = ops.render_gmm_parts_geometry(big)
    assert kchunk == 64 * 1024 // 4 // (4 * 15 * 15 + 7) == 18 < 24   # chunked
    assert (tiles, ppb) == (7, 256)                              # one round per workgroup
