"""Validation image logging, the host side (no GPU): the sheet layout of ``ops.image_sheet``
against the rules restated here in numpy, the two C-ABI symbols, the argument checks of both
entry points, and which ``GaussianMixture.mode`` / ``.mean`` calls take the fused
render-and-mode kernel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sheet_by_the_rules(t, nrow, padding, pad_value):
    """The sheet of a batch t (N, C, H, W), from the rules of include/scae_hip.h: xmaps =
    min(nrow, N) images per row, ymaps = ceil(N / xmaps) rows, cells of (H + padding,
    W + padding), a sheet of (3, ymaps (H + padding) + padding, xmaps (W + padding) + padding)
    filled with pad_value, image k at row (k // xmaps)(H + padding) + padding and column
    (k % xmaps)(W + padding) + padding; one channel repeated to three; N = 1: the image."""
    N, C, H, W = t.shape
    if C == 1:
        t = np.repeat(t, 3, axis=1)
    if N == 1:
        return t[0].copy()
    xmaps = min(nrow, N)
    ymaps = (N + xmaps - 1) // xmaps
    sheet = np.full((3, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding),
                    pad_value, dtype=np.float32)
    for k in range(N):
        y = (k // xmaps) * (H + padding) + padding
        x = (k % xmaps) * (W + padding) + padding
        sheet[:, y:y + H, x:x + W] = t[k]
    return sheet


SHEETS = [
    # counts of the sources, C, H, W, nrow, padding, pad_value
    ((8,), 1, 5, 7, 8, 1, 0.0),           # one full row
    ((8, 8), 1, 5, 7, 8, 1, 0.0),         # two rows of images
    ((8, 8, 8, 8), 1, 6, 4, 8, 1, 0.0),   # the recons sheet with alternatives
    ((24,), 1, 5, 5, 4, 1, 0.0),          # templates: nrow = int(sqrt(24))
    ((25,), 3, 4, 6, 4, 1, 0.0),          # N not a multiple of nrow
    ((3, 4), 3, 4, 6, 5, 2, 0.25),        # two sources, a last row with empty cells
    ((3,), 1, 4, 6, 8, 1, 0.5),           # N < nrow
    ((1,), 1, 4, 6, 8, 1, 0.5),           # N = 1: the image, no padding
    ((1,), 3, 4, 6, 3, 2, 0.5),
    ((1, 1), 3, 3, 3, 1, 0, 0.0),         # one column, no padding
    ((5, 2, 1), 1, 2, 3, 3, 0, -1.0),     # three sources, padding 0
    ((2, 3, 1, 4), 3, 3, 2, 4, 2, 1.5),   # four sources, padding 2
]


@pytest.mark.parametrize("counts,C,H,W,nrow,padding,pad_value", SHEETS)
def test_image_sheet_on_cpu_tensors_follows_the_rules(counts, C, H, W, nrow, padding,
                                                      pad_value):
    from torch_scae_amd import ops
    g = torch.Generator().manual_seed(sum(counts) + 10 * C + H)
    sources = [torch.rand(n, C, H, W, generator=g) for n in counts]
    got = ops.image_sheet(sources, nrow, padding=padding, pad_value=pad_value)
    want = sheet_by_the_rules(torch.cat(sources, 0).numpy(), nrow, padding, pad_value)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy(), want)
    N = sum(counts)
    assert ops.image_sheet_shape(N, H, W, nrow, padding)[2:] == want.shape[1:]


def test_image_sheet_refuses_what_the_rules_do_not_cover():
    from torch_scae_amd import ops
    ok = torch.zeros(2, 1, 3, 3)
    with pytest.raises(ValueError):
        ops.image_sheet([torch.zeros(2, 2, 3, 3)], 2)            # C = 2
    with pytest.raises(ValueError):
        ops.image_sheet([torch.zeros(2, 4, 3, 3)], 2)            # C = 4
    with pytest.raises(ValueError):
        ops.image_sheet([ok] * 5, 2)                              # five sources
    with pytest.raises(ValueError):
        ops.image_sheet([], 2)
    with pytest.raises(ValueError):
        ops.image_sheet([ok, torch.zeros(2, 1, 3, 4)], 2)        # another size
    with pytest.raises(ValueError):
        ops.image_sheet([ok], 0)
    with pytest.raises(ValueError):
        ops.image_sheet([ok], 2, padding=-1)
    with pytest.raises(ValueError):
        ops.image_sheet([torch.zeros(3, 3)], 2)


def test_header_declares_and_binding_binds_the_two_symbols():
    from torch_scae_amd import _lib
    header = open(os.path.join(ROOT, "include", "scae_hip.h")).read()
    lib = _lib.load()
    for name in ("scae_render_gmm_mode_f32", "scae_image_sheet_f32"):
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["scae_render_gmm_mode_f32"]) == 6
    assert len(_lib.SIGNATURES["scae_image_sheet_f32"]) == 11


def _desc(**kw):
    """A descriptor the check accepts as far as a host can tell: the pointers are
    never read, because every call below fails an argument check before any launch."""
    from torch_scae_amd import _lib
    keep = (ctypes.c_float * 8)()
    p = ctypes.cast(keep, ctypes.c_void_p)
    f = dict(templates=p, templates_alpha=p, pose=p, presence=None, bg_image=None,
             bg_value=p, bg_mixing_logit=p, temperature_logit=None, out_scale=None,
             B=4, M=2, C=1, th=3, tw=3, H=8, W=8, template_repeat=0)
    f.update(kw)
    names = [n for n, _ in _lib.DecoderDesc._fields_]
    assert set(names) == set(f), set(names) ^ set(f)
    return _lib.DecoderDesc(*[f[n] for n in names]), keep


def test_render_gmm_mode_rejects_bad_arguments_before_any_launch():
    """include/scae_hip.h: check of the descriptor, 0 <= first, count > 0,
    first + count <= B, out non-null, what in {0, 1} -> SCAE_ERR_BAD_ARG (-1)."""
    from torch_scae_amd import _lib
    lib = _lib.load()
    fn = lib.scae_render_gmm_mode_f32
    d, keep = _desc()
    out = ctypes.cast((ctypes.c_float * 8)(), ctypes.c_void_p)
    with _lib.recorder() as launches:
        assert fn(None, out, 0, 0, 1, None) == -1                      # no descriptor
        assert fn(_lib.DecoderDesc(), out, 0, 0, 1, None) == -1        # an empty one
        assert fn(d, None, 0, 0, 1, None) == -1                        # no output
        assert fn(d, out, 2, 0, 1, None) == -1                         # what
        assert fn(d, out, -1, 0, 1, None) == -1
        assert fn(d, out, 0, -1, 1, None) == -1                        # first < 0
        assert fn(d, out, 0, 0, 0, None) == -1                         # count = 0
        assert fn(d, out, 0, 0, -3, None) == -1
        assert fn(d, out, 0, 0, 5, None) == -1                         # beyond B = 4
        assert fn(d, out, 0, 4, 1, None) == -1
        assert fn(d, out, 1, 3, 2, None) == -1
        assert fn(d, out, 0, 2 ** 31 - 1, 2 ** 31 - 1, None) == -1     # no overflow either
        bad, _k = _desc(templates_alpha=None)      # neither alpha planes nor a temperature
        assert fn(bad, out, 0, 0, 1, None) == -1
        wide, _k = _desc(C=5)                      # beyond SCAE_MAX_CHANNELS
        assert fn(wide, out, 0, 0, 1, None) == -2
    assert launches == []


def test_image_sheet_entry_point_rejects_bad_arguments_before_any_launch():
    from torch_scae_amd import _lib
    lib = _lib.load()
    fn = lib.scae_image_sheet_f32
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ptrs, none = (ctypes.c_void_p * 4)(p, p, p, p), (ctypes.c_void_p * 4)()
    n, zero = (ctypes.c_int * 4)(1, 1, 1, 1), (ctypes.c_int * 4)(1, 0, 1, 1)
    with _lib.recorder() as launches:
        assert fn(0, ptrs, n, 1, 2, 2, 2, 1, 0.0, p, None) == -1     # no source
        assert fn(5, ptrs, n, 1, 2, 2, 2, 1, 0.0, p, None) == -1     # more than four
        assert fn(2, None, n, 1, 2, 2, 2, 1, 0.0, p, None) == -1
        assert fn(2, ptrs, None, 1, 2, 2, 2, 1, 0.0, p, None) == -1
        assert fn(2, none, n, 1, 2, 2, 2, 1, 0.0, p, None) == -1     # a null source
        assert fn(2, ptrs, zero, 1, 2, 2, 2, 1, 0.0, p, None) == -1  # an empty source
        assert fn(2, ptrs, n, 2, 2, 2, 2, 1, 0.0, p, None) == -1     # C = 2
        assert fn(2, ptrs, n, 4, 2, 2, 2, 1, 0.0, p, None) == -1     # C = 4
        assert fn(2, ptrs, n, 1, 0, 2, 2, 1, 0.0, p, None) == -1     # H = 0
        assert fn(2, ptrs, n, 1, 2, 2, 0, 1, 0.0, p, None) == -1     # nrow = 0
        assert fn(2, ptrs, n, 1, 2, 2, 2, -1, 0.0, p, None) == -1    # padding < 0
        assert fn(2, ptrs, n, 1, 2, 2, 2, 1, 0.0, None, None) == -1  # no sheet
    assert launches == []


# ---------------------------------------------------------------- routing -----
class _StubInputs:
    """What GaussianMixture reads of ops.DecoderInputs."""

    def __init__(self, requires_grad=False, C=1, alpha=True):
        self.templates = torch.zeros(2, 3, C, 4, 4, requires_grad=requires_grad)
        self.templates_alpha = torch.zeros(1, 3, 1, 4, 4) if alpha else None
        self.pose = torch.zeros(2, 3, 6)
        self.output_size = (5, 6)

    def tensors(self):
        return [self.templates, self.templates_alpha, self.pose]


class _Rendered:
    def __init__(self):
        self.out = None


def _lazy_mixture(inputs, rendered=None):
    """A mixture as the lazy decoder builds it: thunks for both rendered tensors (they
    count the renders they are asked for)."""
    from torch_scae_amd.distributions import GaussianMixture, _NormalView
    B, K, C = 2, 4, inputs.templates.shape[2]
    Cm = 1 if inputs.templates_alpha is not None else C
    asked = []

    def loc():
        asked.append("loc")
        return torch.zeros(B, K, C, 5, 6)

    def logits():
        asked.append("logits")
        return torch.zeros(B, K, Cm, 5, 6)
    pdf = GaussianMixture(_NormalView(loc, torch.ones(1)), logits, _decoder_inputs=inputs)
    if rendered is not None:
        pdf._rendered = rendered
    return pdf, asked


@pytest.fixture
def spy(monkeypatch):
    """ops.render_gmm_mode and the materialising ops replaced by recorders."""
    from torch_scae_amd import ops
    calls = []

    def fused(inputs, mean=False, first=0, count=None):
        calls.append(("fused", bool(mean), first, count))
        return torch.full((2, inputs.templates.shape[2], 5, 6), 7.0)

    def gmm_mode(loc, ml, sigma, maximum=False):
        calls.append(("gmm_mode", bool(maximum)))
        return torch.zeros(loc.shape[0], *loc.shape[2:])

    def gmm_mean(loc, ml):
        calls.append(("gmm_mean",))
        return torch.zeros(loc.shape[0], *loc.shape[2:])
    monkeypatch.setattr(ops, "render_gmm_mode", fused)
    monkeypatch.setattr(ops, "gmm_mode", gmm_mode)
    monkeypatch.setattr(ops, "gmm_mean", gmm_mean)
    return calls


def test_mode_and_mean_take_the_fused_kernel_on_an_unrendered_mixture(spy):
    inputs = _StubInputs()
    pdf, asked = _lazy_mixture(inputs, _Rendered())
    out = pdf.mode()
    assert spy == [("fused", False, 0, None)] and float(out[0, 0, 0, 0]) == 7.0
    assert pdf.mean().shape == (2, 1, 5, 6)
    assert pdf.mode(maximum=True).shape == (2, 1, 5, 6)     # a shared scale: same winner
    assert spy == [("fused", False, 0, None), ("fused", True, 0, None),
                   ("fused", False, 0, None)]
    assert asked == [], "a fused call rendered the mixture"
    assert callable(pdf._mixing_logits) and callable(pdf.dist._loc)   # still lazy
    # inputs that require grad, but grad mode is off: no gradient can be asked
    pdf, asked = _lazy_mixture(_StubInputs(requires_grad=True))
    with torch.no_grad():
        pdf.mode()
        pdf.mean()
    assert spy[3:] == [("fused", False, 0, None), ("fused", True, 0, None)] and asked == []


def test_mode_and_mean_keep_the_materialising_path_elsewhere(spy):
    from torch_scae_amd.distributions import GaussianMixture
    # a gradient can be asked of the result
    pdf, asked = _lazy_mixture(_StubInputs(requires_grad=True))
    pdf.mode()
    pdf.mean()
    assert spy == [("gmm_mode", False), ("gmm_mean",)] and set(asked) == {"loc", "logits"}
    del spy[:]
    # the straight-through estimator is composed from the rendered tensors
    pdf, asked = _lazy_mixture(_StubInputs())
    out = pdf.mode(straight_through_gradient=True)
    assert spy == [] and set(asked) == {"loc", "logits"} and out.shape == (2, 1, 5, 6)
    # rendered already, through the mixture's own properties ...
    pdf, asked = _lazy_mixture(_StubInputs())
    pdf.dist.loc
    pdf.mode()
    assert spy == [("gmm_mode", False)]
    del spy[:]
    pdf, asked = _lazy_mixture(_StubInputs())
    pdf.mixing_logits
    pdf.mean()
    assert spy == [("gmm_mean",)]
    del spy[:]
    # ... or through the decoder's result (its transformed_templates entry)
    rendered = _Rendered()
    pdf, asked = _lazy_mixture(_StubInputs(), rendered)
    rendered.out = (torch.zeros(2, 4, 1, 5, 6), torch.zeros(2, 4, 1, 5, 6))
    pdf.mode()
    assert spy == [("gmm_mode", False)]
    del spy[:]
    # a mixture of plain tensors has no decoder inputs
    GaussianMixture.make_from_stats(torch.zeros(2, 4, 1, 5, 6), torch.ones(1),
                                    torch.zeros(2, 4, 1, 5, 6)).mode()
    assert spy == [("gmm_mode", False)]


def test_fused_mode_keeps_the_reference_broadcast_error():
    """maximum=True with one logit channel and C > 1: the reference's in-place add cannot
    broadcast (distributions.py:65) -- on the fused route too, before any kernel."""
    pdf, asked = _lazy_mixture(_StubInputs(C=3, alpha=True))
    with pytest.raises(RuntimeError, match="broadcast shape"):
        pdf.mode(maximum=True)
    assert asked == []


def test_validation_images_needs_a_device_model():
    from torch_scae_amd import EvalStep, ops
    model = torch.nn.Linear(2, 2)
    step = EvalStep(model, 4, (1, 8, 8))
    with pytest.raises(ops.ScaeHipError):
        step.validation_images()
