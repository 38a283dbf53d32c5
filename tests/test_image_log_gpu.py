"""Validation image logging on the GPU: the fused render-and-mode kernel bit for bit against
the materialising path (render, then the generic mode / mean over the rendered tensors), its
slices, the reference's recorded values through ``pdf.mode()`` / ``.mean()`` of a lazy
decoder, the memory it saves, ``EvalStep.validation_images`` against the sheets assembled
the materialising way, and an evaluation step with ``recon_mse_weight`` > 0."""
import numpy as np
import pytest
import torch

from tests.golden_util import assert_close, load, sub
from tests.test_hip_model import full_size_params
from tests.test_hip_ops import decoder_cases, make_decoder

pytestmark = pytest.mark.gpu


def _inputs(B, M, C, H, W, th, tw, alpha, bg_image, presence, scale, repeat=1, seed=0):
    """Random compact decoder inputs on the device: poses around the scale at which a
    template covers a good part of the image, so that every component wins somewhere."""
    from torch_scae_amd import ops
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)          # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g)        # noqa: E731
    pose = torch.tensor([1.6, 0.0, 0.0, 0.0, 1.6, 0.0]) + \
        rn(B, M, 6) * torch.tensor([0.4, 0.3, 0.5, 0.3, 0.4, 0.5])
    t = dict(templates=r(B // repeat, M, C, th, tw),
             templates_alpha=rn(1, M, 1, th, tw) * 2 if alpha else None,
             pose=pose, presence=0.7 + 0.3 * r(B, M) if presence else None,
             bg_image=0.3 * r(B, C, H, W) if bg_image else None,
             bg_value=None if bg_image else rn(1) - 1.5,
             bg_mixing_logit=rn(1),
             temperature_logit=None if alpha else 0.3 * rn(1) - 1.5,
             out_scale=rn(1) if scale else None)
    return ops.DecoderInputs((H, W), **{k: None if v is None else v.cuda()
                                        for k, v in t.items()})


def _materialised(inputs, mean=False):
    """mode / mean the materialising way: render both tensors, then the generic kernel."""
    from torch_scae_amd import ops
    tt, ml = ops.render_templates(inputs)
    B, K, C, H, W = tt.shape
    loc, logits = tt.view(B, K, C, H * W), ml.view(B, K, ml.shape[2], H * W)
    if mean:
        return ops.gmm_mean(loc, logits).view(B, C, H, W)
    sigma = torch.ones(1, device=tt.device)
    return ops.gmm_mode(loc, logits, sigma).view(B, C, H, W)


SMALL = dict(H=13, W=17, th=5, tw=6, M=5, B=6)
CASES = {
    # every flag of the decoder's golden cases, at a small odd size (the 13 x 17 pixels
    # are not whole quads: the one-component-per-workgroup render form) ...
    "alpha": dict(SMALL, C=1, alpha=True, bg_image=False, presence=True, scale=False),
    "alpha_rgb_bgimage_scale": dict(SMALL, C=3, alpha=True, bg_image=True, presence=False,
                                    scale=True),
    "noalpha_scale": dict(SMALL, C=1, alpha=False, bg_image=False, presence=True,
                          scale=True),
    "noalpha_rgb_bgimage": dict(SMALL, C=3, alpha=False, bg_image=True, presence=True,
                                scale=False),
    "noalpha_nopresence": dict(SMALL, C=1, alpha=False, bg_image=False, presence=False,
                               scale=False),
    "alpha_repeat": dict(SMALL, C=1, alpha=True, bg_image=False, presence=True,
                         scale=False, repeat=3),
    "noalpha_rgb_repeat": dict(SMALL, C=3, alpha=False, bg_image=False, presence=True,
                               scale=True, repeat=2),
    # ... and in whole quads (12 x 12: the quad-store render form of the alpha mode)
    "alpha_quads_bgimage": dict(SMALL, H=12, W=12, C=1, alpha=True, bg_image=True,
                                presence=True, scale=False),
    "alpha_rgb_quads_repeat": dict(SMALL, H=12, W=12, C=3, alpha=True, bg_image=False,
                                   presence=False, scale=True, repeat=2),
    # the factory's shapes: cfg-2, cfg-5 (CIFAR, 3 channels: the planes of its 32 templates
    # are staged in chunks) and 48/64 at B = 64 (chunks too)
    "cfg2": dict(B=128, M=24, C=1, H=40, W=40, th=11, tw=11, alpha=True, bg_image=False,
                 presence=True, scale=False),
    "cfg2_noalpha": dict(B=32, M=24, C=1, H=40, W=40, th=11, tw=11, alpha=False,
                         bg_image=False, presence=True, scale=True),
    "cfg5": dict(B=32, M=32, C=3, H=32, W=32, th=11, tw=11, alpha=True, bg_image=False,
                 presence=True, scale=False),
    "cfg5_noalpha_bgimage": dict(B=16, M=32, C=3, H=32, W=32, th=11, tw=11, alpha=False,
                                 bg_image=True, presence=True, scale=False),
    "cfg3_b64": dict(B=64, M=48, C=1, H=40, W=40, th=11, tw=11, alpha=True, bg_image=False,
                     presence=True, scale=False),
}


def _compare(name, mean):
    from torch_scae_amd import ops
    case = CASES[name]
    inputs = _inputs(seed=sorted(CASES).index(name), **case)
    B = case["B"]
    want = _materialised(inputs, mean)
    got = ops.render_gmm_mode(inputs, mean=mean)
    assert got.shape == want.shape
    diff = (got != want)
    print(f"{name} mean={mean}: {int(diff.sum())} of {diff.numel()} elements differ, "
          f"max |d| {float((got - want).abs().max()):.3e}")
    # slices are rows of the full result, whatever that is
    for first, count in ((0, 1), (1, 1), (B - 1, 1), (2, 3), (B - 2, 2)):
        part = ops.render_gmm_mode(inputs, mean=mean, first=first, count=count)
        assert torch.equal(part, got[first:first + count]), (mean, first, count)
    assert torch.equal(got, want)
    return inputs


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_mode_is_the_materialising_path_bit_for_bit(name):
    """No tolerance: the fused kernel computes every component's value and logit with the
    roundings of the render kernel the materialising entry point takes for the same
    descriptor (csrc/render_gmm_mode.hip spells them out), and then applies the generic
    kernel's rule, the first largest logit.  Slices are rows of the full result."""
    from torch_scae_amd import ops
    inputs = _compare(name, mean=False)
    B = CASES[name]["B"]
    # (a check of the inputs: background and several templates win somewhere, so the
    # comparison above exercises the arg-max and not one constant winner)
    winners = ops.render_templates(inputs)[1].argmax(1).unique()
    print(f"{name}: {winners.numel()} different winning components")
    assert winners.numel() >= 3, winners
    with pytest.raises(ValueError):
        ops.render_gmm_mode(inputs, first=B, count=1)
    with pytest.raises(ValueError):
        ops.render_gmm_mode(inputs, first=0, count=B + 1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_mean_is_the_materialising_path_bit_for_bit(name):
    """Bitwise, not the golden bar: the summation order is shared.  The fused mean runs the
    generic kernel's two-pass softmax over the same components in the same order -- the
    maximum, then the sum of exponentials and the weighted sum, each product rounded before
    it is added as gmm_mean_mode_kernel does -- on logits and values that have the
    materialising kernels' bits (the test above), with the exponential and ``log_safe``'s
    logarithm evaluated by the instruction sequences those kernels execute
    (csrc/render_gmm_mode.hip: mode_expf, mode_log_safe)."""
    _compare(name, mean=True)


@pytest.mark.parametrize("alpha", [True, False])
def test_fused_mode_and_mean_follow_the_scalar_parameters_bit_for_bit(alpha):
    """The decoder's scalar parameters pass through softplus / sigmoid (load_scalars) in both
    paths, compiled with different contraction settings: a last-bit difference in the
    temperature, the background logit or the background value would show in every pixel.
    400 values of each, over the ranges training moves them in and beyond (softplus's
    linear branch above 20, saturated sigmoids), on a small shape: mode and mean stay equal
    to the materialising path."""
    from torch_scae_amd import ops
    inputs = _inputs(B=2, M=4, C=3 if not alpha else 1, H=9, W=11, th=5, tw=5, alpha=alpha,
                     bg_image=False, presence=True, scale=True, seed=40 + alpha)
    g = torch.Generator().manual_seed(7)
    n = 400
    sweep = torch.cat([torch.linspace(-12, 24, n // 2), 3 * torch.randn(n // 2, generator=g)])
    bad = []
    for i in range(n):
        v = sweep[i:i + 1].cuda()
        inputs.bg_value = sweep[(i * 7) % n:(i * 7) % n + 1].cuda()
        inputs.out_scale = sweep[(i * 3) % n:(i * 3) % n + 1].cuda()
        if alpha:
            inputs.bg_mixing_logit = v
        else:
            inputs.temperature_logit = v
        for mean in (False, True):
            if not torch.equal(ops.render_gmm_mode(inputs, mean=mean),
                               _materialised(inputs, mean)):
                bad.append((float(sweep[i]), float(inputs.bg_value), mean))
    print(f"alpha={alpha}: {len(bad)} of {2 * n} comparisons differ {bad[:5]}")
    assert not bad, bad[:10]


@pytest.mark.parametrize("name", decoder_cases())
def test_lazy_decoder_mode_and_mean_vs_golden_on_the_fused_kernel(name):
    """The reference's recorded mode / mean / mode(maximum=True) through a lazy decoder
    under no_grad, at the bars tests/test_hip_ops.py sets for these keys -- and the launch
    record shows the fused kernel ran and the materialising render did not."""
    from torch_scae_amd import _lib
    blob, meta = load("op_image_decoder")
    c = sub(blob, name + "/")
    dec = make_decoder(meta[name], sub(c, "param/"))
    dec.lazy_render = True
    i = {k: v.cuda() for k, v in sub(c, "in/").items() if k not in ("x", "w")}
    with torch.no_grad(), _lib.recorder() as launches:
        r = dec(i["templates"], i["pose"], i.get("presence"), i.get("bg_image"))
        assert_close(r.pdf.mode(), c["out/mode"], 2e-5, 1e-4, "mode")
        assert_close(r.pdf.mean(), c["out/mean"], 2e-5, 1e-4, "mean")
        if "out/mode_max" in c:
            assert_close(r.pdf.mode(maximum=True), c["out/mode_max"], 2e-5, 1e-4,
                         "mode_max")
        else:
            with pytest.raises(RuntimeError):
                r.pdf.mode(maximum=True)
    names = [fn.__name__ for fn, _args, _keep in launches]
    assert names.count("scae_render_gmm_mode_f32") == (3 if "out/mode_max" in c else 2)
    assert "scae_template_render_fwd_f32" not in names, names
    assert not dict.__contains__(r, "transformed_templates")      # still unrendered
    # with gradients on, the same calls keep the materialising path
    with _lib.recorder() as launches:
        r = dec(i["templates"], i["pose"], i.get("presence"), i.get("bg_image"))
        assert_close(r.pdf.mode(), c["out/mode"], 2e-5, 1e-4, "mode (materialised)")
    names = [fn.__name__ for fn, _args, _keep in launches]
    assert "scae_render_gmm_mode_f32" not in names
    assert "scae_template_render_fwd_f32" in names and "scae_gmm_mode_f32" in names


def test_fused_mode_allocates_less_than_one_rendered_tensor():
    """The point of the feature, at cfg-2 shapes: ``pdf.mode()`` of a fresh lazy decoder
    output needs its (B, C, H, W) result and nothing of the size of a (B, M+1, C, H, W)
    tensor -- the materialising path allocates two of those (and the result)."""
    from torch_scae_amd.part_decoder import TemplateBasedImageDecoder
    B, M, C, H, W = 128, 24, 1, 40, 40
    dec = TemplateBasedImageDecoder(M, (11, 11), (H, W), use_alpha_channel=True).cuda()
    dec.lazy_render = True
    g = torch.Generator().manual_seed(5)
    templates = torch.rand(B, M, C, 11, 11, generator=g).cuda()
    pose = (torch.tensor([1.6, 0, 0, 0, 1.6, 0]) +
            0.3 * torch.randn(B, M, 6, generator=g)).cuda()
    presence = torch.rand(B, M, generator=g).cuda()
    with torch.no_grad():
        r = dec(templates, pose, presence)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = r.pdf.mode()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    one_tensor = B * (M + 1) * C * H * W * 4
    print(f"peak rise {rise} bytes; one rendered tensor {one_tensor}; result "
          f"{out.numel() * 4}")
    assert out.shape == (B, C, H, W)
    assert rise < one_tensor, (rise, one_tensor)
    assert not dict.__contains__(r, "transformed_templates")
    assert callable(r.pdf._mixing_logits) and r.pdf._rendered.out is None


def _model(cfg, sd):
    from torch_scae_amd import factory
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(cfg)
    model.load_state_dict(sd)
    return model.cuda().train()


def _sheets_the_materialising_way(step, res, n):
    """validation_epoch_end's three tensors (base_experiment.py:152-182) as before the
    fused kernel: every mixture rendered, ``mode()`` over the rendered tensors, the sheet
    laid out by torch ops on the CPU."""
    from torch_scae_amd import _lib, ops
    with torch.no_grad(), _lib.recorder() as launches:
        rows = [step.image[:n].cpu()]
        for key in ("rec", "bottom_up_rec", "top_down_rec"):
            if key == "rec" or step.model.reconstruct_alternatives:
                res[key].transformed_templates            # renders the whole batch
                rows.append(res[key].pdf.mode().cpu()[:n])
        templates = res.templates.cpu()[0]
        nrow = int(templates.shape[0] ** 0.5)
        out = {"recons": ops.image_sheet(rows, nrow=n, padding=1, pad_value=0.0),
               "templates": ops.image_sheet([templates], nrow=nrow),
               "transformed_templates": ops.image_sheet(
                   [res.transformed_templates.cpu()[0]], nrow=nrow)}
    assert "scae_render_gmm_mode_f32" not in [fn.__name__ for fn, _a, _k in launches]
    return out


@pytest.mark.parametrize("name,B,alternatives", [("cfg2", 16, False), ("cfg2", 16, True),
                                                 ("cfg2", 5, True), ("cfg5", 12, False)])
def test_validation_images_equal_the_sheets_assembled_the_materialising_way(
        name, B, alternatives):
    from torch_scae_amd import EvalStep, _lib, ops
    cfg, _, sd, g = full_size_params(name)
    cfg = dict(cfg, scae_params=dict(cfg["scae_params"],
                                     reconstruct_alternatives=alternatives))
    model = _model(cfg, sd)
    C, H, W = cfg["image_shape"]
    step = EvalStep(model, B, cfg["image_shape"])
    image = torch.rand(B, C, H, W, generator=g).cuda()
    label = torch.randint(0, cfg["n_classes"], (B,), generator=g).cuda()

    def replay():
        torch.manual_seed(11)
        ops.reset_noise()           # the step's generator restarts: the same draws
        return step(image, label).clone()
    step.capture()                  # (its warm-up batches draw noise too)
    loss_before = replay()
    means_before = step.epoch_means()
    acc_before = step.acc.clone()

    res = step._eager_result()
    with _lib.recorder() as launches:
        sheets = step.validation_images(res)
    names = [fn.__name__ for fn, _a, _k in launches]
    rows = 4 if alternatives else 2
    n = min(B, 8)
    assert names.count("scae_render_gmm_mode_f32") == rows - 1
    assert names.count("scae_image_sheet_f32") == 3
    assert names.count("scae_template_render_fwd_f32") == 1        # image 0 alone
    for key in ("rec", "bottom_up_rec", "top_down_rec")[:rows - 1]:
        assert not dict.__contains__(res[key], "transformed_templates"), key
    assert sorted(sheets) == ["recons", "templates", "transformed_templates"]
    assert tuple(sheets["recons"].shape) == (3, rows * (H + 1) + 1, n * (W + 1) + 1)
    for v in sheets.values():
        assert v.is_cuda and v.dtype == torch.float32 and v.dim() == 3 and v.shape[0] == 3

    # the call left the step alone
    assert torch.equal(step.acc, acc_before)
    means_after = step.epoch_means()
    assert means_before.keys() == means_after.keys()
    for k in means_before:
        assert np.array_equal(np.asarray(means_before[k]), np.asarray(means_after[k])), k

    want = _sheets_the_materialising_way(step, res, n)
    for k in want:
        assert tuple(sheets[k].shape) == tuple(want[k].shape), k
        assert torch.equal(sheets[k].cpu(), want[k]), k
    # the default result (one eager forward of the staged batch) gives the same sheets
    again = step.validation_images()
    for k in want:
        assert torch.equal(again[k], sheets[k]), k
    assert torch.equal(replay(), loss_before)


def test_eval_step_with_recon_mse_is_unchanged_by_the_fused_mode(monkeypatch):
    """SCAE.loss's ``res.rec.pdf.mode()`` (recon_mse_weight > 0) under the evaluation
    step's no_grad now comes from the fused kernel: the same loss, bit for bit, as with
    the routing switched off."""
    from torch_scae_amd import EvalStep, _lib, ops
    from torch_scae_amd.distributions import GaussianMixture
    cfg, _, sd, g = full_size_params("cfg2")
    cfg = dict(cfg, scae_params=dict(cfg["scae_params"], recon_mse_weight=0.7))
    B = 32
    image = torch.rand(B, *cfg["image_shape"], generator=g).cuda()
    label = torch.randint(0, cfg["n_classes"], (B,), generator=g).cuda()
    losses, ran = [], []
    for fused in (True, False):
        if not fused:
            monkeypatch.setattr(GaussianMixture, "_fused_image", lambda self: False)
        model = _model(cfg, sd)
        step = EvalStep(model, B, cfg["image_shape"], use_graph=False)
        torch.manual_seed(3)
        ops.reset_noise()
        with _lib.recorder() as launches:
            losses.append(step(image, label).clone())
        ran.append("scae_render_gmm_mode_f32" in [fn.__name__ for fn, _a, _k in launches])
        assert not step.fused
    assert ran == [True, False]
    assert torch.equal(losses[0], losses[1]), losses
