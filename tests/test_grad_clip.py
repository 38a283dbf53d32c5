"""Clipping by global norm (Lightning's Trainer(gradient_clip_val), which applies
torch.nn.utils.clip_grad_norm_ before every optimiser step) without a GPU: the flat optimisers'
CPU forms against clip_grad_norm_ followed by stock torch.optim RMSprop / Adam, or followed by
the unclipped CPU RAdam / LookAhead forms (test_optimizers.py holds those to the reference's
trajectories); the settings' validation and factory.make_train_step's reading of
``trainer.gradient_clip_val``.  The HIP kernels and TrainStep's use of them:
test_grad_clip_gpu.py."""
import copy
import math

import pytest
import torch
import torch.nn as nn

from tests.test_optimizers import REF_CFG, YAML


class Net(nn.Module):
    """Two linear layers, a parameter that never gets a gradient and one that gets a gradient
    on even steps only (its flat slot then has to be zero on odd steps)."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.body = nn.Sequential(nn.Linear(6, 5), nn.ReLU(), nn.Linear(5, 3))
        self.unused = nn.Parameter(torch.randn(4))
        self.sometimes = nn.Parameter(torch.randn(3))

    def loss(self, x, it):
        out = (self.body(x) ** 2).sum()
        if it % 2 == 0:
            out = out + (self.sometimes * x[:, :3]).sum()
        return out


def batch(it):
    g = torch.Generator().manual_seed(100 + it)
    return torch.randn(8, 6, generator=g) * 3


def flat_run(kind, wd, la, clip, steps=6):
    """The flat optimiser's CPU form with ``gradient_clip_val=clip``: parameters and the norm
    after every step."""
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    net = Net()
    flat = FlatParameters(net)
    opt = make_optimizer(kind, flat, lr=1e-2, eps=1e-3, weight_decay=wd, look_ahead=la,
                         look_ahead_k=2, gradient_clip_val=clip)
    out = []
    for it in range(steps):
        flat.clear_grads()
        net.loss(batch(it), it).backward()
        flat.gather_grads()
        if it % 2:    # the slot of a parameter without a gradient holds zeros
            off = flat.offsets[[id(p) for p in flat.params].index(id(net.sometimes))]
            assert float(flat.flat_grad[off:off + 3].abs().max()) == 0.0
        opt.step()
        norm = float(opt.grad_norm) if opt.max_norm else None
        out.append(({k: v.detach().clone() for k, v in net.named_parameters()}, norm))
    return out


def torch_run(kind, wd, clip, steps=6):
    """clip_grad_norm_ over the parameters that have a gradient, then torch.optim."""
    net = Net()
    params = list(net.parameters())
    opt = torch.optim.RMSprop(params, lr=1e-2, momentum=0.9, eps=1e-3, weight_decay=wd) \
        if kind == "rmsprop" else torch.optim.Adam(params, lr=1e-2, eps=1e-3, weight_decay=wd)
    out = []
    for it in range(steps):
        opt.zero_grad(set_to_none=True)
        net.loss(batch(it), it).backward()
        norm = float(nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], clip))
        opt.step()
        out.append(({k: v.detach().clone() for k, v in net.named_parameters()}, norm))
    return out


def clip_then_flat_run(kind, wd, la, clip, steps=6):
    """clip_grad_norm_ on the module's own gradients, then the UNCLIPPED flat optimiser."""
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    net = Net()
    flat = FlatParameters(net)
    opt = make_optimizer(kind, flat, lr=1e-2, eps=1e-3, weight_decay=wd, look_ahead=la,
                         look_ahead_k=2)
    out = []
    for it in range(steps):
        flat.clear_grads()
        net.loss(batch(it), it).backward()
        norm = float(nn.utils.clip_grad_norm_(
            [p for p in flat.params if p.grad is not None], clip))
        flat.gather_grads()
        opt.step()
        out.append(({k: v.detach().clone() for k, v in net.named_parameters()}, norm))
    return out


def assert_same_runs(ours, ref, skip=()):
    for it, ((pa, na), (pb, nb)) in enumerate(zip(ours, ref)):
        assert na == pytest.approx(nb, rel=1e-6), (it, na, nb)
        for k in pa:
            if k in skip:
                continue
            err = float((pa[k] - pb[k]).abs().max())
            assert err <= 1e-6 * max(float(pb[k].abs().max()), 1e-30), (it, k, err)


# clip 0.5: below every step's norm (coef < 1); 1e6: far above it (coef == 1)
@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("clip", [0.5, 1e6])
def test_cpu_forms_equal_clip_grad_norm_and_torch_optim(kind, wd, clip):
    """Every step's norm and parameters.  The intermittent parameter's values are compared
    for RMSprop with weight decay only -- the unclipped passes' behaviour, outside clipping:
    without weight decay the flat passes run over the whole buffer, where a zero gradient
    slot still moves with the momentum (torch skips a parameter without a gradient), and
    Adam's bias corrections follow one step count for the whole buffer (torch counts per
    parameter)."""
    ours, ref = flat_run(kind, wd, False, clip), torch_run(kind, wd, clip)
    norms = [n for _, n in ref]
    assert (min(norms) > clip) if clip < 1 else (max(norms) < clip), norms
    assert_same_runs(ours, ref, skip=() if wd and kind == "rmsprop" else ("sometimes",))
    # the parameter without a gradient is untouched (torch.optim skips it, weight decay too)
    assert torch.equal(ours[-1][0]["unused"], Net().unused.detach())


@pytest.mark.parametrize("kind,wd,la", [("radam", 0.0, False), ("radam", 1e-2, False),
                                        ("radam", 0.0, True), ("adam", 1e-2, True),
                                        ("rmsprop", 0.0, True)])
@pytest.mark.parametrize("clip", [0.5, 1e6])
def test_cpu_forms_equal_clip_grad_norm_then_the_unclipped_form(kind, wd, la, clip):
    ours, ref = flat_run(kind, wd, la, clip), clip_then_flat_run(kind, wd, la, clip)
    assert_same_runs(ours, ref)


def test_large_clip_value_gives_the_unclipped_bits():
    """coef == 1: multiplying by 1.0 is exact, so a clip far above the norm is the unclipped
    step bit for bit."""
    for kind in ("rmsprop", "adam", "radam"):
        a, b = flat_run(kind, 1e-2, False, 1e6), flat_run(kind, 1e-2, False, 0.0)
        for (pa, _), (pb, _) in zip(a, b):
            for k in pa:
                assert torch.equal(pa[k], pb[k]), (kind, k)


@pytest.mark.parametrize("value,want", [(0, 0.0), (0.0, 0.0), (-1.5, 0.0), (1, 1.0),
                                        (0.25, 0.25)])
def test_clip_value_off_and_on(value, want):
    from torch_scae_amd.data_parallel import FlatParameters, clip_value, make_optimizer
    assert clip_value(value) == want
    opt = make_optimizer("adam", FlatParameters(Net()), lr=1e-3, eps=1e-8,
                         gradient_clip_val=value)
    assert opt.max_norm == want and (opt.grad_norm is None) == (want == 0.0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), "1.0", None, True,
                                 [1.0]])
def test_bad_clip_values_raise(bad):
    from torch_scae_amd.data_parallel import FlatParameters, clip_value, make_optimizer
    from torch_scae_amd.train_step import TrainStep
    with pytest.raises(ValueError):
        clip_value(bad)
    with pytest.raises(ValueError):
        make_optimizer("rmsprop", FlatParameters(Net()), lr=1e-3, eps=1e-8,
                       gradient_clip_val=bad)
    with pytest.raises(ValueError):
        TrainStep(Net(), 4, (1, 16, 16), gradient_clip_val=bad)


def test_clipping_needs_an_optimizer():
    from torch_scae_amd.train_step import TrainStep
    with pytest.raises(ValueError):
        TrainStep(Net(), 4, (1, 16, 16), optimizer=None, gradient_clip_val=1.0)


def test_make_train_step_reads_trainer_gradient_clip_val(monkeypatch):
    """Absent (no trainer section, or one without the key): no argument, TrainStep's default
    (off); 0 or negative: off; positive: on; a bad value raises."""
    from torch_scae_amd import factory, train_step
    seen = []

    class Spy:
        def __init__(self, model, batch_size, image_shape, **kw):
            seen.append(kw)

    monkeypatch.setattr(train_step, "TrainStep", Spy)
    base = dict(REF_CFG, optimizer=YAML["rmsprop"])
    factory.make_train_step(None, base)
    assert "gradient_clip_val" not in seen[-1]
    factory.make_train_step(None, dict(base, trainer=dict(max_epochs=3)))
    assert "gradient_clip_val" not in seen[-1]
    for value, want in ((0, 0.0), (-2.0, 0.0), (1.0, 1.0), (0.5, 0.5)):
        factory.make_train_step(None, dict(base, trainer=dict(gradient_clip_val=value)))
        assert seen[-1]["gradient_clip_val"] == want
    for bad in ("x", float("nan"), float("inf")):
        with pytest.raises(ValueError):
            factory.make_train_step(None, dict(base, trainer=dict(gradient_clip_val=bad)))


def test_make_train_step_builds_a_clipping_step():
    """End to end on the CPU side: the TrainStep built from a config with
    trainer.gradient_clip_val carries it into its optimiser."""
    from torch_scae_amd import factory
    cfg = dict(REF_CFG, optimizer=YAML["adam"], trainer=dict(gradient_clip_val=0.75))
    step = factory.make_train_step(copy.deepcopy(Net()), cfg)
    assert step.opt.max_norm == 0.75 and step.last_grad_norm() is step.opt.grad_norm
    step = factory.make_train_step(Net(), dict(cfg, trainer=dict(gradient_clip_val=0)))
    assert step.opt.max_norm == 0.0 and step.last_grad_norm() is None
    assert math.isclose(factory.make_train_step(
        Net(), dict(cfg, trainer={})).opt.max_norm + 1.0, 1.0)
