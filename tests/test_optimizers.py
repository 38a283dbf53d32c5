"""The optimisers the reference offers besides RMSprop -- Adam, RAdam, LookAhead over any of
the three (base_experiment.py:44-77, torch_scae/optimizers.py) -- on the flat buffers:
the CPU forms and the state-dict interchange here, without a GPU; the fused HIP passes
(scae_flat_opt_step_f32 / scae_flat_opt_sums_step_f32) and TrainStep's use of them in
test_optimizers_gpu.py.

tests/golden/optim_trajectories.npz (tests/golden/make_optimizer_golden.py) holds 12
steps of the reference's own RAdam / LookAhead and stock torch.optim Adam / RMSprop."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "optim_trajectories.npz")
LR, GAMMA, DECAY_AFTER, EPS = 1e-2, 0.9, 6, 1e-2 / 128.0 ** 2
STATE_KEYS = {"rmsprop": ("square_avg", "momentum_buffer"),
              "adam": ("exp_avg", "exp_avg_sq"), "radam": ("exp_avg", "exp_avg_sq")}
# (optimiser, weight decay, LookAhead): the cases tests/golden/make_optimizer_golden.py records
CASES = [(kind, wd, False) for kind in ("rmsprop", "adam", "radam") for wd in (0.0, 1e-2)] + \
    [(kind, 0.0, True) for kind in ("rmsprop", "adam", "radam")] + [("adam", 1e-2, True)]


def case_name(kind, wd, la):
    return f"{kind}_wd{wd:g}" + ("_la" if la else "")


def golden():
    return np.load(GOLDEN)


class Three(nn.Module):
    """The golden file's three tensors as the parameters of a module."""

    def __init__(self, init):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(torch.as_tensor(x).clone()) for x in init])


def make_flat_opt(kind, flat, wd, la, **kw):
    from torch_scae_amd.data_parallel import make_optimizer
    return make_optimizer(kind, flat, lr=LR, eps=EPS, weight_decay=wd, look_ahead=la,
                          look_ahead_k=5, look_ahead_alpha=0.5, **kw)


def state_of(opt, kind):
    if kind == "rmsprop":
        return {"square_avg": opt.square_avg, "momentum_buffer": opt.buf}
    return {"exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}


@pytest.mark.parametrize("kind,wd,la", CASES, ids=[case_name(*c) for c in CASES])
def test_cpu_forms_follow_the_reference_trajectories(kind, wd, la):
    """RMSpropFlat / AdamFlat / RAdamFlat (with and without LookAhead) in their CPU form,
    12 steps from the golden start on the golden gradients, one ExponentialLR step
    between steps 6 and 7: parameters, moments and slow weights after every step within
    1e-6 of the tensor's largest entry of the reference's."""
    from torch_scae_amd.data_parallel import FlatParameters
    d = golden()
    name = case_name(kind, wd, la)
    net = Three([d[f"init{j}"] for j in range(3)])
    flat = FlatParameters(net)
    opt = make_flat_opt(kind, flat, wd, la)
    keys = STATE_KEYS[kind] + (("slow_buffer",) if la else ())
    for s in range(12):
        assert opt.lr == pytest.approx(float(d[f"{name}/lr"][s]), rel=1e-12)
        for j, (p, off) in enumerate(zip(flat.params, flat.offsets)):
            flat.flat_grad[off:off + p.numel()] = torch.from_numpy(d[f"grad{j}"][s])
        opt.step()
        # (plain RMSprop keeps no step count: its update does not depend on one)
        assert int(opt.step_state[0]) == (s + 1 if la or kind != "rmsprop" else 0)
        mine = dict(state_of(opt, kind), slow_buffer=opt.slow)
        for j, (p, off) in enumerate(zip(flat.params, flat.offsets)):
            sl = slice(off, off + p.numel())
            for key, ours in [("param", flat.flat_param)] + [(k, mine[k]) for k in keys]:
                ref = torch.from_numpy(d[f"{name}/{key}{j}"][s])
                err = float((ours[sl] - ref).abs().max())
                assert err <= 1e-6 * max(float(ref.abs().max()), 1e-30), \
                    (name, s + 1, key, j, err)
        if s + 1 == DECAY_AFTER:
            opt.decay_lr(GAMMA)
    # the trajectories do what the fixture is for: RAdam's switch, LookAhead's syncs
    moved = d[f"{name}/param1"]
    assert np.abs(moved[-1] - d["init1"]).max() > 1e-4


def stock(kind, params, wd=0.0):
    if kind == "rmsprop":
        return torch.optim.RMSprop(params, lr=LR, momentum=0.9, eps=EPS, weight_decay=wd)
    if kind == "adam":
        return torch.optim.Adam(params, lr=LR, eps=EPS, weight_decay=wd)
    return torch.optim.RAdam(params, lr=LR, eps=EPS, weight_decay=wd,
                             decoupled_weight_decay=True)


def small_net():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(6, 5), nn.ReLU(), nn.Linear(5, 3))
    net.unused = nn.Parameter(torch.zeros(4))      # never gets a gradient
    return net


@pytest.mark.parametrize("kind", ["rmsprop", "adam", "radam"])
def test_state_dict_round_trip_with_stock_torch_optim(kind):
    """optimizer_state_dict after 7 CPU steps loads into the stock optimiser over the
    model's parameters, and one more step on both sides agrees; the other way round, a
    stock optimiser's state after 7 steps loads into ours and the next steps agree."""
    from torch_scae_amd.data_parallel import (FlatParameters, load_optimizer_state_dict,
                                              optimizer_state_dict)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(7, 6, generator=g) for _ in range(9)]

    def ours_step(net, flat, opt, x):
        flat.clear_grads()
        net(x).square().sum().backward()
        flat.gather_grads()
        opt.step()

    def stock_step(net, opt, x):
        opt.zero_grad()
        net(x).square().sum().backward()
        opt.step()

    # ours -> stock
    a, b = small_net(), small_net()
    flat = FlatParameters(a)
    opt_a = make_flat_opt(kind, flat, 0.0, False)
    for x in xs[:7]:
        ours_step(a, flat, opt_a, x)
    sd = optimizer_state_dict(opt_a, list(a.parameters()), steps=7)
    assert set(sd["state"]) == set(range(len(list(a.parameters()))))
    assert all(float(st["step"]) == 7 for st in sd["state"].values())
    assert set(sd["state"][0]) == {"step", *STATE_KEYS[kind]}
    with torch.no_grad():
        for pb, pa in zip(b.parameters(), a.parameters()):
            pb.copy_(pa)
    opt_b = stock(kind, list(b.parameters()))
    opt_b.load_state_dict(sd)
    for x in xs[7:]:
        ours_step(a, flat, opt_a, x)
        stock_step(b, opt_b, x)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-6, atol=1e-7), (kind, (pa - pb).abs().max())
    # stock -> ours
    c, e = small_net(), small_net()
    opt_c = stock(kind, list(c.parameters()))
    for x in xs[:7]:
        stock_step(c, opt_c, x)
    with torch.no_grad():
        for pe, pc in zip(e.parameters(), c.parameters()):
            pe.copy_(pc)
    flat_e = FlatParameters(e)
    opt_e = make_flat_opt(kind, flat_e, 0.0, False)
    assert load_optimizer_state_dict(opt_e, list(e.parameters()), opt_c.state_dict()) == 7
    assert int(opt_e.step_state[0]) == 7
    for x in xs[7:]:
        stock_step(c, opt_c, x)
        ours_step(e, flat_e, opt_e, x)
    for pc, pe in zip(c.parameters(), e.parameters()):
        assert torch.allclose(pc, pe, rtol=1e-6, atol=1e-7), (kind, (pc - pe).abs().max())
    # hyper-parameters a captured step holds cannot be swapped in
    bad = opt_c.state_dict()
    bad["param_groups"][0]["eps"] = 1e-3
    with pytest.raises(ValueError):
        load_optimizer_state_dict(opt_e, list(e.parameters()), bad)


def test_look_ahead_state_dict_keys_slow_weights_by_parameter_index():
    """With LookAhead the export carries the slow weights keyed by parameter index (the
    reference keys them by id()), and loading it back reproduces the run."""
    from torch_scae_amd.data_parallel import (FlatParameters, load_optimizer_state_dict,
                                              optimizer_state_dict)
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(7, 6, generator=g) for _ in range(12)]
    runs = []
    for resume in (False, True):
        net = small_net()
        flat = FlatParameters(net)
        opt = make_flat_opt("adam", flat, 0.0, True)
        for i, x in enumerate(xs):
            if resume and i == 7:
                sd = optimizer_state_dict(opt, list(net.parameters()))
                assert sd["param_groups"][0]["lookahead_k"] == 5
                assert set(sd["slow_state"]) == set(sd["state"])
                net2 = small_net()
                with torch.no_grad():
                    for p2, p in zip(net2.parameters(), net.parameters()):
                        p2.copy_(p)
                net, flat = net2, FlatParameters(net2)
                opt = make_flat_opt("adam", flat, 0.0, True)
                load_optimizer_state_dict(opt, list(net.parameters()), sd)
            flat.clear_grads()
            net(x).square().sum().backward()
            flat.gather_grads()
            opt.step()
        runs.append(flat.flat_param.clone())
    assert torch.equal(runs[0], runs[1])


REF_CFG = dict(data_loader=dict(batch_size=128),
               meta_optimizer=dict(look_ahead=False, look_ahead_k=5, look_ahead_alpha=0.5),
               lr_scheduler=dict(active=True, decay_rate=0.997),
               model=dict(image_shape=[1, 16, 16]))
YAML = {"rmsprop": dict(type="RMSprop", learning_rate=3e-5, momentum=0.9, weight_decay=0.0),
        "adam": dict(type="Adam", learning_rate=3e-5, weight_decay=0.0),
        "radam": dict(type="RAdam", learning_rate=3e-5, weight_decay=0.0)}


def test_make_train_step_maps_the_reference_config(monkeypatch):
    """factory.make_train_step: each of the reference's three optimizer yaml files, the
    LookAhead switch (k, alpha read from meta_optimizer) and the scheduler switch give
    the matching TrainStep arguments; an unknown type raises."""
    from torch_scae_amd import factory, train_step
    seen = []

    class Spy:
        def __init__(self, model, batch_size, image_shape, **kw):
            seen.append((batch_size, image_shape, kw))

    monkeypatch.setattr(train_step, "TrainStep", Spy)
    for kind, opt in YAML.items():
        factory.make_train_step(None, dict(REF_CFG, optimizer=opt))
        bs, shape, kw = seen[-1]
        assert bs == 128 and shape == (1, 16, 16)
        assert kw["optimizer"] == kind and kw["lr"] == 3e-5 and kw["weight_decay"] == 0.0
        assert kw["lr_decay_rate"] == 0.997 and kw["look_ahead"] is False
        assert ("momentum" in kw) == (kind == "rmsprop")
    cfg = dict(REF_CFG, optimizer=YAML["radam"],
               meta_optimizer=dict(look_ahead=True, look_ahead_k=6, look_ahead_alpha=0.25),
               lr_scheduler=dict(active=False, decay_rate=0.997))
    factory.make_train_step(None, cfg)
    kw = seen[-1][2]
    assert kw["look_ahead"] is True and kw["look_ahead_k"] == 6
    assert kw["look_ahead_alpha"] == 0.25 and kw["lr_decay_rate"] is None
    with pytest.raises(ValueError):
        factory.make_train_step(None, dict(REF_CFG, optimizer=dict(YAML["adam"], type="SGD")))


def test_make_optimizer_choices():
    from torch_scae_amd.data_parallel import (AdamFlat, FlatParameters, RAdamFlat,
                                              RMSpropFlat, make_optimizer)
    flat = FlatParameters(small_net())
    for name, cls in (("rmsprop", RMSpropFlat), ("Adam", AdamFlat), ("RAdam", RAdamFlat)):
        opt = make_optimizer(name, flat, lr=1e-3, eps=1e-8)
        assert type(opt) is cls and opt.slow is None and opt.look_ahead_k == 0
    assert make_optimizer("adam", flat, 1e-3, 1e-8, look_ahead=True).slow is not None
    with pytest.raises(ValueError):
        make_optimizer("sgd", flat, lr=1e-3, eps=1e-8)
    with pytest.raises(ValueError):
        make_optimizer("adam", flat, 1e-3, 1e-8, look_ahead=True, look_ahead_k=0)
