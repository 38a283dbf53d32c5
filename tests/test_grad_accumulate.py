"""Gradient accumulation (Lightning's Trainer(accumulate_grad_batches=k)) without a GPU: the flat
optimisers' CPU forms -- ``accumulate()`` then ``step(grad_scale=1/k)`` -- against stock
torch.optim RMSprop / Adam (or the reference-checked CPU RAdam + LookAhead) stepped on
(g_1 + ... + g_k) / k, with and without weight decay and clipping; the host's schedule of
optimiser steps over a view's epoch; the settings' validation and factory.make_train_step's
reading of ``trainer.accumulate_grad_batches``; two gloo ranks that accumulate and all-reduce
once per group.  The HIP kernels and TrainStep's use of them: test_grad_accumulate_gpu.py."""
import copy
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from tests.test_data_parallel import _free_port
from tests.test_optimizers import REF_CFG, YAML


class Net(nn.Module):
    """Two linear layers, a parameter that never gets a gradient and one that gets a gradient
    on every fourth batch only (so a group of 3 has it in some batches, or in none)."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.body = nn.Sequential(nn.Linear(6, 5), nn.ReLU(), nn.Linear(5, 3))
        self.unused = nn.Parameter(torch.randn(4))
        self.sometimes = nn.Parameter(torch.randn(3))

    def loss(self, x, it):
        out = (self.body(x) ** 2).sum()
        if it % 4 == 0:
            out = out + (self.sometimes * x[:, :3]).sum()
        return out


def batch(it):
    g = torch.Generator().manual_seed(100 + it)
    return torch.randn(8, 6, generator=g) * 3


def groups(steps, k):
    """Lightning's groups of batch indices: k at a time, the last one short."""
    return [list(range(i, min(i + k, steps))) for i in range(0, steps, k)]


def flat_run(kind, wd, la, clip, k, steps=8):
    """The flat optimiser accumulating k batches: parameters (and the norm) after every
    optimiser step."""
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    net = Net()
    flat = FlatParameters(net)
    opt = make_optimizer(kind, flat, lr=1e-2, eps=1e-3, weight_decay=wd, look_ahead=la,
                         look_ahead_k=2, gradient_clip_val=clip, accumulate_grad_batches=k)
    out = []
    for grp in groups(steps, k):
        for it in grp:
            flat.clear_grads()
            net.loss(batch(it), it).backward()
            flat.gather_grads()
            if it != grp[-1]:
                opt.accumulate()
        opt.step(grad_scale=1.0 / k)
        assert float(opt.acc.abs().max()) == 0.0
        norm = float(opt.grad_norm) if opt.max_norm else None
        out.append(({n: v.detach().clone() for n, v in net.named_parameters()}, norm))
    return out


def group_grads(net, grp, k):
    """{parameter: (g_1 + g_2 + ...) * fp32(1/k)} over the group's batches, in batch order; a
    parameter without a gradient in any of them is absent."""
    sums = {}
    for it in grp:
        for p in net.parameters():
            p.grad = None
        net.loss(batch(it), it).backward()
        for p in net.parameters():
            if p.grad is not None:
                sums[p] = p.grad.clone() if p not in sums else sums[p] + p.grad
    return {p: g * (1.0 / k) for p, g in sums.items()}


def torch_run(kind, wd, clip, k, steps=8):
    net = Net()
    params = list(net.parameters())
    opt = torch.optim.RMSprop(params, lr=1e-2, momentum=0.9, eps=1e-3, weight_decay=wd) \
        if kind == "rmsprop" else torch.optim.Adam(params, lr=1e-2, eps=1e-3, weight_decay=wd)
    out = []
    for grp in groups(steps, k):
        grads = group_grads(net, grp, k)
        for p in params:
            p.grad = grads.get(p)
        norm = float(nn.utils.clip_grad_norm_(list(grads), clip)) if clip else None
        opt.step()
        out.append(({n: v.detach().clone() for n, v in net.named_parameters()}, norm))
    return out


def sum_then_flat_run(kind, wd, la, clip, k, steps=8):
    """(g_1 + ...) / k (clipped by clip_grad_norm_) fed to the NON-accumulating flat
    optimiser, with the group's parameters marked as having a gradient."""
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    net = Net()
    flat = FlatParameters(net)
    opt = make_optimizer(kind, flat, lr=1e-2, eps=1e-3, weight_decay=wd, look_ahead=la,
                         look_ahead_k=2)
    out = []
    for grp in groups(steps, k):
        grads = group_grads(net, grp, k)
        norm = float(nn.utils.clip_grad_norm_(
            [_holder(g) for g in grads.values()], clip)) if clip else None
        if clip:
            grads = {p: g * min(1.0, clip / (norm + 1e-6)) for p, g in grads.items()}
        flat.flat_grad.zero_()
        for p, off in zip(flat.params, flat.offsets):
            p._flat_was_set = p in grads
            if p in grads:
                flat.flat_grad[off:off + p.numel()].copy_(grads[p].reshape(-1))
        opt.step()
        out.append(({n: v.detach().clone() for n, v in net.named_parameters()}, norm))
    return out


def _holder(g):
    h = torch.zeros_like(g, requires_grad=True)
    h.grad = g.clone()
    return h


def assert_same_runs(ours, ref, rel=1e-6, skip=()):
    assert len(ours) == len(ref)
    for it, ((pa, na), (pb, nb)) in enumerate(zip(ours, ref)):
        if nb is not None:
            assert na == pytest.approx(nb, rel=1e-6), (it, na, nb)
        for key in pa:
            if key in skip:
                continue
            err = float((pa[key] - pb[key]).abs().max())
            assert err <= rel * max(float(pb[key].abs().max()), 1e-30), (it, key, err)


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("k", [2, 3])
def test_cpu_forms_equal_torch_optim_on_the_group_mean(kind, wd, clip, k):
    """8 batches in groups of k (the last one short, still scaled by 1/k): the accumulating
    flat optimiser equals torch.optim stepped on (g_1 + ...) / k; clip 0.5 is below every
    group's norm.  The intermittent parameter is compared for RMSprop with weight decay, as
    test_grad_clip.py does (the flat passes' behaviour without accumulation: without weight
    decay they run over the whole buffer, where a zero slot still moves with the momentum,
    and Adam keeps one step count): a group in which only an earlier batch gave it a gradient
    decays it, a group without one skips it, as torch does."""
    ours, ref = flat_run(kind, wd, False, clip, k), torch_run(kind, wd, clip, k)
    if clip:
        assert min(n for _, n in ref) > clip
    assert_same_runs(ours, ref, skip=() if wd and kind == "rmsprop" else ("sometimes",))
    assert torch.equal(ours[-1][0]["unused"], Net().unused.detach())


@pytest.mark.parametrize("kind,wd,la", [("radam", 0.0, False), ("radam", 1e-2, False),
                                        ("radam", 1e-2, True), ("adam", 0.0, True),
                                        ("rmsprop", 1e-2, True)])
@pytest.mark.parametrize("clip", [0.0, 0.5])
def test_cpu_forms_equal_the_plain_form_on_the_group_mean(kind, wd, la, clip):
    """RAdam and the LookAhead forms (whose CPU forms test_optimizers.py holds to the
    reference's trajectories): accumulating 3 batches equals the plain form stepped on the
    group's mean; LookAhead's k counts optimiser steps."""
    assert_same_runs(flat_run(kind, wd, la, clip, 3), sum_then_flat_run(kind, wd, la, clip, 3))


def test_flush_steps_on_acc_alone():
    """``flush`` (a group cut short): the step on acc with the flat gradient buffer zeroed."""
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    outs = []
    for flush in (True, False):
        net = Net()
        flat = FlatParameters(net)
        opt = make_optimizer("adam", flat, lr=1e-2, eps=1e-3, accumulate_grad_batches=4)
        for it in range(2):
            flat.clear_grads()
            net.loss(batch(it), it).backward()
            flat.gather_grads()
            if flush or it == 0:
                opt.accumulate()
        if flush:
            opt.flush(0.25)
        else:
            opt.step(grad_scale=0.25)
        outs.append(flat.flat_param.clone())
        assert float(opt.acc.abs().max()) == 0.0
    assert torch.equal(*outs)


# -- the schedule -----------------------------------------------------------------------------
def _cpu_dataset(n, h=4, out=8):
    from torch_scae_amd import data as D
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (n, 1, h, h), generator=g, dtype=torch.uint8)
    return D.ResidentDataset(imgs, torch.arange(n) % 10, out_size=(out, out), device="cpu")


@pytest.mark.parametrize("n", [40, 47, 56, 9])
@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_update_schedule_follows_lightnings_rule(n, drop_last, k):
    """Over two epochs of a view (B = 8), the host marks batch i of the epoch as an optimiser
    step exactly when (i + 1) % k == 0 or i is the epoch's last batch (the short one too)."""
    from torch_scae_amd.train_step import update_at
    B = 8
    view = _cpu_dataset(n).view(shuffle=True, seed=1, drop_last=drop_last)
    spe = n // B + (0 if drop_last or n % B == 0 else 1)
    assert view.steps_in_epoch(B) == spe
    got, want = [], []
    for epoch in range(2):
        for i in range(spe):
            got.append(update_at(view, B, k))
            at = view.take_step(B)
            assert at[0] == epoch
            want.append((i + 1) % k == 0 or i == spe - 1)
    assert got == want
    assert sum(got) == 2 * -(-spe // k)


# -- settings -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, -1, True, False, 2.0, "2", None, {0: 2}, 1.5])
def test_bad_accumulate_values_raise(bad):
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    from torch_scae_amd.train_step import TrainStep
    with pytest.raises(ValueError):
        make_optimizer("rmsprop", FlatParameters(Net()), lr=1e-3, eps=1e-3,
                       accumulate_grad_batches=bad)
    with pytest.raises(ValueError):
        TrainStep(Net(), 4, (1, 16, 16), accumulate_grad_batches=bad)


def test_accumulation_needs_an_optimizer_and_k1_keeps_no_buffer():
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    from torch_scae_amd.train_step import TrainStep
    with pytest.raises(ValueError):
        TrainStep(Net(), 4, (1, 16, 16), optimizer=None, accumulate_grad_batches=2)
    opt = make_optimizer("adam", FlatParameters(Net()), lr=1e-3, eps=1e-3)
    assert opt.acc is None and opt.accumulate_grad_batches == 1
    with pytest.raises(ValueError):
        opt.accumulate()


def test_make_train_step_reads_trainer_accumulate_grad_batches(monkeypatch):
    """Absent: no argument (TrainStep's default 1); an int >= 1 passes; a bad value raises."""
    from torch_scae_amd import factory, train_step
    seen = []

    class Spy:
        def __init__(self, model, batch_size, image_shape, **kw):
            seen.append(kw)

    monkeypatch.setattr(train_step, "TrainStep", Spy)
    base = dict(REF_CFG, optimizer=YAML["rmsprop"])
    factory.make_train_step(None, base)
    assert "accumulate_grad_batches" not in seen[-1]
    factory.make_train_step(None, dict(base, trainer=dict(max_epochs=3)))
    assert "accumulate_grad_batches" not in seen[-1]
    for value in (1, 2, 7):
        factory.make_train_step(None, dict(base, trainer=dict(accumulate_grad_batches=value)))
        assert seen[-1]["accumulate_grad_batches"] == value
    for bad in (0, "x", 2.5, True, {5: 2}):
        with pytest.raises(ValueError):
            factory.make_train_step(None, dict(base, trainer=dict(accumulate_grad_batches=bad)))


def test_make_train_step_builds_an_accumulating_step():
    from torch_scae_amd import factory
    cfg = dict(REF_CFG, optimizer=YAML["adam"], trainer=dict(accumulate_grad_batches=4))
    step = factory.make_train_step(copy.deepcopy(Net()), cfg)
    assert step.accumulate_grad_batches == 4 and step.opt.acc is not None
    assert step.opt.acc.shape == step.flat.flat_grad.shape
    step = factory.make_train_step(Net(), dict(cfg, trainer={}))
    assert step.accumulate_grad_batches == 1 and step.opt.acc is None


# -- two ranks -----------------------------------------------------------------------------------
K, WORLD, GROUPS = 3, 2, 2


def _net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Linear(6, 5), nn.Tanh(), nn.Linear(5, 3))


def _global_batch(i):
    return torch.randn(8, 6, generator=torch.Generator().manual_seed(50 + i))


def _acc_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from torch_scae_amd.data_parallel import (FlatParameters, all_reduce_gradients,
                                              make_optimizer)
    net = _net()
    flat = FlatParameters(net)
    opt = make_optimizer("adam", flat, lr=1e-2, eps=1e-3, accumulate_grad_batches=K)
    calls = []
    real = dist.all_reduce

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    dist.all_reduce = counted
    try:
        for i in range(K * GROUPS):
            shard = _global_batch(i)[rank * 4:(rank + 1) * 4]
            flat.clear_grads()
            net(shard).square().sum().backward()
            flat.gather_grads()
            if (i + 1) % K:
                opt.accumulate()
                continue
            opt.fold()                          # acc + g, one SUM all-reduce of it
            all_reduce_gradients(flat, average=False)
            opt.step(grad_scale=1.0 / (K * world), with_acc=False)
    finally:
        dist.all_reduce = real
    out[rank] = (flat.flat_param.clone(), len(calls))
    dist.destroy_process_group()


def test_two_ranks_accumulate_and_all_reduce_once_per_group():
    """Each rank accumulates its shard's gradients; one all-reduce per optimiser step; the
    result equals one process accumulating the global batches' mean-over-ranks gradients."""
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_acc_worker, args=(WORLD, _free_port(), out), nprocs=WORLD, join=True)
    (p0, c0), (p1, c1) = out[0], out[1]
    assert torch.equal(p0, p1) and c0 == c1 == GROUPS
    net = _net()
    flat = FlatParameters(net)
    opt = make_optimizer("adam", flat, lr=1e-2, eps=1e-3, accumulate_grad_batches=K)
    for i in range(K * GROUPS):
        flat.clear_grads()
        (net(_global_batch(i)).square().sum() / WORLD).backward()
        flat.gather_grads()
        if (i + 1) % K:
            opt.accumulate()
        else:
            opt.step(grad_scale=1.0 / K)
    assert torch.allclose(flat.flat_param, p0, rtol=1e-5, atol=1e-7)


def test_a_step_without_active_parameters_still_clears_acc():
    """With weight decay, a group in which no parameter got a gradient updates nothing, and
    acc is 0 afterwards all the same (the GPU forms' invariant)."""
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    for kind in ("adam", "radam", "rmsprop"):
        net = Net()
        flat = FlatParameters(net)
        opt = make_optimizer(kind, flat, lr=1e-2, eps=1e-3, weight_decay=1e-2, look_ahead=True,
                             accumulate_grad_batches=2)
        for p in flat.params:
            p._flat_was_set = False
        opt.acc.fill_(1.0)
        before = flat.flat_param.clone()
        opt.step(grad_scale=0.5)
        assert float(opt.acc.abs().max()) == 0.0, kind
        assert torch.equal(flat.flat_param, before), kind


def test_loading_optimizer_state_drops_a_pending_group():
    """load_optimizer_state_dict in the middle of a group: acc zeroed, nothing pending, both
    counts at the state's step count."""
    from torch_scae_amd.train_step import TrainStep
    step = TrainStep(Net(), 4, (1, 16, 16), optimizer="adam", accumulate_grad_batches=3)
    step._acc_state.update(pending=2, optimizer_steps=5)
    step.steps = 17
    sd = step.optimizer_state_dict()
    assert sd["state"][0]["step"] == 0     # (the device count: no optimiser step taken here)
    sd["state"] = {i: dict(st, step=torch.tensor(4.0)) for i, st in sd["state"].items()}
    step.opt.acc.fill_(2.0)
    step.load_optimizer_state_dict(sd)
    assert float(step.opt.acc.abs().max()) == 0.0
    assert step._acc_state == {"pending": 0, "optimizer_steps": 4} and step.steps == 4
