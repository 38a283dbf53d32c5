"""``flip=``, ``max_shift=`` and ``interpolation="bilinear"`` views on the GPU: the standalone
gather (scae_gather_batch_f32) equals the views' CPU path bit for bit -- uint8 and fp32 data,
an unpadded and an asymmetrically padded size, rank 1 of 2, the wrapped short step, a second
epoch's table; a ``step_from(view)`` trajectory (the prologue's staging AND image-layer
workgroups sample the dataset) equals the one fed the CPU path's batches, in both replay
forms; ``evaluate`` of a bilinear test view equals that of its materialised batches; a default
view's step issues the launches it always did."""
import numpy as np
import pytest
import torch

from torch_scae_amd import data as D

pytestmark = pytest.mark.gpu

N, C, h, w, B = 21, 3, 6, 5, 4
WARP = dict(degrees=30, scale=(0.7, 1.3), shear=10)
CFG2 = dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24,
            scae_params=dict(reconstruct_alternatives=False))
CIFAR = dict(image_shape=(3, 32, 32), n_classes=10, n_part_caps=32, n_obj_caps=32,
             scae_params=dict(reconstruct_alternatives=False))
VIEWS = {
    "flip": dict(flip=True),
    "flip_shift": dict(flip=True, max_shift=(2, 3)),
    "flip_nearest_affine": dict(flip=True, affine=WARP),
    "bilinear_affine": dict(affine=WARP, interpolation="bilinear"),
    "bilinear_flip": dict(affine=WARP, interpolation="bilinear", flip=True, max_shift=(1, 2)),
}


def _small(u8, out):
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (N, C, h, w), generator=g, dtype=torch.uint8) if u8 \
        else torch.rand(N, C, h, w, generator=g)
    return D.ResidentDataset(imgs, torch.arange(N) % 10, out_size=out, device="cuda")


@pytest.mark.parametrize("kind", sorted(VIEWS))
@pytest.mark.parametrize("out", [(6, 5), (9, 8)])
@pytest.mark.parametrize("u8", [True, False])
def test_gather_equals_the_cpu_path(u8, out, kind):
    ds = _small(u8, out)
    view = ds.view(shuffle=True, seed=77, rank=1, world=2, drop_last=False, **VIEWS[kind])
    spe, b = view.steps_per_epoch(B), view.remainder(B)
    assert (spe, b) == (2, 3) and int(view.positions(spe, B).max()) >= N    # (a wrapped one)
    tables = []
    for epoch in (0, 1):
        for step in range(spe):
            image, label = view.gather(B, epoch=epoch, step=step)
            want_i, want_l = view.batch(epoch, step, B)
            assert torch.equal(image.cpu(), want_i), (epoch, step)
            assert torch.equal(label.cpu(), want_l), (epoch, step)
        image, label = view.gather(b, epoch=epoch, position=spe * 2 * B)
        want_i, want_l = view.batch(epoch, spe, B)
        assert want_i.shape[0] == b
        assert torch.equal(image.cpu(), want_i), epoch
        assert torch.equal(label.cpu(), want_l), epoch
        d = view.desc(epoch, 0)
        assert d.affine_rows == N + 1 and d.translate == (2 if "bilinear" in kind else 1)
        tables.append(d.affine)
    assert tables[0] != tables[1] and len(view._tables) == 2
    # the options did something: the view without them gives other pixels
    assert not torch.equal(view.gather(B, epoch=0, step=0)[0],
                           ds.view(shuffle=True, seed=77, rank=1, world=2,
                                   drop_last=False).gather(B, epoch=0, step=0)[0])


# -- trajectories -----------------------------------------------------------------------------
def _train_step(cfg, batch, **kw):
    from torch_scae_amd import factory
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(cfg).cuda().train()
    return TrainStep(model, batch, cfg["image_shape"], **kw)


def _big(n, Cn, hh, out):
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (n, Cn, hh, hh), generator=g, dtype=torch.uint8)
    return D.ResidentDataset(imgs, torch.randint(0, 10, (n,), generator=g),
                             out_size=(out, out), device="cuda")


def _three_steps_equal_staged_batches(cfg, batch, hh, **kw):
    from torch_scae_amd import ops
    Cn, H = cfg["image_shape"][0], cfg["image_shape"][1]
    step = _train_step(cfg, batch, **kw)
    step.capture()                   # (the warm-ups draw noise: before the snapshot)
    snap = step.snapshot()
    ds = _big(3 * batch + 5, Cn, hh, H)
    args = dict(shuffle=True, seed=3, affine=dict(degrees=15, scale=(0.9, 1.1)), flip=True,
                max_shift=(3, 4), interpolation="bilinear")

    def run(feed, **view_args):
        step.restore(snap)
        torch.manual_seed(5)
        ops.reset_noise()
        view = ds.view(**view_args)
        losses = [float(feed(view)) for _ in range(3)]
        return losses, step.snapshot()

    def via_cpu(view):
        epoch, pos = view.take_step(batch)
        image, label = view.batch(epoch, pos // batch, batch)
        return step(image.cuda(), label.cuda())
    la, sa = run(step.step_from, **args)
    lb, sb = run(via_cpu, **args)
    assert la == lb
    assert sa.keys() == sb.keys()
    for k, v in sa.items():
        if torch.is_tensor(v):
            assert torch.equal(v, sb[k]), k
        else:
            assert v == sb[k], k
    # the batches were sampled bilinearly: the nearest view's trajectory is another
    assert run(step.step_from, **dict(args, interpolation="nearest"))[0] != la


@pytest.mark.parametrize("replay", ["graph", "launches"])
def test_step_from_trajectory_equals_staged_batches(replay):
    _three_steps_equal_staged_batches(CFG2, 128, 28, replay=replay)


@pytest.mark.parametrize("replay", ["graph", "launches"])
def test_step_from_trajectory_on_unpadded_three_channel_images(replay):
    _three_steps_equal_staged_batches(CIFAR, 64, 32, replay=replay)


# -- evaluation ---------------------------------------------------------------------------------
def test_evaluate_of_a_bilinear_test_view():
    from torch_scae_amd import EvalStep, factory, ops
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(CFG2).cuda().train()
    batch = 128
    ev = EvalStep(model, batch, CFG2["image_shape"])
    ds = _big(2 * batch + 37, 1, 28, 40)
    val = ds.view(translate=False, seed=4, affine=dict(degrees=20), interpolation="bilinear")
    ev.evaluate(val)                 # (captures the full and the remainder step)
    images, labels = val.materialise()
    assert not torch.equal(images, ds.view(translate=False, seed=4,
                                           affine=dict(degrees=20)).materialise(val.epoch)[0])
    torch.manual_seed(9)
    ops.reset_noise()
    want = ev.evaluate(images.cuda(), labels.cuda())
    torch.manual_seed(9)
    ops.reset_noise()
    got = ev.evaluate(val)
    assert want["batches"] == got["batches"] == 3
    for k in want:
        assert torch.equal(torch.as_tensor(got[k]), torch.as_tensor(want[k])), k


# -- the default path ---------------------------------------------------------------------------
def test_a_default_views_step_issues_the_launches_it_always_did(monkeypatch):
    """A view built without the new arguments: a NULL table, `translate` 0 / 1, and per step
    the one prologue call plus the replay -- the library calls and the runtime's launch events
    of a step handed device tensors directly."""
    from torch.profiler import ProfilerActivity, profile
    from torch_scae_amd import ops
    batch = 128
    step = _train_step(CFG2, batch)
    ds = _big(6 * batch, 1, 28, 40)
    view = ds.view(shuffle=True, seed=1)
    d = view.desc(0, 0)
    assert not d.affine and d.affine_rows == 0 and d.translate == 1 and not view._tables
    step.step_from(view)             # (capture)
    image, label = view.gather(batch, epoch=0, step=0)
    step(image, label)
    torch.cuda.synchronize()
    seen = []
    real = ops._lib.call

    def spy(name, *a):
        seen.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops._lib, "call", spy)

    def events(fn):
        del seen[:]
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events()]
        assert not [n for n in names if n.startswith("aten::") or "memcpy" in n.lower()], names
        return list(seen), sorted(n for n in names if n.startswith("hip") and "Launch" in n)
    calls, launches = events(lambda: step.step_from(view))
    assert calls == ["scae_step_prologue_source_f32"], calls
    direct_calls, direct_launches = events(lambda: step(image, label))
    assert len(direct_calls) == 1 and launches and launches == direct_launches, \
        (launches, direct_launches)
    assert not view._tables
