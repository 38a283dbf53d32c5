"""A device-resident dataset on the GPU: the standalone gather (scae_gather_batch_f32) equals
the views' CPU path bit for bit; a training trajectory fed by ``TrainStep.step_from`` (the
source mode of the step prologue: its staging AND image-layer workgroups read the dataset)
equals the one fed the CPU path's batches through ``step(image, label)``; an epoch wrap;
no torch operator and no copy in a source-fed step; ``EvalStep.evaluate(view)``."""
import numpy as np
import pytest
import torch

from torch_scae_amd import data as D

pytestmark = pytest.mark.gpu

CFG2 = dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24,
            scae_params=dict(reconstruct_alternatives=False))
CFG3 = dict(CFG2, n_part_caps=48, n_obj_caps=64)    # BASELINE configs[2]'s shape


def _dataset(n, C, h, out, u8=True, label_u8=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (n, C, h, h), generator=g, dtype=torch.uint8)
    if not u8:
        imgs = torch.rand(n, C, h, h, generator=g)
    labels = torch.randint(0, 10, (n,), generator=g)
    if label_u8:
        labels = labels.to(torch.uint8)
    return D.ResidentDataset(imgs, labels, out_size=(out, out), device="cuda")


GATHER_CASES = [
    # u8 image, u8 label, C, h -> H, n, index (split), shuffle, translate, (rank, world)
    (True, True, 1, 28, 40, 1001, False, True, True, (0, 1)),
    (True, False, 1, 28, 40, 1001, True, True, True, (1, 2)),
    (False, False, 3, 32, 32, 999, True, False, True, (0, 2)),
    (False, True, 3, 28, 40, 777, False, False, False, (1, 2)),
    (True, False, 3, 32, 32, 513, True, True, False, (0, 1)),
]


@pytest.mark.parametrize("case", GATHER_CASES)
def test_gather_equals_the_cpu_path(case):
    u8, lu8, C, h, H, n, split, shuffle, translate, (rank, world) = case
    ds = _dataset(n + 40 if split else n, C, h, H, u8, lu8)
    args = dict(shuffle=shuffle, translate=translate, seed=77, rank=rank, world=world)
    view = ds.split([n, 40], generator=torch.Generator().manual_seed(1), **args)[0] \
        if split else ds.view(**args)
    B = 48
    for epoch, step in ((0, 0), (3, view.steps_per_epoch(B) - 1)):
        image, label = view.gather(B, epoch=epoch, step=step)
        want_i, want_l = view.batch(epoch, step, B)
        assert torch.equal(image.cpu(), want_i), (epoch, step)
        assert torch.equal(label.cpu(), want_l), (epoch, step)


def _train_step(cfg, B, **kw):
    from torch_scae_amd import factory
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(cfg).cuda().train()
    return TrainStep(model, B, cfg["image_shape"], **kw)


def _trajectory_parity(cfg, B, K, **kw):
    from torch_scae_amd import ops
    step = _train_step(cfg, B, **kw)
    step.capture()                   # (the warm-ups draw noise: before the snapshot)
    snap = step.snapshot()
    ds = _dataset(B * K + 11, 1, 28, 40)

    def run(feed):
        step.restore(snap)
        torch.manual_seed(5)
        ops.reset_noise()
        view = ds.view(shuffle=True, seed=3)
        losses = [float(feed(view)) for _ in range(K)]
        return losses, step.snapshot()

    def via_cpu(view):
        epoch, pos = view.take_step(B)
        image, label = view.batch(epoch, pos // B, B)
        return step(image.cuda(), label.cuda())
    la, sa = run(step.step_from)
    lb, sb = run(via_cpu)
    assert la == lb
    assert sa.keys() == sb.keys()
    for k, v in sa.items():
        if torch.is_tensor(v):
            assert torch.equal(v, sb[k]), k
        else:
            assert v == sb[k], k


@pytest.mark.parametrize("replay", ["graph", "launches"])
def test_step_from_trajectory_equals_staged_batches(replay):
    _trajectory_parity(CFG2, 128, 4, replay=replay)


def test_step_from_without_prologue_equals_staged_batches():
    _trajectory_parity(CFG2, 128, 3, prologue=False)


def test_step_from_bf16_at_configs2_shape():
    _trajectory_parity(CFG3, 1024, 3, autocast_dtype=torch.bfloat16)


def test_epoch_wrap_advances_the_epoch_and_decays_lr_once():
    B = 128
    step = _train_step(CFG2, B)
    ds = _dataset(3 * B + 5, 1, 28, 40)
    view = ds.view(shuffle=True, seed=1)
    lr = step.opt.lr
    step.step_from(view)
    assert (view.epoch, view.cursor) == (0, 1)
    loss = step.train_epoch(view)
    assert loss.is_cuda and torch.isfinite(loss)
    assert (view.epoch, view.cursor, step.steps) == (1, 0, 3)
    assert step.opt.lr == pytest.approx(lr * step.lr_decay_rate, rel=1e-12)


def test_source_fed_step_runs_no_torch_operator_and_no_copy():
    from torch.profiler import ProfilerActivity, profile
    B = 128
    step = _train_step(CFG2, B)
    ds = _dataset(4 * B, 1, 28, 40)
    view = ds.view(shuffle=True, seed=1)
    step.step_from(view)             # (capture)
    torch.cuda.synchronize()

    def names(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events()]
    src = names(lambda: step.step_from(view))
    assert not [n for n in src if n.startswith("aten::") or "memcpy" in n.lower()], src

    def path_b():
        rows = torch.randint(0, ds.n, (B,), device="cuda")
        image = D.pad_and_translate(ds.images[rows], (40, 40))
        step(image, ds.labels[rows])
    ops_b = names(path_b)
    assert sum(n.startswith("aten::") for n in ops_b) > 10
    assert any("memcpy" in n.lower() for n in ops_b)


def test_evaluate_view_equals_evaluate_of_the_materialised_split():
    from torch_scae_amd import EvalStep, factory, ops
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(CFG2).cuda().train()
    B = 128
    ev = EvalStep(model, B, CFG2["image_shape"])
    ds = _dataset(1000, 1, 28, 40)
    val = ds.split([2 * B + 37, 1000 - 2 * B - 37],
                   generator=torch.Generator().manual_seed(2), seed=4)[0]
    ev.evaluate(val)                 # (captures the full and the remainder step)
    images, labels = val.materialise()
    epoch = val.epoch
    torch.manual_seed(9)
    ops.reset_noise()
    want = ev.evaluate(images.cuda(), labels.cuda())
    torch.manual_seed(9)
    ops.reset_noise()
    got = ev.evaluate(val)
    assert val.epoch == epoch + 1
    assert want["batches"] == got["batches"] == 3
    for k in want:
        assert torch.equal(torch.as_tensor(got[k]), torch.as_tensor(want[k])), k
