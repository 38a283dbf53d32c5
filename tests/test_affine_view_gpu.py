"""``affine=`` views on the GPU: the standalone gather (scae_gather_batch_f32) equals the
views' CPU path bit for bit -- uint8 and fp32 datasets, 1 and 3 channels, 28 -> 40 and
32 -> 32, shuffled, split, wrapped short steps, rank 1 of 2, pure scale -- and Pillow's
recorded pixels on the fixture's coefficients; a ``step_from(view)`` trajectory (the step
prologue's staging AND image-layer workgroups resample the dataset) equals the one fed the CPU
path's batches, in every replay form and across an epoch boundary; ``evaluate`` / ``predict`` /
``encode`` of an affine view equal those of its materialised batches; a mid-epoch source-fed
step runs no torch operator and no copy, an epoch's first exactly one (the table upload)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from torch_scae_amd import data as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "affine_nearest_pil.npz")
CFG2 = dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24,
            scae_params=dict(reconstruct_alternatives=False))
CIFAR = dict(image_shape=(3, 32, 32), n_classes=10, n_part_caps=32, n_obj_caps=32,
             scae_params=dict(reconstruct_alternatives=False))    # BASELINE configs[4]'s shape
FULL = dict(degrees=25, scale=(0.8, 1.2), shear=(-10, 10, -5, 5))
SCALE = dict(degrees=0, scale=(0.6, 1.5))          # pure scale: k1 = k3 = 0


def _dataset(n, C=1, h=28, out=40, u8=True, label_u8=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (n, C, h, h), generator=g, dtype=torch.uint8)
    if not u8:
        imgs = torch.rand(n, C, h, h, generator=g)
    labels = torch.randint(0, 10, (n,), generator=g)
    if label_u8:
        labels = labels.to(torch.uint8)
    return D.ResidentDataset(imgs, labels, out_size=(out, out), device="cuda")


# -- 1. the gather ---------------------------------------------------------------------------------
GATHER_CASES = [
    # u8 image, u8 label, C, h -> H, n, index (split), shuffle, translate, (rank, world), affine
    (True, True, 1, 28, 40, 1001, False, True, True, (0, 1), FULL),
    (True, False, 1, 28, 40, 1001, True, True, True, (1, 2), FULL),
    (False, False, 3, 32, 32, 999, True, False, True, (0, 2), FULL),
    (False, True, 3, 28, 40, 777, False, False, False, (1, 2), dict(degrees=(-180, 180))),
    (True, False, 3, 32, 32, 513, True, True, False, (0, 1), dict(degrees=10, shear=15)),
    (False, False, 1, 32, 32, 300, False, True, True, (1, 2), FULL),
    (True, False, 1, 28, 40, 640, False, True, True, (0, 1), SCALE),
    (False, False, 3, 32, 32, 640, True, False, True, (1, 2), SCALE),
    (True, True, 1, 28, 40, 333, False, True, True, (0, 1), dict(degrees=0)),
]


@pytest.mark.parametrize("case", GATHER_CASES)
def test_gather_equals_the_cpu_path(case):
    u8, lu8, C, h, H, n, split, shuffle, translate, (rank, world), affine = case
    ds = _dataset(n + 40 if split else n, C, h, H, u8, lu8)
    args = dict(shuffle=shuffle, translate=translate, seed=77, rank=rank, world=world,
                affine=affine)
    view = ds.split([n, 40], generator=torch.Generator().manual_seed(1), **args)[0] \
        if split else ds.view(**args)
    B = 48
    for epoch, step in ((0, 0), (3, view.steps_per_epoch(B) - 1), (3, 1)):
        image, label = view.gather(B, epoch=epoch, step=step)
        want_i, want_l = view.batch(epoch, step, B)
        assert torch.equal(image.cpu(), want_i), (epoch, step)
        assert torch.equal(label.cpu(), want_l), (epoch, step)
    if affine == SCALE:
        k = view.coefficients(0, view.positions(0, B))
        assert bool(((k[:, 1] == 0) & (k[:, 3] == 0) & (k[:, 0] != 65536)).all())
    if affine == dict(degrees=0):      # the bits of the view without the argument
        plain = ds.view(**dict(args, affine=None))
        assert torch.equal(view.gather(B, epoch=2, step=1)[0], plain.gather(B, epoch=2, step=1)[0])
    else:
        plain = ds.view(**dict(args, affine=None))
        assert not torch.equal(view.gather(B, epoch=2, step=1)[0],
                               plain.gather(B, epoch=2, step=1)[0])


WRAP_CASES = [
    # u8, C, h -> H, n, split, shuffle, world, B, affine
    (True, 1, 28, 40, 1001, False, True, 2, 48, FULL),
    (False, 3, 32, 32, 999, True, False, 2, 64, FULL),
    (True, 1, 28, 40, 100, True, True, 3, 48, FULL),          # n < world * B
    (False, 1, 28, 40, 97, False, False, 2, 48, SCALE),       # r = 1 < world
]


@pytest.mark.parametrize("case", WRAP_CASES)
def test_gather_of_the_wrapped_short_step_equals_the_cpu_path(case):
    u8, C, h, H, n, split, shuffle, world, B, affine = case
    ds = _dataset(n + 40 if split else n, C, h, H, u8)
    views = []
    for rank in range(world):
        args = dict(shuffle=shuffle, seed=77, rank=rank, world=world, drop_last=False,
                    affine=affine)
        views.append(ds.split([n, 40], generator=torch.Generator().manual_seed(1), **args)[0]
                     if split else ds.view(**args))
    spe, b = views[0].steps_per_epoch(B), views[0].remainder(B)
    assert b > 0
    wrapped = 0
    for epoch in (0, 3):
        for v in views:
            image, label = v.gather(b, epoch=epoch, position=spe * world * B)
            want_i, want_l = v.batch(epoch, spe, B)
            assert want_i.shape[0] == b
            assert torch.equal(image.cpu(), want_i), (epoch, v.rank)
            assert torch.equal(label.cpu(), want_l), (epoch, v.rank)
            wrapped += int((v.positions(spe, B) >= n).sum())
            assert v.desc(epoch, 0).affine_rows == n + world - 1
    assert wrapped == 2 * (world * b - (n - spe * world * B)) > 0


@pytest.mark.parametrize("group, out", [("a", 40), ("b", 32)])
@pytest.mark.parametrize("u8", [True, False])
def test_gather_on_the_fixture_equals_pillows_recorded_pixels(group, out, u8):
    """The fixture's coefficients handed to the launch as its table: the device's pixels are
    Pillow's (uint8 / 255, as ToTensor)."""
    from torch_scae_amd import _lib
    z = np.load(GOLDEN)
    images, coeffs = torch.from_numpy(z["images_" + group]), torch.from_numpy(z["coeffs_" + group])
    want = torch.from_numpy(z["pil_" + group]).to(torch.float32) / 255.0
    N = images.shape[0]
    ds = D.ResidentDataset(images if u8 else images.to(torch.float32) / 255.0,
                           torch.arange(N) % 10, out_size=(out, out), device="cuda")
    table = coeffs.to(torch.int32).contiguous().cuda()
    d = ds.view(translate=False).desc(0, 0)
    d.affine, d.affine_rows = table.data_ptr(), N
    image = torch.empty(N, ds.C, out, out, device="cuda")
    label = torch.empty(N, dtype=torch.int64, device="cuda")
    _lib.call("scae_gather_batch_f32", ctypes.c_void_p(image.data_ptr()),
              ctypes.c_void_p(label.data_ptr()), N, ctypes.byref(d),
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert torch.equal(image.cpu(), want)
    assert torch.equal(label.cpu(), torch.arange(N) % 10)
    assert torch.equal(image.cpu(), D.affine_warp(images, coeffs, (out, out)))


# -- 2. trajectories -----------------------------------------------------------------------------
def _train_step(cfg, B, **kw):
    from torch_scae_amd import factory
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(cfg).cuda().train()
    return TrainStep(model, B, cfg["image_shape"], **kw)


def _trajectory_parity(cfg, B, r, affine, **kw):
    """Two epochs of ``step_from`` over a ``drop_last=False`` view (2 full steps and a short
    one of r each) against ``step(image, label)`` on the CPU path's batches."""
    from torch_scae_amd import ops
    C, H = cfg["image_shape"][0], cfg["image_shape"][1]
    step = _train_step(cfg, B, **kw)
    step.capture()                   # (the warm-ups draw noise: before the snapshot)
    step.remainder_step(r).capture()
    snap = step.snapshot()
    ds = _dataset(2 * B + r, C, 28 if H == 40 else 32, H)

    def run(feed):
        step.restore(snap)
        torch.manual_seed(5)
        ops.reset_noise()
        view = ds.view(shuffle=True, seed=3, drop_last=False, affine=affine)
        losses = [float(feed(view)) for _ in range(6)]
        assert (view.epoch, view.cursor) == (2, 0)
        return losses, step.snapshot()

    def via_cpu(view):
        at = view.take_step(B)
        image, label = view.batch(at[0], at[1] // B, B)
        assert image.shape[0] == at.size
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
    # the batches were warped ones: the plain view's trajectory is another
    step.restore(snap)
    torch.manual_seed(5)
    ops.reset_noise()
    plain = ds.view(shuffle=True, seed=3, drop_last=False)
    assert [float(step.step_from(plain)) for _ in range(6)] != la


@pytest.mark.parametrize("replay", ["graph", "launches"])
def test_step_from_trajectory_equals_staged_batches(replay):
    _trajectory_parity(CFG2, 128, 88, FULL, replay=replay)


def test_step_from_without_prologue_equals_staged_batches():
    _trajectory_parity(CFG2, 128, 88, FULL, prologue=False)


def test_step_from_trajectory_on_unpadded_three_channel_images():
    _trajectory_parity(CIFAR, 64, 40, dict(degrees=15, scale=(0.9, 1.1)))


# -- 3. evaluation ---------------------------------------------------------------------------------
def _reseed():
    from torch_scae_amd import ops
    torch.manual_seed(9)
    ops.reset_noise()


def test_evaluate_predict_and_encode_of_an_affine_view():
    from torch_scae_amd import EvalStep, factory
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(CFG2).cuda().train()
    B = 128
    ev = EvalStep(model, B, CFG2["image_shape"])
    ds = _dataset(1000, 1, 28, 40)
    N = 2 * B + 37
    val = ds.split([N, 1000 - N], generator=torch.Generator().manual_seed(2), seed=4,
                   translate=False, affine=FULL)[0]
    ev.evaluate(val)                 # (captures the full and the remainder step)
    images, labels = val.materialise()
    plain = D.DatasetView(ds, val.index, translate=False, seed=4).materialise()[0]
    assert not torch.equal(images, plain)
    epoch = val.epoch
    _reseed()
    want = ev.evaluate(images.cuda(), labels.cuda())
    _reseed()
    got = ev.evaluate(val)
    assert val.epoch == epoch + 1
    assert want["batches"] == got["batches"] == 3
    for k in want:
        assert torch.equal(torch.as_tensor(got[k]), torch.as_tensor(want[k])), k
    # per-example records and capsule features of the warped examples, row for row
    ev.predict(val)
    images, labels = val.materialise()
    _reseed()
    pv = ev.predict(val)
    _reseed()
    pt = ev.predict(images.cuda(), labels.cuda())
    assert pv["rows"] == N and torch.equal(pv["label_int"], labels.cuda())
    assert torch.equal(pv["records"], pt["records"])
    assert torch.equal(pv["confusion"], pt["confusion"])
    ev.encode(val)
    images, labels = val.materialise()
    _reseed()
    fv = ev.encode(val)
    _reseed()
    ft = ev.encode(images.cuda(), labels.cuda())
    assert torch.equal(fv["label"], labels.cuda())
    assert torch.equal(fv["features"], ft["features"])
    assert torch.equal(fv["means"]["loss"], ft["means"]["loss"])


# -- 4. what a step costs on the host ----------------------------------------------------------
def test_mid_epoch_step_runs_no_torch_operator_and_no_copy_the_first_one_upload():
    from torch.profiler import ProfilerActivity, profile
    B = 128
    step = _train_step(CFG2, B)
    ds = _dataset(4 * B, 1, 28, 40)
    view = ds.view(shuffle=True, seed=1, affine=FULL)
    step.step_from(view)             # (capture; epoch 0's table)
    torch.cuda.synchronize()

    def names(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events()]

    def copies(ns):
        return [n for n in ns if "memcpy" in n.lower()]
    for _ in range(2):               # steps 1 and 2 of epoch 0
        src = names(lambda: step.step_from(view))
        assert not [n for n in src if n.startswith("aten::")] and not copies(src), src
    step.step_from(view)
    assert (view.epoch, view.cursor) == (1, 0)
    first = names(lambda: step.step_from(view))      # epoch 1's first step: its table
    # (one upload is two profiler events: the runtime call and the device's activity)
    calls = [n for n in copies(first) if n.startswith("hip")]
    moved = [n for n in copies(first) if n.startswith("Memcpy")]
    assert len(calls) == 1 and len(moved) == 1 and len(copies(first)) == 2, first
    assert "HtoD" in moved[0], first
    src = names(lambda: step.step_from(view))
    assert not [n for n in src if n.startswith("aten::")] and not copies(src), src
    # both epochs' tables are alive, no more
    assert len(view._tables) == 2
