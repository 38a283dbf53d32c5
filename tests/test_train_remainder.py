"""An epoch's short last batch without a GPU: the positions, rows and shifts a
``drop_last=False`` view hands its ranks (DistributedSampler's padding: positions past the
view's end read its first examples again, with shifts of their own), ``take_step`` through
spe + 1 steps, the view's state across a pending remainder, and how ``TrainStep`` builds its
remainder step -- sharing the parameters, optimiser and counters of the full step.  The
device gather and the trained trajectories are in test_train_remainder_gpu.py."""
import numpy as np
import pytest
import torch

from torch_scae_amd import data as D


def _cpu_dataset(n, h=4, out=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (n, 1, h, h), generator=g, dtype=torch.uint8)
    return D.ResidentDataset(imgs, torch.arange(n) % 10, out_size=(out, out), device="cpu")


# (n, B, world): r = n - spe*world*B divisible by world, not divisible, r < world, n < world*B
POSITION_CASES = [(70, 16, 1), (70, 8, 2), (71, 8, 2), (49, 16, 3), (50, 16, 3), (97, 16, 3),
                  (98, 16, 3), (33, 16, 2), (20, 16, 2), (40, 16, 3), (5, 16, 3), (3, 16, 3)]


@pytest.mark.parametrize("n,B,world", POSITION_CASES)
@pytest.mark.parametrize("shuffle", [False, True])
def test_remainder_positions_cover_the_epoch(n, B, world, shuffle):
    ds = _cpu_dataset(n)
    views = [ds.view(shuffle=shuffle, seed=5, rank=k, world=world, drop_last=False)
             for k in range(world)]
    spe = n // (world * B)
    r = n - spe * world * B
    b = -(-r // world)
    assert all(v.steps_per_epoch(B) == spe for v in views)
    assert all(v.remainder(B) == b for v in views)
    assert all(v.steps_in_epoch(B) == spe + (r > 0) for v in views)
    done = spe * world * B
    epoch = 2
    rows, positions = [], []
    for k, v in enumerate(views):
        for s in range(spe):
            rows.append(v.indices_and_shifts(epoch, s, B)[0])
        if not r:
            continue
        p = v.positions(spe, B)
        assert torch.equal(p, done + k * b + torch.arange(b))
        positions.append(p)
        rr, shifts = v.rows_and_shifts(epoch, p)
        rows.append(rr)
        assert rr.numel() == b
        # a wrapped position repeats the row of the epoch's position p - n ...
        wrapped = p >= n
        if bool(wrapped.any()):
            first = v.rows_and_shifts(epoch, p[wrapped] - n)[0]
            assert torch.equal(rr[wrapped], first)
        # ... and draws its shift from the unwrapped position
        assert torch.equal(shifts, D.translate_shifts(p, epoch, v.seed, ds.pads))
    seen = torch.cat(rows)
    assert torch.equal(torch.unique(seen), torch.arange(n))
    if r:
        allp = torch.cat(positions)
        assert allp.numel() == world * b and int(allp.max()) < 2 * n
        assert int((allp >= n).sum()) == world * b - r
    if world == 1:
        assert not any(bool((p >= n).any()) for p in positions)


def test_wrapped_rows_are_the_epochs_first_and_the_batch_is_their_transform():
    ds = _cpu_dataset(50)
    v = ds.view(shuffle=True, seed=3, rank=2, world=3, drop_last=False)
    B = 16                               # spe 1, r 2: ranks take 1 each, rank 2 wraps
    assert v.remainder(B) == 1
    p = v.positions(1, B)
    assert p.tolist() == [50]
    rows, shifts = v.rows_and_shifts(4, p)
    assert torch.equal(rows, D.feistel_order(torch.tensor([0]), 50, v.seed, 4))
    image, label = v.batch(4, 1, B)
    assert image.shape == (1, 1, 8, 8) and label.shape == (1,)
    want = D.pad_and_translate(ds.images[rows], (8, 8), shifts=shifts)
    assert torch.equal(image, want)
    assert torch.equal(label, ds.labels[rows])
    # the same view with drop_last: positions and batches as before
    w = ds.view(shuffle=True, seed=3, rank=2, world=3)
    assert w.remainder(B) == 0 and w.steps_in_epoch(B) == 1
    assert torch.equal(w.positions(1, B), 1 * 3 * B + 2 * B + torch.arange(B))


def test_take_step_goes_through_the_short_step_then_wraps():
    ds = _cpu_dataset(70)
    v = ds.view(shuffle=True, seed=1, drop_last=False)
    got = [v.take_step(16) for _ in range(11)]
    assert got == [(0, 0), (0, 16), (0, 32), (0, 48), (0, 64),
                   (1, 0), (1, 16), (1, 32), (1, 48), (1, 64), (2, 0)]
    assert [a.size for a in got] == [16, 16, 16, 16, 6] * 2 + [16]
    # two ranks: 70 = 2*2*16 + 6 -> 3 each, from position 64
    r1 = ds.view(rank=1, world=2, drop_last=False)
    got = [r1.take_step(16) for _ in range(4)]
    assert got == [(0, 0), (0, 32), (0, 64), (1, 0)]
    assert [a.size for a in got] == [16, 16, 3, 16]
    # n < world * B: every step is the short one
    small = _cpu_dataset(5).view(rank=0, world=2, drop_last=False)
    got = [small.take_step(16) for _ in range(3)]
    assert got == [(0, 0), (1, 0), (2, 0)] and {a.size for a in got} == {3}


def test_drop_last_views_take_steps_as_before():
    ds = _cpu_dataset(70)
    v = ds.view(shuffle=True, seed=1)
    assert v.drop_last
    got = [v.take_step(16) for _ in range(5)]
    assert got == [(0, 0), (0, 16), (0, 32), (0, 48), (1, 0)]
    assert {a.size for a in got} == {16}
    views = ds.split([60, 10], generator=torch.Generator().manual_seed(0), drop_last=False)
    assert [w.drop_last for w in views] == [False, False]
    assert views[0].remainder(16) == 12 and views[1].remainder(16) == 10


def test_state_round_trips_a_pending_remainder():
    ds = _cpu_dataset(70)
    v = ds.view(shuffle=True, seed=1, drop_last=False)
    for _ in range(4):
        v.take_step(16)
    sd = v.state_dict()
    assert sd["drop_last"] is False and (sd["epoch"], sd["cursor"]) == (0, 4)
    w = ds.view(shuffle=True, seed=1)            # (drop_last comes with the state)
    w.load_state_dict(sd)
    assert not w.drop_last
    a, b = v.take_step(16), w.take_step(16)
    assert a == b == (0, 64) and a.size == b.size == 6
    assert [v.take_step(16) for _ in range(6)] == [w.take_step(16) for _ in range(6)]


def test_views_without_drop_last_need_an_example_per_rank():
    ds = _cpu_dataset(5)
    with pytest.raises(ValueError):
        ds.view(rank=0, world=6, drop_last=False)
    assert ds.view(rank=4, world=5, drop_last=False).remainder(16) == 1


def test_descriptors_carry_wrap_only_without_drop_last():
    ds = _cpu_dataset(10)
    assert ds.view().desc(0, 0).wrap == 0
    assert ds.view(drop_last=False).desc(0, 0).wrap == 1


def test_wrap_bounds_of_the_entry_points_without_a_gpu():
    """wrap = 1 lets positions run to 2n (no further); wrap = 0 keeps the old bound; any
    other wrap is refused.  Every call here is refused before a HIP call."""
    import ctypes
    from torch_scae_amd import _lib
    lib = _lib.load()

    def desc(**kw):
        d = _lib.BatchSourceDesc()
        d.images, d.labels, d.rows, d.n = 0x1000, 0x1000, 100, 100
        d.C, d.h, d.w, d.H, d.W, d.world = 1, 28, 28, 40, 40, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    fake = ctypes.c_void_p(0x1000)
    assert ctypes.sizeof(_lib.BatchSourceDesc) >= _lib.BatchSourceDesc.wrap.offset + 4
    for bad in (dict(position=97), dict(position=197, wrap=1), dict(position=0, wrap=2),
                dict(position=193, rank=1, world=2, wrap=1)):
        assert lib.scae_gather_batch_f32(fake, fake, 4, ctypes.byref(desc(**bad)), None) == -1, bad
        assert lib.scae_step_prologue_source_f32(fake, fake, 4, ctypes.byref(desc(**bad)), None,
                                                 0, None, None, None, None) == -1, bad


# -- TrainStep's remainder step: construction and routing (no forward runs here) ------------
SMALL = dict(image_shape=(1, 16, 16), n_classes=4, n_part_caps=5, n_obj_caps=4,
             pcae_cnn_encoder_params=dict(out_channels=[64, 64], kernel_sizes=[3, 3],
                                          strides=[2, 1]),
             pcae_template_generator_params=dict(template_size=(5, 5)),
             ocae_encoder_set_transformer_params=dict(dim_hidden=8, dim_out=64, n_layers=2),
             ocae_decoder_capsule_params=dict(dim_caps=4, hidden_sizes=(8,)),
             scae_params=dict(reconstruct_alternatives=False))


@pytest.mark.parametrize("optimizer,la", [("rmsprop", False), ("adam", False), ("radam", True)])
def test_remainder_step_shares_the_training_state(optimizer, la):
    from torch_scae_amd import factory
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(SMALL)
    B = 8
    step = TrainStep(model, B, (1, 16, 16), use_graph=False, optimizer=optimizer,
                     look_ahead=la, weight_decay=0.0)
    ptr = step.flat.flat_param.data_ptr()
    rem = step.remainder_step(3)
    assert step.flat.flat_param.data_ptr() == ptr
    assert rem.flat is step.flat and rem.opt is step.opt and rem.model is step.model
    assert rem.opt.eps == 1e-2 / B ** 2
    assert rem.plan is not step.plan and rem.plan.noise_salt != step.plan.noise_salt == 0
    assert rem.image.shape == (3, 1, 16, 16) and rem.label.shape == (3,)
    assert step.image.shape == (B, 1, 16, 16)
    for k in ("use_graph", "replay", "autocast_dtype", "collective", "split",
              "in_graph_collective", "fuse_kernels", "lr_decay_rate", "world"):
        assert getattr(rem, k) == getattr(step, k), k
    assert rem.plan.sums_to_optimizer == step.plan.sums_to_optimizer
    # one host count for both
    rem.steps += 2
    step.steps += 1
    assert step.steps == rem.steps == 3
    # cached for its size, rebuilt for another
    assert step.remainder_step(3) is rem
    other = step.remainder_step(5)
    assert other is not rem and other.image.shape[0] == 5 and step.remainder_step(5) is other
    with pytest.raises(ValueError):
        other.remainder_step(2)


def test_short_batches_out_of_range_are_refused():
    from torch_scae_amd import factory
    from torch_scae_amd.train_step import TrainStep
    torch.manual_seed(0)
    step = TrainStep(factory.make_scae(SMALL), 4, (1, 16, 16), use_graph=False)
    for b in (0, 5, 9):
        with pytest.raises(ValueError):
            step(torch.zeros(b, 1, 16, 16), torch.zeros(b, dtype=torch.long))
        with pytest.raises(ValueError):
            step.training_step(torch.zeros(b, 1, 16, 16), torch.zeros(b, dtype=torch.long))
    for b in (0, 4, -1, 2.0):
        with pytest.raises(ValueError):
            step.remainder_step(b)
    assert step.steps == 0 and step._rem is None


def test_a_dropped_step_frees_its_remainder_step_without_the_cycle_collector():
    """No reference cycle between the two steps: refcounting frees them where they are
    dropped, never the cyclic collector at some later point (which could free their graphs
    in the middle of another step's capture)."""
    import gc
    import weakref
    from torch_scae_amd import factory
    from torch_scae_amd.train_step import TrainStep
    torch.manual_seed(0)
    step = TrainStep(factory.make_scae(SMALL), 4, (1, 16, 16), use_graph=False)
    gone = weakref.ref(step.remainder_step(3))
    was = gc.isenabled()
    gc.disable()
    try:
        del step
        assert gone() is None
    finally:
        if was:
            gc.enable()
