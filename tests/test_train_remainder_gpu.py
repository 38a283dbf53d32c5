"""An epoch's short last batch on the GPU: the gather with wrapped positions equals the views'
CPU path bit for bit for every rank; a trajectory of batches 4, 4, 3 follows the oracle
stepped by stock torch optimisers (and the CPU RAdam / LookAhead forms); ``train_epoch`` over
a ``drop_last=False`` view equals the same batches staged through ``step(image, label)``, in
every replay form; the remainder step shares the full step's state and log; a source-fed
remainder step runs no torch operator and no copy; collective modes match the plain step."""
import numpy as np
import pytest
import torch

from oracle import scae_oracle as O
from torch_scae_amd import data as D

pytestmark = pytest.mark.gpu

CFG2 = dict(image_shape=(1, 40, 40), n_classes=10, n_part_caps=24, n_obj_caps=24,
            scae_params=dict(reconstruct_alternatives=False))
CFG3 = dict(CFG2, n_part_caps=48, n_obj_caps=64)    # BASELINE configs[2]'s shape
SMALL = dict(image_shape=(1, 16, 16), n_classes=4, n_part_caps=5, n_obj_caps=4,
             pcae_cnn_encoder_params=dict(out_channels=[64, 64], kernel_sizes=[3, 3],
                                          strides=[2, 1]),
             pcae_template_generator_params=dict(template_size=(5, 5)),
             ocae_encoder_set_transformer_params=dict(dim_hidden=8, dim_out=64, n_layers=2),
             ocae_decoder_capsule_params=dict(dim_caps=4, hidden_sizes=(8,)),
             scae_params=dict(reconstruct_alternatives=False))


def _dataset(n, C=1, h=28, out=40, u8=True, label_u8=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (n, C, h, h), generator=g, dtype=torch.uint8)
    if not u8:
        imgs = torch.rand(n, C, h, h, generator=g)
    labels = torch.randint(0, 10, (n,), generator=g)
    if label_u8:
        labels = labels.to(torch.uint8)
    return D.ResidentDataset(imgs, labels, out_size=(out, out), device="cuda")


def _close(a, b, atol, rtol, what):
    """|a - b| <= atol + rtol |b| elementwise (golden_util.assert_close's bar)."""
    a, b = a.double(), b.double()
    excess = (a - b).abs() - (atol + rtol * b.abs())
    assert a.shape == b.shape and float(excess.max()) <= 0, (what, float(excess.max()))


# -- 1. the gather with wrapped positions ------------------------------------------------------
GATHER_CASES = [
    # u8 image, u8 label, C, h -> H, n, index (split), shuffle, translate, world, B
    (True, True, 1, 28, 40, 1001, False, True, True, 2, 48),
    (True, False, 1, 28, 40, 1001, True, True, True, 3, 48),
    (False, False, 3, 32, 32, 999, True, False, True, 2, 64),
    (False, True, 3, 28, 40, 777, False, False, False, 3, 48),
    (True, False, 1, 28, 40, 100, True, True, False, 3, 48),    # n < world * B
    (False, False, 1, 28, 40, 97, False, False, True, 2, 48),   # r = 1 < world
]


@pytest.mark.parametrize("case", GATHER_CASES)
def test_gather_of_the_short_step_equals_the_cpu_path(case):
    u8, lu8, C, h, H, n, split, shuffle, translate, world, B = case
    ds = _dataset(n + 40 if split else n, C, h, H, u8, lu8)
    views = []
    for rank in range(world):
        args = dict(shuffle=shuffle, translate=translate, seed=77, rank=rank, world=world,
                    drop_last=False)
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
            if spe:    # the full steps of a wrapping view: as before
                image, label = v.gather(B, epoch=epoch, step=spe - 1)
                want_i, want_l = v.batch(epoch, spe - 1, B)
                assert torch.equal(image.cpu(), want_i) and torch.equal(label.cpu(), want_l)
    assert wrapped == 2 * (world * b - (n - spe * world * B))


# -- 2. a trajectory against the oracle -----------------------------------------------------------
def _mirror(kind, la, P, lr, wd, B):
    """(step(grads), decay(gamma)) of the CPU side: stock torch.optim RMSprop / Adam, or the
    CPU RAdam / LookAhead forms test_optimizers.py holds to the reference, over P."""
    import torch.nn as nn
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    eps = 1e-2 / B ** 2
    if not la and kind in ("rmsprop", "adam"):
        ps = list(P.values())
        opt = torch.optim.RMSprop(ps, lr=lr, momentum=0.9, eps=eps, weight_decay=wd) \
            if kind == "rmsprop" else torch.optim.Adam(ps, lr=lr, eps=eps, weight_decay=wd)

        def step(grads):
            opt.zero_grad(set_to_none=True)
            for k, p in P.items():
                p.grad = grads[k]
            opt.step()

        def decay(gamma):
            for grp in opt.param_groups:
                grp["lr"] *= gamma
        return step, decay
    mod = nn.Module()
    names = list(P)
    for i, k in enumerate(names):
        setattr(mod, f"p{i}", nn.Parameter(P[k].detach().clone()))
    flat = FlatParameters(mod)
    opt = make_optimizer(kind, flat, lr=lr, eps=eps, weight_decay=wd, look_ahead=la,
                         look_ahead_k=5, look_ahead_alpha=0.5)
    for i, k in enumerate(names):        # P now reads the flat buffer
        P[k] = getattr(mod, f"p{i}")

    offset = {id(p): off for p, off in zip(flat.params, flat.offsets)}

    def step(grads):
        flat.flat_grad.zero_()
        for i, k in enumerate(names):
            if grads[k] is not None:
                p = getattr(mod, f"p{i}")
                flat.flat_grad[offset[id(p)]:offset[id(p)] + p.numel()] = grads[k].reshape(-1)
        opt.step()
    return step, opt.decay_lr


@pytest.mark.parametrize("kind,la,n", [("rmsprop", False, 11), ("adam", False, 11),
                                       ("radam", False, 11), ("adam", True, 11),
                                       ("rmsprop", False, 9)])
def test_epochs_with_a_short_batch_follow_the_oracle(kind, la, n):
    """Two epochs of batches 4, 4, n - 8 (eager, fixed noise): loss and log keys within 1e-4
    of the oracle's, final parameters within the bars of
    test_hip_model.py::test_training_step_trajectory_vs_oracle_and_torch_rmsprop; eps is the
    configured B's throughout (base_experiment.py:47)."""
    from torch_scae_amd import factory
    from torch_scae_amd.nn_utils import fixed_noise
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(SMALL)
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.normal_(0, 0.1)
    B = 4
    lr, wd = (2e-3, 1e-3) if kind == "rmsprop" else (1e-3, 0.0)
    P = {k: v.clone().requires_grad_(True) for k, v in model.state_dict().items()}
    ocfg = O.prepare_model_params(**SMALL)
    cpu_step, cpu_decay = _mirror(kind, la, P, lr, wd, B)
    model = model.cuda().train()
    step = TrainStep(model, B, (1, 16, 16), lr=lr, use_graph=False, optimizer=kind,
                     look_ahead=la, weight_decay=wd, lr_decay_rate=0.5)
    g = torch.Generator().manual_seed(7)
    sizes = [B] * (n // B) + ([n % B] if n % B else [])
    for epoch in range(2):
        for it, b in enumerate(sizes):
            image = torch.rand(b, 1, 16, 16, generator=g)
            label = torch.randint(0, 4, (b,), generator=g)
            noise = [torch.rand(b, 5, generator=g), torch.rand(b, 4, 1, generator=g),
                     torch.rand(b, 4, 5, generator=g)]
            ref_loss, ref_log, ref_grads = O.train_step(P, ocfg, image, label, noise)
            cpu_step(ref_grads)
            with fixed_noise([x.clone() for x in noise]):
                out = step.training_step(image.cuda(), label.cuda())
            what = (epoch, it, b)
            assert abs(float(out["loss"]) - float(ref_loss)) <= \
                1e-4 * max(1.0, abs(float(ref_loss))), (what, float(out["loss"]),
                                                        float(ref_loss))
            assert set(out["log"]) == set(ref_log) | {"loss", "accuracy"}
            for k, v in ref_log.items():
                assert abs(float(out["log"][k]) - float(v)) <= \
                    1e-4 * max(1.0, abs(float(v))), (what, k)
        step.end_epoch()
        cpu_decay(0.5)
    assert step.steps == 2 * len(sizes)
    assert step._rem is not None and step._rem.image.shape[0] == sizes[-1]
    if step.opt.counts_steps:
        assert int(step.opt.step_state[0]) == 2 * len(sizes)
    sd = model.state_dict()
    for k, p in P.items():
        _close(sd[k].cpu(), p.detach(), 1e-4, 2e-3, "param " + k)


# -- 3. replayed epochs against staged batches ---------------------------------------------------
def _train_step(cfg, B, **kw):
    from torch_scae_amd import factory
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(cfg).cuda().train()
    return TrainStep(model, B, cfg["image_shape"], **kw)


def _state(step):
    torch.cuda.synchronize()
    return step.snapshot()


def _assert_same_state(sa, sb):
    assert sa.keys() == sb.keys()
    for k, v in sa.items():
        if torch.is_tensor(v):
            assert torch.equal(v, sb[k]), k
        else:
            assert v == sb[k], k


def _epochs_parity(cfg, B, r, epochs=2, **kw):
    from torch_scae_amd import ops
    step = _train_step(cfg, B, **kw)
    step.capture()                   # (the warm-ups draw noise: before the snapshot)
    ptr = step.flat.flat_param.data_ptr()
    step.remainder_step(r).capture()
    assert step.flat.flat_param.data_ptr() == ptr
    snap = step.snapshot()
    ds = _dataset(2 * B + r if B < 1024 else B + r)
    spe = (ds.n - r) // B

    def run(feed):
        step.restore(snap)
        torch.manual_seed(5)
        ops.reset_noise()
        view = ds.view(shuffle=True, seed=3, drop_last=False)
        assert view.steps_in_epoch(B) == spe + 1 and view.remainder(B) == r
        losses = []
        for _ in range(epochs):
            losses += feed(view)
        return losses, _state(step)

    def via_source(view):
        out = []
        epoch = view.epoch
        while view.epoch == epoch:
            out.append(float(step.step_from(view)))
        step.end_epoch()
        return out

    def via_cpu(view):
        out = []
        for s in range(view.steps_in_epoch(B)):
            at = view.take_step(B)
            image, label = view.batch(at[0], s, B)
            assert image.shape[0] == at.size
            out.append(float(step(image.cuda(), label.cuda())))
        step.end_epoch()
        return out

    def via_train_epoch(view):
        step.train_epoch(view)
        return []
    la, sa = run(via_source)
    lb, sb = run(via_cpu)
    _, sc = run(via_train_epoch)
    assert la == lb and len(la) == epochs * (spe + 1)
    _assert_same_state(sa, sb)
    _assert_same_state(sa, sc)
    assert sa["steps"] == epochs * (spe + 1)
    assert step.flat.flat_param.data_ptr() == ptr
    return step


@pytest.mark.parametrize("replay", ["graph", "launches"])
def test_train_epoch_equals_staged_batches(replay):
    step = _epochs_parity(CFG2, 128, 88, replay=replay)
    if replay == "launches":
        assert step._klist and step._rem._klist, "a step did not replay as a launch list"


def test_train_epoch_without_prologue_equals_staged_batches():
    _epochs_parity(CFG2, 128, 88, prologue=False)


def test_train_epoch_bf16_at_configs2_shape():
    _epochs_parity(CFG3, 1024, 728, autocast_dtype=torch.bfloat16)


# -- 4. shared state ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,la", [("rmsprop", False), ("radam", True)])
def test_counts_lr_and_snapshot_across_the_short_step(kind, la):
    from torch_scae_amd import ops
    B = 128
    step = _train_step(CFG2, B, optimizer=kind, look_ahead=la)
    ds = _dataset(2 * B + 88)
    view = ds.view(shuffle=True, seed=2, drop_last=False)
    lr0 = step.opt.lr
    for e in range(2):
        step.train_epoch(view)
        assert (view.epoch, view.cursor, step.steps) == (e + 1, 0, 3 * (e + 1))
        assert step.opt.lr == pytest.approx(lr0 * step.lr_decay_rate ** (e + 1), rel=1e-12)
    if step.opt.counts_steps:
        assert int(step.opt.step_state[0]) == 6
    # snapshot before a short step; the rest of the epoch twice from it
    step.step_from(view)
    step.step_from(view)
    snap = step.snapshot()
    vsd = view.state_dict()
    outs = []
    for _ in range(2):
        step.restore(snap)
        view.load_state_dict(vsd)
        torch.manual_seed(11)
        ops.reset_noise()
        loss = float(step.step_from(view))      # the short step
        assert view.cursor == 0
        step.step_from(view)                    # a full one behind it
        outs.append((loss, _state(step)))
    assert outs[0][0] == outs[1][0]
    _assert_same_state(outs[0][1], outs[1][1])
    assert outs[0][1]["steps"] == 10


def test_short_batches_outside_a_view_and_their_errors():
    """``step(image, label)`` and ``training_step`` with a short batch (an ordinary
    drop_last=False loader): the remainder step runs; another size rebuilds it."""
    B = 128
    step = _train_step(CFG2, B)
    g = torch.Generator().manual_seed(1)
    for b in (88, 88, 5):
        image = torch.rand(b, 1, 40, 40, generator=g).cuda()
        label = torch.randint(0, 10, (b,), generator=g).cuda()
        out = step.training_step(image, label)
        assert out["log"]["loss"].shape == () and torch.isfinite(out["loss"])
        assert step._rem.image.shape[0] == b
    assert step.steps == 3 and step.graph is None     # (the full step never ran)
    with pytest.raises(ValueError):
        step(torch.zeros(B + 1, 1, 40, 40, device="cuda"),
             torch.zeros(B + 1, dtype=torch.long, device="cuda"))


# -- 5. the training log ----------------------------------------------------------------------------
def test_log_holds_the_short_steps_row():
    B = 128
    step = _train_step(CFG2, B, log_steps=8)
    ds = _dataset(2 * B + 88)
    view = ds.view(shuffle=True, seed=4, drop_last=False)
    for e in range(2):
        loss = step.train_epoch(view)
        torch.cuda.synchronize()
        assert loss.data_ptr() == step._rem.loss.data_ptr()
        hist, steps = step.log_history()
        assert steps == list(range(3 * (e + 1)))
        assert hist["loss"][-1].item() == loss.item()
        assert step.last_log()["loss"].item() == loss.item()
        assert int(step.train_log.step) == step.train_log.count == 3 * (e + 1)
        m = step.training_epoch_end()
        assert m["batches"] == 3
        rows = hist["loss"][-3:].double()
        assert float(m["loss"]) == float(np.float32(float(rows.sum()) / 3))
    lr = hist["learning_rate"].tolist()
    assert lr[0] == lr[1] == lr[2] and lr[3] == lr[4] == lr[5] < lr[2]


# -- 6. no operator, no copy --------------------------------------------------------------------------
def test_source_fed_short_step_runs_no_torch_operator_and_no_copy():
    from torch.profiler import ProfilerActivity, profile
    B = 128
    step = _train_step(CFG2, B, log_steps=4)
    ds = _dataset(2 * B + 88)
    view = ds.view(shuffle=True, seed=1, drop_last=False)
    step.train_epoch(view)           # (captures both steps)
    step.step_from(view)
    step.step_from(view)
    torch.cuda.synchronize()
    assert view.cursor == 2
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step.step_from(view)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    assert not [x for x in names if x.startswith("aten::") or "memcpy" in x.lower()], names
    assert view.cursor == 0 and int(step.train_log.step) == 6


# -- 7. collectives ---------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_collective_short_steps_match_the_plain_step(nccl_group, use_graph):
    from torch_scae_amd import factory, ops
    from torch_scae_amd.train_step import TrainStep
    B = 8
    ds = _dataset(2 * B + 5, h=12, out=16)

    def run(**kw):
        np.random.seed(0)
        torch.manual_seed(0)
        ops.reset_noise()
        model = factory.make_scae(SMALL).cuda().train()
        step = TrainStep(model, B, (1, 16, 16), lr=1e-3, use_graph=use_graph, **kw)
        view = ds.view(shuffle=True, seed=6, drop_last=False)
        losses = []
        for _ in range(2):
            epoch = view.epoch
            while view.epoch == epoch:
                losses.append(float(step.step_from(view)))
            step.end_epoch()
        torch.cuda.synchronize()
        return step, losses, {k: v.clone() for k, v in model.state_dict().items()}
    plain, l0, sd0 = run()
    two, l2, sd2 = run(force_collective=True)
    assert two.split and two._rem.split and two._rem.collective
    one, l1, sd1 = run(force_collective=True, overlap=False)
    assert one.collective and not one.split and not one._rem.split
    assert len(l0) == 6 and l0 == l1 == l2, (l0, l1, l2)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), ("1 bucket", k)
        assert torch.equal(sd0[k], sd2[k]), ("2 buckets", k)
