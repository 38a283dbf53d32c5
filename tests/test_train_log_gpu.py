"""The training log of a replayed step (TrainStep(log_steps=N)): every step's `log` of
BaseExperiment.training_step as one row of a device ring, written by the loss tail's batch
combine (include/scae_hip.h, scae_train_log_desc) -- the same values as
``training_step()``'s torch-computed log, no launch and no torch operator more, training
untouched; the ring, the step counter and the epoch means; the C ABI against the plain
combine; models outside the fused tail (scae_train_log_f32); the collective modes."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_hip_model import FULL

pytestmark = pytest.mark.gpu


def _params(cfg):
    """A state dict of ``cfg`` with the all-zero parameters filled (every term carries a
    gradient), as tests/test_hip_model.full_size_params makes them."""
    from torch_scae_amd import factory
    np.random.seed(1)
    torch.manual_seed(1)
    proto = factory.make_scae(cfg)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for p in proto.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return {k: v.clone() for k, v in proto.state_dict().items()}


def _step(cfg, B, sd, **kw):
    from torch_scae_amd import factory, ops
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(0)
    torch.manual_seed(1234)
    ops.reset_noise()
    model = factory.make_scae(cfg)
    model.load_state_dict(sd)
    return TrainStep(model.cuda().train(), B, cfg["image_shape"], **kw)


def _batches(cfg, B, K, seed=3):
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(K, B, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, cfg["n_classes"], (K, B), generator=g).cuda()
    return images, labels


def _dataset(n, out=40):
    from torch_scae_amd import data as D
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (n, 1, 28, 28), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (n,), generator=g)
    return D.ResidentDataset(imgs, labels, out_size=(out, out), device="cuda")


def _reset_noise():
    from torch_scae_amd import ops
    torch.manual_seed(5)
    ops.reset_noise()


def _check_accuracy(row_acc, torch_acc, B):
    """count / B in fp32, within one ulp of torch's mean"""
    n = round(float(row_acc) * B)
    assert float(torch.tensor(float(n)) / B) == float(row_acc), (float(row_acc), B)
    t = np.float32(float(torch_acc))
    assert abs(np.float32(float(row_acc)) - t) <= np.spacing(t), (float(row_acc), float(t))


def _row_parity(cfg, B, K=4, fused=True, sd=None, **kw):
    """K steps of ``training_step()`` against K logged steps from the same state, noise and
    batches: the rows are its log values bit for bit (the accuracy as count / B)."""
    sd = _params(cfg) if sd is None else sd
    ref = _step(cfg, B, sd, **kw)
    logged = _step(cfg, B, sd, log_steps=8, **kw)
    images, labels = _batches(cfg, B, K + 1)
    snaps = ref.snapshot(), logged.snapshot()
    ref.training_step(images[K], labels[K])     # (the captures draw noise: before the reset)
    logged(images[K], labels[K])
    ref.restore(snaps[0])
    logged.restore(snaps[1])
    logged.reset_log()
    _reset_noise()
    want = []
    for i in range(K):
        out = ref.training_step(images[i], labels[i])
        want.append({k: v.detach().clone() for k, v in out["log"].items()})
    _reset_noise()
    got = []
    for i in range(K):
        loss = logged(images[i], labels[i])
        last = logged.last_log()
        assert torch.equal(last["loss"], loss.reshape(()))
        got.append({k: v.clone() for k, v in last["log"].items()})
    torch.cuda.synchronize()
    assert logged.train_log.fused == fused
    hist, steps = logged.log_history()
    assert steps == list(range(K))
    for i in range(K):
        w, g = want[i], got[i]
        assert set(g) == set(w) | {"learning_rate"}, (set(g), set(w))
        for k, v in w.items():
            if k == "accuracy":
                _check_accuracy(g[k], v, B)
            else:
                assert torch.equal(v.reshape(()).float(), g[k]), (i, k, float(v), float(g[k]))
        assert float(g["learning_rate"]) == float(logged.opt.lr_dev)
        for k in g:
            assert float(hist[k][i]) == float(g[k]) or \
                (np.isnan(float(hist[k][i])) and np.isnan(float(g[k]))), (i, k)
    # the row's two heads and their maximum
    from torch_scae_amd import ops
    row = logged.train_log.rows[K - 1].cpu()
    I = ops.TRAIN_LOG_INDEX
    assert float(row[I["accuracy"]]) == max(float(row[I["prior_accuracy"]]),
                                            float(row[I["posterior_accuracy"]]))
    return ref, logged


@pytest.mark.parametrize("replay", ["graph", "launches"])
def test_rows_are_the_training_step_log_cfg2(replay):
    """cfg-2: the combine is the deferred workgroup of the tail's backward launch."""
    cfg, B = FULL["cfg2"]
    _row_parity(cfg, B, replay=replay)


@pytest.mark.parametrize("bf16", [False, True])
def test_rows_are_the_training_step_log_at_configs2_shape(bf16):
    """48 / 64 capsules at B = 1024: the standalone combine launch after the forward."""
    cfg, B = FULL["cfg3_shape"]
    _row_parity(cfg, B, K=2, autocast_dtype=torch.bfloat16 if bf16 else None)


@pytest.mark.parametrize("what", ["40 classes", "recon_mse_weight"])
def test_rows_outside_the_fused_tail(what):
    """A model the fused tail does not complete logs through scae_train_log_f32."""
    cfg, B = FULL["cfg2"]
    if what == "40 classes":
        cfg = dict(cfg, n_classes=40)
        _row_parity(cfg, B, K=3, fused=False)
    else:
        sd = _params(cfg)
        cfg = dict(cfg, scae_params=dict(cfg["scae_params"], recon_mse_weight=0.7))
        ref, logged = _row_parity(cfg, B, K=3, fused=False, sd=sd)
        assert "mse" in logged.last_log()["log"]


def test_logging_leaves_training_and_the_launch_list_untouched():
    """step_from with and without the log: the same parameters and optimiser state bit for
    bit after K steps, the same number of recorded launches (the log adds none), and
    replay="launches" takes its list."""
    from torch_scae_amd import _lib
    cfg, B = FULL["cfg2"]
    sd = _params(cfg)
    ds = _dataset(4 * B + 7)
    out = []
    for log_steps in (0, 16):
        step = _step(cfg, B, sd, replay="launches", log_steps=log_steps)
        step.capture()
        snap = step.snapshot()
        step.restore(snap)
        _reset_noise()
        view = ds.view(shuffle=True, seed=3)
        losses = [float(step.step_from(view)) for _ in range(5)]
        torch.cuda.synchronize()
        assert step._klist, step.graph_nodes
        names = [getattr(fn, "__name__", "?") for fn, _, _ in step._launches]
        assert "scae_train_log_f32" not in names
        out.append((losses, step.snapshot(), step.graph_nodes, names,
                    _lib.load().scae_launch_list_size(step._klist)))
        if log_steps:
            hist, steps = step.log_history()
            assert steps == list(range(5))
            assert hist["loss"].tolist() == losses
    (la, sa, ga, na, ka), (lb, sb, gb, nb, kb) = out
    assert la == lb
    assert ga == gb and na == nb and ka == kb, (ga, gb, ka, kb)
    assert sa.keys() == sb.keys()
    for k, v in sa.items():
        if torch.is_tensor(v):
            assert torch.equal(v, sb[k]), k
        else:
            assert v == sb[k], k


def test_logged_step_from_runs_no_torch_operator_and_no_copy():
    from torch.profiler import ProfilerActivity, profile
    cfg, B = FULL["cfg2"]
    step = _step(cfg, B, _params(cfg), log_steps=8)
    ds = _dataset(4 * B)
    view = ds.view(shuffle=True, seed=1)
    step.step_from(view)             # (capture)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step.step_from(view)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    assert not [n for n in names if n.startswith("aten::") or "memcpy" in n.lower()], names
    assert int(step.train_log.step) == 2 and step.train_log.fused


def test_ring_counter_wrap_and_epoch_means():
    """Capacity 4, 10 steps over epochs of 4: the history is steps 6 - 9, the learning rate
    changes at the wrap, the counter is 10, and each epoch's means are the fp64 means of its
    rows."""
    from torch_scae_amd import ops
    from torch_scae_amd.eval_step import ACC_KEYS
    cfg, B = FULL["cfg2"]
    step = _step(cfg, B, _params(cfg), log_steps=4)
    ds = _dataset(4 * B + 5)
    view = ds.view(shuffle=True, seed=2)
    assert view.steps_per_epoch(B) == 4
    I = ops.TRAIN_LOG_INDEX

    def epoch_check():
        rows = step.train_log.rows.cpu()
        slots, _ = ops.ring_order(step.train_log.count, 4)
        m = step.training_epoch_end()
        assert m["batches"] == 4
        for k, i in ACC_KEYS.items():
            s = 0.0
            for r in slots:
                s += float(rows[r, I[k]])
            assert float(m[k]) == float(np.float32(s / 4)), (k, float(m[k]), s / 4)
        assert float(step.train_log.acc.abs().sum()) == 0.0

    step.train_epoch(view)
    epoch_check()
    step.train_epoch(view)
    epoch_check()
    step.step_from(view)
    step.step_from(view)
    torch.cuda.synchronize()
    assert int(step.train_log.step) == 10 and step.train_log.count == 10
    hist, steps = step.log_history()
    assert steps == [6, 7, 8, 9]
    lr = hist["learning_rate"].tolist()
    assert lr[0] == lr[1] and lr[2] == lr[3] and lr[2] < lr[1], lr
    assert lr[3] == float(step.opt.lr_dev)
    assert torch.isfinite(hist["loss"]).all()
    assert step.last_log()["loss"].item() == hist["loss"][-1].item()
    step.reset_log()
    assert step.last_log() is None and step.log_history() == ({}, [])


@pytest.mark.parametrize("B,O,M", [(128, 24, 24), (1024, 64, 48)])
def test_logged_combine_is_the_tail_combine_bit_for_bit(B, O, M):
    """The combine with the log's epilogue against the plain combine (both workgroup sizes):
    the same 12-vector; accuracies against torch.argmax on probabilities with ties and NaNs;
    the standalone epilogue writes the same row; the deferred combine in the backward launch
    leaves the same gradients and 12-vector as without the log."""
    from torch_scae_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(B)
    ncls, dev = 10, "cuda"
    lpp = (torch.randn(B, M, generator=g) - 3).to(dev)
    post = torch.softmax(torch.randn(B, O + 1, M, generator=g), 1).to(dev)
    cp = torch.rand(B, O, generator=g).to(dev)
    w = (torch.randn(ncls, O, generator=g) * 0.1).to(dev)
    b = torch.randn(ncls, generator=g).to(dev)
    label = torch.randint(0, ncls, (B,), generator=g).to(dev)
    rec = torch.randn(B, 7, generator=g).to(dev)
    reg = torch.rand(1, generator=g).to(dev)
    ws = torch.empty(lib.scae_loss_tail_workspace_floats(B, O, ncls), device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    w5 = (ctypes.c_float * 5)(1.0, 0.5, 0.3, 0.2, 0.1)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    prior = torch.rand(B, ncls, generator=g)
    postp = torch.rand(B, ncls, generator=g)
    prior[::3] = 0.25                     # ties: the first index wins
    prior[1::7, 4] = float("nan")         # a NaN is maximal
    postp[2::5] = prior[2::5]
    postp[5::11, 2] = float("nan")
    prior, postp = prior.to(dev), postp.to(dev)
    lr = torch.full((1,), 3e-5, device=dev)
    R = _lib.TRAIN_LOG_ROW

    def extras(out):
        ex = _lib.LossExtras()
        ex.rec_sums, ex.n_rec = rec.data_ptr(), rec.numel()
        ex.reg, ex.w_reg, ex.loss = reg.data_ptr(), 0.7, out[12:].data_ptr()
        return ex

    def log():
        t = (torch.full((3, R), -1.0, device=dev), torch.zeros(1, device=dev, dtype=torch.int64),
             torch.zeros(_lib.EVAL_ACC_DOUBLES, device=dev, dtype=torch.float64))
        d = _lib.TrainLogDesc()
        d.rows, d.step, d.acc, d.capacity = t[0].data_ptr(), t[1].data_ptr(), \
            t[2].data_ptr(), 3
        d.prior_prob, d.post_prob, d.label, d.ncls = prior.data_ptr(), postp.data_ptr(), \
            label.data_ptr(), ncls
        d.lr = lr.data_ptr()
        return t, d

    head = lambda out, ex: (P(lpp), P(post), P(cp), P(w), P(b), P(label),  # noqa: E731
                            ctypes.byref(ex), P(out), P(ws), B, O, M, ncls, ncls, 2, 1, 1, w5,
                            float("nan"))
    outs = [torch.zeros(16, device=dev) for _ in range(3)]
    ex0 = extras(outs[0])
    assert lib.scae_loss_tail_fwd_f32(*head(outs[0], ex0), st) == 0
    (rows, counter, acc), d = log()
    ex1 = extras(outs[1])
    ex1.train_log = ctypes.pointer(d)
    assert lib.scae_loss_tail_combine_f32(*head(outs[1], ex1), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert int(counter) == 1
    row = rows[0].cpu()
    pa = (prior.argmax(-1) == label).float().mean()
    qa = (postp.argmax(-1) == label).float().mean()
    assert torch.equal(row[2], pa.cpu()) and torch.equal(row[3], qa.cpu())
    assert float(row[1]) == max(float(pa), float(qa))
    assert torch.equal(row[0], outs[0][0].cpu()) and torch.equal(row[4:16], outs[0][:12].cpu())
    assert float(row[16]) == float(lr) and float(row[17]) == 0.0 and float(row[18]) == 0.0
    assert torch.equal(rows[1:], torch.full((2, R), -1.0, device=dev))
    want_acc = torch.tensor([1.0, float(row[0]), float(row[1]), float(row[2]), float(row[3])]
                            + [float(v) for v in outs[0][:12]], dtype=torch.float64)
    assert torch.equal(acc.cpu(), want_acc)
    # the epilogue alone, from the same inputs: the next row, the same values
    extra2 = torch.tensor([1.5, -2.0], device=dev)
    assert lib.scae_train_log_f32(P(outs[0][12:]), P(outs[0]), P(extra2), ctypes.byref(d), B,
                                  st) == 0
    torch.cuda.synchronize()
    assert int(counter) == 2
    assert torch.equal(rows[1, :17].cpu(), row[:17])
    assert rows[1, 17:].tolist() == [1.5, -2.0]
    assert torch.equal(acc[1:].cpu(), 2 * want_acc[1:])
    if not lib.scae_loss_tail_defer_preferred(B, O):
        return
    # the deferred combine inside the backward launch, with and without the log
    gouts = []
    for logged in (False, True):
        (rows, counter, acc), d = log()
        ex = extras(outs[2])
        ex.defer_combine, ex.out12 = 1, outs[2].data_ptr()
        if logged:
            ex.train_log = ctypes.pointer(d)
        grads = [torch.full_like(t, 7.0) for t in (lpp, post, cp, w, b, rec, reg)]
        ex.g_rec_sums, ex.g_reg = grads[5].data_ptr(), grads[6].data_ptr()
        gout = torch.linspace(0.5, 1.5, 12, device=dev)
        outs[2].zero_()
        assert lib.scae_loss_tail_bwd_f32(
            P(lpp), P(post), P(cp), P(w), P(b), P(label), ctypes.byref(ex), P(gout), P(ws),
            *[P(t) for t in grads[:5]], B, O, M, ncls, ncls, 2, 1, 1, w5, float("nan"),
            st) == 0
        torch.cuda.synchronize()
        gouts.append((grads, outs[2].clone()))
        if logged:
            assert int(counter) == 1
            assert torch.equal(rows[0, :16].cpu(), row[:16])
    (ga, oa), (gb, ob) = gouts
    assert torch.equal(oa, ob) and torch.equal(oa, outs[0])
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)


@pytest.mark.parametrize("mode", ["2 buckets", "1 bucket"])
def test_collective_steps_write_rows(nccl_group, mode):
    cfg, B = FULL["cfg2"]
    kw = dict(force_collective=True, log_steps=4)
    if mode == "1 bucket":
        kw["overlap"] = False
    step = _step(cfg, B, _params(cfg), **kw)
    assert step.collective and step.split == (mode == "2 buckets")
    images, labels = _batches(cfg, B, 3)
    losses = [float(step(images[i], labels[i])) for i in range(3)]
    torch.cuda.synchronize()
    assert int(step.train_log.step) == 3
    hist, steps = step.log_history()
    assert hist["loss"].tolist() == losses
    rows = step.train_log.rows.cpu()
    m = step.training_epoch_end(all_ranks=True)
    assert m["batches"] == 3
    s = 0.0
    for r in range(3):
        s += float(rows[r, 0])
    assert float(m["loss"]) == float(np.float32(s / 3))
