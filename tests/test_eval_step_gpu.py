"""The replayed evaluation step (eval_step.EvalStep) on the GPU: oracle parity of the
loss, its 12 entries, the class probabilities and the accuracies on the step's OWN noise
draws (predicted from a copy of its generator state, as tests/test_timed_path.py does),
the fp64 epoch accumulator, the launch structure, isolation from a training step,
recapture after the parameters are re-homed, the bf16 operand path, the standalone
epilogue of a model outside the fused tail, and ``evaluate()`` over a split with a
remainder batch.

The reference: BaseExperiment.validation_step / test_step
(torch_scae_experiments/base_experiment.py:128-202) -- forward, SCAE.loss and
SCAE.calculate_accuracy under model.eval() and no_grad."""
import numpy as np
import pytest
import torch

from oracle import scae_oracle as O
from tests.test_hip_model import FULL, full_size_params
from tests.test_timed_path import predict_noise

pytestmark = pytest.mark.gpu

LOG12 = ["loss", "log_prob", "prior_within_sparsity_loss", "prior_between_sparsity_loss",
         "posterior_within_sparsity_loss", "posterior_between_sparsity_loss",
         "prior_cls_xe", "posterior_cls_xe", "rec_ll", "rec_ll_loss", "log_prob_loss",
         "cpr_dynamic_reg_loss"]


def _model(cfg, sd, train=True):
    from torch_scae_amd import factory
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(cfg)
    model.load_state_dict(sd)
    return model.cuda().train(train)


def _batch(cfg, B, g):
    image = torch.rand(B, *cfg["image_shape"], generator=g)
    label = torch.randint(0, cfg["n_classes"], (B,), generator=g)
    return image, label


def _replay_with_noise(step, image, label):
    """One replay on (image, label); -> the two noise draws it used (CPU), checked bit for
    bit against the prediction from a copy of the generator state."""
    cfg_O, B = step.model.obj_decoder.n_obj_capsules, step.batch_size
    M = step.model.part_encoder.n_caps
    step.capture()
    want = predict_noise(step)
    step(image.cuda(), label.cuda())
    torch.cuda.synchronize()
    assert torch.equal(step._pro.noise, want), "the replay drew other noise"
    n1, n2 = want.split([B * cfg_O, B * cfg_O * M])
    return [None, n1.view(B, cfg_O, 1).cpu(), n2.view(B, cfg_O, M).cpu()]


def _oracle(cfg, sd, image, label, noise):
    ocfg = O.prepare_model_params(**cfg)
    with torch.no_grad():
        ores = O.scae_forward(sd, ocfg, image, noise, training=False)
        oloss, olog = O.scae_loss(ocfg, ores, image, label)
    return ores, oloss, olog


def _vec12(oloss, olog):
    rec = float(olog["rec_ll_loss"])
    return [float(oloss), -float(olog["log_prob_loss"]),
            *[float(olog.get(k, 0.0)) for k in LOG12[2:8]], -rec, rec,
            float(olog["log_prob_loss"]), float(olog["cpr_dynamic_reg_loss"])]


def _check_parity(step, cfg, sd, image, label, noise, tol=1e-4):
    ores, oloss, olog = _oracle(cfg, sd, image, label, noise)
    m = step.epoch_means()
    assert m["batches"] == 1
    got = {k: float(m[k]) for k in LOG12[1:]}
    want = dict(zip(LOG12, _vec12(oloss, olog)))
    assert abs(float(step.loss) - float(oloss)) <= tol * abs(float(oloss)), \
        (float(step.loss), float(oloss))
    for k in LOG12[1:]:
        assert abs(got[k] - want[k]) <= tol * max(1.0, abs(want[k])), (k, got[k], want[k])
    return ores


def _accuracy_of(prior, post, label):
    B = label.shape[0]
    pa = np.float32((prior.argmax(-1) == label).sum().item()) / np.float32(B)
    qa = np.float32((post.argmax(-1) == label).sum().item()) / np.float32(B)
    return max(pa, qa), pa, qa


@pytest.mark.parametrize("name", ["cfg2", "cfg5", "mnist_40_32"])
def test_replayed_eval_step_vs_oracle(name):
    from torch_scae_amd import EvalStep, nn_utils
    cfg, B, sd, g = full_size_params(name)
    model = _model(cfg, sd)
    step = EvalStep(model, B, cfg["image_shape"])
    image, label = _batch(cfg, B, g)
    noise = _replay_with_noise(step, image, label)
    assert step.fused and model.training
    ores = _check_parity(step, cfg, sd, image, label, noise)
    # the class probabilities the epilogue read: the same fused forward run eagerly in
    # the step's plan on the replay's noise gives them
    with step._eval_mode(), step.plan.active(), step.plan.fusing(step.image), \
            nn_utils.fixed_noise([n.cuda() for n in noise[1:]]):
        res = model(step.image)
    # (read after the fusing scope, which launches the parked class probabilities)
    prior, post = res.prior_cls_prob.float().cpu(), res.posterior_cls_prob.float().cpu()
    for got, k in ((prior, "prior_cls_prob"), (post, "posterior_cls_prob")):
        scale = float(ores[k].abs().max())
        assert float((got - ores[k]).abs().max()) <= 1e-4 * scale, k
    # accuracies: exactly torch.argmax over the step's own probabilities
    best, pa, qa = _accuracy_of(prior, post, label)
    got = step.batch_acc.cpu().numpy()
    assert got.tolist() == [best, pa, qa], (got, best, pa, qa)


def test_accumulator_means_are_the_batches_mean():
    from torch_scae_amd import EvalStep
    cfg, B, sd, g = full_size_params("cfg2")
    step = EvalStep(_model(cfg, sd), B, cfg["image_shape"])
    losses, accs = [], []
    for _ in range(5):
        image, label = _batch(cfg, B, g)
        loss = step(image.cuda(), label.cuda())
        losses.append(float(loss))                        # read one by one
        accs.append([float(a) for a in step.batch_acc.cpu()])
    m = step.epoch_means()
    assert m["batches"] == 5
    s = 0.0
    for v in losses:
        s += v
    assert float(m["loss"]) == np.float32(s / 5)
    for j, k in enumerate(("accuracy", "prior_accuracy", "posterior_accuracy")):
        s = 0.0
        for a in accs:
            s += a[j]
        assert float(m[k]) == np.float32(s / 5), k
    ref = float(torch.tensor(losses).mean())
    assert abs(float(m["loss"]) - ref) <= 1e-6 * abs(ref)
    end = step.validation_epoch_end()
    assert float(end["val_loss"]) == float(m["loss"])
    assert float(step.acc.abs().sum()) == 0.0


def test_launch_structure_and_launch_replay_at_cfg2():
    """With the parameters in flat buffers, as a TrainStep on the model lays them out (the
    capsule MLPs' weights then lie back to back and their pack is an alias): the
    captured batch is library launches only -- the training forward's 10 and the
    epilogue.  (Parameters left where the model made them cost one torch concatenation
    of those weights per batch; the launch list then defers to the graph.)"""
    from torch_scae_amd import EvalStep
    from torch_scae_amd.data_parallel import FlatParameters
    cfg, B, sd, g = full_size_params("cfg2")
    model = _model(cfg, sd)
    flat = FlatParameters(model)
    batches = [_batch(cfg, B, g) for _ in range(3)]
    outs = []
    for replay in ("graph", "launches"):
        torch.manual_seed(3)
        step = EvalStep(model, B, cfg["image_shape"], replay=replay)
        step.capture()
        from torch_scae_amd import ops
        torch.manual_seed(3)
        ops.reset_noise()
        losses = [float(step(x.cuda(), y.cuda())) for x, y in batches]
        outs.append((losses, step.acc.cpu().clone()))
        nodes, kernels, recorded = step.graph_nodes
        print(f"[eval step cfg2 {replay}] graph nodes {nodes}, kernel nodes {kernels}, "
              f"recorded launches {recorded}")
        assert nodes == kernels == recorded and kernels <= 11, step.graph_nodes
        assert step.fused
        if replay == "launches":
            assert step._klist
        del step
    assert outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1])
    del flat


def _trajectory(cfg, sd, batches, with_eval, g_eval):
    from torch_scae_amd import EvalStep
    from torch_scae_amd.train_step import TrainStep
    model = _model(cfg, sd)
    torch.manual_seed(11)
    from torch_scae_amd import ops
    ops.reset_noise()
    B = batches[0][0].shape[0]
    ts = TrainStep(model, B, cfg["image_shape"])
    losses, noises = [], []
    for i, (x, y) in enumerate(batches):
        if i == 2 and with_eval:
            ev = EvalStep(model, B, cfg["image_shape"])
            for _ in range(3):
                ev.validation_step(*(t.cuda() for t in _batch(cfg, B, g_eval)), 1)
            ev.validation_epoch_end()
            assert model.training
        losses.append(float(ts(x.cuda(), y.cuda())))
        noises.append(ts._pro.noise.clone())
    return losses, noises, ts.flat.flat_param.clone()


def test_eval_epoch_leaves_the_training_trajectory_untouched():
    cfg, B, sd, g = full_size_params("cfg2")
    batches = [_batch(cfg, B, g) for _ in range(4)]
    a = _trajectory(cfg, sd, batches, False, None)
    b = _trajectory(cfg, sd, batches, True, torch.Generator().manual_seed(9))
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert torch.equal(a[2], b[2])


def test_recapture_after_the_parameters_are_rehomed():
    from torch_scae_amd import EvalStep, ops
    from torch_scae_amd.train_step import TrainStep
    cfg, B, sd, g = full_size_params("cfg2")
    model = _model(cfg, sd)
    old = EvalStep(model, B, cfg["image_shape"])
    old.capture()
    ts = TrainStep(model, B, cfg["image_shape"])        # re-homes into flat buffers
    ts(*(t.cuda() for t in _batch(cfg, B, g)))
    fresh = EvalStep(model, B, cfg["image_shape"])
    fresh.capture()
    old.capture()                                        # detects the re-homing
    assert old._home == fresh._home
    image, label = _batch(cfg, B, g)
    torch.manual_seed(21)
    ops.reset_noise()
    la = float(old(image.cuda(), label.cuda()))
    lb = float(fresh(image.cuda(), label.cuda()))
    assert la == lb
    assert torch.equal(old.acc, fresh.acc)
    assert torch.equal(old.batch_acc, fresh.batch_acc)


def test_bf16_eval_step_at_the_configs2_shape():
    from torch_scae_amd import EvalStep
    cfg, B, sd, g = full_size_params("cfg3_shape")
    model = _model(cfg, sd)
    step = EvalStep(model, B, cfg["image_shape"], autocast_dtype=torch.bfloat16)
    image, label = _batch(cfg, B, g)
    noise = _replay_with_noise(step, image, label)
    _, oloss, _ = _oracle(cfg, sd, image, label, noise)
    tol = 2.0 ** -7
    assert abs(float(step.loss) - float(oloss)) <= tol * abs(float(oloss))


def test_standalone_epilogue_outside_the_fused_tail():
    from torch_scae_amd import EvalStep
    cfg, B, sd, g = full_size_params("cfg2")
    cfg = dict(cfg, scae_params=dict(cfg["scae_params"], recon_mse_weight=0.7))
    model = _model(cfg, sd)
    step = EvalStep(model, B, cfg["image_shape"])
    image, label = _batch(cfg, B, g)
    noise = _replay_with_noise(step, image, label)
    assert not step.fused
    ores, oloss, olog = _oracle(cfg, sd, image, label, noise)
    assert "mse" in olog
    _check_parity(step, cfg, sd, image, label, noise)


def test_evaluate_a_split_with_a_remainder():
    from torch_scae_amd import EvalStep, nn_utils
    cfg, B, sd, g = full_size_params("cfg2")
    model = _model(cfg, sd)
    step = EvalStep(model, B, cfg["image_shape"])
    N = 5 * B + 40
    images = torch.rand(N, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (N,), generator=g).cuda()
    step.capture()
    m = step.evaluate(images, labels)
    assert m["batches"] == 6 and step._tail_step.batch_size == 40
    # the same batches eagerly: each with the noise its replay drew (the generators are
    # counter based: re-run both steps' sequences from the same states)
    from torch_scae_amd import ops
    torch.manual_seed(5)
    ops.reset_noise()
    per = []
    for i in range(6):
        s = step if i < 5 else step._tail_step
        x, y = images[i * B:(i + 1) * B], labels[i * B:(i + 1) * B]
        noise = _replay_with_noise(s, x.cpu(), y.cpu())
        with s._eval_mode(), nn_utils.fixed_noise([n.cuda() for n in noise[1:]]):
            res = model(x)
            loss, _ = model.loss(res, x, y)
        per.append(float(loss))
        s.reset()
    ref = sum(per) / 6
    torch.manual_seed(5)
    ops.reset_noise()
    m2 = step.evaluate(images, labels)
    assert abs(float(m2["loss"]) - ref) <= 1e-5 * abs(ref), (float(m2["loss"]), ref)
    assert model.training


@pytest.mark.parametrize("B,O,M", [(128, 24, 24), (1024, 64, 48)])
def test_epilogue_combine_is_the_tail_combine_bit_for_bit(B, O, M):
    """scae_eval_tail_f32's combine against scae_loss_tail_fwd_f32's on the same workspace
    (both combine workgroup sizes), and its accuracies against torch.argmax on
    probabilities with ties and NaNs."""
    import ctypes
    from torch_scae_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(B)
    ncls = 10
    dev = "cuda"
    lpp = (torch.randn(B, M, generator=g) - 3).to(dev)
    post = torch.softmax(torch.randn(B, O + 1, M, generator=g), 1).to(dev)
    cp = torch.rand(B, O, generator=g).to(dev)
    w, b = (torch.randn(ncls, O, generator=g) * 0.1).to(dev), torch.randn(ncls, generator=g).to(dev)
    label = torch.randint(0, ncls, (B,), generator=g).to(dev)
    rec = torch.randn(B, 7, generator=g).to(dev)
    reg = torch.rand(1, generator=g).to(dev)
    ws = torch.empty(lib.scae_loss_tail_workspace_floats(B, O, ncls), device=dev)
    outs = [torch.zeros(16, device=dev) for _ in range(2)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    w5 = (ctypes.c_float * 5)(1.0, 0.5, 0.3, 0.2, 0.1)

    def extras(out):
        ex = _lib.LossExtras()
        ex.rec_sums, ex.n_rec = rec.data_ptr(), rec.numel()
        ex.reg, ex.w_reg, ex.loss = reg.data_ptr(), 0.7, out[12:].data_ptr()
        return ex
    head = lambda out, ex: (P(lpp), P(post), P(cp), P(w), P(b), P(label),  # noqa: E731
                            ctypes.byref(ex), P(out), P(ws), B, O, M, ncls, ncls, 2, 1, 1, w5,
                            float("nan"))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ex0 = extras(outs[0])
    assert lib.scae_loss_tail_fwd_f32(*head(outs[0], ex0), st) == 0
    prior = torch.rand(B, ncls, generator=g)
    postp = torch.rand(B, ncls, generator=g)
    prior[::3] = 0.25                     # ties: the first index wins
    prior[1::7, 4] = float("nan")         # a NaN is maximal
    postp[2::5] = prior[2::5]
    postp[5::11, 2] = float("nan")
    prior, postp = prior.to(dev), postp.to(dev)
    acc = torch.zeros(_lib.EVAL_ACC_DOUBLES, device=dev, dtype=torch.float64)
    batch3 = torch.zeros(3, device=dev)
    ex1 = extras(outs[1])
    assert lib.scae_eval_tail_f32(*head(outs[1], ex1), P(prior), P(postp), P(acc), P(batch3),
                                  st) == 0
    torch.cuda.synchronize()
    assert torch.equal(outs[0][:13], outs[1][:13])
    best, pa, qa = _accuracy_of(prior.cpu(), postp.cpu(), label.cpu())
    assert batch3.cpu().tolist() == [best, pa, qa]
    a = acc.cpu()
    assert a[0] == 1 and a[1] == float(outs[0][12]) and a[2] == float(best)
    assert a[5:].tolist() == outs[0][:12].double().cpu().tolist()


# the model of the package's smoke run
SMALL = dict(image_shape=(1, 16, 16), n_classes=4, n_part_caps=5, n_obj_caps=4,
             pcae_cnn_encoder_params=dict(out_channels=[64, 64], kernel_sizes=[3, 3],
                                          strides=[2, 1]),
             pcae_template_generator_params=dict(template_size=(5, 5)),
             ocae_encoder_set_transformer_params=dict(dim_hidden=8, dim_out=64, n_layers=2),
             ocae_decoder_capsule_params=dict(dim_caps=4, hidden_sizes=(8,)),
             scae_params=dict(reconstruct_alternatives=False))


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    return torch.equal(torch.as_tensor(a), torch.as_tensor(b))


@pytest.mark.parametrize("source", ["tensors", "view"])
def test_evaluate_encode_and_predict_share_the_walk_and_the_captured_graphs(source):
    """evaluate, encode, predict, evaluate on one step, B = 4 and N = 10 (two full batches and
    a tail of 2), round after round.  The first round captures: once, again when encode
    attaches the sink, again when predict attaches the records, and not for the evaluate after
    them.  Its batches draw the noise that follows the captures' warm-up draws, so its values
    are no yardstick; the two rounds after it are the ones compared: the same graph objects
    throughout (nothing recaptured), every result bit for bit the round before's, and
    evaluate's means those of a fresh step that never had a descriptor attached."""
    from torch_scae_amd import EvalStep, data, factory, ops
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(SMALL)
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.normal_(0, 0.1)
    model = model.cuda().train()
    g = torch.Generator().manual_seed(11)
    ds = data.ResidentDataset(torch.rand(10, 1, 16, 16, generator=g),
                              torch.randint(0, 4, (10,), generator=g), out_size=(16, 16),
                              device="cuda")
    view = ds.view(shuffle=False, translate=False)
    args = (view,) if source == "view" else tuple(t.cuda() for t in view.materialise())

    def seeded(call):
        torch.manual_seed(5)
        ops.reset_noise()
        return call(*args)

    step = EvalStep(model, 4, (1, 16, 16), use_graph=True)

    def one_round():
        results, graphs = [], []
        for call in (step.evaluate, step.encode, step.predict, step.evaluate):
            results.append(seeded(call))
            graphs.append((step.graph, step._tail_step.graph))
        return results, graphs

    _, graphs = one_round()
    assert step._tail_step.batch_size == 2
    for which in (0, 1):                   # the step and its tail step
        a, b, c, d = (pair[which] for pair in graphs)
        assert a is not None and b is not a and c is not b and d is c
    captured = graphs[-1]
    rounds = [one_round() for _ in range(2)]
    for _, graphs in rounds:
        for pair in graphs:
            assert pair[0] is captured[0] and pair[1] is captured[1]
    first, second = rounds[0][0], rounds[1][0]
    assert first[0]["batches"] == 3 and first[1]["rows"] == first[2]["rows"] == 10
    for a, b in zip(first, second):
        assert _same(a, b)
    fresh = EvalStep(model, 4, (1, 16, 16), use_graph=True)
    fresh.evaluate(*args)                  # (captures the step and its tail step)
    want = seeded(fresh.evaluate)
    assert fresh.epi.sink is None and fresh.epi.records is None
    for got in (first[0], first[3], first[1]["means"], first[2]["means"]):
        assert _same(got, want)
    assert float(step.acc.abs().sum()) == 0.0 and float(step._tail_step.acc.abs().sum()) == 0.0
