"""``EvalStep.predict`` on the GPU: the records against the eager forward of the same model on
the replay's own noise (bit for bit where both run the same kernels), against the oracle,
the confusion matrices, the launch structure (no launch more than the plain step), that
``evaluate`` / ``encode`` are left alone, the stand-alone records launch of a model outside
the fused tail, overflow and the labels-absent case."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import scae_oracle as O
from tests.golden_util import load, sub
from tests.test_eval_step_gpu import _model, _replay_with_noise
from tests.test_hip_model import full_size_params

pytestmark = pytest.mark.gpu

BAR = 1e-4      # the project's parity bar: of the compared tensor's largest magnitude


def _reseed():
    from torch_scae_amd import ops
    torch.manual_seed(5)
    ops.reset_noise()


def _tail_lpp(lpp, posterior, cp):
    """The loss tail's per-image sum of ``lpp`` (workspace entry part[b][0]) from its own
    per-image launch."""
    from torch_scae_amd import _lib
    lib = _lib.load()
    B, O1, M = posterior.shape
    ws = torch.zeros(lib.scae_loss_tail_workspace_floats(B, O1 - 1, 0), device="cuda")
    out = torch.zeros(16, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    w5 = (ctypes.c_float * 5)(1.0, 0.0, 0.0, 0.0, 0.0)
    lpp, posterior, cp = lpp.contiguous(), posterior.contiguous(), cp.contiguous()
    rc = lib.scae_loss_tail_fwd_f32(
        P(lpp), P(posterior), P(cp), None, None, None, None, P(out), P(ws), B, O1 - 1, M, 0, 0,
        1, 1, 0, w5, float("nan"), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ws[:B * 8].view(B, 8)[:, 0].clone()


def _eager_columns(step, noise):
    """The staged batch's record columns from an eager no-grad forward in the step's own plan
    (the launches the replay holds) on the replay's noise."""
    from torch_scae_amd import nn_utils
    model, plan = step.model, step.plan
    with step._eval_mode(), plan.active(), plan.precision(False), plan.fusing(step.image), \
            plan.evaluating(step.epi), nn_utils.fixed_noise([n.cuda() for n in noise[1:]]):
        res = model(step.image)
        sums = res.rec.pdf.log_prob_tile_sums(step.image)
    torch.cuda.synchronize()
    with step._eval_mode():
        pixels = res.rec.pdf.log_prob(step.image)
    B = step.batch_size
    rec = torch.zeros(B, device="cuda")
    for t in range(sums.shape[1]):              # the tile sums added in tile order
        rec = rec + sums[:, t]
    lpp = res["_log_prob_per_point"]
    return dict(prior=res.prior_cls_prob.float(), post=res.posterior_cls_prob.float(),
                rec=rec, rec_pixels=pixels.reshape(B, -1).sum(-1),
                lpp_tail=_tail_lpp(lpp, res["_posterior_full"], res.caps_presence),
                lpp=lpp.sum(-1))


def _check_rows(rows, labels, cols):
    """One batch's records against its eager columns."""
    prior, post = cols["prior"], cols["post"]
    assert torch.equal(rows[:, 0], labels.float())
    pc, qc = prior.argmax(-1), post.argmax(-1)
    assert torch.equal(rows[:, 1], pc.float()) and torch.equal(rows[:, 2], qc.float())
    assert torch.equal(rows[:, 3], prior.gather(1, pc[:, None])[:, 0])
    assert torch.equal(rows[:, 4], post.gather(1, qc[:, None])[:, 0])
    assert torch.equal(rows[:, 5], prior.gather(1, labels[:, None])[:, 0])
    assert torch.equal(rows[:, 6], post.gather(1, labels[:, None])[:, 0])
    d7 = float((rows[:, 7] - cols["rec"]).abs().max())
    d8 = float((rows[:, 8] - cols["lpp_tail"]).abs().max())
    s7, s8 = float(cols["rec_pixels"].abs().max()), float(cols["lpp"].abs().max())
    e7 = float((rows[:, 7] - cols["rec_pixels"]).abs().max())
    e8 = float((rows[:, 8] - cols["lpp"]).abs().max())
    print(f"[records] rec_ll: {d7:.3e} off the tile-ordered sum, {e7:.3e} off the per-pixel "
          f"sum (largest {s7:.4e}); log_prob: {d8:.3e} off the tail's, {e8:.3e} off "
          f"lpp.sum (largest {s8:.4e})")
    assert d7 == 0.0 and d8 == 0.0
    assert e7 <= BAR * s7 and e8 <= BAR * s8


def _eager_check(step, images, labels, records):
    """Every batch of the split replayed once more on predicted noise and re-run eagerly;
    ``records`` (of a predict() after the same reseed) row block by row block."""
    B, N = step.batch_size, images.shape[0]
    _reseed()
    for lo in range(0, N, B):
        s = step if lo + B <= N else step._tail_step
        x, y = images[lo:lo + B], labels[lo:lo + B]
        noise = _replay_with_noise(s, x.cpu(), y.cpu())
        _check_rows(records[lo:lo + B], y, _eager_columns(s, noise))
        s.reset()


def _check_confusion(got, N, ncls=10):
    rec, conf = got["records"], got["confusion"]
    assert conf.shape == (2, ncls, ncls) and conf.dtype == torch.int64 and conf.is_cuda
    for h in (0, 1):
        cells = rec[:, 0].long() * ncls + rec[:, 1 + h].long()
        assert torch.equal(conf[h].flatten(), torch.bincount(cells, minlength=ncls * ncls))
        assert int(conf[h].sum()) == N


@pytest.mark.parametrize("name,replay", [("cfg2", "graph"), ("cfg2", "launches"),
                                         ("cfg5", "graph"), ("mnist_40_32", "graph")])
def test_records_are_the_eager_forwards_bit_for_bit(name, replay):
    from torch_scae_amd import EvalStep
    from torch_scae_amd import data as D
    from torch_scae_amd.data_parallel import FlatParameters
    cfg, B, sd, g = full_size_params(name)
    model = _model(cfg, sd)
    flat = FlatParameters(model) if replay == "launches" else None
    N = 2 * B + 40
    images = torch.rand(N, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (N,), generator=g).cuda()
    step = EvalStep(model, B, cfg["image_shape"], replay=replay)
    step.predict(images, labels)                 # captures both steps with the records
    graph = step.graph
    assert step.fused and step._tail_step.batch_size == 40
    if replay == "launches":
        assert step._klist
    _reseed()
    got = step.predict(images, labels)
    assert step.graph is graph, "predict recaptured"
    assert got["rows"] == N and not got["overflow"]
    assert got["records"].shape == (N, 9) and got["records"].is_cuda
    assert torch.equal(got["label_int"], labels)
    assert got["prior_class_int"].dtype == torch.int64
    _check_confusion(got, N)
    records, conf = got["records"].clone(), got["confusion"].clone()
    _eager_check(step, images, labels, records)
    # again: the same bits, rows and counts
    _reseed()
    again = step.predict(images, labels)
    assert torch.equal(again["records"], records) and torch.equal(again["confusion"], conf)
    if name != "cfg2" or replay != "graph":
        del flat
        return
    # a device-resident view: the records of its materialised split, bit for bit
    u8 = (images[:, 0] * 255).to(torch.uint8).cpu()
    ds = D.ResidentDataset(u8, labels.cpu(), out_size=(40, 40), device="cuda")
    view = D.DatasetView(ds, shuffle=True, translate=False, seed=9)
    mi, ml = view.materialise()
    _reseed()
    pv = step.predict(view)
    assert view.epoch == 1 and torch.equal(pv["label_int"], ml.cuda())
    _reseed()
    pt = step.predict(mi.cuda(), ml.cuda())
    assert torch.equal(pv["records"], pt["records"])
    assert torch.equal(pv["confusion"], pt["confusion"])
    assert torch.equal(pv["means"]["loss"], pt["means"]["loss"])
    _check_confusion(pv, N)


def _oracle_columns(cfg, sd, image, label, noise, monkeypatch):
    """Columns [3..8] and both heads' class probabilities from the oracle; the per-image
    capsule log-likelihood from its capsule_likelihood on one image at a time (its
    ``log_prob`` is the batch mean of the per-image sums)."""
    calls = []
    orig = O.capsule_likelihood

    def spy(*a, **k):
        calls.append((a, k))
        return orig(*a, **k)
    monkeypatch.setattr(O, "capsule_likelihood", spy)
    ocfg = O.prepare_model_params(**cfg)
    with torch.no_grad():
        ores = O.scae_forward(sd, ocfg, image, noise, training=False)
        monkeypatch.setattr(O, "capsule_likelihood", orig)
        (a, k), = calls
        assert not k and len(a) == 6
        B = image.shape[0]
        lpp = torch.stack([orig(a[0][b:b + 1], a[1][b:b + 1], a[2][b:b + 1], a[3],
                                a[4][b:b + 1], a[5][b:b + 1]).log_prob for b in range(B)])
        assert abs(float(lpp.mean()) - float(ores.log_prob)) <= 1e-5 * abs(float(ores.log_prob))
        lp = O.gmm_log_prob(ores.rec.transformed_templates, ores.rec.scale,
                            ores.rec.mixing_logits, image)
    prior, post = ores.prior_cls_prob, ores.posterior_cls_prob
    return prior, post, lp.reshape(B, -1).sum(-1), lpp


def _check_against_oracle(cfg, sd, B, image, label, monkeypatch):
    from torch_scae_amd import EvalStep
    from tests.test_timed_path import predict_noise
    model = _model(cfg, sd)
    step = EvalStep(model, B, cfg["image_shape"])
    step.predict(image.cuda(), label.cuda())        # captures with the records
    want = predict_noise(step)
    got = step.predict(image.cuda(), label.cuda())
    torch.cuda.synchronize()
    assert torch.equal(step._pro.noise, want), "the replay drew other noise"
    Oc, M = model.obj_decoder.n_obj_capsules, model.part_encoder.n_caps
    n1, n2 = want.split([B * Oc, B * Oc * M])
    noise = [None, n1.view(B, Oc, 1).cpu(), n2.view(B, Oc, M).cpu()]
    prior, post, rec, lpp = _oracle_columns(cfg, sd, image, label, noise, monkeypatch)
    rows = got["records"].cpu()
    lab = label[:, None]
    for h, p in enumerate((prior, post)):
        cls = rows[:, 1 + h].long()
        # no row excluded: the oracle's probability of the device's class is within two
        # bars (one for each of the two probabilities compared) of the oracle's maximum
        gap = p.max(-1).values - p.gather(1, cls[:, None])[:, 0]
        print(f"[oracle] head {h}: largest gap to the oracle's maximum {float(gap.max()):.3e}")
        assert float(gap.max()) <= 2 * BAR
    for j, ref in ((3, prior.gather(1, rows[:, 1].long()[:, None])[:, 0]),
                   (4, post.gather(1, rows[:, 2].long()[:, None])[:, 0]),
                   (5, prior.gather(1, lab)[:, 0]), (6, post.gather(1, lab)[:, 0]),
                   (7, rec), (8, lpp)):
        scale = float(ref.abs().max())
        err = float((rows[:, j] - ref).abs().max())
        print(f"[oracle] column {j}: error {err:.3e}, largest magnitude {scale:.4e}")
        assert err <= BAR * scale, (j, err, scale)


def test_records_vs_oracle_at_cfg2(monkeypatch):
    from tests.test_eval_step_gpu import _batch
    cfg, B, sd, g = full_size_params("cfg2")
    image, label = _batch(cfg, B, g)
    _check_against_oracle(cfg, sd, B, image, label, monkeypatch)


def test_records_vs_oracle_on_a_golden_model(monkeypatch):
    blob, meta = load("scae_kernels")
    image, label = blob["in/image"], blob["in/label"]
    _check_against_oracle(meta["config"], sub(blob, "param/"), image.shape[0], image, label,
                          monkeypatch)


def test_records_add_no_launch_at_cfg2():
    """The captured batch with the records attached is the plain batch's launches -- the
    epilogue's combine workgroup writes them -- and still replays from the launch list."""
    from torch_scae_amd import EvalStep
    from torch_scae_amd.data_parallel import FlatParameters
    cfg, B, sd, g = full_size_params("cfg2")
    model = _model(cfg, sd)
    flat = FlatParameters(model)
    images = torch.rand(2 * B, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (2 * B,), generator=g).cuda()
    outs = []
    for replay in ("graph", "launches"):
        plain = EvalStep(model, B, cfg["image_shape"], replay=replay)
        plain.capture()
        step = EvalStep(model, B, cfg["image_shape"], replay=replay)
        _reseed()
        got = step.predict(images, labels)
        nodes, kernels, recorded = step.graph_nodes
        print(f"[predict cfg2 {replay}] graph nodes {nodes}, kernel nodes {kernels}, recorded "
              f"launches {recorded}; plain step {plain.graph_nodes}")
        assert step.graph_nodes == plain.graph_nodes
        assert nodes == kernels == recorded and kernels <= 11
        assert step.fused and not step.epi.records_alone
        names = [getattr(fn, "__name__", "?") for fn, _, _ in step._launches]
        assert names[-1] == "scae_eval_tail_records_f32", names
        if replay == "launches":
            assert step._klist
        outs.append((got["records"].clone(), got["confusion"].clone(), got["means"]["loss"]))
        del step, plain
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    del flat


def test_predict_leaves_evaluate_and_encode_alone():
    from torch_scae_amd import EvalStep
    cfg, B, sd, g = full_size_params("cfg2")
    model = _model(cfg, sd)
    N = 2 * B + 40
    images = torch.rand(N, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (N,), generator=g).cuda()
    # (a capture's warm-up batches draw noise: every capture comes before the reseed of the
    # call it serves)
    fresh = EvalStep(model, B, cfg["image_shape"])
    fresh.evaluate(images, labels)             # captures the step and its tail step
    _reseed()
    m0 = fresh.evaluate(images, labels)
    fresh.encode(images, labels)               # recaptures both with the feature sink
    _reseed()
    e0 = fresh.encode(images, labels)
    step = EvalStep(model, B, cfg["image_shape"])
    step.predict(images, labels)               # captures both with the records
    graph = step.graph
    _reseed()
    p = step.predict(images, labels)
    _reseed()
    m1 = step.evaluate(images, labels)
    assert step.graph is graph
    step.encode(images, labels)                # recaptures: the sink beside the records
    _reseed()
    e1 = step.encode(images, labels)
    _reseed()
    p2 = step.predict(images, labels)          # (now with the feature sink attached too)
    assert set(m0) == set(m1) == set(p["means"])
    for k in m0:
        for other in (m1, p["means"], e0["means"], e1["means"], p2["means"]):
            assert torch.equal(torch.as_tensor(m0[k]), torch.as_tensor(other[k])), k
    assert torch.equal(e0["features"], e1["features"])
    assert torch.equal(p["records"], p2["records"])
    assert torch.equal(p["confusion"], p2["confusion"])
    # the means' accuracies are the records'
    for k, j in (("prior_accuracy", 1), ("posterior_accuracy", 2)):
        per = [(p["records"][lo:lo + B, j] == p["records"][lo:lo + B, 0]).float().mean()
               for lo in range(0, N, B)]
        assert abs(float(torch.stack(per).mean()) - float(m0[k])) <= 1e-6, k


def test_stand_alone_records_outside_the_fused_tail():
    from torch_scae_amd import EvalStep
    cfg, B, sd, g = full_size_params("cfg2")
    cfg = dict(cfg, scae_params=dict(cfg["scae_params"], recon_mse_weight=0.7))
    model = _model(cfg, sd)
    N = B + 40
    images = torch.rand(N, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (N,), generator=g).cuda()
    plain = EvalStep(model, B, cfg["image_shape"])
    plain.evaluate(images, labels)             # captures the step and its tail step
    step = EvalStep(model, B, cfg["image_shape"])
    step.predict(images, labels)
    assert not step.fused and step.epi.records_alone
    names = [getattr(fn, "__name__", "?") for fn, _, _ in step._launches]
    assert "scae_eval_records_f32" in names, names
    assert "scae_eval_tail_records_f32" not in names
    _reseed()
    got = step.predict(images, labels)
    assert got["rows"] == N and not got["overflow"]
    _check_confusion(got, N)
    records = got["records"].clone()
    _eager_check(step, images, labels, records)
    _reseed()
    want = plain.evaluate(images, labels)
    for k in ("loss", "accuracy", "log_prob", "rec_ll"):
        assert torch.equal(got["means"][k], want[k]), k


def test_stand_alone_records_from_a_per_pixel_map():
    """scae_eval_records_f32 on its own: the per-image sums of a per-pixel map and of lpp by
    one wave per image, more classes than the fused tail takes, labels outside the classes."""
    from torch_scae_amd import ops
    g = torch.Generator().manual_seed(3)
    B, ncls, M, npix = 70, 40, 24, 1600
    prior = torch.softmax(torch.randn(B, ncls, generator=g), -1).cuda()
    post = torch.softmax(torch.randn(B, ncls, generator=g), -1).cuda()
    prior[::3] = 0.025                    # ties: the first index wins
    post[8::7, 4] = float("nan")          # a NaN is maximal
    label = torch.randint(0, ncls, (B,), generator=g)
    label[5], label[6] = -1, ncls         # outside: not counted, no label probability
    label = label.cuda()
    lpp = (torch.randn(B, M, generator=g) - 3).cuda()
    pixels = (torch.randn(B, 1, 40, 40, generator=g) - 1).cuda()
    rec = ops.EvalRecords("cuda")
    rows = torch.full((B + 5, 9), 7.0, device="cuda")
    conf = torch.zeros(2, ncls, ncls, dtype=torch.int64, device="cuda")
    rec.point(rows, conf)
    rec.launch_alone(prior, post, label, lpp, rec_pixels=pixels)
    torch.cuda.synchronize()
    assert rec.status() == (B, False)
    got = rows[:B]
    assert float(rows[B:].min()) == 7.0
    assert torch.equal(got[:, 0], label.float())
    pc, qc = prior.argmax(-1), post.argmax(-1)
    assert torch.equal(got[:, 1], pc.float()) and torch.equal(got[:, 2], qc.float())
    assert torch.equal(got[:, 3], prior.gather(1, pc[:, None])[:, 0])
    qconf = post.gather(1, qc[:, None])[:, 0]
    assert bool(qconf.isnan().any()) and torch.equal(got[:, 4].isnan(), qconf.isnan())
    assert torch.equal(got[:, 4].nan_to_num(nan=-5.0), qconf.nan_to_num(nan=-5.0))
    ok = (label >= 0) & (label < ncls)
    at = prior.gather(1, label.clamp(0, ncls - 1)[:, None])[:, 0]
    assert torch.equal(got[:, 5], torch.where(ok, at, torch.zeros_like(at)))
    ref7 = pixels.double().reshape(B, -1).sum(-1)
    ref8 = lpp.double().sum(-1)
    # fp32 sums of n terms in a tree of partial sums: well inside the parity bar
    assert float((got[:, 7].double() - ref7).abs().max()) <= BAR * float(ref7.abs().max())
    assert float((got[:, 8].double() - ref8).abs().max()) <= BAR * float(ref8.abs().max())
    for h, cls in enumerate((pc, qc)):
        cells = label[ok] * ncls + cls[ok]
        assert torch.equal(conf[h].flatten(), torch.bincount(cells, minlength=ncls * ncls))
    # a second batch lands behind the first; a third one overflows and is not counted
    rec.launch_alone(prior, post, label, lpp, rec_pixels=pixels)
    torch.cuda.synchronize()
    assert rec.status() == (2 * B, True)
    assert torch.equal(rows[B:], rows[:5])
    assert int(conf.sum()) == 2 * (int(ok.sum()) + int(ok[:5].sum()))
    rec.off()
    before = rows.clone()
    rec.launch_alone(prior, post, label, lpp, rec_pixels=pixels)
    torch.cuda.synchronize()
    assert rec.status() == (0, False)
    assert torch.equal(rows.nan_to_num(nan=-5.0), before.nan_to_num(nan=-5.0))


def test_overflow_and_the_labels_absent_case():
    from torch_scae_amd import EvalStep
    cfg, B, sd, g = full_size_params("cfg2")
    model = _model(cfg, sd)
    N = B + 40
    images = torch.rand(N, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (N,), generator=g).cuda()
    step = EvalStep(model, B, cfg["image_shape"])
    step.predict(images, labels)               # captures (the warm-up batches draw noise)
    graph = step.graph
    _reseed()
    full = step.predict(images, labels)
    records = full["records"].clone()
    short = torch.full((B + 3, 9), -7.0, device="cuda")
    _reseed()
    got = step.predict(images, labels, out=short)
    assert step.graph is graph
    assert got["rows"] == B + 3 and got["overflow"]
    assert torch.equal(short, records[:B + 3])
    _check_confusion(got, B + 3)
    # no labels: the step's loss sees zeros; the records carry no label
    _reseed()
    zl = step.predict(images, torch.zeros_like(labels))["records"].clone()
    _reseed()
    nol = step.predict(images)
    assert step.graph is graph
    rec = nol["records"]
    assert torch.equal(rec[:, 0], torch.full((N,), -1.0, device="cuda"))
    assert float(rec[:, 5:7].abs().sum()) == 0.0
    assert torch.equal(rec[:, [1, 2, 3, 4, 7, 8]], zl[:, [1, 2, 3, 4, 7, 8]])
    assert int(nol["confusion"].abs().sum()) == 0
    assert np.isfinite(float(nol["means"]["loss"]))
