"""Unsupervised classification on the GPU: the k-means kernels (csrc/kmeans.hip) against
the fp64 host restatement (cluster.kmeans_host) -- one Lloyd step, a whole fit, k-means++
draws -- and EvalStep.encode's feature sink (the loss tail's per-image launch, or the
standalone launch) against eager forwards on the replays' own noise, with the evaluation
means, launch counts and overflow; then unsupervised_accuracy end to end."""
import numpy as np
import pytest
import torch

from tests.test_eval_step_gpu import _model, _replay_with_noise
from tests.test_hip_model import full_size_params
from torch_scae_amd import cluster as C

pytestmark = pytest.mark.gpu


def _blobs(N, k, F, seed, spread=20.0, noise=1.0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(k, F, generator=g, dtype=torch.float64) * spread
    y = torch.randint(0, k, (N,), generator=g)
    x = centres[y] + torch.randn(N, F, generator=g, dtype=torch.float64) * noise
    return x.float(), y, g


def _screened_label_check(x, cent, got):
    """Labels identical wherever the fp64 best / second-best gap exceeds 1e-5 of the
    distance; -> the fraction excluded."""
    d = C._dist_host(x.double().numpy(), np.asarray(cent, dtype=np.float64))
    srt = np.sort(d, 1)
    clear = (srt[:, 1] - srt[:, 0]) > 1e-5 * np.maximum(srt[:, 0], 1e-30)
    want = np.argmin(d, 1)
    assert np.array_equal(got[clear], want[clear])
    return 1.0 - clear.mean()


def test_one_lloyd_step_against_the_host():
    # overlapping blobs: many points sit near a boundary
    x, _, g = _blobs(60000, 10, 24, 0, spread=1.0)
    init = x[torch.randperm(60000, generator=g)[:10]].clone()
    xd = x.cuda()
    one = C.kmeans(xd, 10, init=init, max_iter=1)
    assert one.n_iter == 1 and not one.converged and one.restart == 0
    assert torch.equal(one.centroids.cpu(), init)        # no update after the last assignment
    lab1 = one.labels.cpu().numpy()
    assert _screened_label_check(x, init.double().numpy(), lab1) <= 1e-3
    d = C._dist_host(x.double().numpy(), init.double().numpy())
    inertia = d[np.arange(60000), lab1].sum()
    assert abs(one.inertia - inertia) <= 1e-5 * inertia
    # the update: the means of the device's own assignment
    two = C.kmeans(xd, 10, init=init, max_iter=2)
    assert two.n_iter == 2
    X = x.double().numpy()
    want = np.stack([X[lab1 == c].mean(0) for c in range(10)])
    got = two.centroids.cpu().double().numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert _screened_label_check(x, got, two.labels.cpu().numpy()) <= 1e-3
    assert torch.equal(C.assign(xd, two.centroids), two.labels)


def test_full_fit_from_a_given_init_matches_the_host_and_repeats_bitwise():
    x, y, g = _blobs(60000, 10, 24, 1)
    init = torch.stack([x[torch.randperm(60000, generator=g)[:10]] for _ in range(4)])
    xd = x.cuda()
    got = C.kmeans(xd, 10, init=init.cuda(), max_iter=100, check_every=3)
    want = C.kmeans_host(x, 10, init=init, max_iter=100)
    assert got.restart == want.restart and got.n_iter == want.n_iter
    assert got.converged == want.converged
    assert torch.equal(got.labels.cpu(), want.labels)
    assert abs(got.inertia - want.inertia) <= 1e-5 * want.inertia
    assert float((got.centroids.cpu().double() - want.centroids).abs().max()) <= \
        1e-5 * float(want.centroids.abs().max())
    again = C.kmeans(xd, 10, init=init.cuda(), max_iter=100, check_every=3)
    assert torch.equal(again.labels, got.labels) and torch.equal(again.centroids, got.centroids)
    assert again.inertia == got.inertia and again.n_iter == got.n_iter
    # the whole loop stays on the device: k-means++ restarts too, reproducible
    a = C.kmeans(xd, 10, n_init=4, seed=3)
    b = C.kmeans(xd, 10, n_init=4, seed=3)
    assert torch.equal(a.labels, b.labels) and a.inertia == b.inertia
    assert C.match_clusters(a.labels, y.cuda(), 10, 10)[1] >= 0.0


def test_kmeans_pp_on_the_device_draws_the_host_rows():
    x, _, _ = _blobs(20000, 10, 24, 2, spread=2.0)
    xd = x.cuda()
    checked = total = 0
    for seed in (0, 1):
        dev = C.kmeans(xd, 10, n_init=8, seed=seed, max_iter=1).init_index.numpy()
        _, want, margin = C.kmeans_pp_host(x, 10, n_init=8, seed=seed)
        for r in range(8):
            for j in range(10):
                total += 1
                if margin[r, j] <= 1e-5:
                    break          # (later draws follow from this one)
                assert dev[r, j] == want[r, j], (seed, r, j)
                checked += 1
    assert checked > total // 2, (checked, total)


def _noise_run(step, images, labels, B):
    """The eager forwards of every batch of a split on the noise its replay draws; ->
    (presence (N, O), mass (N, O))."""
    from torch_scae_amd import nn_utils
    N = images.shape[0]
    pres, mass = [], []
    for lo in range(0, N, B):
        s = step if lo + B <= N else step._tail_step
        x, y = images[lo:lo + B], labels[lo:lo + B]
        noise = _replay_with_noise(s, x.cpu(), y.cpu())
        with s._eval_mode(), nn_utils.fixed_noise([n.cuda() for n in noise[1:]]):
            res = s.model(x)
        pres.append(res.caps_presence.float())
        mass.append(res.posterior_mixing_prob.sum(-1).float())
        s.reset()
    return torch.cat(pres), torch.cat(mass)


@pytest.mark.parametrize("variant", ["fused", "outside_tail"])
def test_encode_rows_means_launches_and_overflow(variant):
    from torch_scae_amd import EvalStep, ops
    from torch_scae_amd import data as D
    cfg, B, sd, g = full_size_params("cfg2")
    if variant == "outside_tail":
        cfg = dict(cfg, scae_params=dict(cfg["scae_params"], recon_mse_weight=0.7))
    model = _model(cfg, sd)
    O = cfg["n_obj_caps"]
    N = 2 * B + 40
    images = torch.rand(N, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (N,), generator=g).cuda()
    plain = EvalStep(model, B, cfg["image_shape"])
    plain.capture()
    step = EvalStep(model, B, cfg["image_shape"])
    step.encode(images, labels)                      # captures both steps with the sink
    graph, nodes = step.graph, step.graph_nodes
    extra = 0 if variant == "fused" else 1           # the standalone launch
    assert step.fused == (variant == "fused")
    assert nodes[2] == plain.graph_nodes[2] + extra, (nodes, plain.graph_nodes)
    torch.manual_seed(5)
    ops.reset_noise()
    enc = step.encode(images, labels)
    assert step.graph is graph, "encode recaptured"
    assert enc["rows"] == N and not enc["overflow"]
    assert enc["prior"].shape == (N, O) and torch.equal(enc["label"], labels)
    torch.manual_seed(5)
    ops.reset_noise()
    pres, mass = _noise_run(step, images, labels, B)
    assert float((enc["prior"] - pres).abs().max()) <= 1e-5
    assert float((enc["posterior"] - mass).abs().max()) <= 1e-5 * max(1.0, float(mass.abs().max()))
    torch.manual_seed(5)
    ops.reset_noise()
    want = step.evaluate(images, labels)
    for k in ("loss", "accuracy", "log_prob", "rec_ll"):
        assert torch.equal(enc["means"][k], want[k]), k
    # another output, no recapture; a short one reports the overflow
    torch.manual_seed(5)
    ops.reset_noise()
    short = torch.full((B + 3, 2, O), -1.0, device="cuda")
    enc2 = step.encode(images, labels, out=short)
    assert step.graph is graph
    assert enc2["rows"] == B + 3 and enc2["overflow"]
    assert torch.equal(enc2["features"], enc["features"][:B + 3])
    # the sink is off again: evaluate() gives the same bits as the plain step
    torch.manual_seed(5)
    ops.reset_noise()
    assert torch.equal(step.evaluate(images, labels)["loss"], want["loss"])
    if variant != "fused":
        return
    # a device-resident view: the rows of its materialised split, bit for bit
    u8 = (images[:, 0] * 255).to(torch.uint8).cpu()
    ds = D.ResidentDataset(u8, labels.cpu(), out_size=(40, 40), device="cuda")
    view = D.DatasetView(ds, shuffle=True, translate=False, seed=9)
    mi, ml = view.materialise()
    torch.manual_seed(5)
    ops.reset_noise()
    ev = step.encode(view)
    assert view.epoch == 1 and torch.equal(ev["label"], ml.cuda())
    torch.manual_seed(5)
    ops.reset_noise()
    et = step.encode(mi.cuda(), ml.cuda())
    assert torch.equal(ev["features"], et["features"])
    assert torch.equal(ev["means"]["loss"], et["means"]["loss"])


def test_unsupervised_accuracy_after_a_short_training_run():
    from torch_scae_amd import EvalStep, ops
    from torch_scae_amd import data as D
    from torch_scae_amd.train_step import TrainStep
    cfg, B, sd, _ = full_size_params("cfg2")
    model = _model(cfg, sd)
    imgs, labs = D.stroke_batches(12, B, cfg["image_shape"], seed=4)
    torch.manual_seed(0)
    ts = TrainStep(model, B, cfg["image_shape"], lr=1e-4)
    for i in range(8):
        ts(imgs[i].cuda(), labs[i].cuda())
    torch.cuda.synchronize()
    step = EvalStep(model, B, cfg["image_shape"])
    # (both splits leave a remainder of 4: one tail step, captured by the first encode)
    fit = (imgs[:8].flatten(0, 1).cuda()[:900], labs[:8].flatten().cuda()[:900])
    test = (imgs[8:].flatten(0, 1).cuda()[:260], labs[8:].flatten().cuda()[:260])
    step.encode(*fit)
    g = torch.Generator().manual_seed(8)
    init = torch.rand(3, 10, cfg["n_obj_caps"], generator=g).cuda()
    torch.manual_seed(5)
    ops.reset_noise()
    out = C.unsupervised_accuracy(step, fit, test, k=10, feature="prior", init=init)
    assert 0.0 <= out["fit_accuracy"] <= 1.0 and 0.0 <= out["test_accuracy"] <= 1.0
    # the same pieces by hand on the same encoded features
    torch.manual_seed(5)
    ops.reset_noise()
    ef, et = step.encode(*fit), step.encode(*test)
    res = C.kmeans(ef["prior"].contiguous(), 10, init=init)
    mapping, acc = C.match_clusters(res.labels, fit[1], 10, 10)
    assert out["fit_accuracy"] == acc and out["mapping"].tolist() == mapping.tolist()
    cid = C.assign(et["prior"].contiguous(), res.centroids)
    assert out["test_accuracy"] == C.mapped_accuracy(cid, test[1], mapping, 10)
    assert out["inertia"] == res.inertia and out["n_iter"] == res.n_iter
    # against the fp64 host pipeline: one assignment from the same init, the labels equal
    # wherever the host's best / second-best gap is clear, the accuracies within the share
    # of points that is not
    x = ef["prior"].contiguous()
    dev1 = C.kmeans(x, 10, init=init, max_iter=1)
    host1 = C.kmeans_host(x.cpu(), 10, init=init.cpu(), max_iter=1)
    assert dev1.restart == host1.restart
    excluded = _screened_label_check(x.cpu(), init[dev1.restart].cpu().double().numpy(),
                                     dev1.labels.cpu().numpy())
    a_dev = C.match_clusters(dev1.labels, fit[1], 10, 10)[1]
    a_host = C.match_clusters(host1.labels, fit[1].cpu(), 10, 10)[1]
    assert abs(a_dev - a_host) <= excluded + 1e-12, (a_dev, a_host, excluded)
