"""The linear probe on the GPU: the kernels of csrc/linear_probe.hip against the numpy
restatement (probe.fit_host and its pieces) -- moments entry by entry, one iteration from a
random state, whole fits, predictions -- bit reproducibility, a stopped problem beside a
running one, argument errors, and linear_probe_accuracy end to end.

Bars.  The device works in fp32 where the host restatement works in fp64, so a compared tensor
may differ from the fp64 host by what fp32 arithmetic costs: 4 x the largest entry-wise distance
between the host run in fp32 and in fp64 on the same input (the 4: the device sums in another
order than numpy), with a floor of 8 fp32 ulp of the tensor's largest magnitude.  Labels are
compared on the rows whose fp64 top-two logit gap exceeds twice the largest fp32-host /
fp64-host logit difference; at most 1 % of the rows may fall under it."""
import numpy as np
import pytest
import torch

from tests.test_probe import synthetic
from torch_scae_amd import _lib
from torch_scae_amd import probe as P

pytestmark = pytest.mark.gpu


def bar(h32, h64):
    h32, h64 = np.asarray(h32, dtype=np.float64), np.asarray(h64, dtype=np.float64)
    floor = 8.0 * float(np.spacing(np.float32(np.abs(h64).max())))
    return max(4.0 * float(np.abs(h32 - h64).max()), floor)


def within(name, got, h32, h64, case=""):
    b = bar(h32, h64)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(h64, np.float64)).max())
    d32 = float(np.abs(np.asarray(h32, dtype=np.float64) - np.asarray(h64, np.float64)).max())
    print(f"{case} {name}: device error {err:.3e}, fp32 host {d32:.3e} (bar {b:.3e})")
    assert err <= b, (case, name, err, b)


def clear_rows(l32, l64):
    """Rows whose fp64 top-two gap exceeds twice the largest fp32 / fp64 logit difference."""
    thr = 2.0 * float(np.abs(l32.astype(np.float64) - l64).max())
    top = np.sort(l64, 1)
    clear = (top[:, -1] - top[:, -2]) > thr if l64.shape[1] > 1 else np.ones(len(l64), bool)
    assert (~clear).mean() <= 0.01, (~clear).mean()
    return clear


@pytest.mark.parametrize("N, F, C", [(1, 1, 2), (63, 3, 3), (64, 24, 10), (65, 24, 33),
                                     (257, 255, 2), (4099, 3, 10), (4099, 255, 33)])
def test_moments_entry_by_entry_and_the_outside_count(N, F, C):
    x, y = synthetic(N, F, C, 10 + N)
    y[::3] = C + 1
    if N > 1:
        y[1] = -1
    outside = int(((y < 0) | (y >= C)).sum())
    G, count = P._moments_device(x.cuda(), y.cuda(), C)
    X1 = np.concatenate([x.double().numpy(), np.ones((N, 1))], 1)
    want, mag = X1.T @ X1, np.abs(X1).T @ np.abs(X1)
    rel = float((np.abs(G - want) / mag).max())
    print(f"moments ({N}, {F}): worst entry {rel:.3e} of sum |x_i x_j|")
    assert rel <= 1e-13
    assert np.array_equal(G, G.T) and G[F, F] == N
    assert count == outside
    # without labels nothing is counted
    assert P._moments_device(x.cuda(), None, C)[1] == 0


STEP_SHAPES = [(1, 3, 2), (63, 1, 3), (64, 24, 10), (65, 3, 33), (257, 24, 2), (4099, 24, 10),
               (65, 63, 256), (257, 255, 64), (4099, 255, 33)]


@pytest.mark.parametrize("N, F, C", STEP_SHAPES)
def test_one_iteration_from_a_random_state(N, F, C):
    case = f"({N}, {F}, {C})"
    x, y = synthetic(N, F, C, 100 + N + F, constant=1 if F >= 3 else None)
    l2s = [1e-3, 1e-1]
    p = P.DeviceProblems(x.cuda(), y.cuda(), C, l2s, [0.0, 0.0], 5)
    assert p.desc.G == _lib.load().scae_probe_groups(N, F)
    rng = np.random.default_rng(7 + N)
    W = (0.3 * rng.standard_normal((2, C, F + 1))).astype(np.float32)
    V = (W + 0.1 * rng.standard_normal((2, C, F + 1))).astype(np.float32)
    t = np.array([3.7, 1.0])
    p.load_state(W, V, t)
    p.run(1)
    torch.cuda.synchronize()
    hist, state = p.history.cpu().numpy(), p.state.cpu().numpy()
    assert state[-1] == 0 and state[0] == 0 and state[1] == 1 and state[5] == 1
    yn = y.numpy()
    Z64 = P.standardise(x, p.mean, p.scale)
    Z32 = P.standardise(x, p.mean, p.scale, np.float32)
    skipped = 0
    for r in range(2):
        h64 = P.step_host(Z64, yn, W[r].astype(np.float64), V[r].astype(np.float64), t[r],
                          l2s[r], p.L[r])
        h32 = P.step_host(Z32, yn, W[r], V[r], t[r], l2s[r], p.L[r], dtype=np.float32)
        within("J", hist[r, 0, 0], h32["J"], h64["J"], case)
        within("grad", p.grad[r].cpu().numpy(), h32["grad"], h64["grad"], case)
        within("max |g|", hist[r, 0, 1], h32["grad_norm"], h64["grad_norm"], case)
        within("W", p.W[r].cpu().numpy(), h32["W"], h64["W"], case)
        within("V", p.V[r].cpu().numpy(), h32["V"], h64["V"], case)
        if abs(h64["dot"]) <= bar(h32["dot"], h64["dot"]):
            skipped += 1           # (the restart sum is too close to zero to call)
            continue
        assert hist[r, 0, 2] == float(h64["restart"]) and state[4 * r + 3] == int(h64["restart"])
        within("t", float(p.t[r]), h32["t"], h64["t"], case)
    assert skipped == 0
    # the constant column takes no part: its gradient is the penalty's alone
    if F >= 3:
        assert p.scale[1] == 0.0
        for r in range(2):
            assert torch.equal(p.grad[r, :, 1].cpu(),
                               torch.from_numpy(np.float32(l2s[r]) * V[r, :, 1]))


@pytest.fixture(scope="module")
def problem():
    """(4099, 24, 10) with a constant column, and the fp64 / fp32 host fits."""
    x, y = synthetic(4099, 24, 10, 1, constant=5)
    h64 = P.fit_host(x, y, 10, l2=1e-3)
    h32 = P.fit_host(x, y, 10, l2=1e-3, dtype=np.float32)
    return x, y, h64, h32


def _logits(x, res, dtype=np.float64):
    return P._logits_host(x, res.weight.cpu().numpy(), res.bias.cpu().numpy(), dtype)


def test_whole_fit_against_the_host(problem):
    x, y, h64, h32 = problem
    got = P.fit(x.cuda(), y.cuda(), 10, l2=1e-3)
    print(f"iterations: device {got.n_iter}, fp64 host {h64.n_iter}, fp32 host {h32.n_iter}")
    assert got.converged == h64.converged is True
    assert got.weight.is_cuda and got.weight.dtype == torch.float32
    assert got.history.shape == (got.n_iter, 3) and got.grad_norm <= 1e-5
    within("loss", got.loss, h32.loss, h64.loss)
    assert torch.all(got.weight[:, 5] == 0.0)
    l64 = _logits(x, h64)
    clear = clear_rows(_logits(x, h32, np.float32), l64)
    lab, _ = P.predict(x.cuda(), got)
    assert np.array_equal(lab.cpu().numpy()[clear], l64.argmax(1)[clear])
    wgap = float((got.weight.cpu().double() - h64.weight).abs().max())
    print(f"largest weight distance: device {wgap:.3e}, fp32 host "
          f"{float((h32.weight - h64.weight).abs().max()):.3e}")


def _same(a, b):
    return torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias) and \
        torch.equal(a.history, b.history) and a.n_iter == b.n_iter and a.loss == b.loss


def test_bits_repeat_across_runs_chunking_and_neighbours(problem):
    x, y = problem[0].cuda(), problem[1].cuda()
    a = P.fit(x, y, 10, l2=1e-2, max_iter=120)
    assert _same(a, P.fit(x, y, 10, l2=1e-2, max_iter=120))
    assert _same(a, P.fit(x, y, 10, l2=1e-2, max_iter=120, check_every=1))
    three = P.fit(x, y, 10, l2=[1e-4, 1e-2, 1.0], max_iter=120)
    assert _same(a, three[1]) and [r.l2 for r in three] == [1e-4, 1e-2, 1.0]
    assert not torch.equal(three[0].weight, three[1].weight)
    # non-contiguous input is taken by copy
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous() and _same(a, P.fit(xt, y, 10, l2=1e-2, max_iter=120))


def test_a_stopped_problem_keeps_its_state_while_the_other_runs(problem):
    x, y = problem[0].cuda(), problem[1].cuda()
    solo = P.fit(x, y, 10, l2=1e-3, tol=1e-2, max_iter=300)
    assert solo.converged and solo.n_iter < 100
    p = P.DeviceProblems(x, y, 10, [1e-3, 1e-3], [1e-2, 1e-6], 300)
    p.run(solo.n_iter)
    assert p.stopped() == 1
    W, V, g, t = p.W[0].clone(), p.V[0].clone(), p.grad[0].clone(), p.t[0].clone()
    p.run(100)
    assert p.stopped() == 1
    assert torch.equal(p.W[0], W) and torch.equal(p.V[0], V) and torch.equal(p.grad[0], g)
    assert torch.equal(p.t[0], t) and not torch.equal(p.W[1], W)
    pair = p.results()
    assert _same(pair[0], solo) and pair[0].converged and pair[1].n_iter == solo.n_iter + 100
    both = P.fit(x, y, 10, l2=[1e-3, 1e-3], tol=[1e-2, 1e-6], max_iter=300)
    assert _same(both[0], solo) and both[1].n_iter > solo.n_iter


@pytest.mark.parametrize("N, F, C", [(1, 3, 2), (65, 24, 10), (4099, 255, 33), (257, 255, 64)])
def test_predict_against_the_host(N, F, C):
    x, y = synthetic(N, F, C, 200 + N)
    g = torch.Generator().manual_seed(N)
    res = P.ProbeResult(torch.randn(C, F, generator=g) * 2 / np.sqrt(F),
                        torch.randn(C, generator=g), 0.0, 0, False, 0.0, 0.0, None)
    lab, logp = P.predict(x.cuda(), res)
    ce = P.mean_cross_entropy(x.cuda(), y.cuda(), res)
    assert lab.dtype == torch.int64 and lab.shape == logp.shape == (N,)
    l64, l32 = _logits(x, res), _logits(x, res, np.float32)
    clear = clear_rows(l32, l64)
    assert np.array_equal(lab.cpu().numpy()[clear], l64.argmax(1)[clear])
    rows = np.arange(N)[clear]
    lp64 = (l64.max(1) - P._lse_rows(l64))[rows]
    lp32 = (l32.max(1) - P._lse_rows(l32))[rows]
    within("log_prob", logp.cpu().numpy()[rows], lp32, lp64, f"({N}, {F}, {C})")
    yn = y.numpy()
    ce64 = float((P._lse_rows(l64) - l64[np.arange(N), yn]).mean())
    ce32 = float((P._lse_rows(l32) - l32[np.arange(N), yn]).astype(np.float64).mean())
    within("mean cross-entropy", ce, ce32, ce64, f"({N}, {F}, {C})")
    assert ce64 == pytest.approx(P.mean_cross_entropy(x, y, res), rel=1e-12)


def test_an_exact_tie_goes_to_the_lower_class():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(4, 24, generator=g)
    w[3] = w[1]
    b = torch.tensor([0.0, 0.3, 0.1, 0.3])
    x = torch.rand(300, 24, generator=g)
    res = P.ProbeResult(w, b, 0.0, 0, False, 0.0, 0.0, None)
    lab = P.predict(x.cuda(), res)[0].cpu()
    assert not bool((lab == 3).any()) and bool((lab == 1).any())
    assert torch.equal(lab, P.predict(x, res)[0])


def test_errors_on_the_device():
    x, y = synthetic(100, 4, 3, 5)
    xd, yd = x.cuda(), y.cuda()
    bad = yd.clone()
    bad[:7] = 3
    bad[50] = -2
    with pytest.raises(ValueError, match=r"8 labels outside \[0, 3\)"):
        P.fit(xd, bad, 3)
    with pytest.raises(ValueError, match="x must be fp32"):
        P.fit(xd.double(), yd, 3)
    with pytest.raises(ValueError, match="the probe takes"):
        P.fit(torch.zeros(10, 257, device="cuda"), yd[:10], 3)
    with pytest.raises(ValueError, match="the probe takes"):
        P.fit(torch.zeros(10, 255, device="cuda"), yd[:10], 65)
    with pytest.raises(ValueError, match="at most 16 l2 values"):
        P.fit(xd, yd, 3, l2=[1e-3] * 17)
    with pytest.raises(ValueError, match="check_every"):
        P.fit(xd, yd, 3, check_every=0)
    with pytest.raises(ValueError, match=r"8 labels outside \[0, 3\)"):
        P.mean_cross_entropy(xd, bad, P.fit(xd, yd, 3, max_iter=2))
    lib = _lib.load()
    d = P.DeviceProblems(xd, yd, 3, [1e-3], [1e-5], 4).desc
    d.G += 1                                     # a descriptor of another grouping is refused
    assert lib.scae_probe_fit_f32(d, 1, None) == -1


def test_linear_probe_accuracy_end_to_end_is_the_host_pipeline():
    from tests.test_eval_step_gpu import _model
    from tests.test_hip_model import full_size_params
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
    fit = (imgs[:8].flatten(0, 1).cuda()[:900], labs[:8].flatten().cuda()[:900])
    test = (imgs[8:].flatten(0, 1).cuda()[:260], labs[8:].flatten().cuda()[:260])
    step.encode(*fit)
    l2s = (1e-4, 1e-2)
    torch.manual_seed(5)
    ops.reset_noise()
    out = P.linear_probe_accuracy(step, fit, test, l2=l2s, select=fit, n_classes=10,
                                  max_iter=400)
    assert out["confusion"].shape == (10, 10) and out["confusion"].sum() == 260
    assert out["test_accuracy"] == np.trace(out["confusion"]) / 260
    # the host path on the same encode output
    torch.manual_seed(5)
    ops.reset_noise()
    ef, et = step.encode(*fit), step.encode(*test)
    xf, xt = ef["prior"].cpu(), et["prior"].cpu()
    yf, yt = fit[1].cpu(), test[1].cpu()
    h64 = P.fit_host(xf, yf, 10, l2=list(l2s), max_iter=400)
    h32 = P.fit_host(xf, yf, 10, l2=list(l2s), max_iter=400, dtype=np.float32)
    accs = [float((P.predict(xf, r)[0] == yf).double().mean()) for r in h64]
    best = max(range(2), key=lambda i: (accs[i], l2s[i]))
    print(f"host accuracies on the fit split {accs}, device chose l2 = {out['l2']}")
    assert out["l2"] == l2s[best]
    for x, y, key in ((xf, yf, "fit_accuracy"), (xt, yt, "test_accuracy")):
        l64 = _logits(x, h64[best])
        clear = clear_rows(_logits(x, h32[best], np.float32), l64)
        lab = P.predict(x.cuda(), out["result"])[0].cpu().numpy()
        assert np.array_equal(lab[clear], l64.argmax(1)[clear])
        assert int((lab[clear] == y.numpy()[clear]).sum()) == \
            int((l64.argmax(1)[clear] == y.numpy()[clear]).sum())
        assert out[key] == float((lab == y.numpy()).mean())
