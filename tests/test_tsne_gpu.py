"""t-SNE on the GPU: the kernels of csrc/tsne.hip against the numpy restatement (embed.*_host)
-- the affinities from the device's own beta, one iteration from a chosen state, whole runs --
bit reproducibility across runs and ``check_every``, argument errors, and capsule_embedding end
to end.

Bars (tests/test_probe_gpu.py's scheme).  The device works in fp32 where the host restatement
works in fp64, so a compared tensor may differ from the fp64 host by what fp32 arithmetic costs:
4 x the largest entry-wise distance between the host run in fp32 and in fp64 on the same input
(the 4: the device sums in another order than numpy), with a floor of 8 fp32 ulp of the tensor's
largest magnitude.  Gains are compared on the entries whose fp64 |g * velocity| exceeds twice the
largest fp32-host / fp64-host difference of that product; at most 1 % of the entries may fall
under it."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_probe_gpu import bar, within
from tests.test_tsne import blobs, duplicates_and_outlier, purity_1nn, uniform
from torch_scae_amd import _lib
from torch_scae_amd import embed as E

pytestmark = pytest.mark.gpu

SHAPES = [(4, 1, 1.0), (63, 3, 5.0), (64, 24, 10.0), (65, 24, 21.0), (257, 255, 30.0),
          (4099, 24, 30.0)]
# for one iteration besides: two update workgroups and a nearly empty third (the recentring's grid)
ITERATION_SHAPES = SHAPES + [(513, 24, 30.0)]


def _input(N, F, kind):
    return uniform(N, F, 20 + N) if kind == "uniform" else duplicates_and_outlier(N, F, 20 + N)


@pytest.mark.parametrize("N, F, perplexity, kind",
                         [s + ("uniform",) for s in SHAPES] + [(65, 24, 21.0, "duplicates")])
def test_affinities_from_the_devices_own_beta(N, F, perplexity, kind):
    case = f"({N}, {F}, {perplexity}, {kind})"
    x = _input(N, F, kind)
    P, beta, plogp = E.affinities(x.cuda(), perplexity)
    assert P.is_cuda and P.shape == (N, N) and P.dtype == torch.float32 and beta.shape == (N,)
    b = beta.cpu()
    assert bool(torch.isfinite(b).all()) and bool((b > 0).all())
    H64, H32 = E.entropy_host(x, b), E.entropy_host(x, b, np.float32)
    slack = 4.0 * float(np.abs(H32.astype(np.float64) - H64).max())
    err = float(np.abs(H64 - math.log(perplexity)).max())
    print(f"{case} entropy: worst |H64(beta) - log perplexity| {err:.3e} (1e-5 + {slack:.3e})")
    assert err <= 1e-5 + slack
    P64, pl64 = E.joint_host(x, b)
    P32, pl32 = E.joint_host(x, b, np.float32)
    within("P", P.cpu().numpy(), P32, P64, case)
    assert torch.equal(P, P.T.contiguous()) and bool((P.diagonal() == 0).all())
    within("sum P log P", plogp, pl32, pl64, case)


@functools.lru_cache(maxsize=None)
def _joint(N):
    """The device's P of the uniform input at N -> (P on the device, P fp32 numpy, sum P log P
    of those fp32 values in fp64)."""
    _, F, perplexity = next(s for s in ITERATION_SHAPES if s[0] == N)
    P, _, _ = E.affinities(uniform(N, F, 20 + N).cuda(), perplexity)
    Pn = P.cpu().numpy()
    pos = Pn[Pn > 0].astype(np.float64)
    return P, Pn, float((pos * np.log(pos)).sum())


def one_iteration_state(N, scale):
    """-> (Y, velocity, gains) fp32: Y ~ scale N(0, 1), velocity ~ 0.1 scale N(0, 1), gains
    uniform in [0.01, 2]."""
    rng = np.random.default_rng(1000 + N)
    Y = (scale * rng.standard_normal((N, 2))).astype(np.float32)
    vel = (0.1 * scale * rng.standard_normal((N, 2))).astype(np.float32)
    return Y, vel, rng.uniform(0.01, 2.0, (N, 2)).astype(np.float32)


def clear_gains(h32, h64):
    """Entries whose fp64 |g * velocity| exceeds twice the largest fp32 / fp64 difference."""
    thr = 2.0 * float(np.abs(h32["gv"].astype(np.float64) - h64["gv"]).max())
    clear = np.abs(h64["gv"]) > thr
    assert (~clear).mean() <= 0.01, (~clear).mean()
    return clear


@pytest.mark.parametrize("scale, it", [(1e-4, 3), (5.0, 300)])
@pytest.mark.parametrize("N", [s[0] for s in ITERATION_SHAPES])
def test_one_iteration_from_a_chosen_state(N, scale, it):
    case = f"(N = {N}, Y ~ {scale}, iteration {it})"
    P, Pn, plogp = _joint(N)
    lr = max(N / 12.0 / 4.0, 50.0)
    p = E._TsneProblem(P, plogp, torch.zeros(N, 2), 1000, 12.0, 250, lr, 1)
    G = _lib.load().scae_tsne_groups(N)
    assert p.desc.G == G and (G > 1) == (N >= 257)
    Y, vel, gains = one_iteration_state(N, scale)
    p.load_state(Y, vel, gains)
    p.run(it, 1)
    torch.cuda.synchronize()
    ex, mom = E._schedule(it, 250, 12.0)
    assert ex == (12.0 if scale < 1 else 1.0)
    h64 = E.step_host(Pn, Y, vel, gains, ex, mom, np.float32(lr), plogp)
    h32 = E.step_host(Pn, Y, vel, gains, ex, mom, np.float32(lr), plogp, dtype=np.float32)
    print(f"{case} fp32-host gradient error "
          f"{float(np.abs(h32['grad'] - h64['grad']).max()):.3e} against "
          f"{float(np.abs(h64['grad']).max()):.3e}")
    got = p.Y.cpu().numpy()
    within("Y", got, h32["Y"], h64["Y"], case)
    # every workgroup of the finish launch recentres its own rows: the columns sum to zero
    # (test_bits_repeat's bar), and each workgroup's first and last row moved by the host's amount
    assert float(np.abs(got.astype(np.float64).mean(0)).max()) <= 1e-6 * float(np.abs(got).max())
    m32, m64 = h32["Y"].astype(np.float64) - Y, h64["Y"] - Y
    ends = sorted({0, min(255, N - 1), min(256, N - 1), N - 1})
    err = float(np.abs((got.astype(np.float64) - Y - m64)[ends]).max())
    print(f"{case} movement of rows {ends}: error {err:.3e} (bar {bar(m32, m64):.3e})")
    assert err <= bar(m32, m64), (case, ends, err)
    within("velocity", p.velocity.cpu().numpy(), h32["velocity"], h64["velocity"], case)
    hist = p.history.cpu().numpy()
    assert hist[it - 1, 0] == it and not hist[:it - 1].any() and not hist[it:].any()
    within("KL", hist[it - 1, 1], h32["kl"], h64["kl"], case)
    within("|g|", hist[it - 1, 2], h32["grad_norm"], h64["grad_norm"], case)
    clear = clear_gains(h32, h64)
    print(f"{case} gains: {int((~clear).sum())} of {clear.size} entries under the threshold")
    within("gains", p.gains.cpu().numpy()[clear], h32["gains"][clear], h64["gains"][clear], case)


def _same(a, b):
    return torch.equal(a.y, b.y) and torch.equal(a.history, b.history) and a.kl == b.kl and \
        torch.equal(a.beta, b.beta)


@pytest.mark.parametrize("N", [257, 4099])
def test_bits_repeat_across_runs_and_check_every(N):
    x = uniform(N, 24, 3).cuda()
    kw = dict(n_iter=60, exaggeration_iter=20)
    a = E.tsne(x, check_every=60, **kw)
    assert a.y.is_cuda and a.y.shape == (N, 2) and bool(torch.isfinite(a.y).all())
    assert a.history.shape == (1, 3) and a.history[0, 0] == 60 and a.kl == float(a.history[0, 1])
    assert _same(a, E.tsne(x, check_every=60, **kw))
    one, seven = E.tsne(x, check_every=1, **kw), E.tsne(x, check_every=7, **kw)
    assert torch.equal(one.y, a.y) and torch.equal(seven.y, a.y)
    assert one.history.shape == (60, 3) and seven.history.shape == (9, 3)
    assert one.history[:, 0].tolist() == [float(i) for i in range(1, 61)]
    assert torch.equal(one.history[6::7][:8], seven.history[:8])
    assert torch.equal(one.history[-1], seven.history[-1]) and one.kl == a.kl
    assert float(a.y.double().mean(0).abs().max()) <= 1e-6 * float(a.y.abs().max())
    # non-contiguous input is taken by copy
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous() and _same(a, E.tsne(xt, check_every=60, **kw))


# The whole run's KL margin.  The dynamics amplify rounding, so the device's final KL is held to
# the fp64 host run's times (1 + KL_MARGIN), KL_MARGIN = twice the worst relative
# |KL32 - KL64| / KL64 of tsne_host in fp32 and in fp64 on seeds 0 - 4 of this input (data seed =
# init seed = s): MEASURED_REL below.
MEASURED_REL = (6.72e-4, 3.30e-3, 8.74e-3, 8.12e-4, 9.04e-3)       # -> KL_MARGIN = 0.0181
KL_MARGIN = 2.0 * max(MEASURED_REL)
WHOLE = dict(perplexity=30.0, n_iter=300, exaggeration_iter=100, init="random", seed=0)


@pytest.fixture(scope="module")
def whole():
    x, y = blobs(400, 24, 10, 0)
    return x, y, E.tsne_host(x, **WHOLE)


def test_a_whole_run_against_the_host(whole):
    x, y, host = whole
    got = E.tsne(x.cuda(), **WHOLE)
    assert got.n_iter == 300 and got.history.shape == (6, 3)
    assert got.history[:, 0].tolist() == [50.0, 100.0, 150.0, 200.0, 250.0, 300.0]
    # the reported KL is the KL of the returned Y under the device's P
    P, _, plogp = E.affinities(x.cuda(), 30.0)
    Pn, Yn = P.cpu().numpy(), got.y.cpu().numpy()
    pos = Pn[Pn > 0].astype(np.float64)
    pl = float((pos * np.log(pos)).sum())
    within("reported KL", got.kl, E.kl_host(Pn, Yn, pl, np.float32), E.kl_host(Pn, Yn, pl))
    within("sum P log P", plogp, pl, pl)
    pd, ph = purity_1nn(Yn, y), purity_1nn(host.y.numpy(), y)
    print(f"1-NN purity: device {pd:.4f}, fp64 host {ph:.4f}; KL: device {got.kl:.6f}, fp64 "
          f"host {host.kl:.6f} (margin {KL_MARGIN:.4f})")
    assert pd >= ph - 0.01
    assert got.kl <= host.kl * (1.0 + KL_MARGIN)


def test_errors_on_the_device():
    x = uniform(100, 4, 5).cuda()
    with pytest.raises(ValueError, match="x must be fp32"):
        E.tsne(x.double(), perplexity=5.0)
    with pytest.raises(ValueError, match="x must be fp32"):
        E.affinities(x.double(), 5.0)
    with pytest.raises(ValueError, match=rf"N = {E.MAX_N + 1}"):
        E.tsne(torch.zeros(E.MAX_N + 1, 2, device="cuda"))
    with pytest.raises(ValueError, match=r"perplexity = 34.0, N = 100"):
        E.tsne(x, perplexity=34.0)
    lib = _lib.load()
    P, _, plogp = E.affinities(x, 5.0)
    d = E._TsneProblem(P, plogp, torch.zeros(100, 2), 10, 12.0, 5, 50.0, 5).desc
    assert lib.scae_tsne_run_f32(d, 8, 3, None) == -1   # past n_iter
    d.G += 1                                            # a descriptor of another grouping
    assert lib.scae_tsne_run_f32(d, 0, 1, None) == -1


def test_capsule_embedding_end_to_end_is_tsne_on_the_encoded_features():
    from tests.test_eval_step_gpu import _model
    from tests.test_hip_model import full_size_params
    from torch_scae_amd import EvalStep, cluster, ops
    from torch_scae_amd import data as D
    cfg, B, sd, _ = full_size_params("cfg2")
    model = _model(cfg, sd)
    imgs, labs = D.stroke_batches(3, B, cfg["image_shape"], seed=4)
    step = EvalStep(model, B, cfg["image_shape"])
    split = (imgs.flatten(0, 1).cuda()[:260], labs.flatten().cuda()[:260])
    step.encode(*split)
    kw = dict(perplexity=20.0, n_iter=40, exaggeration_iter=15, check_every=20)
    torch.manual_seed(5)
    ops.reset_noise()
    out = E.capsule_embedding(step, split, **kw)
    assert out["y"].shape == (260, 2) and bool(torch.isfinite(out["y"]).all())
    assert torch.equal(out["label"], split[1]) and out["history"].shape == (2, 3)
    torch.manual_seed(5)
    ops.reset_noise()
    res = E.tsne(cluster.features(step.encode(*split), "prior"), **kw)
    assert torch.equal(out["y"], res.y) and out["kl"] == res.kl
    assert torch.equal(out["history"], res.history)
