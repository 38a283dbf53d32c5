"""Host side of t-SNE (torch_scae_amd/embed.py): the fp64 numpy restatement's rules -- every
row's entropy at its beta, P symmetric with a zero diagonal and unit sum, the gradient against a
central finite difference of the restatement's own KL, duplicates and an outlier, the two
initialisations, argument checks, and ``tsne`` on a CPU tensor."""
import math

import numpy as np
import pytest
import torch

from torch_scae_amd import _lib
from torch_scae_amd import embed as E


def uniform(N, F, seed):
    return torch.from_numpy(np.random.default_rng(seed).random((N, F)).astype(np.float32))


def duplicates_and_outlier(N, F, seed):
    """Uniform rows; rows 3 .. 10 are one point, the last row lies 1e3 away."""
    x = uniform(N, F, seed)
    x[3:11] = x[3]
    x[-1, 0] += 1e3
    return x


def blobs(N, F, k, seed):
    """k Gaussian clusters, centres ~ 4 N(0, 1), unit noise -> (x fp32, labels)."""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((k, F))
    y = rng.integers(0, k, N)
    x = centres[y] + rng.standard_normal((N, F))
    return torch.from_numpy(x.astype(np.float32)), y


def purity_1nn(Y, labels):
    """The share of points whose nearest other point has their label."""
    Y = np.asarray(Y, dtype=np.float64)
    d = ((Y[:, None] - Y[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return float((labels[d.argmin(1)] == labels).mean())


@pytest.mark.parametrize("N, F, perplexity", [(91, 3, 10.0), (257, 24, 30.0)])
def test_entropy_at_beta_and_the_joint_matrix(N, F, perplexity):
    x = uniform(N, F, N)
    P, beta, plogp = E.affinities_host(x, perplexity)
    H = E.entropy_host(x, beta)
    assert float(np.abs(H - math.log(perplexity)).max()) <= 1e-5
    P = P.numpy()
    assert P.dtype == np.float64 and np.array_equal(P, P.T)
    assert np.all(np.diagonal(P) == 0.0) and abs(P.sum() - 1.0) <= 1e-12
    pos = P[P > 0]
    assert plogp == pytest.approx(float((pos * np.log(pos)).sum()), rel=1e-12)
    # the conditional rows: p_{j|i} = exp(-beta_i (d_ij - min)) / S, written out
    X = x.double().numpy()
    D = ((X[:, None] - X[None]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    C = np.exp(-beta.numpy()[:, None] * (D - D.min(1, keepdims=True)))
    C /= C.sum(1, keepdims=True)
    assert np.abs(P - (C + C.T) / (2 * N)).max() <= 1e-15


def test_gradient_is_the_finite_difference_of_the_restatements_kl():
    N = 40
    x = uniform(N, 5, 1)
    P, _, plogp = E.affinities_host(x, 8.0)
    rng = np.random.default_rng(2)
    Y = rng.standard_normal((N, 2))
    zero, one = np.zeros((N, 2)), np.ones((N, 2))
    g = E.step_host(P, Y, zero, one, 1.0, 0.8, 10.0, plogp)["grad"]
    assert E.step_host(P, Y, zero, one, 1.0, 0.8, 10.0, plogp)["kl"] == \
        pytest.approx(E.kl_host(P, Y, plogp), rel=1e-14)
    h = 1e-5
    worst = 0.0
    for i in range(N):
        for k in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, k] += h
            Ym[i, k] -= h
            fd = (E.kl_host(P, Yp, plogp) - E.kl_host(P, Ym, plogp)) / (2 * h)
            worst = max(worst, abs(fd - g[i, k]))
    # central difference: the truncation term h^2 |KL'''| / 6 and rounding 1e-16 |KL| / h
    assert worst <= 1e-8 * max(1.0, float(np.abs(g).max())), worst
    # KL itself, written out
    Pn = P.numpy()
    d = ((Y[:, None] - Y[None]) ** 2).sum(-1)
    q = 1.0 / (1.0 + d)
    np.fill_diagonal(q, 0.0)
    Q = q / q.sum()
    m = Pn > 0
    assert E.kl_host(P, Y, plogp) == pytest.approx(float((Pn[m] * np.log(Pn[m] / Q[m])).sum()),
                                                   rel=1e-12)


def test_one_update_follows_the_gain_velocity_and_recentring_rules():
    N = 30
    x = uniform(N, 4, 3)
    P, _, plogp = E.affinities_host(x, 5.0)
    rng = np.random.default_rng(4)
    Y, vel = rng.standard_normal((N, 2)), 0.1 * rng.standard_normal((N, 2))
    gains = rng.uniform(0.01, 2.0, (N, 2))
    gains[0] = 0.011
    s = E.step_host(P, Y, vel, gains, 12.0, 0.5, 100.0, plogp)
    g = s["grad"]
    want_gain = np.maximum(np.where(g * vel < 0, gains + 0.2, gains * 0.8), 0.01)
    assert np.array_equal(s["gains"], want_gain) and s["gains"].min() >= 0.01
    want_vel = 0.5 * vel - 100.0 * want_gain * g
    assert np.allclose(s["velocity"], want_vel, rtol=1e-14, atol=0)
    moved = Y + want_vel
    assert np.allclose(s["Y"], moved - moved.mean(0), rtol=1e-12, atol=1e-15)
    # (each entry's subtraction rounds: a few ulp of the largest |y|)
    assert np.abs(s["Y"].mean(0)).max() <= 8 * np.spacing(np.abs(s["Y"]).max())
    assert s["grad_norm"] == pytest.approx(float(np.sqrt((g ** 2).sum())), rel=1e-14)


def test_duplicates_and_an_outlier_give_finite_beta_and_p():
    x = duplicates_and_outlier(65, 24, 5)
    for perplexity in (21.0, 5.0):      # (5 < the 7 zero-distance neighbours: beta runs up)
        P, beta, plogp = E.affinities_host(x, perplexity)
        assert bool(torch.isfinite(beta).all()) and bool((beta > 0).all())
        assert bool(torch.isfinite(P).all()) and math.isfinite(plogp)
        assert abs(float(P.sum()) - 1.0) <= 1e-12
    H = E.entropy_host(x, E.affinities_host(x, 21.0)[1])
    assert float(np.abs(H - math.log(21.0)).max()) <= 1e-5


def test_initialisations_are_deterministic_and_follow_their_rules():
    a, b = E.init_random(300, 7), E.init_random(300, 7)
    assert a.dtype == torch.float32 and a.shape == (300, 2) and torch.equal(a, b)
    assert not torch.equal(a, E.init_random(300, 8))
    assert torch.equal(E.init_random(100, 7), a[:100])       # (a point's draw is its own)
    big = E.init_random(20000, 0).double()
    assert abs(float(big.mean())) <= 3e-6 and abs(float(big.std()) / 1e-4 - 1.0) <= 0.02
    x = uniform(200, 6, 9) * torch.tensor([5.0, 1.0, 3.0, 1.0, 1.0, 1.0])
    p = E.init_pca(x)
    assert p.dtype == torch.float32 and torch.equal(p, E.init_pca(x))
    assert float(p[:, 0].double().std(unbiased=False)) == pytest.approx(1e-4, rel=1e-5)
    # written out: descending eigenvalues, each axis with its largest-magnitude entry positive
    X = x.double().numpy()
    Xc = X - X.mean(0)
    _, V = np.linalg.eigh(Xc.T @ Xc / 200)
    V = V[:, ::-1][:, :2].copy()
    for k in range(2):
        if V[np.argmax(np.abs(V[:, k])), k] < 0:
            V[:, k] *= -1
    assert V[0, 0] > 0.9                                     # (the column scaled by 5)
    proj = Xc @ V
    assert np.allclose(p.double().numpy(), proj * (1e-4 / proj[:, 0].std()), rtol=1e-6,
                       atol=1e-12)
    assert torch.equal(E.init_pca(uniform(10, 1, 0))[:, 1], torch.zeros(10))


def test_argument_errors():
    x = uniform(50, 4, 0)
    with pytest.raises(ValueError, match=r"perplexity = 17.0, N = 50"):
        E.tsne(x, perplexity=17.0)
    with pytest.raises(ValueError, match="perplexity must be a positive float"):
        E.affinities(x, perplexity=0.0)
    with pytest.raises(ValueError, match=r"F = 257"):
        E.tsne(torch.zeros(1000, 257))
    with pytest.raises(ValueError, match=rf"N = {E.MAX_N + 1}"):
        E.tsne(torch.zeros(E.MAX_N + 1, 1))
    with pytest.raises(ValueError, match="x must be an"):
        E.tsne(torch.zeros(5))
    for name in ("n_iter", "check_every"):
        with pytest.raises(ValueError, match=name):
            E.tsne(x, perplexity=5.0, **{name: 0})
    with pytest.raises(ValueError, match="exaggeration_iter"):
        E.tsne(x, perplexity=5.0, exaggeration_iter=-1)
    with pytest.raises(ValueError, match="learning_rate"):
        E.tsne(x, perplexity=5.0, learning_rate="fast")
    with pytest.raises(ValueError, match="learning_rate"):
        E.tsne(x, perplexity=5.0, learning_rate=0.0)
    with pytest.raises(ValueError, match="early_exaggeration"):
        E.tsne(x, perplexity=5.0, early_exaggeration=0.0)
    with pytest.raises(ValueError, match="init must be"):
        E.tsne(x, perplexity=5.0, init="spectral")
    with pytest.raises(ValueError, match=r"\(50, 2\)"):
        E.tsne(x, perplexity=5.0, init=torch.zeros(49, 2))
    assert (E.MAX_N, E.MAX_F) == (_lib.TSNE_MAX_N, _lib.TSNE_MAX_F) == (32768, 256)


def test_the_library_answers_limits_and_groups_without_a_gpu():
    lib = _lib.load()
    assert lib.scae_tsne_supported(32768, 256) == 1 and lib.scae_tsne_supported(2, 1) == 1
    for N, F in ((32769, 24), (1, 24), (100, 0), (100, 257)):
        assert lib.scae_tsne_supported(N, F) == 0
    assert [lib.scae_tsne_groups(n) for n in (0, 4, 256, 257, 2048, 2049, 4099, 10000, 32768,
                                              32769)] == [0, 1, 1, 2, 8, 3, 5, 10, 32, 0]
    d = _lib.TsneDesc()
    assert lib.scae_tsne_run_f32(d, 0, 1, None) == -1           # an empty descriptor is refused


def test_tsne_on_a_cpu_tensor_is_the_host_run():
    x, y = blobs(120, 8, 4, 0)
    kw = dict(perplexity=10.0, n_iter=120, exaggeration_iter=40, init="random", seed=3,
              check_every=50)
    a, b = E.tsne(x, **kw), E.tsne_host(x, **kw)
    assert torch.equal(a.y, b.y) and torch.equal(a.history, b.history) and a.kl == b.kl
    assert a.y.dtype == torch.float64 and a.n_iter == 120 and a.beta.shape == (120,)
    assert a.history[:, 0].tolist() == [50.0, 100.0, 120.0] and a.kl == float(a.history[-1, 1])
    P, _, plogp = E.affinities_host(x, 10.0)
    assert a.kl == pytest.approx(E.kl_host(P, a.y, plogp), rel=1e-12)
    assert float(a.y.mean(0).abs().max()) <= 1e-12
    # check_every changes the rows that are kept, not the run
    c = E.tsne(x, **dict(kw, check_every=7))
    assert torch.equal(c.y, a.y) and c.history.shape == (18, 3)
    assert purity_1nn(a.y.numpy(), y) >= 0.95
    pca = E.tsne(x, perplexity=10.0, n_iter=20)
    assert pca.history[:, 0].tolist() == [20.0] and bool(torch.isfinite(pca.y).all())
