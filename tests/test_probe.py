"""Host side of the linear probe (torch_scae_amd/probe.py): the fp64 numpy restatement against
torch's cross_entropy and its autograd gradient, the optimum recomputed independently, constant
columns, absent classes, one row, duplicates, separable data, argument checks, and
linear_probe_accuracy on a stub EvalStep."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from torch_scae_amd import probe as P


def synthetic(N, F, C, seed, constant=None):
    """Class prototypes rng.random((C, F)) < 0.3; x = clip(proto[y] * U + 0.15 * U', 0, 1)."""
    rng = np.random.default_rng(seed)
    proto = (rng.random((C, F)) < 0.3).astype(np.float64)
    y = rng.integers(0, C, N)
    x = np.clip(proto[y] * rng.random((N, F)) + 0.15 * rng.random((N, F)), 0, 1)
    x = x.astype(np.float32)
    if constant is not None:
        x[:, constant] = 0.25
    return torch.from_numpy(x), torch.from_numpy(y.astype(np.int64))


@pytest.fixture(scope="module")
def fitted():
    x, y = synthetic(6000, 24, 10, 0, constant=5)
    return x, y, P.fit_host(x, y, 10, l2=1e-3, max_iter=2000, tol=1e-5)


def _standardised(x):
    G = P.moments_host(x)
    mean, scale = P.standardisation(G)
    return G, mean, scale, P.standardise(x, mean, scale)


def _torch_objective(Z, y, V, l2):
    Vt = torch.tensor(V, requires_grad=True)
    J = torch.nn.functional.cross_entropy(torch.from_numpy(Z) @ Vt.T, y) + \
        0.5 * l2 * (Vt[:, :-1] ** 2).sum()
    J.backward()
    return float(J.detach()), Vt.grad.numpy()


def test_objective_and_gradient_match_torch_cross_entropy_in_fp64():
    x, y = synthetic(500, 7, 4, 1, constant=2)
    _, _, _, Z = _standardised(x)
    assert Z.dtype == np.float64 and np.array_equal(Z[:, -1], np.ones(500))
    rng = np.random.default_rng(2)
    for l2 in (0.0, 1e-3, 0.5):
        V = rng.standard_normal((4, 8))
        J, g = P.objective_host(Z, y.numpy(), V, l2)
        Jt, gt = _torch_objective(Z, y, V, l2)
        assert abs(J - Jt) <= 1e-12 * abs(Jt)
        assert np.abs(g - gt).max() <= 1e-12 * np.abs(gt).max()


def test_moments_standardisation_and_step_size():
    x, _ = synthetic(300, 6, 3, 3, constant=4)
    G, mean, scale, Z = _standardised(x)
    X = x.double().numpy()
    assert G.shape == (7, 7) and G[6, 6] == 300
    assert np.allclose(mean, X.mean(0), rtol=1e-13, atol=0)
    live = np.arange(6) != 4
    assert scale[4] == 0.0 and np.allclose(scale[live], 1 / X.std(0)[live], rtol=1e-10)
    assert np.all(Z[:, 4] == 0.0)
    # the algebraic Z^T Z against the product itself
    lam = np.linalg.eigvalsh(Z.T @ Z / 300)[-1]
    assert abs(P.lipschitz(G, mean, scale, 0.25) - (0.5 * lam + 0.25)) <= 1e-10 * lam


def test_converged_fit_is_a_stationary_point_in_raw_coordinates(fitted):
    x, y, res = fitted
    assert res.converged and res.n_iter < 500 and res.grad_norm <= 1e-5
    assert res.history.shape == (res.n_iter, 3) and res.history.dtype == torch.float64
    assert float(res.history[-1, 1]) == res.grad_norm
    assert res.weight.shape == (10, 24) and res.bias.shape == (10,)
    # J starts at log C (V = 0) and ends below it
    assert float(res.history[-1, 0]) < float(res.history[0, 0]) == pytest.approx(np.log(10))
    # the gradient at the result, recomputed by torch on the standardised features
    G, mean, scale, Z = _standardised(x)
    W = np.zeros((10, 25))
    live = scale > 0
    W[:, :24][:, live] = res.weight.numpy()[:, live] / scale[live]
    W[:, 24] = res.bias.numpy() + res.weight.numpy() @ mean
    _, g = _torch_objective(Z, y, W, 1e-3)
    assert np.abs(g).max() <= 1e-5
    # raw-coordinate weight / bias reproduce the standardised logits
    raw = x.double().numpy() @ res.weight.numpy().T + res.bias.numpy()
    assert np.abs(raw - Z @ W.T).max() <= 1e-10
    # loss: the mean cross-entropy of the result, without the penalty
    ce = float(torch.nn.functional.cross_entropy(torch.from_numpy(raw), y))
    assert abs(res.loss - ce) <= 1e-12
    assert abs(P.mean_cross_entropy(x, y, res) - ce) <= 1e-12
    # the constant column: weight exactly 0, nothing NaN
    assert torch.all(res.weight[:, 5] == 0.0)
    assert torch.isfinite(res.weight).all() and torch.isfinite(res.bias).all()
    lab, logp = P.predict(x, res)
    assert lab.dtype == torch.int64 and torch.equal(lab, torch.from_numpy(raw).argmax(1))
    want = torch.log_softmax(torch.from_numpy(raw), 1).max(1).values
    assert float((logp - want).abs().max()) <= 1e-12
    assert float((lab == y).double().mean()) > 0.9


def test_fp32_host_arithmetic_ends_close_to_fp64(fitted):
    x, y, res = fitted
    r32 = P.fit_host(x, y, 10, l2=1e-3, max_iter=2000, tol=1e-5, dtype=np.float32)
    assert r32.converged
    gap = float((r32.weight - res.weight).abs().max())
    assert gap <= 1e-3 * float(res.weight.abs().max()), gap
    assert torch.all(r32.weight[:, 5] == 0.0)


def test_cpu_tensors_take_the_host_path(fitted):
    x, y, res = fitted
    again = P.fit(x[:400], y[:400], 10, l2=1e-2, max_iter=50)
    want = P.fit_host(x[:400], y[:400], 10, l2=1e-2, max_iter=50)
    assert torch.equal(again.weight, want.weight) and torch.equal(again.bias, want.bias)
    assert again.n_iter == want.n_iter == 50 and not again.converged
    assert again.weight.dtype == torch.float64
    both = P.fit(x[:400], y[:400], 10, l2=[1e-2, 1.0], max_iter=50)
    assert isinstance(both, list) and [r.l2 for r in both] == [1e-2, 1.0]
    assert torch.equal(both[0].weight, want.weight)
    assert float(both[1].weight.abs().max()) < float(both[0].weight.abs().max())


def test_absent_class_one_row_and_duplicate_rows():
    x, y = synthetic(200, 5, 4, 4)
    y = torch.where(y == 2, torch.zeros_like(y), y)          # class 2 never occurs
    res = P.fit_host(x, y, 4, l2=1e-2, max_iter=3000)
    assert res.converged and torch.isfinite(res.weight).all()
    lab, _ = P.predict(x, res)
    assert not bool((lab == 2).any())
    # N = 1: every column is constant, only the bias moves
    one = P.fit_host(x[:1], y[:1], 4, l2=1e-2, max_iter=20)
    assert torch.all(one.weight == 0.0) and torch.isfinite(one.bias).all()
    assert int(one.bias.argmax()) == int(y[0]) and one.n_iter == 20
    assert P.predict(x[:1], one)[0].tolist() == [int(y[0])]
    # duplicates: every row twice is the same problem
    a = P.fit_host(x, y, 4, l2=1e-2, max_iter=100)
    b = P.fit_host(torch.cat([x, x]), torch.cat([y, y]), 4, l2=1e-2, max_iter=100)
    assert a.n_iter == b.n_iter == 100
    assert float((a.weight - b.weight).abs().max()) <= 1e-9
    assert abs(a.loss - b.loss) <= 1e-12 and torch.equal(a.history[:, 2], b.history[:, 2])


def test_separable_data_without_a_penalty_stops_at_max_iter():
    x = torch.tensor([[0.0, 1.0], [0.1, 0.9], [1.0, 0.0], [0.9, 0.2]])
    y = torch.tensor([0, 0, 1, 1])
    res = P.fit_host(x, y, 2, l2=0.0, max_iter=200, tol=1e-12)
    assert not res.converged and res.n_iter == 200
    assert torch.isfinite(res.weight).all() and torch.isfinite(res.bias).all()
    assert np.isfinite(res.loss) and res.loss < 0.1
    assert P.predict(x, res)[0].tolist() == [0, 0, 1, 1]


def test_ties_go_to_the_lowest_class():
    res = P.ProbeResult(torch.tensor([[1.0, 0.0], [2.0, -1.0], [2.0, -1.0]]),
                        torch.tensor([0.0, 0.5, 0.5]), 0.0, 0, False, 0.0, 0.0,
                        torch.zeros(0, 3))
    lab, logp = P.predict(torch.tensor([[3.0, 1.0], [-3.0, 0.0]]), res)
    assert lab.tolist() == [1, 0]
    assert float(logp[0]) == pytest.approx(5.5 - np.log(np.exp(3.0) + 2 * np.exp(5.5)))


@pytest.mark.parametrize("call, message", [
    (lambda x, y: P.fit(x[0], y, 3), "x must be an (N, F) tensor"),
    (lambda x, y: P.fit(torch.zeros(0, 4), y[:0], 3), "x must be an (N, F) tensor"),
    (lambda x, y: P.fit(x, y[:5], 3), "y must be an (N,)"),
    (lambda x, y: P.fit(x, y.float(), 3), "y must be an (N,)"),
    (lambda x, y: P.fit(x, y, 0), "n_classes must be a positive int"),
    (lambda x, y: P.fit(x, y, 257), "the probe takes"),
    (lambda x, y: P.fit(torch.zeros(10, 257), y, 3), "the probe takes"),
    (lambda x, y: P.fit(torch.zeros(10, 255), y, 65), "the probe takes"),     # C (F + 1) > 16384
    (lambda x, y: P.fit(x, y, 3, l2=[1e-3] * 17), "at most 16 l2 values"),
    (lambda x, y: P.fit(x, y, 3, l2=[]), "non-empty sequence"),
    (lambda x, y: P.fit(x, y, 3, l2=-1e-3), "l2 must be finite and >= 0"),
    (lambda x, y: P.fit(x, y, 3, l2=[1e-3, float("nan")]), "l2 must be finite and >= 0"),
    (lambda x, y: P.fit(x, y, 3, max_iter=0), "max_iter must be a positive int"),
    (lambda x, y: P.fit(x, y, 3, tol=-1.0), "tol must be a float >= 0"),
    (lambda x, y: P.fit(x, y, 3, l2=[1e-3, 1e-2], tol=[1e-5]), "tol must be a float >= 0"),
    (lambda x, y: P.fit(x, y, 2), "4 labels outside [0, 2)"),
    (lambda x, y: P.fit(x, y - 1, 3), "3 labels outside [0, 3)"),
    (lambda x, y: P.predict(x, P.ProbeResult(torch.zeros(3, 5), torch.zeros(3), 0.0, 0, False,
                                             0.0, 0.0, None)), "result must hold weight"),
    (lambda x, y: P.mean_cross_entropy(x, y, P.ProbeResult(
        torch.zeros(2, 4), torch.zeros(2), 0.0, 0, False, 0.0, 0.0, None)),
     "4 labels outside [0, 2)"),
])
def test_arguments_are_checked(call, message):
    x = torch.rand(10, 4, generator=torch.Generator().manual_seed(0))
    y = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2, 2])
    with pytest.raises(ValueError) as e:
        call(x, y)
    assert message in str(e.value)


def test_probe_entry_points_reject_bad_arguments_without_a_gpu():
    from torch_scae_amd import _lib
    lib = _lib.load()
    assert lib.scae_probe_supported(24, 10, 8) == 1 and lib.scae_probe_supported(255, 64, 16) == 1
    assert lib.scae_probe_supported(255, 65, 1) == 0 and lib.scae_probe_supported(257, 2, 1) == 0
    assert lib.scae_probe_supported(24, 10, 17) == 0
    # whole 64-row tiles, a function of (N, F) alone
    assert lib.scae_probe_groups(1, 24) == 1 and lib.scae_probe_groups(64, 24) == 1
    assert lib.scae_probe_groups(65, 24) == 2 and lib.scae_probe_groups(4099, 255) == 33
    assert lib.scae_probe_groups(60000, 24) == 235 and lib.scae_probe_groups(60000, 255) == 63
    assert lib.scae_probe_groups(0, 24) == 0 and lib.scae_probe_groups(10, 257) == 0
    assert lib.scae_probe_predict_blocks(1) == 1 and lib.scae_probe_predict_blocks(10 ** 7) == 1024
    assert lib.scae_probe_fit_f32(None, 1, None) == -1
    assert lib.scae_probe_moments_f64(None, None, 10, 4, 2, None, None, None, None) == -1
    assert lib.scae_probe_predict_f32(None, 10, 4, 2, None, None, None, None, None, None, None,
                                      None) == -1
    d = _lib.ProbeDesc()
    assert lib.scae_probe_fit_f32(d, 1, None) == -1


class StubStep:
    """The surface linear_probe_accuracy reads of an EvalStep: ``encode`` returns fixed
    features for a split (here the images ARE the features), ``model.n_classes``."""

    def __init__(self, n_classes):
        self.model = SimpleNamespace(n_classes=n_classes)
        self.encoded = 0

    def encode(self, images, labels=None):
        self.encoded += 1
        return {"prior": images, "posterior": images * 2, "label": labels,
                "features": torch.stack([images, images * 2], 1)}


def test_linear_probe_accuracy_on_a_stub_step():
    x, y = synthetic(900, 8, 3, 7)
    fit, val, test = (x[:500], y[:500]), (x[500:700], y[500:700]), (x[700:], y[700:])
    step = StubStep(3)
    out = P.linear_probe_accuracy(step, fit, test, l2=1e-2, max_iter=300)
    assert set(out) == {"fit_accuracy", "test_accuracy", "loss", "l2", "n_iter", "converged",
                        "confusion", "result"}
    assert step.encoded == 2
    res = P.fit_host(*fit, 3, l2=1e-2, max_iter=300)
    assert torch.equal(out["result"].weight, res.weight) and out["loss"] == res.loss
    assert out["l2"] == 1e-2 and out["n_iter"] == res.n_iter and out["converged"] == res.converged
    lab = P.predict(test[0], res)[0]
    assert out["test_accuracy"] == float((lab == test[1]).double().mean())
    assert out["fit_accuracy"] == float((P.predict(fit[0], res)[0] == fit[1]).double().mean())
    conf = out["confusion"]
    assert conf.shape == (3, 3) and conf.sum() == 200
    assert conf[1, 2] == int(((lab == 1) & (test[1] == 2)).sum())      # (predicted, label)
    # names: several splits, default and given; no other split: no table
    out = P.linear_probe_accuracy(step, fit, val, test, l2=1e-2, max_iter=50)
    assert {"split1_accuracy", "split2_accuracy"} <= set(out) and out["confusion"].sum() == 200
    out = P.linear_probe_accuracy(step, fit, val, test, names=["val", "test"], l2=1e-2,
                                  max_iter=50, feature="both")
    assert {"val_accuracy", "test_accuracy"} <= set(out)
    assert out["result"].weight.shape == (3, 16)
    assert P.linear_probe_accuracy(step, fit, l2=1e-2, max_iter=50)["confusion"] is None
    with pytest.raises(ValueError, match="one name per split"):
        P.linear_probe_accuracy(step, fit, val, names=["a", "b"])
    with pytest.raises(ValueError, match="select"):
        P.linear_probe_accuracy(step, fit, val, l2=[1e-3, 1e-2])
    with pytest.raises(ValueError, match="feature must be"):
        P.linear_probe_accuracy(step, fit, feature="mass")


def test_select_chooses_the_l2_and_ties_go_to_the_largest():
    x, y = synthetic(900, 8, 3, 7)
    fit, val, test = (x[:500], y[:500]), (x[500:700], y[500:700]), (x[700:], y[700:])
    step = StubStep(3)
    l2s = [1e-4, 1e-2, 30.0]
    out = P.linear_probe_accuracy(step, fit, test, l2=l2s, select=val, max_iter=300)
    assert step.encoded == 3
    results = P.fit_host(*fit, 3, l2=l2s, max_iter=300)
    accs = [float((P.predict(val[0], r)[0] == val[1]).double().mean()) for r in results]
    assert accs[2] < max(accs)                   # (the heavy penalty loses: a real choice)
    best = max(range(3), key=lambda i: (accs[i], l2s[i]))
    assert out["l2"] == l2s[best] and torch.equal(out["result"].weight, results[best].weight)
    # select may be a split already given: it is encoded once
    step = StubStep(3)
    P.linear_probe_accuracy(step, fit, test, l2=l2s, select=test, max_iter=20)
    assert step.encoded == 2
    # a tie: the same l2 twice next to a smaller one that fits the same rows
    sep_x = torch.tensor([[0.0, 1.0], [0.1, 0.9], [1.0, 0.0], [0.9, 0.2]] * 5)
    sep_y = torch.tensor([0, 0, 1, 1] * 5)
    out = P.linear_probe_accuracy(StubStep(2), (sep_x, sep_y), l2=[1e-3, 1e-1, 1e-2],
                                  select=(sep_x, sep_y), max_iter=100)
    assert out["fit_accuracy"] == 1.0 and out["l2"] == 1e-1
