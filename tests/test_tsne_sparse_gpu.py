"""Sparse t-SNE on the GPU (csrc/tsne_sparse.hip, the wide search of csrc/knn.hip) against the
numpy restatement (embed.*_host): the neighbour lists bit for bit, the affinities from the
device's own lists and beta, one iteration from a chosen state, a hub row, bit reproducibility,
a size past the dense limit, a whole run, and capsule_embedding end to end.

Bars are tests/test_probe_gpu.py's (``bar`` / ``within``): 4 x the largest entry-wise distance
between the host in fp32 and in fp64 on the same input, with a floor of 8 fp32 ulp; both host runs
use the device's own lists (and, for an iteration, the device's own CSR).  Gains are compared as in
tests/test_tsne_gpu.py (``clear_gains``): the entries whose fp64 |g * velocity| lies within twice
the largest fp32-host / fp64-host difference of that product are left out, at most 1 % of them;
the states' seeds (1000 + N) keep the fp32 host under that cap at every case below (checked on the
CPU with the host's own fp32 lists)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_probe_gpu import within
from tests.test_tsne import blobs, duplicates_and_outlier, purity_1nn, uniform
from tests.test_tsne_gpu import KL_MARGIN as DENSE_KL_MARGIN
from tests.test_tsne_gpu import clear_gains, one_iteration_state
from tests.test_tsne_sparse import check_csr
from torch_scae_amd import _lib, neighbors
from torch_scae_amd import embed as E

pytestmark = pytest.mark.gpu

# (N, F, K): both sides of the search's old k limit, the maximum, F above the register form, and
# a size where the search splits the base (scae_knn_groups > 1)
SHAPES = [(5, 1, 3), (66, 3, 64), (67, 24, 65), (130, 24, 128), (257, 255, 90), (4099, 24, 90)]
DUPLICATES = (65, 24, 63)
RING, SPHERE = (300, 2, 9), (300, 64, 9)


def ring_and_centre(N):
    """N - 1 points on a ring of radius 50 and the centre, the last row."""
    a = 2.0 * np.pi * np.arange(N - 1) / (N - 1)
    x = np.concatenate([50.0 * np.stack([np.cos(a), np.sin(a)], 1), np.zeros((1, 2))])
    return torch.from_numpy(x.astype(np.float32))


def sphere_and_centre(N, F):
    """N - 1 random points on a sphere of radius 50 in F dimensions and the centre, the last row:
    two points of the sphere lie about 50 sqrt(2) apart, the centre 50 from each -- it is every
    point's nearest neighbour, and its row of the symmetric CSR holds all N - 1 others."""
    g = np.random.default_rng(7).standard_normal((N - 1, F))
    x = np.concatenate([50.0 * g / np.linalg.norm(g, axis=1, keepdims=True), np.zeros((1, F))])
    return torch.from_numpy(x.astype(np.float32))


def _input(shape):
    N, F, K = shape
    if shape == DUPLICATES:
        return duplicates_and_outlier(N, F, 20 + N)
    if shape == RING:
        return ring_and_centre(N)
    if shape == SPHERE:
        return sphere_and_centre(N, F)
    return uniform(N, F, 20 + N)


@functools.lru_cache(maxsize=None)
def _device(shape):
    """-> (x, the device's lists on the CPU, its Csr / beta / sum P log P (a (1,) tensor))"""
    N, F, K = shape
    x = _input(shape)
    lists = E.neighbor_lists(x.cuda(), K)
    csr, beta, plogp = E._affinities_knn_device(x.cuda(), K / 3.0, K)
    return x, neighbors.KnnResult(lists.idx.cpu(), lists.d2.cpu()), csr, beta, plogp


def _csr_numpy(csr):
    """The device's Csr on the host, and sum P log P of its values in fp64"""
    c = E.Csr(*(a.cpu().numpy() for a in csr))
    pos = c.values[c.values > 0].astype(np.float64)
    return c, float((pos * np.log(pos)).sum())


@pytest.mark.parametrize("shape", SHAPES)
def test_the_devices_lists_are_the_hosts_bit_for_bit(shape):
    N, F, K = shape
    x, lists, _, _, _ = _device(shape)
    assert lists.idx.shape == (N, K) and lists.idx.dtype == torch.int64
    host = E.neighbor_lists_host(x, K)
    assert torch.equal(lists.idx, host.idx) and torch.equal(lists.d2, host.d2)
    if K <= neighbors.MAX_K:
        ref = neighbors.knn_host(x, K)
        assert torch.equal(lists.idx, ref.idx) and torch.equal(lists.d2, ref.d2)
    G = _lib.load().scae_knn_groups(N, N)
    assert (G > 1) == (N == 4099)


@pytest.mark.parametrize("shape", SHAPES + [DUPLICATES])
def test_affinities_from_the_devices_own_lists_and_beta(shape):
    N, F, K = shape
    perplexity, case = K / 3.0, str(shape)
    x, lists, csr, beta, plogp = _device(shape)
    got = E.affinities_knn(x.cuda(), perplexity, K)
    assert all(torch.equal(a, b) for a, b in zip(got[:4], tuple(csr) + (beta,)))
    assert got[4] == float(plogp) and got[2].dtype == torch.float32 and got[0].is_cuda
    b = beta.cpu()
    assert bool(torch.isfinite(b).all()) and bool((b > 0).all())
    c64, H64 = E.conditionals_knn_host(lists.d2, b)
    c32, H32 = E.conditionals_knn_host(lists.d2, b, np.float32)
    slack = 4.0 * float(np.abs(H32.astype(np.float64) - H64).max())
    err = float(np.abs(H64 - math.log(perplexity)).max())
    print(f"{case} entropy: worst |H64(beta) - log perplexity| {err:.3e} (1e-5 + {slack:.3e})")
    assert err <= 1e-5 + slack
    P64, pl64 = E.joint_knn_host(lists.idx, c64)
    P32, pl32 = E.joint_knn_host(lists.idx, c32, np.float32)
    assert torch.equal(csr.indptr.cpu(), torch.from_numpy(P64.indptr))
    assert torch.equal(csr.indices.cpu(), torch.from_numpy(P64.indices))
    within("P", csr.values.cpu().numpy(), P32.values, P64.values, case)
    check_csr(*csr, K)
    within("sum P log P", float(plogp), pl32, pl64, case)


def _one_iteration(shape, scale, it, dense=False):
    N, F, K = shape
    case = f"({shape}, Y ~ {scale}, iteration {it})"
    _, _, csr, _, _ = _device(shape)
    Pn, plogp = _csr_numpy(csr)
    lr = max(N / 12.0 / 4.0, 50.0)
    p = E._SparseProblem(csr, plogp, torch.zeros(N, 2), 1000, 12.0, 250, lr, 1)
    assert p.desc.G == _lib.load().scae_tsne_sparse_groups(N)
    Y, vel, gains = one_iteration_state(N, scale)
    p.load_state(Y, vel, gains)
    p.run(it, 1)
    torch.cuda.synchronize()
    ex, mom = E._schedule(it, 250, 12.0)
    assert ex == (12.0 if scale < 1 else 1.0)
    hosts = [("the host step on the device's CSR", Pn)]
    if dense:       # every pair is stored: the dense restatement on the dense P, another path
        hosts.append(("the dense host step", E.densify(*Pn)))
    for name, P in hosts:
        h64 = E.step_host(P, Y, vel, gains, ex, mom, np.float32(lr), plogp)
        h32 = E.step_host(P, Y, vel, gains, ex, mom, np.float32(lr), plogp, dtype=np.float32)
        tag = f"{case} {name}:"
        within("Y", p.Y.cpu().numpy(), h32["Y"], h64["Y"], tag)
        within("velocity", p.velocity.cpu().numpy(), h32["velocity"], h64["velocity"], tag)
        hist = p.history.cpu().numpy()
        assert hist[it - 1, 0] == it and not hist[:it - 1].any() and not hist[it:].any()
        within("KL", hist[it - 1, 1], h32["kl"], h64["kl"], tag)
        within("|g|", hist[it - 1, 2], h32["grad_norm"], h64["grad_norm"], tag)
        clear = clear_gains(h32, h64)                  # (asserts the 1 % cap)
        print(f"{tag} gains: {int((~clear).sum())} of {clear.size} entries under the threshold")
        within("gains", p.gains.cpu().numpy()[clear], h32["gains"][clear], h64["gains"][clear],
               tag)


@pytest.mark.parametrize("scale, it", [(1e-4, 3), (5.0, 300)])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_iteration_from_a_chosen_state(shape, scale, it):
    _one_iteration(shape, scale, it)


@pytest.mark.parametrize("scale, it", [(1e-4, 3), (5.0, 300)])
def test_one_iteration_with_every_pair_stored_is_the_dense_step(scale, it):
    _one_iteration((66, 3, 65), scale, it, dense=True)


def test_one_update_kernel_two_strides():
    """The dense and the sparse path run one update kernel over ``block`` rows 128 and 1024
    apart.  N = 300 (two update workgroups), every pair stored with P = 2^-17, Y on (0, 0) and
    (1, 0): d is 0 or 1, q 1 or 1/2, every term of every sum a multiple of a power of two, so both
    paths leave the same ``rows`` whatever their order of summation (checked), and the partials
    of y0, y1 and |g|^2 -- from random velocities and gains -- must agree bit for bit, segment k
    of one at k x its stride with segment k of the other."""
    N, nb, lr = 300, 2, 50.0
    rng = np.random.default_rng(5)
    Y = np.stack([rng.integers(0, 2, N), np.zeros(N)], 1).astype(np.float32)
    vel = (0.1 * rng.standard_normal((N, 2))).astype(np.float32)
    gains = rng.uniform(0.01, 2.0, (N, 2)).astype(np.float32)
    P = torch.full((N, N), 2.0 ** -17).fill_diagonal_(0.0).cuda()
    off = ~torch.eye(N, dtype=torch.bool)
    csr = E.Csr(torch.arange(N + 1, dtype=torch.int64).cuda() * (N - 1),
                torch.arange(N).repeat(N, 1)[off].cuda(), P.cpu()[off].cuda())
    dense = E._TsneProblem(P, 0.0, torch.zeros(N, 2), 1000, 12.0, 250, lr, 1)
    sparse = E._SparseProblem(csr, 0.0, torch.zeros(N, 2), 1000, 12.0, 250, lr, 1)
    for p in (dense, sparse):
        p.load_state(Y, vel, gains)
        p.run(3, 1)
    torch.cuda.synchronize()
    assert torch.equal(dense.rows[:5 * N], sparse.rows[:5 * N]) and bool(dense.rows[:N].any())
    sd, ss = _lib.TSNE_BLOCK_DOUBLES // 5, _lib.TSNE_SPARSE_BLOCK_DOUBLES // 5
    assert (sd, ss) == (128, 1024)
    for k, name in ((0, "Z"), (2, "y0"), (3, "y1"), (4, "|g|^2")):
        a, b = dense.block[k * sd:k * sd + nb], sparse.block[k * ss:k * ss + nb]
        print(f"{name}: dense {a.tolist()}, sparse {b.tolist()}")
        assert torch.equal(a, b) and bool((a != 0).all()), name
        assert not bool(dense.block[k * sd + nb:(k + 1) * sd].any())
        assert not bool(sparse.block[k * ss + nb:(k + 1) * ss].any())
    assert torch.equal(dense.Y, sparse.Y) and torch.equal(dense.gains, sparse.gains)


@pytest.mark.parametrize("shape", [RING, SPHERE])
def test_a_hub_row(shape):
    """A ring in the plane, and a sphere in 64 dimensions.  In the plane a ring point
    has a third of the ring nearer than the centre, so nobody lists the centre and its row keeps
    its own 9 entries; on the sphere the centre is everybody's nearest neighbour and its row
    holds all N - 1 others: the attraction kernel's long row."""
    N, F, K = shape
    _, _, csr, _, plogp = _device(shape)
    check_csr(*csr, K)
    hub = int(csr.indptr[N]) - int(csr.indptr[N - 1])
    print(f"{shape}: the centre's row has {hub} entries")
    assert hub == (N - 1 if shape == SPHERE else K)
    assert abs(float(csr.values.double().sum()) - 1.0) <= 1e-5
    for scale, it in ((1e-4, 3), (5.0, 300)):
        _one_iteration(shape, scale, it)


def _same(a, b):
    return torch.equal(a.y, b.y) and torch.equal(a.history, b.history) and a.kl == b.kl and \
        torch.equal(a.beta, b.beta)


@pytest.mark.parametrize("N", [257, 4099])
def test_bits_repeat_across_runs_and_check_every(N):
    x = uniform(N, 24, 3).cuda()
    kw = dict(n_iter=60, exaggeration_iter=20, neighbors="auto")
    a = E.tsne(x, check_every=50, **kw)
    assert a.y.is_cuda and a.y.shape == (N, 2) and bool(torch.isfinite(a.y).all())
    assert a.history.shape == (2, 3) and a.history[:, 0].tolist() == [50.0, 60.0]
    assert a.kl == float(a.history[1, 1])
    assert _same(a, E.tsne(x, check_every=50, **kw))
    seven = E.tsne(x, check_every=7, **kw)
    assert torch.equal(seven.y, a.y) and seven.history.shape == (9, 3)
    assert torch.equal(seven.history[-1], a.history[-1]) and seven.kl == a.kl
    assert float(a.y.double().mean(0).abs().max()) <= 1e-6 * float(a.y.abs().max())
    assert _same(a, E.tsne(x, check_every=50, n_iter=60, exaggeration_iter=20, neighbors=90))


def test_past_the_dense_limit():
    N, K, S = E.MAX_N + 65, 15, 64
    x = uniform(N, 2, 11)
    xc = x.cuda()
    with pytest.raises(ValueError, match=rf"N = {N}, F = 2: t-SNE takes N <= {E.MAX_N}"):
        E.tsne(xc, perplexity=5.0, n_iter=2, check_every=1)
    kw = dict(perplexity=5.0, n_iter=2, check_every=1)
    res = E.tsne(xc, neighbors=K, **kw)
    assert res.y.shape == (N, 2) and bool(torch.isfinite(res.y).all())
    assert res.history[:, 0].tolist() == [1.0, 2.0] and math.isfinite(res.kl)
    assert float(res.y.double().mean(0).abs().max()) <= 1e-6 * float(res.y.abs().max())
    # the lists of sampled rows against the float32 rule computed for those rows alone
    rows = np.sort(np.random.default_rng(5).choice(N, S, replace=False))
    rows[0], rows[-1] = 0, N - 1
    lists = E.neighbor_lists(xc, K)
    X = x.numpy()
    d = np.zeros((S, N), dtype=np.float32)
    for f in range(2):
        u = X[rows, None, f] - X[None, :, f]
        d += u * u
    d[np.arange(S), rows] = np.inf
    idx, d2 = neighbors._least(d, K)
    assert np.array_equal(lists.idx[rows].cpu().numpy(), idx)
    assert np.array_equal(lists.d2[rows].cpu().numpy(), d2)
    # the whole CSR, on the device
    csr, beta, plogp = E._affinities_knn_device(xc, 5.0, K)
    assert torch.equal(beta, res.beta)
    counts = csr.indptr[1:] - csr.indptr[:-1]
    assert int(csr.indptr[0]) == 0 and int(csr.indptr[-1]) == csr.indices.numel()
    assert int(counts.min()) >= K
    r = torch.arange(N, device="cuda").repeat_interleave(counts)
    keys, mirrored = r * N + csr.indices, csr.indices * N + r
    assert bool((keys[1:] > keys[:-1]).all()) and not bool((r == csr.indices).any())
    order = torch.sort(mirrored, stable=True).indices
    assert torch.equal(mirrored[order], keys) and torch.equal(csr.values[order], csr.values)
    assert abs(float(csr.values.double().sum()) - 1.0) <= 1e-5
    # the same run through the problem object: the same bits, and the rows' sums of the result
    p = E._SparseProblem(csr, plogp, E._init(x, "pca", 0), 2, 12.0, 250,
                         max(N / 12.0 / 4.0, 50.0), 1)
    p.run(0, 2)
    assert torch.equal(p.Y, res.y) and torch.equal(p.history.cpu(), res.history)
    got = p.rows.reshape(6, N)[:, torch.from_numpy(rows).cuda()].cpu().numpy()
    Pn, _ = _csr_numpy(csr)
    Yn = res.y.cpu().numpy()
    at = np.concatenate([np.arange(Pn.indptr[i], Pn.indptr[i + 1]) for i in rows])
    sub = E.Csr(np.concatenate([[0], np.cumsum(np.diff(Pn.indptr)[rows])]), Pn.indices[at],
                Pn.values[at])
    # (edge_sums_host pairs row i of the Csr with Y[i]: the sampled rows first, then all of Y)
    Ys = np.concatenate([Yn[rows], Yn])
    sub = sub._replace(indices=sub.indices + S)
    e = {t: E.edge_sums_host(sub, Ys, t) for t in (np.float32, np.float64)}
    s = {t: E.pair_sums_host(Yn, t, rows) for t in (np.float32, np.float64)}
    within("attraction", got[:2].T, e[np.float32]["att"], e[np.float64]["att"])
    within("P log1p(d)", got[5], e[np.float32]["kl"], e[np.float64]["kl"])
    within("repulsion", got[2:4].T, s[np.float32]["rep"], s[np.float64]["rep"])
    within("Z", got[4], s[np.float32]["z"], s[np.float64]["z"])


# The whole run's KL margin, measured as the dense test's was: twice the worst relative
# |KL32 - KL64| / KL64 of tsne_host(neighbors="auto") in fp32 and in fp64 on seeds 0 - 4 of this
# input (data seed = init seed = s): MEASURED_REL below.
MEASURED_REL = (4.03e-3, 2.51e-3, 6.63e-3, 1.13e-3, 1.46e-4)        # -> KL_MARGIN = 0.0133
KL_MARGIN = 2.0 * max(MEASURED_REL)
WHOLE = dict(perplexity=30.0, n_iter=300, exaggeration_iter=100, init="random", seed=0,
             neighbors="auto")


def test_a_whole_run_against_the_host():
    x, y = blobs(400, 24, 10, 0)
    host = E.tsne_host(x, **WHOLE)
    got = E.tsne(x.cuda(), **WHOLE)
    assert got.n_iter == 300 and got.history.shape == (6, 3)
    assert got.history[:, 0].tolist() == [50.0, 100.0, 150.0, 200.0, 250.0, 300.0]
    # the reported KL is the KL of the returned Y under the device's CSR
    csr, _, plogp = E._affinities_knn_device(x.cuda(), 30.0, 90)
    Pn, pl = _csr_numpy(csr)
    Yn = got.y.cpu().numpy()
    within("reported KL", got.kl, E.kl_host(Pn, Yn, pl, np.float32), E.kl_host(Pn, Yn, pl))
    within("sum P log P", float(plogp), pl, pl)
    pd, ph = purity_1nn(Yn, y), purity_1nn(host.y.numpy(), y)
    print(f"1-NN purity: device {pd:.4f}, fp64 host {ph:.4f}; KL: device {got.kl:.6f}, fp64 "
          f"host {host.kl:.6f} (margin {KL_MARGIN:.4f}; the dense test's {DENSE_KL_MARGIN:.4f})")
    assert pd == 1.0
    assert got.kl <= host.kl * (1.0 + KL_MARGIN)


def test_capsule_embedding_forwards_neighbors():
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
    kw = dict(perplexity=20.0, n_iter=40, exaggeration_iter=15, check_every=20, neighbors="auto")
    torch.manual_seed(5)
    ops.reset_noise()
    out = E.capsule_embedding(step, split, trustworthiness_k=12, **kw)
    assert out["y"].shape == (260, 2) and bool(torch.isfinite(out["y"]).all())
    assert torch.equal(out["label"], split[1]) and out["history"].shape == (2, 3)
    assert 0.0 < out["trustworthiness"] <= 1.0
    torch.manual_seed(5)
    ops.reset_noise()
    x = cluster.features(step.encode(*split), "prior")
    res = E.tsne(x, **kw)
    assert torch.equal(out["y"], res.y) and out["kl"] == res.kl
    assert torch.equal(out["history"], res.history)
    assert out["trustworthiness"] == neighbors.trustworthiness(x, res.y, 12)
    dense = E.tsne(x, **{**kw, "neighbors": None})
    assert not torch.equal(dense.y, res.y)          # (the argument reached tsne)
