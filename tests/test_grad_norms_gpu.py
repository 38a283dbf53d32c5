"""Tracked gradient norms on the GPU: scae_segment_norms_f32 entry by entry against an fp64 numpy
reference (every chunk path, every 16-byte phase, sentinels around the segments and the row,
Inf / NaN confined to their segment, the ring's cursor), and TrainStep(track_grad_norm) -- the
three replay forms' rows bit for bit, the trained state bit for bit the untracked step's, the
rows against the step's own flat gradient, the remainder step's row, and the untracked step's
launches unchanged."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.test_optimizers_gpu import batches, small_step, ulp

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
SENTINEL = 1e30


# -- 1. the kernel ----------------------------------------------------------------------------------
def _layout():
    """Segments of every length at which the chunk launch takes another path, with gaps of
    0..3 elements so that the starts cover the four 4-byte phases; the last one ends at n."""
    from torch_scae_amd import _lib
    CH = _lib.NORM_CHUNK
    lengths = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, 3 * CH + 7]
    segs, off = [], 2
    for i, length in enumerate(lengths):
        segs.append((off, length))
        off += length + (i + 1) % 4
    n = segs[-1][0] + segs[-1][1]
    assert {o % 4 for o, _ in segs} == {0, 1, 2, 3}
    return segs, n


_CACHE = {}


def _data():
    """(segments, n, src, acc) -- host fp32 arrays with the sentinel everywhere outside the
    segments -- made once."""
    if "d" not in _CACHE:
        segs, n = _layout()
        rng = np.random.default_rng(0)
        src = np.full(n, SENTINEL, dtype=np.float32)
        acc = np.full(n, SENTINEL, dtype=np.float32)
        for off, length in segs:
            src[off:off + length] = (rng.standard_normal(length) * rng.random(length) ** 3)
            acc[off:off + length] = rng.standard_normal(length) * 0.5
        _CACHE["d"] = (segs, n, src, acc)
    return _CACHE["d"]


def _reference(x, segs, p, scale):
    """fp64: scale * ||x[segment]||_p per segment, then the p-norm of those."""
    scale = float(np.float32(scale))
    vals = []
    for off, length in segs:
        v = np.abs(x[off:off + length].astype(np.float64))
        vals.append(np.sqrt((v * v).sum()) if p == 2 else v.sum() if p == 1 else
                    (np.nan if np.isnan(v).any() else v.max()))
    vals = np.array(vals)
    total = np.sqrt((vals * vals).sum()) if p == 2 else vals.sum() if p == 1 else \
        (np.nan if np.isnan(vals).any() else vals.max())
    return scale * np.append(vals, total)


class Launcher:
    """The device tables of one segment table and a ring with a sentinel tail."""

    def __init__(self, segs, n, capacity=1):
        from torch_scae_amd.data_parallel import norm_chunk_table
        chunks, group_first, seg_first = norm_chunk_table(segs, n)
        self.tables = [torch.tensor(t, dtype=torch.int32).cuda()
                       for t in (chunks, group_first, seg_first)]
        self.n_segs, self.capacity = len(segs), capacity
        self.partials = torch.zeros(len(chunks), dtype=torch.float64, device="cuda")
        self.row = len(segs) + 1
        self.ring = torch.full((capacity * self.row + 7,), -7.0, device="cuda")
        self.cursor = torch.zeros(1, dtype=torch.int64, device="cuda")

    def __call__(self, src, acc, p, scale, cursor=True):
        from torch_scae_amd import _lib
        chunks, group_first, seg_first = self.tables
        _lib.call("scae_segment_norms_f32", P(src.data_ptr()),
                  None if acc is None else P(acc.data_ptr()), src.numel(),
                  P(chunks.data_ptr()), chunks.shape[0], P(group_first.data_ptr()),
                  group_first.numel() - 1, P(seg_first.data_ptr()), self.n_segs,
                  _lib.NORM_INF if math.isinf(p) else int(p), float(scale),
                  P(self.partials.data_ptr()), P(self.ring.data_ptr()),
                  P(self.cursor.data_ptr()) if cursor else None, self.capacity,
                  P(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return self.ring.cpu().numpy()


@pytest.mark.parametrize("p", [1, 2, math.inf])
@pytest.mark.parametrize("with_acc", [False, True])
def test_rows_against_fp64_entry_by_entry(p, with_acc):
    """Each entry and the total within 1 fp32 ulp of fp64 (fp64 accumulation errs by about
    n 2^-53; the one rounding to fp32 can fall either side of a tie against a sum taken in
    another order), for scale 1, 1/4 and 1/3; p = inf with scale 1 exact.  The sentinel
    outside the segments (1e30) would wreck any entry that read it.  The ring's tail is
    untouched and two runs give the same bits."""
    segs, n, src, acc = _data()
    run = Launcher(segs, n)
    d_src = torch.from_numpy(src).cuda()
    d_acc = torch.from_numpy(acc).cuda() if with_acc else None
    x = (acc + src).astype(np.float32) if with_acc else src
    for scale in (1.0, 0.25, 1.0 / 3.0):
        ref = _reference(x, segs, p, scale)
        out = run(d_src, d_acc, p, scale, cursor=False)
        got = out[:run.row].astype(np.float64)
        assert np.isfinite(got).all() and (got[:-1] > 0).all()
        err = np.abs(got - ref) / ulp(ref)
        assert err.max() <= 1.0, (p, with_acc, scale, int(err.argmax()), err.max())
        if math.isinf(p) and scale == 1.0:
            assert (got == ref).all()
        assert (out[run.row:] == -7.0).all()
        again = run(d_src, d_acc, p, scale, cursor=False)
        assert again.tobytes() == out.tobytes()


@pytest.mark.parametrize("p", [1, 2, math.inf])
@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
def test_a_non_finite_value_stays_in_its_segment(p, bad):
    """One Inf (or NaN) planted in one segment -- in src, or in acc for the accumulate form --:
    that entry and the total become inf (nan, for p = inf too, as torch.linalg.vector_norm);
    every other entry keeps its bits."""
    segs, n, src, acc = _data()
    run = Launcher(segs, n)
    d_src, d_acc = torch.from_numpy(src).cuda(), torch.from_numpy(acc).cuda()
    for use_acc in (False, True):
        clean = run(d_src, d_acc if use_acc else None, p, 0.25, cursor=False)[:run.row].copy()
        for s in (0, 7, len(segs) - 1):
            off, length = segs[s]
            dirty = (d_acc if use_acc else d_src).clone()
            dirty[off + length // 2] = bad
            args = (d_src, dirty) if use_acc else (dirty, None)
            got = run(*args, p, 0.25, cursor=False)[:run.row]
            for k in (s, len(segs)):
                assert np.isnan(got[k]) if math.isnan(bad) else np.isposinf(got[k]), (s, k)
            keep = [k for k in range(len(segs)) if k != s]
            assert got[keep].tobytes() == clean[keep].tobytes(), (p, bad, s)


def test_ring_cursor_advances_on_the_device():
    """Three calls into a ring of two rows write rows 0, 1, 0; the cursor counts them; without
    a cursor the call writes row 0 and leaves it alone."""
    segs, n, src, _ = _data()
    run = Launcher(segs, n, capacity=2)
    d_src = torch.from_numpy(src).cuda()
    refs = [_reference(src, segs, 2, sc) for sc in (1.0, 0.25, 1.0 / 3.0)]
    for sc in (1.0, 0.25, 1.0 / 3.0):
        out = run(d_src, None, 2, sc)
    rows = out[:2 * run.row].reshape(2, run.row).astype(np.float64)
    assert int(run.cursor) == 3
    assert (np.abs(rows[0] - refs[2]) <= ulp(refs[2])).all()
    assert (np.abs(rows[1] - refs[1]) <= ulp(refs[1])).all()
    assert (out[2 * run.row:] == -7.0).all()
    out = run(d_src, None, 2, 1.0, cursor=False)
    assert int(run.cursor) == 3
    assert (np.abs(out[:run.row] - refs[0]) <= ulp(refs[0])).all()


# -- 2. the step --------------------------------------------------------------------------------
def _state(step):
    out = [step.flat.flat_param.clone(), step.loss.detach().clone()]
    out += [b.clone() for _, b in step.opt.state_buffers()]
    if step.opt.counts_steps:
        out.append(step.opt.step_state[:2].clone())
    if step.opt.acc is not None:
        out.append(step.opt.acc.clone())
    return out


def _clip():
    """A third of the tiny configuration's first-step gradient norm."""
    if "clip" not in _CACHE:
        _, probe = small_step(noise=False, lr=1e-3, track_grad_norm=2)
        probe(*batches(1)[0])
        _CACHE["clip"] = float(probe.last_grad_norm()) / 3
    return _CACHE["clip"]


def test_replay_forms_write_bit_equal_rows():
    """Eager, graph replay and launch-list replay: the same four rows, bit for bit (the riding
    and the stand-alone column sums give the same gradient; the cursor advances on the device
    under either replay)."""
    data = batches(4)
    hist = []
    for kw in (dict(use_graph=False), dict(replay="graph"), dict(replay="launches")):
        _, step = small_step(noise=False, lr=1e-3, track_grad_norm=2, log_steps=4, **kw)
        for img, lab in data:
            step(img, lab)
        torch.cuda.synchronize()
        if kw.get("replay") == "launches":
            assert step._klist, "the tracked step did not replay as a launch list"
        rows, steps = step.grad_norm_history()
        assert steps == [0, 1, 2, 3] and list(rows) == step.grad_norm_names()
        hist.append(torch.stack([rows[k] for k in rows]))
        assert int(step.grad_norms.cursor) == 4
    assert torch.equal(hist[0], hist[1]) and torch.equal(hist[1], hist[2])
    assert bool((hist[0][-1] > 0).all())


@pytest.mark.parametrize("kind,clipped,k", [("rmsprop", False, 1), ("rmsprop", True, 1),
                                            ("adam", False, 1), ("adam", True, 1),
                                            ("rmsprop", False, 2), ("adam", True, 2)])
def test_tracking_leaves_the_trained_state_bit_equal(kind, clipped, k):
    """Four batches of a tracked step (graph replay) against an untracked one from the same
    seed: loss, parameters and optimiser state bit for bit; one row per optimiser step; with
    clipping and p = 2 the tracked total is the clip's norm to 1 ulp."""
    data = batches(4)
    clip = _clip() if clipped else 0.0
    outs = []
    for track in (None, 2):
        _, step = small_step(noise=False, lr=1e-3, optimizer=kind, gradient_clip_val=clip,
                             accumulate_grad_batches=k, track_grad_norm=track, log_steps=4)
        for i, (img, lab) in enumerate(data):
            step(img, lab)
            if track and clipped and (i + 1) % k == 0:
                a, b = float(step.last_grad_norms()[-1]), float(step.opt.grad_norm)
                assert abs(a - b) <= float(ulp(np.float64(b))) and b > clip, (i, a, b)
        torch.cuda.synchronize()
        outs.append(_state(step))
        if track:
            rows, steps = step.grad_norm_history()
            assert steps == list(range(4 // k)) == list(range(step.optimizer_steps))
            assert int(step.grad_norms.cursor) == 4 // k
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("p", [1, 2, "inf"])
def test_eager_rows_are_the_norms_of_the_flat_gradient(p):
    """An eager tracked step without clipping (the plain optimiser passes read the flat
    gradient and do not write it -- checked here against a copy taken by a second, untracked
    step): every entry within 1 ulp of grad_scale (1) * the fp64 p-norm of its slice of the
    flat gradient, gradient-less parameters absent; parameter_norms() likewise of the
    parameters."""
    data = batches(2)
    model, step = small_step(noise=False, lr=1e-3, use_graph=False, track_grad_norm=p)
    _, plain = small_step(noise=False, lr=1e-3, use_graph=False, optimizer=None)
    pf = float(p)
    for img, lab in data:
        plain.flat.flat_param.copy_(step.flat.flat_param)
        plain(img, lab)
        step(img, lab)
        torch.cuda.synchronize()
        grad = step.flat.flat_grad.cpu().numpy()
        assert grad.tobytes() == plain.flat.flat_grad.cpu().numpy().tobytes()
        segs = [(off, n) for _, off, n in step.grad_norms.segments]
        ref = _reference(grad, segs, pf, 1.0)
        got = step.last_grad_norms().cpu().numpy().astype(np.float64)
        assert (np.abs(got - ref) <= ulp(ref)).all() and got[-1] > 0
    names = step.grad_norm_names()
    assert not any("dummy_vote" in n or "posterior_classifier" in n for n in names)
    live = [n for n, q in model.named_parameters() if q.grad is not None]
    assert sum(n for _, n in segs) == sum(dict(model.named_parameters())[n].numel() for n in live)
    w = step.parameter_norms(pf).cpu().numpy().astype(np.float64)
    ref = _reference(step.flat.flat_param.cpu().numpy(), segs, pf, 1.0)
    assert (np.abs(w - ref) <= ulp(ref)).all()
    if pf == 2.0:
        assert float(step.last_grad_norm()) == got[-1]


def test_a_remainder_batch_writes_the_next_row():
    """Batches of 8, 8, 5: the short one runs on the remainder step and writes row 2 of the
    same ring -- the norms of its own gradient."""
    data = batches(3)
    _, step = small_step(noise=False, lr=1e-3, track_grad_norm=2, log_steps=8)
    for img, lab in data[:2]:
        step(img, lab)
    step(data[2][0][:5], data[2][1][:5])
    torch.cuda.synchronize()
    assert step._rem is not None and step._rem.grad_norms is step.grad_norms
    rows, steps = step.grad_norm_history()
    assert steps == [0, 1, 2] and int(step.grad_norms.cursor) == 3
    segs = [(off, n) for _, off, n in step.grad_norms.segments]
    ref = _reference(step.flat.flat_grad.cpu().numpy(), segs, 2, 1.0)
    got = np.array([float(rows[k][2]) for k in step.grad_norm_names()])
    assert (np.abs(got - ref) <= ulp(ref)).all()
    assert got.tobytes() == step.last_grad_norms().cpu().numpy().astype(np.float64).tobytes()


def test_untracked_step_keeps_its_launches():
    """track_grad_norm=None: the captured step's launches are those of a step built without
    the argument -- same names, same count, none of the new entry points; tracking adds the
    two launches of scae_segment_norms_f32, and (without clipping) one for the column sums
    that otherwise ride in the optimiser pass."""
    from torch_scae_amd import _lib
    img, lab = batches(1)[0]
    seen = {}
    for key, kw in (("bare", {}), ("off", dict(track_grad_norm=None)),
                    ("on", dict(track_grad_norm=2))):
        _, step = small_step(noise=False, lr=1e-3, replay="launches", **kw)
        step(img, lab)
        torch.cuda.synchronize()
        assert step._klist
        seen[key] = ([fn.__name__ for fn, _, _ in step._launches],
                     _lib.load().scae_launch_list_size(step._klist))
    assert seen["off"] == seen["bare"]
    assert not any("segment_norms" in n for n in seen["bare"][0])
    assert seen["on"][0].count("scae_segment_norms_f32") == 1
    print("launches: untracked", seen["bare"][1], "tracked", seen["on"][1])
    assert seen["bare"][1] + 2 <= seen["on"][1] <= seen["bare"][1] + 3
