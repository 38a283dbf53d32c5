"""Clipping by global norm on the GPU: the norm launch (scae_grad_sq_partials_f32 and its form
with the step's last column sums riding in it) against fp64, the clip forms of the optimiser
passes against the plain passes on a pre-scaled gradient (and bit for bit them when the clip is
far above the norm), and TrainStep(gradient_clip_val) -- against the oracle stepped by
clip_grad_norm_ and torch.optim, against its own gradients at cfg-2's size, in every replay
form and collective mode, and on an epoch's short step."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import scae_oracle as O
from tests.test_optimizers_gpu import BETAS, KIND, batches, small_step, ulp
from tests.test_train_remainder_gpu import CFG2, SMALL, _close, _dataset, _mirror

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p


def stream():
    return P(torch.cuda.current_stream().cuda_stream)


def norm_launch(g, n, phase=0, jobs=None, n_jobs=0):
    """-> (partials, count) of the norm launch over g[phase:phase + n]."""
    from torch_scae_amd import _lib
    part = torch.full((_lib.GRAD_SQ_MAX_PARTIALS,), float("nan"), dtype=torch.float64,
                      device="cuda")
    cnt = ctypes.c_int(0)
    ptr = P(g.data_ptr() + 4 * phase)
    if jobs is None:
        _lib.call("scae_grad_sq_partials_f32", ptr, n, P(part.data_ptr()), part.numel(),
                  ctypes.byref(cnt), stream())
    else:
        _lib.call("scae_grad_sq_partials_sums_f32", ptr, n, P(part.data_ptr()), part.numel(),
                  ctypes.byref(cnt), jobs, n_jobs, stream())
    torch.cuda.synchronize()
    return part, cnt.value


# -- 1. the norm launch --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 257, 1023, 4099, 65537, 2414879])
def test_partials_sum_of_squares_against_fp64(n):
    """The partials' sum within 1e-6 relative of the fp64 sum of squares, at each 4-byte phase
    of a 16-byte line (n < 4, n not a multiple of 4, cfg-2's 2 414 879 gradients); every slot
    past the count untouched; two runs give the same bits."""
    gen = torch.Generator().manual_seed(n)
    for phase in range(4):
        g = (torch.randn(n + 8, generator=gen) * torch.rand(n + 8, generator=gen) ** 4).cuda()
        part, cnt = norm_launch(g, n, phase)
        assert 1 <= cnt <= 512
        assert bool(torch.isnan(part[cnt:]).all()) and not bool(torch.isnan(part[:cnt]).any())
        ref = float((g[phase:phase + n].double() ** 2).sum())
        got = float(part[:cnt].sum())
        assert abs(got - ref) <= 1e-6 * ref, (n, phase, got, ref)
        part2, cnt2 = norm_launch(g, n, phase)
        assert cnt2 == cnt and torch.equal(part[:cnt], part2[:cnt])


def _jobs(grad):
    """the column-sum job table of test_optimizers_gpu.py's riding-forms test, destinations
    in `grad` (20011 floats) -- one of them a transposed window, one periodic"""
    from torch_scae_amd import _lib
    g = torch.Generator().manual_seed(11)
    partials = [torch.randn(22, 9 * 40, generator=g).cuda(),
                torch.randn(128, 5 * 12, generator=g).cuda(),
                torch.randn(7, 333, generator=g).cuda(),
                torch.randn(300, 6, generator=g).cuda()]
    layout = [(1, [(0, 360, -40, 360)]),
              (3001, [(0, 5, 12, 50), (5, 12, 12, 70)]),
              (7002, [(0, 100, 0, 100), (120, 333, 0, 213)]),
              (19990, [(0, 6, 0, 6)])]
    keep, jobs = [partials], (_lib.SumJob * len(partials))()
    for job, part, (off, segs) in zip(jobs, partials, layout):
        arr = (_lib.SumSegment * len(segs))()
        pos = off
        for a, (b, e, per, length) in zip(arr, segs):
            a.dst, a.begin, a.end, a.period = grad.data_ptr() + 4 * pos, b, e, per
            pos += length
        keep.append(arr)
        job.src, job.rows, job.cols = part.data_ptr(), part.shape[0], part.shape[1]
        job.segments, job.n_segments = arr, len(segs)
    return jobs, len(partials), keep


def test_riding_sums_equal_sum_rows_and_are_counted():
    """scae_grad_sq_partials_sums_f32: the column sums it writes equal
    scae_sum_rows_multi_f32's bit for bit, and the partials sum to the fp64 sum of squares of
    the whole buffer with them in it (the streaming workgroups skip exactly their ranges:
    stale values left in those slots would be counted otherwise); two runs, same bits."""
    from torch_scae_amd import _lib
    n = 20011
    outs = []
    for fused in (False, True, True):
        grad = torch.randn(n, generator=torch.Generator().manual_seed(5)).cuda()
        jobs, nj, keep = _jobs(grad)
        if fused:
            part, cnt = norm_launch(grad, n, 0, jobs, nj)
            outs.append((grad, part[:cnt].clone()))
        else:
            _lib.call("scae_sum_rows_multi_f32", jobs, nj, stream())
            torch.cuda.synchronize()
            outs.append((grad, None))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[1][0], outs[2][0])
    assert torch.equal(outs[1][1], outs[2][1])
    ref = float((outs[0][0].double() ** 2).sum())
    got = float(outs[1][1].sum())
    assert abs(got - ref) <= 1e-6 * ref, (got, ref)
    # ... and differs from the stale buffer's: the sums ARE in it
    stale = float((torch.randn(n, generator=torch.Generator().manual_seed(5)).double() ** 2).sum())
    assert abs(stale - ref) > 1e-3 * ref


# -- 2. the clip forms of the optimiser passes ---------------------------------------------------
def _opt_launch(kind, la, bufs, n_ranges, clip, st_state, lr_dev, wd, max_norm=None,
                part=None, cnt=0, norm_out=None):
    """One optimiser step over the ranges: the plain pass (clip False) or its clip form."""
    from torch_scae_amd import _lib
    for i, (off, cnt_) in enumerate(n_ranges):
        ptr = lambda k: P(bufs[k].data_ptr() + 4 * off)   # noqa: E731
        tail = (P(part.data_ptr()), cnt, max_norm, P(norm_out.data_ptr()) if i == 0 else None) \
            if clip else ()
        if kind == "rmsprop" and not la:
            _lib.call("scae_rmsprop_clip_step_f32" if clip else "scae_rmsprop_step_f32",
                      ptr("p"), ptr("g"), ptr("v"), ptr("m"), cnt_, 1e-3, P(lr_dev.data_ptr()),
                      0.99, 1e-4, 0.9, wd, 0.5, *tail, stream())
        else:
            _lib.call("scae_flat_opt_clip_step_f32" if clip else "scae_flat_opt_step_f32",
                      ptr("p"), ptr("g"), ptr("m"), ptr("v"), ptr("slow"), cnt_,
                      P(lr_dev.data_ptr()), P(st_state.data_ptr()), KIND[kind], *BETAS[kind],
                      1e-4, wd, 0.5, 5 if la else 0, 0.5, int(i == len(n_ranges) - 1), *tail,
                      stream())


OPT_CASES = [(k, la, wd) for k in ("rmsprop", "adam", "radam") for la in (False, True)
             for wd in (0.0, 1e-2)]


@pytest.mark.parametrize("kind,la,wd", OPT_CASES)
def test_clip_forms_against_the_plain_pass_on_a_prescaled_gradient(kind, la, wd):
    """coef < 1: the clip form within the kernel tests' bars of the plain pass run on the
    gradient pre-scaled in fp64 by the fp64 coefficient (grad_scale 0.5 in both); the norm it
    writes within 1e-6 of the fp64 norm.  max_norm far above the norm: bit for bit the plain
    pass.  With weight decay one launch per range (three ranges with gaps the passes leave
    alone), at a LookAhead sync step (t = 10, slow weights made)."""
    n = 30011
    ranges = [(0, n)] if wd == 0 else [(3, 9000), (9010, 15000), (24020, 5990)]

    def fresh():
        gg = torch.Generator().manual_seed(21)
        b = dict(p=torch.randn(n, generator=gg), g=torch.randn(n, generator=gg),
                 m=torch.randn(n, generator=gg) * .1, v=torch.rand(n, generator=gg),
                 slow=torch.randn(n, generator=gg))
        return {k: x.cuda() for k, x in b.items()}

    def state():
        from torch_scae_amd import _lib
        s = torch.zeros(_lib.FLAT_OPT_STATE_INTS, dtype=torch.int32, device="cuda")
        s[:2] = torch.tensor([9, int(la)], dtype=torch.int32)
        return s
    lr_dev = torch.full((1,), 1e-3, device="cuda")
    g0 = fresh()["g"]
    part, cnt = norm_launch(g0, n)
    norm64 = 0.5 * float((g0.double() ** 2).sum()) ** 0.5
    for max_norm, coef in ((0.3 * norm64, 0.3 * norm64 / (norm64 + 1e-6)), (1e30, 1.0)):
        norm_out = torch.zeros((), device="cuda")
        ours, ref = fresh(), fresh()
        s1, s2 = state(), state()
        _opt_launch(kind, la, ours, ranges, True, s1, lr_dev, wd, max_norm, part, cnt, norm_out)
        if coef < 1:
            ref["g"] = (ref["g"].double() * coef).float()
        _opt_launch(kind, la, ref, ranges, False, s2, lr_dev, wd)
        torch.cuda.synchronize()
        assert abs(float(norm_out) - norm64) <= 1e-6 * norm64
        assert torch.equal(s1, s2)
        if coef == 1.0:
            for k in ours:
                assert torch.equal(ours[k], ref[k]), (k, "coef 1")
            continue
        before = fresh()["p"].double().cpu().numpy()
        r, o = ref["p"].double().cpu().numpy(), ours["p"].double().cpu().numpy()
        upd = np.abs(r - before).max()
        assert upd > 0 and (np.abs(o - r) - ulp(r)).max() <= 1e-5 * upd, kind
        for k in ("m", "v", "slow"):     # (RMSprop's momentum buffer: its tests' 5e-5)
            err = float((ours[k] - ref[k]).abs().max())
            bar = 5e-5 if kind == "rmsprop" and k == "m" else 1e-6
            assert err <= bar * float(ref[k].abs().max()), (k, err)
        keep = torch.zeros(n, dtype=torch.bool, device="cuda")
        for off, c in ranges:
            keep[off:off + c] = True
        for k in ("p", "m", "v"):     # outside the ranges: untouched
            assert torch.equal(ours[k][~keep], fresh()[k][~keep])


# -- 3. TrainStep(gradient_clip_val) ---------------------------------------------------------------
@pytest.mark.parametrize("kind,la", [("rmsprop", False), ("adam", False), ("radam", True)])
def test_trajectory_with_a_short_batch_follows_the_oracle_and_clip_grad_norm(kind, la):
    """Two epochs of batches 4, 4, 3 (the last on the remainder step, which shares the clip
    setting), eager, fixed noise: the oracle's gradients clipped by clip_grad_norm_ at 0.2 of
    the first step's norm, then stock torch.optim (RAdam + LookAhead: the CPU forms the
    reference trajectories hold): loss within 1e-4, every step's norm within 1e-5 of its own
    gradient's (the first step's within 1e-4 of the oracle's), clipping active in every step, final parameters
    within the trajectory tests' bars."""
    from torch_scae_amd import factory
    from torch_scae_amd.nn_utils import fixed_noise
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(0)
    torch.manual_seed(0)
    model = factory.make_scae(SMALL)
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.normal_(0, 0.1)
    # (lr 5e-4: six steps of a piecewise-linear model stay on the oracle's ReLU gates)
    B, lr, wd = 4, 5e-4, (1e-3 if kind == "rmsprop" else 0.0)
    Pm = {k: v.clone().requires_grad_(True) for k, v in model.state_dict().items()}
    ocfg = O.prepare_model_params(**SMALL)
    cpu_step, cpu_decay = _mirror(kind, la, Pm, lr, wd, B)
    g = torch.Generator().manual_seed(7)
    data = []
    for b in [4, 4, 3] * 2:
        data.append((torch.rand(b, 1, 16, 16, generator=g), torch.randint(0, 4, (b,), generator=g),
                     [torch.rand(b, 5, generator=g), torch.rand(b, 4, 1, generator=g),
                      torch.rand(b, 4, 5, generator=g)]))
    clip = None
    step = None
    for i, (image, label, noise) in enumerate(data):
        ref_loss, _, ref_grads = O.train_step(Pm, ocfg, image, label, noise)
        live = [v for v in ref_grads.values() if v is not None]
        total = float(torch.linalg.vector_norm(torch.stack(
            [torch.linalg.vector_norm(v.double()) for v in live])))
        if clip is None:     # (the norm falls to ~0.28 of the first within the six steps)
            clip = 0.2 * total
            model = model.cuda().train()
            step = TrainStep(model, B, (1, 16, 16), lr=lr, use_graph=False, optimizer=kind,
                             look_ahead=la, weight_decay=wd, lr_decay_rate=0.5,
                             gradient_clip_val=clip)
        # (clip_grad_norm_ on tensors standing in for the parameters: it clips their .grad)
        holders = []
        for v in live:
            h = torch.zeros_like(v, requires_grad=True)
            h.grad = v
            holders.append(h)
        torch.nn.utils.clip_grad_norm_(holders, clip)
        cpu_step(ref_grads)
        with fixed_noise([x.clone() for x in noise]):
            loss = step(image.cuda(), label.cuda())
        assert abs(float(loss.detach()) - float(ref_loss)) <= \
            1e-4 * max(1.0, abs(float(ref_loss)))
        norm = float(step.last_grad_norm())
        own = float(step.flat.flat_grad.double().norm())     # this step's own gradient
        assert abs(norm - own) <= 1e-5 * own, (i, norm, own)
        if i == 0:     # (later steps start from parameters that drift within the bars)
            assert abs(norm - total) <= 1e-4 * total, (i, norm, total)
        assert norm > clip, (i, norm, clip)      # clipping active in every step
        if i == 2:
            step.end_epoch()
            cpu_decay(0.5)
    assert step._rem is not None and step._rem.opt is step.opt
    sd = model.state_dict()
    for k, p in Pm.items():
        _close(sd[k].cpu(), p.detach(), 1e-4, 2e-3, "param " + k)


def _cfg2_step(**kw):
    from torch_scae_amd import factory, ops
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(0)
    torch.manual_seed(0)
    ops.reset_noise()
    model = factory.make_scae(CFG2).cuda().train()
    return TrainStep(model, 128, CFG2["image_shape"], lr=1e-3, **kw)


def _cfg2_batches(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(128, 1, 40, 40, generator=g).cuda(),
             torch.randint(0, 10, (128,), generator=g).cuda()) for _ in range(n)]


_FIRST_NORM = {}
CLIP_FRACTION = 0.35     # of the first step's norm: below every later step's in these runs


def _first_norm():
    """cfg-2's first-step gradient norm from _cfg2_step's start on the first batch."""
    if "n" not in _FIRST_NORM:
        step = _cfg2_step(gradient_clip_val=1e30)
        step(*_cfg2_batches(1)[0])
        _FIRST_NORM["n"] = float(step.last_grad_norm())
    return _FIRST_NORM["n"]


def _clipped(grad, clip):
    """clip_grad_norm_'s arithmetic on ONE tensor of the flat gradient -> (clipped, norm): the
    fp32 total rounded from fp64 (torch's own fp32 reduction of cfg-2's 2.4 M squares on the
    CPU is 1e-5 off), coef = min(1, clip / (total + 1e-6)) in fp32.  The flat gradient's
    inactive slots are zero, so its norm is the one over the parameters that have a
    gradient."""
    total = grad.double().norm().float()
    return grad * torch.clamp(clip / (total + 1e-6), max=1.0), float(total)


def _cpu_mirror(kind, la, flat_param):
    """_clipped + the CPU side of test_optimizers_gpu.py's mirror (stock torch.optim RMSprop /
    Adam, the reference-checked CPU RAdam + LookAhead) over ONE tensor of the flat buffer."""
    import torch.nn as nn
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    eps = 1e-2 / 128.0 ** 2
    if not la:
        p = flat_param.detach().cpu().clone().requires_grad_(True)
        opt = torch.optim.RMSprop([p], lr=1e-3, momentum=0.9, eps=eps) if kind == "rmsprop" \
            else torch.optim.Adam([p], lr=1e-3, eps=eps)

        def step(grad, ours, clip):
            with torch.no_grad():
                p.copy_(ours)
            p.grad, norm = _clipped(grad, clip)
            opt.step()
            return p.detach(), norm
        return step
    mod = nn.Module()
    mod.w = nn.Parameter(flat_param.detach().cpu().clone())
    flat = FlatParameters(mod)
    opt = make_optimizer(kind, flat, lr=1e-3, eps=eps, look_ahead=la)

    def step(grad, ours, clip):
        flat.flat_param.copy_(ours)
        g, norm = _clipped(grad, clip)
        flat.flat_grad.copy_(g)
        opt.step()
        return flat.flat_param, norm
    return step


@pytest.mark.parametrize("kind,la", [("rmsprop", False), ("adam", False), ("radam", True)])
def test_cfg2_replays_follow_clip_grad_norm_on_their_own_gradients(kind, la):
    """cfg-2, B = 128, clip at 0.35 of the first step's norm, 8 graph replays: after each, the
    parameters equal clip_grad_norm_'s arithmetic (_clipped) + the CPU optimiser stepped on
    that replay's own flat
    gradient from the same parameters (the kernel tests' bars), last_grad_norm() within 1e-5
    of torch's norm of that gradient and above the clip (active in every step); the slots of
    parameters without a gradient hold zeros, so the whole buffer's norm is theirs."""
    clip = CLIP_FRACTION * _first_norm()
    step = _cfg2_step(optimizer=kind, look_ahead=la, gradient_clip_val=clip)
    step.capture()
    flat = step.flat
    cpu = _cpu_mirror(kind, la, flat.flat_param)
    idle = [(off, p.numel()) for p, off in zip(flat.params, flat.offsets)
            if not getattr(p, "_flat_was_set", True)]
    for i, (img, lab) in enumerate(_cfg2_batches(8)):
        before = flat.flat_param.cpu()
        step(img, lab)
        torch.cuda.synchronize()
        grad = flat.flat_grad.cpu()
        for off, cnt in idle:
            assert float(grad[off:off + cnt].abs().max()) == 0.0
        ref, norm = cpu(grad, before, clip)
        got = float(step.last_grad_norm())
        assert abs(got - norm) <= 1e-5 * norm and got > clip, (i, got, norm, clip)
        ref = ref.double().numpy()
        ours = flat.flat_param.cpu().double().numpy()
        upd = np.abs(ref - before.double().numpy()).max()
        err = (np.abs(ours - ref) - ulp(ref)).max()
        assert upd > 0 and err <= 1e-5 * upd, (i, err, upd)


def test_cfg2_graph_and_launch_list_replays_agree_and_cost_one_launch():
    """RMSprop at cfg-2 (the step's last column sums ride in the norm launch): the launch-list
    replay of the clipped step is bit for bit its graph replay (parameters, moments, norms),
    still replays as a launch list, and records exactly one library launch more than the
    unclipped step."""
    from torch_scae_amd import _lib
    clip = CLIP_FRACTION * _first_norm()
    data = _cfg2_batches(5)
    runs = {}
    for replay in ("graph", "launches"):
        step = _cfg2_step(gradient_clip_val=clip, replay=replay)
        assert step.plan.sums_to_optimizer
        norms = []
        for img, lab in data:
            step(img, lab)
            norms.append(step.last_grad_norm().clone())
        torch.cuda.synchronize()
        runs[replay] = (step.flat.flat_param.clone(), step.opt.square_avg.clone(),
                        step.opt.buf.clone(), torch.stack(norms))
        if replay == "launches":
            assert step._klist, "the clipped step did not replay as a launch list"
            n_clip = _lib.load().scae_launch_list_size(step._klist)
    for a, b in zip(runs["graph"], runs["launches"]):
        assert torch.equal(a, b)
    assert float(runs["graph"][3].min()) > clip
    plain = _cfg2_step(replay="launches")
    plain(*data[0])
    assert plain._klist
    assert n_clip == _lib.load().scae_launch_list_size(plain._klist) + 1


@pytest.mark.parametrize("kind,la", [("rmsprop", False), ("adam", True)])
def test_cfg2_large_clip_reproduces_the_unclipped_trajectory(kind, la):
    """gradient_clip_val far above the norm: coef == 1 and the trajectory is the unclipped
    one bit for bit (the norm launch is one launch more; the clip forms multiply by 1.0)."""
    data = _cfg2_batches(4)
    outs = []
    for kw in (dict(), dict(gradient_clip_val=1e30)):
        step = _cfg2_step(optimizer=kind, look_ahead=la, **kw)
        for img, lab in data:
            step(img, lab)
        torch.cuda.synchronize()
        outs.append([b.clone() for _, b in step.opt.state_buffers()] +
                    [step.flat.flat_param.clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_cfg2_drop_last_false_epoch_clips_its_short_step():
    """A drop_last=False view of 2 x 128 + 40 images: the short step (remainder step, own
    launch list) clips too -- its norm is its own gradient's, and its update is clip_grad_norm_
    + torch.optim.RMSprop on that gradient."""
    clip = CLIP_FRACTION * _first_norm()
    step = _cfg2_step(gradient_clip_val=clip, replay="launches")
    ds = _dataset(2 * 128 + 40)
    view = ds.view(shuffle=True, seed=4, drop_last=False)
    cpu = _cpu_mirror("rmsprop", False, step.flat.flat_param)
    for i in range(3):
        before = step.flat.flat_param.cpu()
        step.step_from(view)
        torch.cuda.synchronize()
        ref, norm = cpu(step.flat.flat_grad.cpu(), before, clip)
        got = float(step.last_grad_norm())
        assert abs(got - norm) <= 1e-5 * norm and got > clip, (i, got, norm)
        ref = ref.double().numpy()
        ours = step.flat.flat_param.cpu().double().numpy()
        upd = np.abs(ref - before.double().numpy()).max()
        assert upd > 0 and (np.abs(ours - ref) - ulp(ref)).max() <= 1e-5 * upd, i
    assert step._rem is not None and step._rem.image.shape[0] == 40 and step._rem._klist


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_collective_modes_match_the_plain_clipped_step(nccl_group, kind):
    """The 1-rank "2 buckets", "1 bucket" and "in graph" modes clip the all-reduced gradient
    and end on the parameters of the collective-free clipped step (three steps, graph replay,
    clip at a third of the first step's norm).  The modes cut the buffer's partial sums
    differently; the fp32 norm is the same unless two fp64 sums straddle an fp32 rounding
    boundary, which these steps do not."""
    data = batches(3)
    outs = []
    clip = None
    for kw in (dict(), dict(force_collective=True),
               dict(force_collective=True, overlap=False),
               dict(force_collective=True, collective_mode="in graph")):
        if clip is None:
            _, probe = small_step(noise=False, lr=1e-3, optimizer=kind, gradient_clip_val=1e30)
            probe(*data[0])
            clip = float(probe.last_grad_norm()) / 3
        model, step = small_step(noise=False, lr=1e-3, optimizer=kind, gradient_clip_val=clip,
                                 **kw)
        norms = []
        for img, lab in data:
            step(img, lab)
            norms.append(float(step.last_grad_norm()))
        torch.cuda.synchronize()
        assert min(norms) > clip
        outs.append((kw, norms, {k: v.clone() for k, v in model.state_dict().items()}))
    assert outs[1][0] and outs[3][0]
    for kw, norms, sd in outs[1:]:
        assert norms == outs[0][1], (kw, norms, outs[0][1])
        for k, v in sd.items():
            assert torch.equal(outs[0][2][k], v), (kw, k)
