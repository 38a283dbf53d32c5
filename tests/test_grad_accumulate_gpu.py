"""Gradient accumulation on the GPU: the accumulate pass (and its form with the step's last
column sums riding in it) against torch bit for bit, the accumulate forms of the optimiser
passes and of the norm launch against the plain ones run on a materialised acc + g, and
TrainStep(accumulate_grad_batches) -- against the oracle's summed gradients, against its own
gradients at cfg-2's size, in every replay form and collective mode, over views with a short
step, across a snapshot."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import scae_oracle as O
from tests.test_grad_clip_gpu import _jobs, _cfg2_batches, _cfg2_step, norm_launch
from tests.test_optimizers_gpu import BETAS, KIND, batches, small_step, ulp
from tests.test_train_remainder_gpu import SMALL, _close, _dataset, _mirror

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
LENGTHS = [1, 2, 3, 5, 6, 7, 257, 1023, 4099, 65537, 2414879]


def stream():
    return P(torch.cuda.current_stream().cuda_stream)


# -- 1. the accumulate pass ----------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_accumulate_pass_is_torch_add(n):
    """acc += g over n floats at each 4-byte phase of a 16-byte line: bit for bit torch's fp32
    add; the floats around the range untouched."""
    from torch_scae_amd import _lib
    gen = torch.Generator().manual_seed(n)
    for phase in range(4):
        g = torch.randn(n + 8, generator=gen).cuda()
        acc = torch.randn(n + 8, generator=gen).cuda()
        want = acc.clone()
        want[phase:phase + n] += g[phase:phase + n]
        _lib.call("scae_grad_accumulate_f32", P(acc.data_ptr() + 4 * phase),
                  P(g.data_ptr() + 4 * phase), n, stream())
        torch.cuda.synchronize()
        assert torch.equal(acc, want), (n, phase)


def test_riding_sums_accumulate_equals_sum_rows_then_add():
    """scae_grad_accumulate_sums_f32: the column sums it writes into `grad` equal
    scae_sum_rows_multi_f32's bit for bit, and acc ends as acc + (the buffer with them in it)
    -- the streaming workgroups skip exactly the sums' ranges."""
    from torch_scae_amd import _lib
    n = 20011
    acc0 = torch.randn(n, generator=torch.Generator().manual_seed(6)).cuda()
    grad = torch.randn(n, generator=torch.Generator().manual_seed(5)).cuda()
    jobs, nj, keep = _jobs(grad)
    _lib.call("scae_sum_rows_multi_f32", jobs, nj, stream())
    torch.cuda.synchronize()
    want_grad, want_acc = grad.clone(), acc0 + grad
    for _ in range(2):
        grad = torch.randn(n, generator=torch.Generator().manual_seed(5)).cuda()
        acc = acc0.clone()
        jobs, nj, keep = _jobs(grad)
        _lib.call("scae_grad_accumulate_sums_f32", P(acc.data_ptr()), P(grad.data_ptr()), n,
                  jobs, nj, stream())
        torch.cuda.synchronize()
        assert torch.equal(grad, want_grad) and torch.equal(acc, want_acc)


# -- 2. the accumulate forms -------------------------------------------------------------------
def _opt(kind, la, bufs, ranges, clip=None, acc=True, st_state=None, lr_dev=None, wd=0.0):
    """One optimiser step over the ranges: the plain pass on bufs["g"] (acc False) or the
    accumulate form on bufs["g"] + bufs["acc"]; clip: (partials, count, max_norm, norm_out)."""
    from torch_scae_amd import _lib
    A = "_acc" if acc else ""
    for i, (off, cnt) in enumerate(ranges):
        ptr = lambda k: P(bufs[k].data_ptr() + 4 * off)   # noqa: E731
        a = (ptr("acc"),) if acc else ()
        tail = (P(clip[0].data_ptr()), clip[1], clip[2],
                P(clip[3].data_ptr()) if i == 0 else None) if clip else ()
        c = "_clip" if clip else ""
        if kind == "rmsprop" and not la:
            _lib.call(f"scae_rmsprop{A}{c}_step_f32", ptr("p"), ptr("g"), *a, ptr("v"),
                      ptr("m"), cnt, 1e-3, P(lr_dev.data_ptr()), 0.99, 1e-4, 0.9, wd, 0.5,
                      *tail, stream())
        else:
            _lib.call(f"scae_flat_opt{A}{c}_step_f32", ptr("p"), ptr("g"), *a, ptr("m"),
                      ptr("v"), ptr("slow"), cnt, P(lr_dev.data_ptr()), P(st_state.data_ptr()),
                      KIND[kind], *BETAS[kind], 1e-4, wd, 0.5, 5 if la else 0, 0.5,
                      int(i == len(ranges) - 1), *tail, stream())


def _fresh(n, seed=21):
    gg = torch.Generator().manual_seed(seed)
    b = dict(p=torch.randn(n, generator=gg), g=torch.randn(n, generator=gg),
             acc=torch.randn(n, generator=gg) * 2, m=torch.randn(n, generator=gg) * .1,
             v=torch.rand(n, generator=gg), slow=torch.randn(n, generator=gg))
    return {k: x.cuda() for k, x in b.items()}


def _state(la):
    from torch_scae_amd import _lib
    s = torch.zeros(_lib.FLAT_OPT_STATE_INTS, dtype=torch.int32, device="cuda")
    s[:2] = torch.tensor([9, int(la)], dtype=torch.int32)
    return s


OPT_CASES = [(k, la, wd) for k in ("rmsprop", "adam", "radam") for la in (False, True)
             for wd in (0.0, 1e-2)]


@pytest.mark.parametrize("kind,la,wd", OPT_CASES)
@pytest.mark.parametrize("clip", [False, True])
def test_update_forms_equal_the_plain_pass_on_acc_plus_g(kind, la, wd, clip):
    """Each accumulate form (plain and clip; with weight decay one launch per range, gaps left
    alone) is bit for bit the existing pass run on a materialised acc + g, at a LookAhead sync
    step; acc is 0 afterwards in the ranges and untouched outside them.  The clip forms read
    the accumulate form of the norm launch, whose partials equal the norm launch's on acc + g
    bit for bit."""
    from torch_scae_amd import _lib
    n = 30011
    ranges = [(0, n)] if wd == 0 else [(3, 9000), (9010, 15000), (24020, 5990)]
    lr_dev = torch.full((1,), 1e-3, device="cuda")
    ours, ref = _fresh(n), _fresh(n)
    ref["g"] = ref["acc"] + ref["g"]
    cl_ours = cl_ref = None
    if clip:
        part, cnt = norm_launch(ref["g"], n)
        part2 = torch.full_like(part, float("nan"))
        cnt2 = ctypes.c_int(0)
        _lib.call("scae_grad_sq_acc_partials_f32", P(ours["g"].data_ptr()),
                  P(ours["acc"].data_ptr()), n, P(part2.data_ptr()), part2.numel(),
                  ctypes.byref(cnt2), stream())
        torch.cuda.synchronize()
        assert cnt2.value == cnt and torch.equal(part[:cnt], part2[:cnt])
        max_norm = 0.3 * 0.5 * float(part[:cnt].sum()) ** 0.5
        cl_ours = (part2, cnt, max_norm, torch.zeros((), device="cuda"))
        cl_ref = (part, cnt, max_norm, torch.zeros((), device="cuda"))
    s1, s2 = _state(la), _state(la)
    _opt(kind, la, ours, ranges, cl_ours, True, s1, lr_dev, wd)
    _opt(kind, la, ref, ranges, cl_ref, False, s2, lr_dev, wd)
    torch.cuda.synchronize()
    assert torch.equal(s1, s2)
    for k in ("p", "m", "v", "slow"):
        assert torch.equal(ours[k], ref[k]), k
    if clip:
        assert torch.equal(cl_ours[3], cl_ref[3])
    keep = torch.zeros(n, dtype=torch.bool, device="cuda")
    for off, c in ranges:
        keep[off:off + c] = True
    assert float(ours["acc"][keep].abs().max()) == 0.0
    assert torch.equal(ours["acc"][~keep], _fresh(n)["acc"][~keep])


@pytest.mark.parametrize("n", [1, 3, 5, 257, 4099, 2414879])
def test_update_forms_at_each_phase_and_length(n):
    """Adam's and RMSprop's accumulate forms equal the plain pass on acc + g at every 4-byte
    phase of a 16-byte line, from one float to cfg-2's 2 414 879."""
    lr_dev = torch.full((1,), 1e-3, device="cuda")
    for kind in ("rmsprop", "adam"):
        for phase in range(4):
            ours, ref = _fresh(n + 8, seed=n + phase), _fresh(n + 8, seed=n + phase)
            ref["g"] = ref["acc"] + ref["g"]
            s1, s2 = _state(False), _state(False)
            _opt(kind, False, ours, [(phase, n)], None, True, s1, lr_dev)
            _opt(kind, False, ref, [(phase, n)], None, False, s2, lr_dev)
            torch.cuda.synchronize()
            for k in ("p", "m", "v"):
                assert torch.equal(ours[k], ref[k]), (kind, phase, k)
            assert float(ours["acc"][phase:phase + n].abs().max()) == 0.0


@pytest.mark.parametrize("kind,la", [("rmsprop", False), ("adam", False), ("radam", True)])
@pytest.mark.parametrize("clip", [False, True])
def test_riding_sums_update_forms_equal_sum_rows_then_the_plain_pass(kind, la, clip):
    """The sums-riding accumulate forms (of the optimiser pass, and of the norm launch ahead of
    a clip form) equal scae_sum_rows_multi_f32 followed by the plain pass on acc + g."""
    from torch_scae_amd import _lib
    n = 20011
    lr_dev = torch.full((1,), 1e-3, device="cuda")
    outs = []
    for fused in (False, True):
        b = _fresh(n, seed=5)
        jobs, nj, keep = _jobs(b["g"])
        st = _state(la)
        if not fused:
            _lib.call("scae_sum_rows_multi_f32", jobs, nj, stream())
            b["g"] = b["acc"] + b["g"]
            cl = None
            if clip:
                part, cnt = norm_launch(b["g"], n)
                cl = (part, cnt, 0.3 * 0.5 * float(part[:cnt].sum()) ** 0.5,
                      torch.zeros((), device="cuda"))
            _opt(kind, la, b, [(0, n)], cl, False, st, lr_dev)
        elif clip:
            part = torch.zeros(_lib.GRAD_SQ_MAX_PARTIALS, dtype=torch.float64, device="cuda")
            cnt = ctypes.c_int(0)
            _lib.call("scae_grad_sq_acc_partials_sums_f32", P(b["g"].data_ptr()),
                      P(b["acc"].data_ptr()), n, P(part.data_ptr()), part.numel(),
                      ctypes.byref(cnt), jobs, nj, stream())
            torch.cuda.synchronize()
            tot = float(part[:cnt.value].sum())
            cl = (part, cnt.value, 0.3 * 0.5 * tot ** 0.5, torch.zeros((), device="cuda"))
            _opt(kind, la, b, [(0, n)], cl, True, st, lr_dev)
        else:
            args = (P(b["p"].data_ptr()), P(b["g"].data_ptr()), P(b["acc"].data_ptr()))
            if kind == "rmsprop" and not la:
                _lib.call("scae_rmsprop_acc_sums_step_f32", *args, P(b["v"].data_ptr()),
                          P(b["m"].data_ptr()), n, 1e-3, P(lr_dev.data_ptr()), 0.99, 1e-4,
                          0.9, 0.5, jobs, nj, stream())
            else:
                _lib.call("scae_flat_opt_acc_sums_step_f32", *args, P(b["m"].data_ptr()),
                          P(b["v"].data_ptr()), P(b["slow"].data_ptr()), n,
                          P(lr_dev.data_ptr()), P(st.data_ptr()), KIND[kind], *BETAS[kind],
                          1e-4, 0.5, 5 if la else 0, 0.5, jobs, nj, stream())
        torch.cuda.synchronize()
        outs.append((b, st))
    (ref, s2), (ours, s1) = outs
    assert torch.equal(s1, s2)
    for k in ("p", "m", "v", "slow"):
        assert torch.equal(ours[k], ref[k]), k
    assert float(ours["acc"].abs().max()) == 0.0


# -- 3. TrainStep(accumulate_grad_batches) ---------------------------------------------------------
@pytest.mark.parametrize("kind,la,clip", [("rmsprop", False, False), ("adam", False, False),
                                          ("radam", True, False), ("adam", False, True)])
def test_trajectory_follows_the_oracles_summed_gradients(kind, la, clip):
    """Two epochs of batches 4, 4, 4, 3 (the last on the remainder step) with k = 3, eager,
    fixed noise: the optimiser steps after batches 2 and 3 of each epoch on the oracle's
    gradients summed over the group and scaled by 1/3 (clip_grad_norm_ first in one case),
    stepped by stock torch.optim / the CPU RAdam + LookAhead; losses and final parameters
    within the trajectory tests' bars; counts per rule 2 and 6."""
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
    B, lr, wd, k = 4, 5e-4, (1e-3 if kind == "rmsprop" else 0.0), 3
    Pm = {n: v.clone().requires_grad_(True) for n, v in model.state_dict().items()}
    ocfg = O.prepare_model_params(**SMALL)
    cpu_step, cpu_decay = _mirror(kind, la, Pm, lr, wd, B)
    g = torch.Generator().manual_seed(7)
    data = []
    for b in [4, 4, 4, 3] * 2:
        data.append((torch.rand(b, 1, 16, 16, generator=g), torch.randint(0, 4, (b,), generator=g),
                     [torch.rand(b, 5, generator=g), torch.rand(b, 4, 1, generator=g),
                      torch.rand(b, 4, 5, generator=g)]))
    step, max_norm, group = None, 0.0, None
    for i, (image, label, noise) in enumerate(data):
        ref_loss, _, ref_grads = O.train_step(Pm, ocfg, image, label, noise)
        if step is None:
            if clip:
                live = [v for v in ref_grads.values() if v is not None]
                max_norm = 0.2 * float(torch.linalg.vector_norm(torch.stack(
                    [torch.linalg.vector_norm(v.double()) for v in live])))
            model = model.cuda().train()
            step = TrainStep(model, B, (1, 16, 16), lr=lr, use_graph=False, optimizer=kind,
                             look_ahead=la, weight_decay=wd, lr_decay_rate=0.5,
                             gradient_clip_val=max_norm, accumulate_grad_batches=k)
        group = {n: (None if v is None else v.clone()) for n, v in ref_grads.items()} \
            if group is None else {n: (v if ref_grads[n] is None else
                                       ref_grads[n].clone() if v is None else v + ref_grads[n])
                                   for n, v in group.items()}
        with fixed_noise([x.clone() for x in noise]):
            loss = step(image.cuda(), label.cuda())
        assert abs(float(loss.detach()) - float(ref_loss)) <= \
            1e-4 * max(1.0, abs(float(ref_loss)))
        pos = i % 4
        if (pos + 1) % k and pos != 3:
            assert step._acc_state["pending"] > 0
            continue
        # the group ends here: (g_1 + ...) * fp32(1/k), clipped, stepped
        scaled = {n: None if v is None else v * (1.0 / k) for n, v in group.items()}
        if clip:
            holders = []
            for v in scaled.values():
                if v is not None:
                    h = torch.zeros_like(v, requires_grad=True)
                    h.grad = v
                    holders.append(h)
            torch.nn.utils.clip_grad_norm_(holders, max_norm)
        cpu_step(scaled)
        group = None
        if pos == 3:     # (the short batch ends the epoch and its group)
            step.end_epoch()
            cpu_decay(0.5)
    assert step.steps == 8 and step.optimizer_steps == 4
    if kind != "rmsprop" or la:
        assert int(step.opt.step_state[0]) == 4
    sd = model.state_dict()
    for n, p in Pm.items():
        _close(sd[n].cpu(), p.detach(), 1e-4, 2e-3, "param " + n)


@pytest.mark.parametrize("replay", ["graph", "launches"])
def test_replayed_forms_compute_the_eager_steps_gradients(replay):
    """The replayed accumulating step (k = 3, both captured forms, graph or launch-list replay)
    against an independent eager k = 1 step without optimiser, fed the same parameters before
    every batch (no noise): each batch's flat gradient and loss agree within 1e-5 of the
    largest gradient; acc holds the fp32 sum of the group's gradients in batch order on the
    batches that do not end a group and is 0 after those that do, when the parameters move."""
    model, step = small_step(noise=False, lr=1e-3, optimizer="adam", accumulate_grad_batches=3,
                             replay=replay)
    _, ref = small_step(noise=False, optimizer=None, use_graph=False)
    assert step.flat.offsets == ref.flat.offsets
    host = None
    for i, (img, lab) in enumerate(batches(7)):
        before = step.flat.flat_param.clone()
        ref.flat.flat_param.copy_(before)
        ref_loss = float(ref(img, lab))
        loss = float(step(img, lab))
        torch.cuda.synchronize()
        g, want = step.flat.flat_grad.cpu(), ref.flat.flat_grad.cpu()
        scale = float(want.abs().max())
        assert scale > 0 and float((g - want).abs().max()) <= 1e-5 * scale, i
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), i
        host = g.clone() if host is None else host + g
        if (i + 1) % 3:
            assert step._form == "acc" and torch.equal(step.flat.flat_param, before), i
            assert torch.equal(step.opt.acc.cpu(), host), i
        else:
            assert step._form == "update" and not torch.equal(step.flat.flat_param, before), i
            assert float(step.opt.acc.abs().max()) == 0.0
            host = None
    assert step._other_cap is not None and step._other_cap.graph is not None
    assert step.optimizer_steps == 2 and int(step.opt.step_state[0]) == 2


def _cpu_opt(kind, flat_param):
    """The stock torch optimiser over ONE tensor of the flat buffer (cfg-2's eps)."""
    p = flat_param.detach().cpu().clone().requires_grad_(True)
    eps = 1e-2 / 128.0 ** 2
    opt = torch.optim.RMSprop([p], lr=1e-3, momentum=0.9, eps=eps) if kind == "rmsprop" \
        else torch.optim.Adam([p], lr=1e-3, eps=eps)

    def step(grad, ours):
        with torch.no_grad():
            p.copy_(ours)
        p.grad = grad
        opt.step()
        return p.detach()
    return step


@pytest.mark.parametrize("kind,bf16", [("rmsprop", False), ("adam", False), ("rmsprop", True)])
def test_cfg2_replays_accumulate_their_own_gradients(kind, bf16):
    """cfg-2, B = 128, k = 3, nine graph replays (that flat_grad is each batch's gradient:
    test_replayed_forms_compute_the_eager_steps_gradients); on a batch that does not end its group the parameters, moments and step count
    are bit for bit what they were and acc is the fp32 sum of the group's gradients in batch
    order; after the group's last batch the parameters match the CPU optimiser stepped on that
    sum scaled by 1/3 (the clip tests' bar), and acc is 0."""
    kw = dict(autocast_dtype=torch.bfloat16) if bf16 else {}
    step = _cfg2_step(optimizer=kind, accumulate_grad_batches=3, **kw)
    flat, opt = step.flat, step.opt
    cpu = _cpu_opt(kind, flat.flat_param)
    host = None
    for i, (img, lab) in enumerate(_cfg2_batches(9)):
        before = flat.flat_param.cpu()
        state = [b.cpu() for _, b in opt.state_buffers()] + [opt.step_state.cpu()]
        step(img, lab)
        torch.cuda.synchronize()
        grad = flat.flat_grad.cpu()
        host = grad.clone() if host is None else host + grad
        if (i + 1) % 3:
            assert torch.equal(flat.flat_param.cpu(), before), i
            for a, (_, b) in zip(state, opt.state_buffers()):
                assert torch.equal(a, b.cpu()), i
            assert torch.equal(state[-1], opt.step_state.cpu())
            assert torch.equal(opt.acc.cpu(), host), i
            continue
        assert float(opt.acc.abs().max()) == 0.0
        ref = cpu(host * (1.0 / 3), before).double().numpy()
        ours = flat.flat_param.cpu().double().numpy()
        upd = np.abs(ref - before.double().numpy()).max()
        err = (np.abs(ours - ref) - ulp(ref)).max()
        assert upd > 0 and err <= 1e-5 * upd, (i, err, upd)
        host = None
    assert step.optimizer_steps == 3 and step.steps == 9


def _launch_count(step):
    from torch_scae_amd import _lib
    return _lib.load().scae_launch_list_size(step._klist) if step._klist else None


def test_k1_is_the_default_step():
    """accumulate_grad_batches=1: bit for bit the default step over 8 replays, the same library
    launch count, no accumulator."""
    data = _cfg2_batches(8)
    outs = []
    for kw in (dict(), dict(accumulate_grad_batches=1)):
        step = _cfg2_step(replay="launches", **kw)
        for img, lab in data:
            step(img, lab)
        torch.cuda.synchronize()
        assert step.opt.acc is None and step._other_cap is None
        outs.append((step.flat.flat_param.clone(), step.opt.square_avg.clone(),
                     step.opt.buf.clone(), _launch_count(step)))
    for a, b in zip(*outs):
        assert (a == b) if not isinstance(a, torch.Tensor) else torch.equal(a, b)
    assert outs[0][3]


@pytest.mark.parametrize("clip", [False, True])
def test_cfg2_forms_are_launch_lists_and_agree_with_graph_replay(clip):
    """k = 4 at cfg-2: launch-list and graph replays agree bit for bit over 10 batches; both
    forms replay as launch lists, the accumulate form with the unaccumulating step's library
    launch count (the accumulate pass in the optimiser's place), the update form with it too
    (one more with clipping: the norm launch)."""
    kw = dict(gradient_clip_val=1e30) if clip else {}
    data = _cfg2_batches(10)
    runs, counts = {}, {}
    for replay in ("graph", "launches"):
        step = _cfg2_step(replay=replay, accumulate_grad_batches=4, **kw)
        assert step.plan.sums_to_optimizer
        for img, lab in data:
            step(img, lab)
            if replay == "launches":
                counts[step._form] = _launch_count(step)
        torch.cuda.synchronize()
        runs[replay] = (step.flat.flat_param.clone(), step.opt.square_avg.clone(),
                        step.opt.buf.clone(), step.opt.acc.clone())
    for a, b in zip(runs["graph"], runs["launches"]):
        assert torch.equal(a, b)
    plain = _cfg2_step(replay="launches")
    plain(*data[0])
    base = _launch_count(plain)
    assert base and counts == {"acc": base, "update": base + int(clip)}, (counts, base)


def test_views_follow_the_schedule_and_flush_pending_groups():
    """A drop_last=False view of 7 x 128 + 40 images (8 steps an epoch, k = 3): train_epoch
    steps the optimiser after batches 2, 5 and the short 7th -> 3 optimiser steps an epoch,
    Adam's device count with them, the learning rate decayed once per epoch; the short step
    updates.  Then step(image, label) twice and end_epoch(): the pending group is stepped."""
    step = _cfg2_step(optimizer="adam", accumulate_grad_batches=3, replay="launches",
                      lr_decay_rate=0.5)
    view = _dataset(7 * 128 + 40).view(shuffle=True, seed=4, drop_last=False)
    assert view.steps_in_epoch(128) == 8
    lr0 = step.opt.lr
    for epoch in range(2):
        before = None
        while True:
            last = view.cursor == 7
            if last:
                before = step.flat.flat_param.clone()
            step.step_from(view)
            if last:
                break
        torch.cuda.synchronize()
        assert not torch.equal(before, step.flat.flat_param)     # the short step updated
        step.end_epoch()
        assert step.optimizer_steps == 3 * (epoch + 1) and step._acc_state["pending"] == 0
        assert int(step.opt.step_state[0]) == 3 * (epoch + 1)
        assert step.opt.lr == lr0 * 0.5 ** (epoch + 1)
    assert step.optimizer_state_dict()["state"][0]["step"] == 6
    data = _cfg2_batches(2)
    for img, lab in data:
        step(img, lab)
    assert step._acc_state["pending"] == 2
    before = step.flat.flat_param.clone()
    step.end_epoch()
    torch.cuda.synchronize()
    assert step._acc_state["pending"] == 0 and step.optimizer_steps == 7
    assert int(step.opt.step_state[0]) == 7 and float(step.opt.acc.abs().max()) == 0.0
    assert not torch.equal(before, step.flat.flat_param)


def test_snapshot_in_the_middle_of_a_group_replays_bit_for_bit():
    """k = 3, a snapshot one batch into a group (acc, pending count and optimiser steps in
    it), four more batches, restore(), the same four again under the same captured forms:
    bitwise the first run."""
    model, step = small_step(noise=False, lr=1e-3, optimizer="adam", accumulate_grad_batches=3)
    data = batches(8)
    for img, lab in data[:4]:
        step(img, lab)
    snap = step.snapshot()
    assert step._acc_state == {"pending": 1, "optimizer_steps": 1}
    runs = []
    for _ in range(2):
        for img, lab in data[4:]:
            step(img, lab)
        torch.cuda.synchronize()
        runs.append((step.flat.flat_param.clone(), step.opt.exp_avg.clone(),
                     step.opt.acc.clone(), step.opt.step_state.clone(),
                     dict(step._acc_state)))
        step.restore(snap)
    assert runs[0][4] == {"pending": 2, "optimizer_steps": 2}
    assert float(runs[0][2].abs().max()) > 0
    for a, b in zip(*runs):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_collective_modes_match_the_plain_accumulating_step(nccl_group, kind):
    """The 1-rank "2 buckets", "1 bucket" and "in graph" modes with k = 2 (acc folded into
    the gradient and all-reduced once per group) end on the parameters of the collective-free
    k = 2 step bit for bit (five steps, graph replay: the last group pending)."""
    data = batches(5)
    outs = []
    for kw in (dict(), dict(force_collective=True),
               dict(force_collective=True, overlap=False),
               dict(force_collective=True, collective_mode="in graph")):
        model, step = small_step(noise=False, lr=1e-3, optimizer=kind,
                                 accumulate_grad_batches=2, **kw)
        for img, lab in data:
            step(img, lab)
        torch.cuda.synchronize()
        assert step.optimizer_steps == 2
        # (acc per parameter: the bucketed modes lay the flat buffer out in another order)
        where = {id(p): off for p, off in zip(step.flat.params, step.flat.offsets)}
        acc = {n: step.opt.acc[where[id(p)]:where[id(p)] + p.numel()].clone()
               for n, p in model.named_parameters()}
        outs.append((kw, {k: v.clone() for k, v in model.state_dict().items()}, acc))
    assert outs[1][0] and outs[3][0]
    assert max(float(a.abs().max()) for a in outs[0][2].values()) > 0
    for kw, sd, acc in outs[1:]:
        for n, a in acc.items():
            assert torch.equal(outs[0][2][n], a), (kw, n)
        for k, v in sd.items():
            assert torch.equal(outs[0][1][k], v), (kw, k)
