"""The fused Adam / RAdam / LookAhead passes (scae_flat_opt_step_f32,
scae_flat_opt_sums_step_f32) on the GPU, and TrainStep training with them: against the
reference's trajectories (tests/golden/optim_trajectories.npz), the riding forms against
the two-launch forms, the device step count under replay, restore and the collective
path."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_optimizers import CASES, EPS, STATE_KEYS, case_name, golden

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
KIND = {"adam": 0, "radam": 1, "rmsprop": 2}
BETAS = {"adam": (0.9, 0.999), "radam": (0.9, 0.999), "rmsprop": (0.9, 0.99)}


def ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("kind,wd,la", CASES, ids=[case_name(*c) for c in CASES])
def test_kernel_steps_against_the_reference_trajectories(kind, wd, la):
    """scae_flat_opt_step_f32, every one of the 12 golden steps from the golden state
    before it (step count, slow weights and learning rate included), the three tensors
    back to back in slices of flat buffers that start at each 4-byte phase of a 16-byte
    line (one launch over all three; with weight decay one launch per tensor, the last
    advancing the count): each step's update within 1e-5 of the tensor's largest update
    (+ one ulp of the parameter: the update is a difference of rounded parameters), the
    moments and slow weights within 1e-6 of the tensor's largest entry.  RMSprop's moments
    (kind 2: optimizer.hip's RMSprop, kept bit for bit) within 5e-5: that pass rounds
    1 - alpha in fp32 where torch rounds it from fp64, 1e-6 apart; square_avg carries that
    1e-6, the momentum buffer amplifies it where 0.9 buf and the step nearly cancel (2e-5
    of the largest entry in this fixture)."""
    from torch_scae_amd import _lib
    d = golden()
    name = case_name(kind, wd, la)
    sizes = [d[f"init{j}"].size for j in range(3)]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offs[-1])
    keys = STATE_KEYS[kind] + (("slow_buffer",) if la else ())
    st = P(torch.cuda.current_stream().cuda_stream)
    for phase in range(4):
        bufs = {k: torch.zeros(n + phase + 4, device="cuda")
                for k in ("param", "grad") + STATE_KEYS[kind] + ("slow_buffer",)}
        state = torch.zeros(_lib.FLAT_OPT_STATE_INTS, dtype=torch.int32, device="cuda")
        lr_dev = torch.zeros(1, device="cuda")

        def put(key, arrs):
            bufs[key][phase:phase + n] = torch.from_numpy(np.concatenate(arrs)).cuda()

        for s in range(12):
            prev = (lambda key: [d[f"{name}/{key}{j}"][s - 1] for j in range(3)]) if s else \
                (lambda key: [d[f"init{j}"] if key == "param" else np.zeros(sizes[j], np.float32)
                              for j in range(3)])
            put("param", prev("param"))
            for key in keys:
                put(key, prev(key))
            put("grad", [d[f"grad{j}"][s] for j in range(3)])
            made = int(la and s >= 5)
            state[:2] = torch.tensor([s, made], dtype=torch.int32)
            lr_dev.fill_(float(d[f"{name}/lr"][s]))
            ranges = [(0, n)] if wd == 0 else [(int(offs[j]), sizes[j]) for j in range(3)]
            for i, (off, cnt) in enumerate(ranges):
                ptr = lambda key: P(bufs[key].data_ptr() + 4 * (phase + off))   # noqa: E731
                _lib.call("scae_flat_opt_step_f32", ptr("param"), ptr("grad"),
                          ptr(STATE_KEYS[kind][1] if kind == "rmsprop" else "exp_avg"),
                          ptr(STATE_KEYS[kind][0] if kind == "rmsprop" else "exp_avg_sq"),
                          ptr("slow_buffer"), cnt, P(lr_dev.data_ptr()), P(state.data_ptr()),
                          KIND[kind], *BETAS[kind], EPS, wd, 1.0, 5 if la else 0, 0.5,
                          int(i == len(ranges) - 1), st)
            torch.cuda.synchronize()
            assert state[:2].tolist() == [s + 1, int(la and s + 1 >= 5)], (name, s, state)
            assert int(state[2:].abs().sum()) == 0     # the arrival counters are back at 0
            for j in range(3):
                sl = slice(phase + int(offs[j]), phase + int(offs[j + 1]))
                before = prev("param")[j].astype(np.float64)
                ref = d[f"{name}/param{j}"][s].astype(np.float64)
                ours = bufs["param"][sl].cpu().numpy().astype(np.float64)
                upd = np.abs(ref - before).max()
                err = np.abs(ours - ref) - ulp(ref)
                assert err.max() <= 1e-5 * upd, (name, phase, s + 1, j, err.max(), upd)
                for key in keys:
                    ref = d[f"{name}/{key}{j}"][s]
                    err = np.abs(bufs[key][sl].cpu().numpy() - ref).max()
                    bar = 5e-5 if kind == "rmsprop" and key != "slow_buffer" else 1e-6
                    assert err <= bar * max(np.abs(ref).max(), 1e-30), \
                        (name, phase, s + 1, key, j, err)
        # nothing outside the slices was written
        for key, b in bufs.items():
            assert float(b[:phase].abs().sum()) == 0 and float(b[phase + n:].abs().sum()) == 0


@pytest.mark.parametrize("kind,la,t", [("adam", False, 2), ("radam", False, 2),
                                       ("radam", False, 8), ("adam", True, 9),
                                       ("radam", True, 14), ("rmsprop", True, 9)])
def test_riding_forms_equal_two_launches_bitwise(kind, la, t):
    """scae_flat_opt_sums_step_f32: the step's last column sums (the job tables of
    test_sums_riding_in_the_optimizer_launch_equal_two_launches_bitwise) as the head of
    the optimiser launch -- bit for bit scae_sum_rows_multi_f32 + scae_flat_opt_step_f32
    on every buffer and the step state, for Adam, RAdam (both regimes) and LookAhead sync
    steps (the first, at t = 5 x 2 with the slow weights made, and RMSprop's)."""
    from torch_scae_amd import _lib
    g = torch.Generator().manual_seed(11)
    n = 20011
    st = P(torch.cuda.current_stream().cuda_stream)

    def fresh():
        gg = torch.Generator().manual_seed(5)
        return [torch.randn(n, generator=gg).cuda() for _ in range(2)] + \
            [torch.randn(n, generator=gg).cuda() * .1, torch.rand(n, generator=gg).cuda(),
             torch.randn(n, generator=gg).cuda()]
    partials = [torch.randn(22, 9 * 40, generator=g).cuda(),
                torch.randn(128, 5 * 12, generator=g).cuda(),
                torch.randn(7, 333, generator=g).cuda(),
                torch.randn(300, 6, generator=g).cuda()]
    layout = [(1, [(0, 360, -40, 360)]),
              (3001, [(0, 5, 12, 50), (5, 12, 12, 70)]),
              (7002, [(0, 100, 0, 100), (120, 333, 0, 213)]),
              (19990, [(0, 6, 0, 6)])]
    lr_dev = torch.full((1,), 1e-3, device="cuda")
    results = []
    for fused in (False, True):
        param, grad, m, v, slow = fresh()
        state = torch.zeros(_lib.FLAT_OPT_STATE_INTS, dtype=torch.int32, device="cuda")
        state[:2] = torch.tensor([t, int(la)], dtype=torch.int32)
        keep, jobs = [], (_lib.SumJob * len(partials))()
        for job, part, (off, segs) in zip(jobs, partials, layout):
            arr = (_lib.SumSegment * len(segs))()
            pos = off
            for a, (b, e, per, length) in zip(arr, segs):
                a.dst, a.begin, a.end, a.period = grad.data_ptr() + 4 * pos, b, e, per
                pos += length
            keep.append(arr)
            job.src, job.rows, job.cols = part.data_ptr(), part.shape[0], part.shape[1]
            job.segments, job.n_segments = arr, len(segs)
        args = (P(param.data_ptr()), P(grad.data_ptr()), P(m.data_ptr()), P(v.data_ptr()),
                P(slow.data_ptr()), n, P(lr_dev.data_ptr()), P(state.data_ptr()), KIND[kind],
                *BETAS[kind], 1e-4)
        la_args = (5 if la else 0, 0.5)
        if fused:
            _lib.call("scae_flat_opt_sums_step_f32", *args, 1.0, *la_args, jobs,
                      len(partials), st)
        else:
            _lib.call("scae_sum_rows_multi_f32", jobs, len(partials), st)
            _lib.call("scae_flat_opt_step_f32", *args, 0.0, 1.0, *la_args, 1, st)
        torch.cuda.synchronize()
        results.append([x.clone() for x in (param, grad, m, v, slow, state)])
    for a, b, what in zip(results[0], results[1], ("param", "grad", "m", "v", "slow", "state")):
        bad = (a != b).nonzero().flatten()
        assert bad.numel() == 0, (what, bad[:8].tolist(), bad.numel())
    assert results[1][5][:2].tolist() == [t + 1, int(la)]
    assert int(results[1][5][2:].abs().sum()) == 0
    assert float((results[0][0] - fresh()[0]).abs().max()) > 0
    if la and (t + 1) % 5 == 0:      # a real sync: the fast weights are the slow ones
        assert torch.equal(results[1][0], results[1][4])


SMALL = dict(image_shape=(1, 16, 16), n_classes=4, n_part_caps=5, n_obj_caps=4,
             pcae_cnn_encoder_params=dict(out_channels=[64, 64], kernel_sizes=[3, 3],
                                          strides=[2, 1]),
             pcae_template_generator_params=dict(template_size=(5, 5)),
             ocae_encoder_set_transformer_params=dict(dim_hidden=8, dim_out=64, n_layers=2),
             ocae_decoder_capsule_params=dict(dim_caps=4, hidden_sizes=(8,)),
             scae_params=dict(reconstruct_alternatives=False))


def small_step(noise=True, seed=3, **kw):
    from torch_scae_amd import factory, ops
    from torch_scae_amd.train_step import TrainStep
    np.random.seed(seed)
    torch.manual_seed(seed)
    ops.reset_noise()
    model = factory.make_scae(SMALL)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    model = model.cuda().train()
    if not noise:
        model.part_encoder.noise_scale = 0.
        model.obj_decoder.capsule_layer.noise_type = None
    return model, TrainStep(model, 8, (1, 16, 16), **kw)


def batches(n, seed=9):
    from torch_scae_amd.data import stroke_batches
    imgs, labels = stroke_batches(n, 8, (1, 16, 16), seed=seed, n_classes=4)
    return [(imgs[i].cuda(), labels[i].cuda()) for i in range(n)]


def mirror(kind, flat_param, la):
    """The CPU side of a replayed run: stock torch.optim.Adam, or the CPU RAdamFlat with
    LookAhead (held to the reference's RAdam / LookAhead by test_optimizers.py), over ONE
    tensor of the whole flat buffer."""
    import torch.nn as nn
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    eps = 1e-2 / 8.0 ** 2
    if kind == "adam" and not la:
        p = flat_param.detach().cpu().clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=1e-3, eps=eps)

        def step(grad, ours):
            with torch.no_grad():
                p.copy_(ours)
            p.grad = grad
            opt.step()
            return p.detach()
        return step
    mod = nn.Module()
    mod.w = nn.Parameter(flat_param.detach().cpu().clone())
    flat = FlatParameters(mod)
    opt = make_optimizer(kind, flat, lr=1e-3, eps=eps, look_ahead=la)

    def step(grad, ours):
        flat.flat_param.copy_(ours)
        flat.flat_grad.copy_(grad)
        opt.step()
        return flat.flat_param
    return step


@pytest.mark.parametrize("kind,la", [("adam", False), ("radam", True)])
def test_step_count_follows_replays(kind, la):
    """TrainStep(optimizer=kind) captured once, then 20 graph replays and 20 launch-list
    replays of the same capture: after every replay the device step count equals the
    steps taken, and the parameters equal the CPU optimiser (stock torch.optim.Adam; the
    reference-checked CPU RAdam + LookAhead) stepped on that replay's own flat gradient
    from the same parameters, its moments carried along -- to the bars of the kernel
    test.  A count frozen at capture fails from the second step on (bias corrections,
    RAdam's regime, LookAhead's syncs at 5, 10, ...)."""
    data = batches(40)
    for replay in ("graph", "launches"):
        model, step = small_step(lr=1e-3, optimizer=kind, look_ahead=la, replay=replay)
        step.capture()
        cpu = mirror(kind, step.flat.flat_param, la)
        for i in range(20):
            before = step.flat.flat_param.cpu()
            step(*data[i + (20 if replay == "launches" else 0)])
            torch.cuda.synchronize()
            assert int(step.opt.step_state[0]) == i + 1 == step.steps, (replay, i)
            ref = cpu(step.flat.flat_grad.cpu(), before).double().numpy()
            ours = step.flat.flat_param.cpu().double().numpy()
            upd = np.abs(ref - before.double().numpy()).max()
            err = (np.abs(ours - ref) - ulp(ref)).max()
            assert upd > 0 and err <= 1e-5 * upd, (replay, i, err, upd)
        if replay == "launches":
            assert step._klist, "the step did not replay as a launch list"


def test_parameters_without_gradient_stay_bitwise_untouched():
    """20 Adam replays: every parameter whose gradient slot stayed zero throughout is
    bitwise what it was (torch.optim skips a parameter whose grad is None)."""
    model, step = small_step(lr=1e-3, optimizer="adam")
    step.capture()
    flat = step.flat
    start = flat.flat_param.clone()
    touched = torch.zeros_like(flat.flat_grad, dtype=torch.bool)
    for img, lab in batches(20):
        step(img, lab)
        touched |= flat.flat_grad != 0
    torch.cuda.synchronize()
    idle = [(p, off) for p, off in zip(flat.params, flat.offsets)
            if not bool(touched[off:off + p.numel()].any())]
    assert idle, "every parameter got a gradient: nothing to check"
    for p, off in idle:
        assert torch.equal(flat.flat_param[off:off + p.numel()], start[off:off + p.numel()])
    assert not torch.equal(flat.flat_param, start)


@pytest.mark.parametrize("kind,la", [("adam", False), ("radam", True)])
def test_restore_replays_from_the_restored_step_count(kind, la):
    """snapshot() at t = 7, 5 more steps, restore(), the same 5 batches again under the
    same captured graph: bitwise the first run (the count, the moments and the slow
    weights -- made at t = 5 -- come back with the parameters)."""
    data = batches(12)
    model, step = small_step(noise=False, lr=1e-3, optimizer=kind, look_ahead=la)
    step.capture()
    for img, lab in data[:7]:
        step(img, lab)
    snap = step.snapshot()
    assert int(snap["step_state"][0]) == 7
    runs = []
    for _ in range(2):
        for img, lab in data[7:]:
            step(img, lab)
        torch.cuda.synchronize()
        runs.append((step.flat.flat_param.clone(), step.opt.exp_avg.clone(),
                     step.opt.step_state.clone()))
        step.restore(snap)
    assert runs[0][2].tolist()[0] == 12
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_in_graph_collective_with_adam_equals_the_plain_step(nccl_group):
    """The 1-rank "in graph" collective mode (all-reduce and the Adam pass captured in
    the one graph) ends on exactly the parameters of the collective-free step; so do the
    "1 bucket" and "2 buckets" modes, where Adam runs after the replay."""
    data = batches(3)
    outs = []
    for kw in (dict(), dict(force_collective=True, collective_mode="in graph"),
               dict(force_collective=True, overlap=False),
               dict(force_collective=True)):
        model, step = small_step(noise=False, lr=1e-3, optimizer="adam", **kw)
        for img, lab in data:
            step(img, lab)
        torch.cuda.synchronize()
        assert int(step.opt.step_state[0]) == 3
        outs.append((kw, {k: v.clone() for k, v in model.state_dict().items()}))
    # (two buckets lay the flat buffers out in another order: compared by name)
    assert outs[1][0] and step.collective and step.split
    for kw, sd in outs[1:]:
        for k, v in sd.items():
            assert torch.equal(outs[0][1][k], v), (kw, k)


def test_rmsprop_form_with_a_step_count_equals_the_rmsprop_pass_bitwise():
    """kind 2 of scae_flat_opt_step_f32 (RMSprop as LookAhead wraps it) is
    scae_rmsprop_step_f32's arithmetic: with LookAhead off, bit for bit the same
    parameters and moments, with and without weight decay, at an odd start."""
    from torch_scae_amd import _lib
    n = 10007
    st = P(torch.cuda.current_stream().cuda_stream)
    lr_dev = torch.full((1,), 1e-3, device="cuda")
    for wd in (0.0, 1e-2):
        outs = []
        for fused in (False, True):
            gg = torch.Generator().manual_seed(6)
            p, g, b = (torch.randn(n + 1, generator=gg).cuda() for _ in range(3))
            v = torch.rand(n + 1, generator=gg).cuda()
            state = torch.zeros(_lib.FLAT_OPT_STATE_INTS, dtype=torch.int32, device="cuda")
            ptr = lambda t: P(t.data_ptr() + 4)   # noqa: E731
            for _ in range(3):
                if fused:
                    _lib.call("scae_flat_opt_step_f32", ptr(p), ptr(g), ptr(b), ptr(v), None,
                              n, P(lr_dev.data_ptr()), P(state.data_ptr()), 2, 0.9, 0.99, 1e-4,
                              wd, 0.5, 0, 0.5, 1, st)
                else:
                    _lib.call("scae_rmsprop_step_f32", ptr(p), ptr(g), ptr(v), ptr(b), n, 1e-3,
                              P(lr_dev.data_ptr()), 0.99, 1e-4, 0.9, wd, 0.5, st)
            torch.cuda.synchronize()
            outs.append((p, v, b))
        assert int(state[0]) == 3
        for x, y in zip(*outs):
            assert torch.equal(x, y), wd
