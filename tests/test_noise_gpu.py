"""The device noise generator (csrc/noise.hip, csrc/noise_dev.h, the same device code in
csrc/step_prologue.hip, ops.uniform) bit for bit against a host Philox4x32-10
(tests/philox_ref.py, itself held to the published vectors by tests/test_philox_ref.py):
every draw size from one float to three passes of the capped grid, seeds and launch counters
with live high words, graph and launch-list replay, the prologue launch in each of its forms,
who gets which slice of a step's draw, and which (seed, launch) stream each plan of a run
consumes.  Every comparison is equality of bits (int32 views)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import philox_ref as R
from tests.philox_ref import effective_seed, first_difference, same_bits, uniform_ref

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
CFG2_N = 128 * 24 + 128 * 24 + 128 * 24 * 24     # cfg-2's training draw


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _check(got, seed, launch, n, what=""):
    torch.cuda.synchronize()
    assert got.numel() == n and got.dtype == torch.float32, (what, got.shape, got.dtype)
    want = uniform_ref(seed, launch, n)
    assert same_bits(got, want), (what, seed, launch, n, first_difference(got, want))


def _state_of(plan, stream=None):
    """The generator state tensor ``plan`` keeps for ``stream`` (default: the current one)."""
    handle = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    found = [st for (_, s), (_, st) in plan.noise.items() if s == handle]
    assert len(found) == 1, (plan.name, len(found))
    return found[0]


def _read(state):
    torch.cuda.synchronize()
    assert state.dtype == torch.int64 and state.shape == (3,)
    return state.cpu().tolist()


def _seed_all(seed):
    from torch_scae_amd import ops
    torch.manual_seed(seed)
    ops.reset_noise()
    assert int(torch.initial_seed()) == seed


class NoiseLaunches:
    """Counts, per generator state (its address), the host's successful calls of the entry
    points that draw noise: ``eager`` the ones that ran, ``captured`` the ones issued into a
    stream capture (they run once per replay of that graph)."""
    # entry point -> positions of (n_noise, noise_state) among its arguments
    WHERE = {"scae_uniform_f32": (1, 2), "scae_step_prologue_f32": (7, 8),
             "scae_step_prologue_first_f32": (7, 8), "scae_step_prologue_source_f32": (5, 6)}

    def __enter__(self):
        from torch_scae_amd import _lib
        self.lib, self.saved = _lib.load(), {}
        self.eager, self.captured = {}, {}
        for name, (n_at, st_at) in self.WHERE.items():
            self.saved[name] = getattr(self.lib, name)
            setattr(self.lib, name, self._counted(self.saved[name], n_at, st_at))
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)
        return False

    def _counted(self, fn, n_at, st_at):
        def counted(*args):
            rc = fn(*args)
            n, st = args[n_at], args[st_at]
            n = n.value if hasattr(n, "value") else n
            if rc == 0 and n and st is not None:
                where = self.captured if torch.cuda.is_current_stream_capturing() \
                    else self.eager
                where[st.value] = where.get(st.value, 0) + 1
            return rc
        counted.__name__ = getattr(fn, "__name__", "counted")
        return counted

    def of(self, state):
        assert self.captured.get(state.data_ptr(), 0) == 0, "a noise draw inside a capture"
        return self.eager.get(state.data_ptr(), 0)


# == 2a. sizes ====
@pytest.mark.parametrize("n", R.DRAW_SIZES)
def test_uniform_equals_the_reference_at_each_size(n):
    """ops.uniform's first two draws of n floats after a reset, and the launcher writing into
    the middle of a buffer: n floats at an odd float offset, every float around them
    untouched."""
    from torch_scae_amd import _lib, ops, step_plan
    ref = torch.zeros(1, device="cuda")
    _seed_all(1234)
    a = ops.uniform(n, ref)
    b = ops.uniform(n, ref)
    assert a.shape == (n,) and a.data_ptr() != b.data_ptr()
    _check(a, 1234, 0, n, "first draw")
    _check(b, 1234, 1, n, "second draw")
    assert _read(_state_of(step_plan.ambient)) == [1234, 2, 0]
    seed, launch, lo = (7 << 32) + 5, 9, 3
    state = torch.tensor([seed, launch, 0], dtype=torch.int64).cuda()
    guard = np.float32(-7.5)
    buf = torch.full((n + 16,), float(guard), device="cuda")
    _lib.call("scae_uniform_f32", P(buf.data_ptr() + 4 * lo), n, P(state.data_ptr()), _stream())
    _check(buf[lo:lo + n], seed, launch, n, "into the middle of a buffer")
    around = torch.cat([buf[:lo], buf[lo + n:]])
    assert same_bits(around, np.full(16, guard, np.float32)), "wrote outside its n floats"
    assert _read(state) == [seed, launch + 1, 0]


# == 2b. seeds and counters ====
@pytest.mark.parametrize("salt", [0, R.NOISE_SALT])
@pytest.mark.parametrize("seed", R.SEEDS)
def test_seeds_salts_and_consecutive_launches(seed, salt):
    """torch.manual_seed(seed) + reset_noise: draw k comes from launch k of seed ^ salt (the
    key's high word live from 2^32 on), and after k draws the state reads [seed ^ salt, k, 0]."""
    from torch_scae_amd import ops, step_plan
    ref = torch.zeros(1, device="cuda")
    plan = ops.StepPlan("noise test") if salt else step_plan.ambient
    plan.noise_salt = salt
    eff = effective_seed(seed, salt)
    assert eff == (seed ^ salt) and (salt == 0 or eff >> 32)
    _seed_all(seed)
    with plan.active():
        for k, n in enumerate([5, 1025, 79872, 3, 4096]):
            out = ops.uniform(n, ref)
            _check(out, eff, k, n, f"draw {k}")
            assert _read(_state_of(plan)) == [eff, k + 1, 0]
        # the same seed set again restarts the stream, in the same state tensor
        state = _state_of(plan)
        _seed_all(seed)
        assert _state_of(plan) is state and _read(state) == [eff, 0, 0]
        _check(ops.uniform(1023, ref), eff, 0, 1023, "after the reset")


@pytest.mark.parametrize("seed", [1234, 2 ** 63 - 1])
def test_the_launch_counter_carries_into_its_high_word(seed):
    from torch_scae_amd import ops, step_plan
    ref = torch.zeros(1, device="cuda")
    _seed_all(seed)
    ops.uniform(4, ref)
    state = _state_of(step_plan.ambient)
    state[1] = R.CARRY_LAUNCHES[0]
    for launch in R.CARRY_LAUNCHES:
        for n in (5, 1025):
            state[1] = launch
            _check(ops.uniform(n, ref), seed, launch, n, "written counter")
            assert _read(state) == [seed, launch + 1, 0]
    state[1] = 2 ** 32 - 1              # two draws across the carry, nothing written between
    a, b = ops.uniform(1025, ref), ops.uniform(1025, ref)
    _check(a, seed, 2 ** 32 - 1, 1025, "before the carry")
    _check(b, seed, 2 ** 32, 1025, "after the carry")
    assert _read(state) == [seed, 2 ** 32 + 1, 0]
    _seed_all(seed)
    assert _read(state) == [seed, 0, 0]


# == 2c. replay ====
REPLAY_SIZES = [300 * 1024 + 7, R.PASS + 5 * 1024 + 3]      # 301 workgroups; above the grid cap


@pytest.mark.parametrize("n", REPLAY_SIZES)
def test_graph_replay_draws_consecutive_launches(n):
    from torch_scae_amd import ops, step_plan
    ref = torch.zeros(1, device="cuda")
    seed = (3 << 32) + 77
    _seed_all(seed)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm = ops.uniform(1000, ref)            # creates the stream's state
    torch.cuda.current_stream().wait_stream(s)
    state = _state_of(step_plan.ambient, s)
    _check(warm, seed, 0, 1000, "warm-up")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        out = ops.uniform(n, ref)
    L0 = _read(state)[1]
    assert L0 == 1                               # the warm-up; the capture ran nothing
    for i in range(6):
        g.replay()
        _check(out, seed, L0 + i, n, f"replay {i}")
    assert _read(state) == [seed, L0 + 6, 0]


@pytest.mark.parametrize("n", REPLAY_SIZES)
def test_launch_list_replay_draws_consecutive_launches(n):
    from torch_scae_amd import _lib
    lib = _lib.load()
    seed, first = (1 << 40) + 9, 2 ** 32 - 3     # (the replays cross the counter's carry)
    state = torch.tensor([seed, first, 0], dtype=torch.int64).cuda()
    out = torch.zeros(n, device="cuda")
    torch.cuda.synchronize()
    st = _stream()
    lst = lib.scae_launch_list_begin(st)
    assert lst
    try:
        _lib.call("scae_uniform_f32", P(out.data_ptr()), n, P(state.data_ptr()), st)
        assert lib.scae_launch_list_end(P(lst)) == 0
        assert lib.scae_launch_list_size(P(lst)) == 1
        _check(out, seed, first, n, "the recorded launch itself")
        L0 = _read(state)[1]
        assert L0 == first + 1
        side = torch.cuda.Stream()
        for i in range(6):
            out.zero_()
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                assert lib.scae_launch_list_run(P(lst), P(side.cuda_stream)) == 0
            side.synchronize()
            _check(out, seed, L0 + i, n, f"replay {i}")
        assert _read(state) == [seed, L0 + 6, 0]
    finally:
        lib.scae_launch_list_free(P(lst))


# == 2d. the prologue form ====
@pytest.mark.parametrize("n", [5, CFG2_N, R.PASS + 1029])
def test_prologue_launch_with_the_noise_alone(n):
    from torch_scae_amd import ops
    ref = torch.zeros(1, device="cuda")
    seed = 2 ** 32 + 11
    _seed_all(seed)
    pro = ops.StepPrologue()
    with NoiseLaunches() as count, ops.step_prologue(pro):
        first = ops.uniform(n, ref)              # establishes the buffer, launches itself
        state = pro.noise_state
        _check(first, seed, 0, n, "the establishing draw")
        for k in (1, 2, 3):
            pro.launch()
            assert pro.noise_fresh
            _check(pro.noise, seed, k, n, f"prologue launch {k}")
            assert _read(state) == [seed, k + 1, 0]
            got = ops.uniform(n, ref)            # no launch: the prologue's draw
            assert got.data_ptr() == pro.noise.data_ptr() and _read(state)[1] == k + 1
        assert count.of(state) == 4
        again = ops.uniform(n, ref)              # consumed: launches itself
        _check(again, seed, 4, n, "a second forward without a prologue launch")
        assert _read(state) == [seed, 5, 0] and count.of(state) == 5


@pytest.mark.parametrize("C0", [1, 3])
def test_prologue_launch_with_fold_image_layer_and_staging(C0):
    """One launch carrying all four parts (the noise workgroups are a block range behind the
    folding products' and the image layer's): the noise is the standalone launch's for the
    same (seed, launch), the state advances by one, and the other parts are what their own
    launches give."""
    from torch_scae_amd import ops
    g = torch.Generator().manual_seed(5 + C0)
    O, C, D = 24, 256, 16
    shapes = [(O, C), (C, C), (C,), (C, C), (C,), (C, C), (C,), (C, C), (C,), (C, D), (C,)]
    vals = [(torch.randn(*s, generator=g) / (s[-1] ** 0.5)).cuda() for s in shapes]
    B, H = 16, 20
    chans, strides = [C0, 64, 128, 64], (2, 1, 1)
    ws = [(torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5)).cuda()
          for ci, co in zip(chans[:-1], chans[1:])]
    bs = [(0.1 * torch.randn(co, generator=g)).cuda() for co in chans[1:]]
    batches = [torch.rand(B, C0, H, H, generator=g).cuda() for _ in range(3)]
    labels = [torch.randint(0, 10, (B,), generator=g).cuda() for _ in range(3)]
    ref_fold = [t.clone() for t in ops.seed_fold(*vals)]
    ref_y = [ops.conv_stack(x, ws, bs, strides).clone() for x in batches]
    resident, rl = torch.zeros_like(batches[0]), torch.zeros_like(labels[0])
    n, seed = CFG2_N, 2 ** 63 - 1
    _seed_all(seed)
    pro = ops.StepPrologue()
    pro.fold_conv_ok = False            # the folding products stay in the prologue launch
    with NoiseLaunches() as count, ops.step_prologue(pro):
        resident.copy_(batches[0])
        _check(ops.uniform(n, resident), seed, 0, n, "the establishing draw")
        ops.seed_fold(*vals)
        assert torch.equal(ops.conv_stack(resident, ws, bs, strides), ref_y[0])
        state = pro.noise_state
        for k in (1, 2):
            pro.noise.fill_(-1.0)
            for t in pro.fold_outs:
                t.fill_(float("nan"))
            pro.launch(resident, batches[k], rl, labels[k])
            assert pro.noise_fresh and pro.fold_fresh and pro.first_fresh
            _check(pro.noise, seed, k, n, f"prologue launch {k}")
            assert _read(state) == [seed, k + 1, 0] and count.of(state) == k + 1
            assert torch.equal(resident, batches[k]) and torch.equal(rl, labels[k])
            for a, b in zip(ops.seed_fold(*vals), ref_fold):
                assert torch.equal(a, b)
            assert torch.equal(ops.conv_stack(resident, ws, bs, strides), ref_y[k])
            assert not pro.first_fresh and not pro.fold_fresh
            assert ops.uniform(n, resident).data_ptr() == pro.noise.data_ptr()
            assert count.of(state) == k + 1


def test_prologue_launch_from_a_batch_source():
    """scae_step_prologue_source_f32: the hand-over gathers from a resident dataset (one
    workgroup per image behind the noise's block range), the image layer reads the dataset."""
    from torch_scae_amd import ops
    from tests.test_train_remainder_gpu import _dataset
    g = torch.Generator().manual_seed(17)
    B, n, seed = 48, 3 * 1024 + 5, 2 ** 32 - 1
    ds = _dataset(300)
    view = ds.view(shuffle=True, translate=True, seed=77)
    chans, strides = [1, 64, 128], (2, 1)
    ws = [(torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5)).cuda()
          for ci, co in zip(chans[:-1], chans[1:])]
    bs = [(0.1 * torch.randn(co, generator=g)).cuda() for co in chans[1:]]
    want = [view.batch(0, k, B) for k in range(3)]
    ref_y = [ops.conv_stack(x.cuda(), ws, bs, strides).clone() for x, _ in want]
    di = torch.zeros(B, 1, 40, 40, device="cuda")
    dl = torch.zeros(B, dtype=torch.int64, device="cuda")
    _seed_all(seed)
    for with_layer in (False, True):
        pro = ops.StepPrologue()
        with NoiseLaunches() as count, ops.step_prologue(pro):
            L = 0 if not with_layer else 4
            _check(ops.uniform(n, di), seed, L, n, "the establishing draw")
            state = pro.noise_state
            if with_layer:
                di.copy_(want[0][0])
                assert torch.equal(ops.conv_stack(di, ws, bs, strides), ref_y[0])
            for k in range(3):
                pro.launch(di, None, dl, source=view.desc(0, k * B))
                assert pro.noise_fresh and pro.first_fresh == with_layer
                _check(pro.noise, seed, L + 1 + k, n, f"source launch {k}")
                assert _read(state) == [seed, L + 2 + k, 0] and count.of(state) == 2 + k
                assert torch.equal(di.cpu(), want[k][0]) and torch.equal(dl.cpu(), want[k][1])
                if with_layer:
                    assert torch.equal(ops.conv_stack(di, ws, bs, strides), ref_y[k])


# == 2e. who gets which numbers ====
def test_draw_noise_hands_out_consecutive_slices_of_one_draw():
    from torch_scae_amd import factory
    from tests.test_hip_model import FULL
    cfg, B = FULL["cfg2"]
    M, Oc = cfg["n_part_caps"], cfg["n_obj_caps"]
    model = factory.make_scae(cfg).cuda().train()
    image = torch.rand(B, *cfg["image_shape"]).cuda()
    seed = 2 ** 32 + 1234
    _seed_all(seed)
    shapes = [(B, M), (B, Oc, 1), (B, Oc, M)]
    sizes = [int(np.prod(s)) for s in shapes]
    assert sum(sizes) == CFG2_N
    for launch in (0, 1):
        got = model._draw_noise(image)
        flat = uniform_ref(seed, launch, sum(sizes))
        assert [tuple(t.shape) for t in got] == shapes
        for t, want in zip(got, np.split(flat, np.cumsum(sizes)[:-1])):
            assert same_bits(t, want), (launch, tuple(t.shape), first_difference(t, want))
    # a part encoder in eval() inside a training SCAE draws nothing: the capsule layer's two
    # tensors then start the stream
    model.part_encoder.eval()
    got = model._draw_noise(image)
    flat = uniform_ref(seed, 2, sum(sizes[1:]))
    assert [tuple(t.shape) for t in got] == shapes[1:]
    for t, want in zip(got, np.split(flat, [sizes[1]])):
        assert same_bits(t, want), (tuple(t.shape), first_difference(t, want))
    assert same_bits(got[0], uniform_ref(seed, 2, sum(sizes))[:sizes[1]])


# == 3. the streams of a run ====
def _noise_of(step):
    pro = step.plan.prologue
    assert pro is not None and pro.noise is not None and pro.noise_state is not None
    return pro.noise, pro.noise_state


RUN_SEED = (5 << 32) + 17
FORMS = {"eager": dict(use_graph=False), "graph": dict(), "launches": dict(replay="launches")}


@pytest.mark.parametrize("form", list(FORMS))
def test_train_step_consumes_one_stream_without_gap_or_repeat(form):
    """Step i of a cfg-2 TrainStep holds uniform_ref(seed, i0 + i, n): i0 is what the build
    (warm-ups, capture, refreshes) consumed -- read from the state and equal to the number of
    noise launches the host has made on that state."""
    from tests.test_grad_clip_gpu import _cfg2_batches, _cfg2_step
    with NoiseLaunches() as count:
        step = _cfg2_step(**FORMS[form])
        _seed_all(RUN_SEED)                      # (before the first draw: the key's high word live)
        seed = effective_seed(RUN_SEED)
        batches = _cfg2_batches(9)
        step(*batches[0])                        # builds the step
        noise, state = _noise_of(step)
        n = noise.numel()
        assert n == CFG2_N
        if form == "launches":
            assert step._klist, step.graph_nodes
        elif form == "graph":
            assert step.graph is not None and not step._klist
        i0 = _read(state)[1]
        assert _read(state) == [seed, i0, 0] and i0 == count.of(state) and i0 >= 1
        _check(noise, seed, i0 - 1, n, "the building step")
        for i in range(8):
            step(*batches[1 + i])
            assert _noise_of(step)[0].data_ptr() == noise.data_ptr()
            _check(noise, seed, i0 + i, n, f"{form} step {i}")
            assert _read(state) == [seed, i0 + i + 1, 0]
        assert count.of(state) == i0 + 8


def test_accumulate_and_update_forms_share_one_counter():
    from tests.test_grad_clip_gpu import _cfg2_batches, _cfg2_step
    with NoiseLaunches() as count:
        step = _cfg2_step(accumulate_grad_batches=2)
        _seed_all(RUN_SEED)
        seed = effective_seed(RUN_SEED)
        batches = _cfg2_batches(8)
        for x, y in batches[:2]:                 # captures the accumulate form, then the update
            step(x, y)
            noise, state = _noise_of(step)
            _check(noise, seed, _read(state)[1] - 1, CFG2_N, "a capturing batch")
        assert step._other_cap is not None and step._other_cap.graph is not None
        assert len(step.plan.noise) == 1         # one generator state for both forms
        i0 = _read(state)[1]
        assert i0 == count.of(state)
        forms = []
        for i, (x, y) in enumerate(batches[2:]):
            step(x, y)
            forms.append(step._form)
            assert _noise_of(step)[1] is state
            _check(_noise_of(step)[0], seed, i0 + i, CFG2_N, f"batch {i} ({step._form})")
            assert _read(state) == [seed, i0 + i + 1, 0]
        assert forms == ["acc", "update"] * 3 and step.optimizer_steps == 4
        assert count.of(state) == i0 + 6


@pytest.fixture(scope="module")
def run():
    """A cfg-2 training step with its remainder step (batch 40), and an evaluation step on the
    same model with its tail step, all built and captured under one launch count."""
    from torch_scae_amd import EvalStep
    from tests.test_grad_clip_gpu import _cfg2_batches, _cfg2_step
    with NoiseLaunches() as count:
        step = _cfg2_step()
        _seed_all(RUN_SEED)
        batches = _cfg2_batches(6)
        step(*batches[0])
        step(batches[1][0][:40].contiguous(), batches[1][1][:40].contiguous())
        ev = EvalStep(step.model, 128, (1, 40, 40))
        images = torch.cat([b[0] for b in batches[:2]])[:128 + 40].contiguous()
        labels = torch.cat([b[1] for b in batches[:2]])[:128 + 40].contiguous()
        ev.evaluate(images, labels)
        # every plan's counter stands at the number of noise launches made on its state
        for s in (step, step._rem, ev, ev._tail_step):
            state = _noise_of(s)[1]
            assert _read(state)[1:] == [count.of(state), 0] and count.of(state) >= 1, s.plan.name
    yield dict(step=step, rem=step._rem, ev=ev, tail=ev._tail_step, batches=batches,
               split=(images, labels))


def _short(batch, b=40):
    return batch[0][:b].contiguous(), batch[1][:b].contiguous()


def test_remainder_step_draws_its_own_salted_stream(run):
    from torch_scae_amd.train_step import REMAINDER_NOISE_SALT
    step, rem, batches = run["step"], run["rem"], run["batches"]
    assert rem is not None and rem.image.shape[0] == 40 and rem.plan is not step.plan
    assert rem.plan.noise_salt == REMAINDER_NOISE_SALT != 0
    torch_seed = int(torch.initial_seed())
    seed, rseed = effective_seed(torch_seed), effective_seed(torch_seed, REMAINDER_NOISE_SALT)
    (noise, state), (rnoise, rstate) = _noise_of(step), _noise_of(rem)
    assert state is not rstate and noise.data_ptr() != rnoise.data_ptr()
    n_rem = 40 * (24 + 24 + 24 * 24)
    assert rnoise.numel() == n_rem and noise.numel() == CFG2_N
    for _ in range(2):
        full, j = _read(state), _read(rstate)[1]
        assert full[::2] == [seed, 0]
        step(*_short(batches[2]))
        assert step._rem is rem
        _check(_noise_of(rem)[0], rseed, j, n_rem, "remainder step")
        assert _read(rstate) == [rseed, j + 1, 0]
        assert _read(state) == full, "the remainder step moved the full step's counter"
        rfull = _read(rstate)
        step(*batches[3])
        _check(noise, seed, full[1], CFG2_N, "full step after a remainder step")
        assert _read(state) == [seed, full[1] + 1, 0]
        assert _read(rstate) == rfull, "the full step moved the remainder step's counter"


def test_reset_noise_restarts_every_live_plan_in_place(run):
    from torch_scae_amd.eval_step import EVAL_NOISE_SALT, EVAL_TAIL_NOISE_SALT
    from torch_scae_amd.train_step import REMAINDER_NOISE_SALT
    step, rem, ev, tail, batches = (run[k] for k in ("step", "rem", "ev", "tail", "batches"))
    steps = [(step, 0), (rem, REMAINDER_NOISE_SALT), (ev, EVAL_NOISE_SALT),
             (tail, EVAL_TAIL_NOISE_SALT)]
    graphs = [s.graph for s, _ in steps]
    states = [_noise_of(s)[1] for s, _ in steps]
    assert all(g is not None for g in graphs)
    for torch_seed in (2 ** 32 + 99, 4321):
        _seed_all(torch_seed)
        for (s, salt), st in zip(steps, states):
            assert s.plan.noise_salt == salt
            assert _noise_of(s)[1] is st and _read(st) == [effective_seed(torch_seed, salt), 0, 0]
        # the captured steps keep working, from launch 0 of their own seeds
        for launch in (0, 1):
            step(*batches[4])
            _check(_noise_of(step)[0], effective_seed(torch_seed), launch, CFG2_N, "full")
            step(*_short(batches[5]))
            _check(_noise_of(rem)[0], effective_seed(torch_seed, REMAINDER_NOISE_SALT), launch,
                   rem.image.shape[0] * 624, "remainder")
            ev(*batches[4])
            _check(_noise_of(ev)[0], effective_seed(torch_seed, EVAL_NOISE_SALT), launch,
                   128 * (24 + 576), "evaluation")
            tail(*_short(batches[5]))
            _check(_noise_of(tail)[0], effective_seed(torch_seed, EVAL_TAIL_NOISE_SALT), launch,
                   40 * (24 + 576), "evaluation tail")
        assert [s.graph for s, _ in steps] == graphs and step._rem is rem
        assert [_read(st)[1:] for st in states] == [[2, 0]] * 4


def test_plans_under_one_torch_seed_consume_disjoint_streams(run):
    """Every (effective seed, launch) pair is drawn by at most one plan: over a short run from
    a common restart the training step, its remainder step, an evaluation step on the same
    model and its tail step each read the stream the reference gives for their own pair,
    the pairs are pairwise disjoint, and no two buffers start with the same floats."""
    step, rem, ev, tail, batches = (run[k] for k in ("step", "rem", "ev", "tail", "batches"))
    images, labels = run["split"]
    names = ["train", "remainder", "eval", "eval tail"]
    plans = [step, rem, ev, tail]
    torch_seed = 2 ** 40 + 5
    _seed_all(torch_seed)
    consumed = {k: set() for k in names}
    heads = {}

    def note(name, s):
        noise, state = _noise_of(s)
        eff, launches, arrivals = _read(state)
        assert eff == effective_seed(torch_seed, s.plan.noise_salt) and arrivals == 0
        _check(noise, eff, launches - 1, noise.numel(), name)
        assert (eff, launches - 1) not in consumed[name], "a stream drawn twice"
        consumed[name].add((eff, launches - 1))
        heads[name, launches - 1] = noise[:1024].clone()

    for i in range(3):
        step(*batches[i])
        note("train", step)
        step(*_short(batches[i + 1]))
        note("remainder", rem)
        ev(*batches[i])                           # validation batch i next to training step i
        note("eval", ev)
        tail(*_short(batches[i]))
        note("eval tail", tail)
    ev.evaluate(images, labels)                   # one full batch, one tail batch
    note("eval", ev)
    note("eval tail", tail)
    assert [len(consumed[k]) for k in names] == [3, 3, 4, 4]
    for a in range(4):
        for b in range(a + 1, 4):
            both = consumed[names[a]] & consumed[names[b]]
            assert not both, (names[a], names[b], sorted(both))
    keys = list(heads)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            assert not same_bits(heads[keys[a]], heads[keys[b]]), (keys[a], keys[b])
    assert len({s.plan.noise_salt for s in plans}) == 4
