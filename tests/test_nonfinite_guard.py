"""The non-finite guard (``nonfinite="skip" | "raise"``: an optimiser step whose gradient holds
a NaN or Inf element writes nothing and is counted) without a GPU: the settings' parsing and
factory.make_train_step's reading of ``trainer.terminate_on_nan`` / ``trainer.nonfinite``, the
flat optimisers' CPU forms -- bit for bit the unguarded ones on finite gradients, untouched on
a poisoned one --, ``TrainStep(nonfinite="raise")``'s check in ``end_epoch`` and two gloo ranks
that take the same decision after the all-reduce.  The guard has no device form yet (asking
for it on a HIP device raises).  Every comparison is bit for bit."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_data_parallel import _free_port
from tests.test_grad_clip import Net, batch
from tests.test_optimizers import REF_CFG, YAML

NAN, INF = float("nan"), float("inf")
KINDS = ("rmsprop", "adam", "radam")
CLIP = 0.5       # below every step's norm of test_grad_clip.py's Net: the coefficient is < 1


# -- 1. the settings -------------------------------------------------------------------------
def test_nonfinite_values_parse():
    from torch_scae_amd.data_parallel import nonfinite_value
    assert nonfinite_value(None) is None
    assert nonfinite_value("skip") == "skip" and nonfinite_value("raise") == "raise"
    assert nonfinite_value("SKIP") == "skip"


@pytest.mark.parametrize("bad", ["", "stop", "none", True, False, 0, 1, 1.0, ["skip"], NAN])
def test_bad_nonfinite_values_raise(bad):
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer, nonfinite_value
    from torch_scae_amd.train_step import TrainStep
    with pytest.raises(ValueError):
        nonfinite_value(bad)
    with pytest.raises(ValueError):
        make_optimizer("adam", FlatParameters(Net()), lr=1e-3, eps=1e-8, nonfinite=bad)
    with pytest.raises(ValueError):
        TrainStep(Net(), 4, (1, 16, 16), nonfinite=bad)


def test_an_optimiser_takes_skip_only_and_the_guard_needs_an_optimiser():
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    from torch_scae_amd.train_step import TrainStep
    with pytest.raises(ValueError):      # ("raise" is TrainStep's: the optimiser never reads)
        make_optimizer("adam", FlatParameters(Net()), lr=1e-3, eps=1e-8, nonfinite="raise")
    for mode in ("skip", "raise"):
        with pytest.raises(ValueError):
            TrainStep(Net(), 4, (1, 16, 16), optimizer=None, nonfinite=mode)


def test_the_guard_is_off_by_default_and_allocates_when_on():
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    off = make_optimizer("adam", FlatParameters(Net()), lr=1e-3, eps=1e-8)
    assert off.nonfinite is None and off.guard_state is None and off.grad_norm is None
    on = make_optimizer("adam", FlatParameters(Net()), lr=1e-3, eps=1e-8, nonfinite="skip")
    assert on.max_norm == 0.0 and on.grad_norm is not None
    assert on.guard_state.dtype == torch.int64 and on.guard_state.tolist() == [0, -1, -1, 0]


def test_make_train_step_reads_both_trainer_keys(monkeypatch):
    """Absent keys: no argument (TrainStep's default, off); terminate_on_nan true -> "raise",
    false -> no argument; nonfinite: skip | raise -> that mode, and it wins over
    terminate_on_nan; anything else raises."""
    from torch_scae_amd import factory, train_step
    seen = []

    class Spy:
        def __init__(self, model, batch_size, image_shape, **kw):
            seen.append(kw)

    monkeypatch.setattr(train_step, "TrainStep", Spy)
    base = dict(REF_CFG, optimizer=YAML["rmsprop"])
    for trainer in (None, {}, dict(max_epochs=3), dict(terminate_on_nan=False),
                    dict(nonfinite=None)):
        factory.make_train_step(None, dict(base, trainer=trainer))
        assert "nonfinite" not in seen[-1], trainer
    for trainer, want in ((dict(terminate_on_nan=True), "raise"),
                          (dict(nonfinite="skip"), "skip"), (dict(nonfinite="raise"), "raise"),
                          (dict(terminate_on_nan=True, nonfinite="skip"), "skip"),
                          (dict(terminate_on_nan=False, nonfinite="raise"), "raise")):
        factory.make_train_step(None, dict(base, trainer=trainer))
        assert seen[-1]["nonfinite"] == want, trainer
    for bad in (dict(terminate_on_nan="yes"), dict(terminate_on_nan=1), dict(nonfinite="stop"),
                dict(nonfinite=True), dict(nonfinite=0)):
        with pytest.raises(ValueError):
            factory.make_train_step(None, dict(base, trainer=bad))


def test_make_train_step_builds_a_guarded_step():
    from torch_scae_amd import factory
    cfg = dict(REF_CFG, optimizer=YAML["adam"], trainer=dict(terminate_on_nan=True))
    step = factory.make_train_step(Net(), cfg)
    assert step.nonfinite == "raise" and step.opt.nonfinite == "skip"
    assert step.last_grad_norm() is step.opt.grad_norm      # the guard's norm, clipping off
    assert step.nonfinite_steps() == dict(skipped=0, first=-1, last=-1, attempts=0)
    plain = factory.make_train_step(Net(), dict(cfg, trainer={}))
    assert plain.nonfinite is None and plain.opt.guard_state is None
    with pytest.raises(ValueError):
        plain.nonfinite_steps()


# -- 2. the CPU forms ------------------------------------------------------------------------
class Run:
    """A flat optimiser on test_grad_clip.py's Net (a parameter without a gradient, one with a
    gradient on even batches only).  ``step(bad)``: one optimiser step on the next k batches;
    ``bad``: a value written into one gradient element first -- for k = 1 into the flat gradient
    after the backward, for k = 2 into acc between the group's two batches."""

    def __init__(self, kind, la, k, clip, nonfinite, wd=0.0):
        from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
        self.net = Net()
        self.flat = FlatParameters(self.net)
        self.k, self.it = k, 0
        self.opt = make_optimizer(kind, self.flat, lr=1e-2, eps=1e-3, weight_decay=wd,
                                  look_ahead=la, look_ahead_k=2, gradient_clip_val=clip,
                                  accumulate_grad_batches=k, nonfinite=nonfinite)

    def _backward(self):
        self.flat.clear_grads()
        self.net.loss(batch(self.it), self.it).backward()
        self.flat.gather_grads()
        self.it += 1

    def skip_batches(self):
        """Pass over the batches a step would have consumed."""
        self.it += self.k

    def step(self, bad=None, where=7):
        self._backward()
        if self.k == 2:
            self.opt.accumulate()
            if bad is not None:
                self.opt.acc[where] = bad
            self._backward()
        elif bad is not None:
            self.flat.flat_grad[where] = bad
        self.opt.step(grad_scale=1.0 / self.k)

    def state(self):
        opt = self.opt
        out = dict(param=self.flat.flat_param, step_state=opt.step_state,
                   **dict(opt.state_buffers()))
        if opt.slow is not None:
            out["slow"] = opt.slow
        if opt.acc is not None:
            out["acc"] = opt.acc
        return {k: v.clone() for k, v in out.items()}


def same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        # (bit for bit; NaN-safe: the buffers compared here must be finite anyway)
        assert torch.equal(a[k], b[k]), (what, k)


OPT_GRID = [(kind, la, k, clip) for kind in KINDS for la in (False, True) for k in (1, 2)
            for clip in (0.0, CLIP)]


@pytest.mark.parametrize("kind,la,k,clip", OPT_GRID)
def test_a_finite_step_equals_the_unguarded_optimisers(kind, la, k, clip):
    """Three steps (LookAhead k = 2: one sync among them) with the guard on equal the
    unguarded optimiser's bit for bit, clipping or not; nothing is skipped, every step is
    counted; the guard's norm is written when it does not clip."""
    ours, ref = Run(kind, la, k, clip, "skip", wd=1e-2), Run(kind, la, k, clip, None, wd=1e-2)
    for i in range(3):
        ours.step()
        ref.step()
        same(ours.state(), ref.state(), i)
        assert ours.opt.guard_state.tolist() == [0, -1, -1, i + 1]
        norm = float(ours.opt.grad_norm)
        assert norm > 0 and norm < INF
        if clip:
            assert norm == float(ref.opt.grad_norm) and norm > clip


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
@pytest.mark.parametrize("kind,la,k,clip", OPT_GRID)
def test_a_poisoned_step_leaves_everything_alone(kind, la, k, clip, bad):
    """One finite step (t = 1), then a step with one NaN / +Inf / -Inf element: every buffer
    and step_state unchanged, acc zero, the state {1, t, t, t + 1}, the norm non-finite."""
    run = Run(kind, la, k, clip, "skip")
    run.step()
    before = run.state()
    run.step(bad)
    after = run.state()
    same(before, after, bad)
    if k == 2:
        assert float(after["acc"].abs().max()) == 0.0
    assert run.opt.guard_state.tolist() == [1, 1, 1, 2]
    assert not bool(torch.isfinite(run.opt.grad_norm))
    for v in after.values():
        assert bool(torch.isfinite(v.double()).all())


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("kind,la,k,clip", OPT_GRID)
def test_finite_bad_finite_equals_two_finite_unguarded_steps(kind, la, k, clip, wd):
    """finite, poisoned, finite == two finite steps of the unguarded optimiser on the same
    batches: with LookAhead k = 2 the sync falls on the step right after the skip (the skipped
    step did not advance the count: Adam's and RAdam's bias corrections follow too)."""
    ours, ref = Run(kind, la, k, clip, "skip", wd), Run(kind, la, k, clip, None, wd)
    ours.step()
    ours.step(NAN)
    ours.step()
    ref.step()
    ref.skip_batches()
    ref.step()
    same(ours.state(), ref.state())
    assert ours.opt.guard_state.tolist() == [1, 1, 1, 3]
    if ours.opt.counts_steps:
        assert int(ours.opt.step_state[0]) == 2
        assert int(ours.opt.step_state[1]) == int(la)


def test_first_and_last_follow_the_skips():
    run = Run("adam", False, 1, 0.0, "skip")
    for i, bad in enumerate([None, INF, None, NAN, -INF, None]):
        run.step(bad)
    assert run.opt.guard_state.tolist() == [3, 1, 4, 6]
    assert int(run.opt.step_state[0]) == 3


def test_a_norm_that_overflows_fp32_is_not_a_skip():
    """Finite elements whose fp32 norm overflows: the fp64 sum of squares is finite, so the
    step is taken (and equals the unguarded one); one Inf among them is a skip."""
    ours, ref = Run("adam", False, 1, 0.0, "skip"), Run("adam", False, 1, 0.0, None)
    for run in (ours, ref):
        run._backward()
        run.flat.flat_grad[3:8] = 3e38
        run.opt.step()
    same(ours.state(), ref.state())
    assert ours.opt.guard_state.tolist() == [0, -1, -1, 1]
    assert float(ours.opt.grad_norm) == INF      # (fp32: the norm itself does overflow)
    before = ours.state()
    ours._backward()
    ours.flat.flat_grad[3:8] = 3e38
    ours.flat.flat_grad[5] = INF
    ours.opt.step()
    same(before, ours.state())
    assert ours.opt.guard_state.tolist() == [1, 1, 1, 2]


def test_flush_of_a_pending_group_is_guarded():
    run = Run("rmsprop", False, 2, 0.0, "skip")
    run.step()
    before = run.state()
    run._backward()
    run.opt.accumulate()
    run.opt.acc[2] = NAN
    run.opt.flush(0.5)
    same(before, run.state())
    assert run.opt.guard_state.tolist() == [1, 1, 1, 2]


@pytest.mark.parametrize("clip", [0.0, CLIP])
@pytest.mark.parametrize("kind", KINDS)
def test_a_step_no_parameter_takes_counts_and_writes_nothing(kind, clip):
    """Weight decay and no parameter with a gradient, in the last backward or the group: no
    range is active, so -- as on the device, which launches no pass then -- the guard counts
    no attempt, the norm is not written and every buffer keeps its bits; acc is zeroed."""
    run = Run(kind, False, 2, clip, "skip", wd=1e-2)
    run.step()
    before, counted, norm = run.state(), run.opt.guard_state.clone(), run.opt.grad_norm.clone()
    run.flat.clear_grads()
    run.flat.gather_grads()                 # no backward: no parameter has a gradient
    assert run.flat.active_ranges() == []
    run.opt.acc.fill_(1.0)
    run.opt.step(grad_scale=0.5)
    after = run.state()
    assert float(after.pop("acc").abs().max()) == 0.0
    before.pop("acc")
    same(before, after, kind)
    assert torch.equal(run.opt.guard_state, counted) and counted.tolist() == [0, -1, -1, 1]
    assert torch.equal(run.opt.grad_norm, norm)


def test_a_tracked_row_is_written_for_a_skipped_step():
    from torch_scae_amd.data_parallel import GradNorms
    run = Run("adam", False, 1, 0.0, "skip")
    run.opt.track = GradNorms(run.flat, run.net, 2.0, capacity=4, split_capsules=False)
    run.step()
    run.step(NAN)
    assert int(run.opt.track.cursor) == 2
    rows = run.opt.track.ring[:2]
    assert bool(torch.isfinite(rows[0]).all())
    assert not bool(torch.isfinite(rows[1, -1]))
    assert int((~torch.isfinite(rows[1, :-1])).sum()) == 1     # the segment that blew up


# -- 3. TrainStep(nonfinite="raise") ---------------------------------------------------------
def _host_step(step, it, bad=None):
    """An optimiser step of ``step`` (a TrainStep on the CPU Net) as _finish issues it."""
    step.flat.clear_grads()
    step.model.loss(batch(it), it).backward()
    step.flat.gather_grads()
    if bad is not None:
        step.flat.flat_grad[4] = bad
    step.opt.step(grad_scale=1.0 / step.world)


def test_raise_raises_at_the_epochs_end_after_a_skipped_step_and_not_otherwise():
    from torch_scae_amd.train_step import NonFiniteGradientError, TrainStep
    assert issubclass(NonFiniteGradientError, ValueError)
    step = TrainStep(Net(), 8, (1, 16, 16), optimizer="adam", nonfinite="raise",
                     use_graph=False, lr_decay_rate=0.5)
    _host_step(step, 0)
    step.end_epoch()                                   # nothing skipped: no error
    assert step.check_nonfinite()["attempts"] == 1
    before = step.flat.flat_param.clone()
    _host_step(step, 1, NAN)
    _host_step(step, 2)
    _host_step(step, 3, INF)
    assert torch.equal(step.snapshot()["guard_state"], torch.tensor([2, 1, 3, 4]))
    with pytest.raises(NonFiniteGradientError) as err:
        step.end_epoch()
    e = err.value
    assert (e.skipped, e.first, e.last, e.attempts) == (2, 1, 3, 4)
    assert "2 of 4" in str(e) and "step 1" in str(e) and "3" in str(e)
    assert bool(torch.isfinite(step.flat.flat_param).all())
    assert not torch.equal(step.flat.flat_param, before)      # (step 2 trained)
    assert step.opt.lr == pytest.approx(3e-5 * 0.25)           # both epochs decayed the lr
    step.end_epoch()                                   # reported once: no new skip, no error
    _host_step(step, 4, -INF)
    with pytest.raises(NonFiniteGradientError):
        step.check_nonfinite()
    assert step.nonfinite_steps() == dict(skipped=3, first=1, last=4, attempts=5)


def test_skip_never_raises_and_restore_brings_the_counters_back():
    from torch_scae_amd.train_step import TrainStep
    step = TrainStep(Net(), 8, (1, 16, 16), optimizer="rmsprop", nonfinite="skip",
                     use_graph=False)
    _host_step(step, 0)
    snap = step.snapshot()
    _host_step(step, 1, NAN)
    step.end_epoch()
    assert step.nonfinite_steps()["skipped"] == 1
    step.restore(snap)
    assert step.nonfinite_steps() == dict(skipped=0, first=-1, last=-1, attempts=1)


def test_plain_rmsprop_reports_the_steps_taken():
    """optimizer_state_dict()'s ``step``: the host's count less the skipped steps for plain
    RMSprop, the device count for Adam."""
    from torch_scae_amd.train_step import TrainStep
    for kind in ("rmsprop", "adam"):
        step = TrainStep(Net(), 8, (1, 16, 16), optimizer=kind, nonfinite="skip",
                         use_graph=False)
        for it, bad in enumerate([None, NAN, None]):
            _host_step(step, it, bad)
            step.steps += 1
        sd = step.optimizer_state_dict()
        assert {float(s["step"]) for s in sd["state"].values()} == {2.0}, kind


# -- 4. two gloo ranks -----------------------------------------------------------------------
def _rank(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from torch_scae_amd.data_parallel import (FlatParameters, all_reduce_gradients,
                                              broadcast_parameters, make_optimizer)
    net = Net()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(rank * 0.5)
    flat = FlatParameters(net)
    broadcast_parameters(flat)
    start = flat.flat_param.clone()
    opt = make_optimizer("adam", flat, lr=1e-2, eps=1e-3, nonfinite="skip")
    states = []
    for it, bad in enumerate([None, NAN]):      # a step both ranks take, then rank 1's NaN
        flat.clear_grads()
        net.loss(batch(2 * it + rank), 0).backward()
        flat.gather_grads()
        if bad is not None and rank == 1:
            flat.flat_grad[9] = bad
        all_reduce_gradients(flat, average=False)
        opt.step(grad_scale=1.0 / world)
        states.append((flat.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(),
                       opt.step_state[:2].clone(), opt.guard_state.clone()))
    out[rank] = (start, states)
    dist.destroy_process_group()


def test_two_ranks_take_the_same_decision_after_the_all_reduce():
    """Rank 1's gradient holds a NaN: the all-reduced gradient holds it on both ranks, both
    skip and count 1, and the parameters are those of the step before, equal on both."""
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_rank, args=(world, _free_port(), out), nprocs=world, join=True)
    (s0, a), (s1, b) = out[0], out[1]
    assert torch.equal(s0, s1)
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    for states in (a, b):
        good, skipped = states
        assert good[4].tolist() == [0, -1, -1, 1] and skipped[4].tolist() == [1, 1, 1, 2]
        for x, y in zip(good[:4], skipped[:4]):
            assert torch.equal(x, y)
        assert not torch.equal(good[0], s0)              # the first step trained
        assert good[3].tolist() == [1, 0]


def test_a_device_without_cpu_forms_raises_instead_of_running_unguarded():
    """The guard has CPU forms only: on any other device the optimiser is not built (no quiet
    step without the guard); with the guard off it is built as before."""
    from torch_scae_amd._lib import ScaeHipError
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    flat = FlatParameters(Net().to("meta"))
    for kind in KINDS:
        with pytest.raises(ScaeHipError):
            make_optimizer(kind, flat, lr=1e-3, eps=1e-8, nonfinite="skip")
        assert make_optimizer(kind, flat, lr=1e-3, eps=1e-8).guard_state is None
