"""The non-finite guard's device branch without a GPU, in the manner of
test_optimizer_dispatch.py (CPU tensors, recording launchers): a guarded optimiser's
``_device_step`` takes the clip path whether it clips or not -- the norm launch with the column
sums riding in it, the tracked norms, then the ``_guard`` form over each active range -- with
every argument in its place: ``max_norm`` or +inf, ``norm_out`` and ``guard_state`` on the first
range only, ``advance`` on the last; and an unguarded optimiser's launches are what they were.
What the launches compute: test_nonfinite_guard_gpu.py."""
import itertools
import math

import pytest
import torch

from tests.test_optimizer_dispatch import (CLIP, LAYOUT, NORMS, OPTIMISERS, RANGES, SCALE,  # noqa: F401
                                           SUMS_ALONE, TOTAL, Four, Tracker, calls, check_step,
                                           expected_values, fake_units, plain, step)
from tests.test_optimizer_dispatch import (ALPHA, BETAS, EPS, LA_ALPHA, LA_K, LR, MOMENTUM)

# the guarded forms: the clip forms' arguments, then guard_state after norm_out
GUARD_LAYOUT = {}
for _name, _fields in LAYOUT.items():
    if _name.endswith("_clip_step_f32"):
        GUARD_LAYOUT[_name.replace("_clip_step", "_guard_step")] = \
            _fields.replace("norm_out stream", "norm_out guard_state stream")
assert sorted(GUARD_LAYOUT) == ["scae_flat_opt_acc_guard_step_f32", "scae_flat_opt_guard_step_f32",
                                "scae_rmsprop_acc_guard_step_f32", "scae_rmsprop_guard_step_f32"]


def make(name, acc, clip, wd, last, nonfinite="skip"):
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    kind, la, _ = OPTIMISERS[name]
    flat = FlatParameters(Four())
    for p, has in zip(flat.params, (True, False, True, last)):
        p._flat_was_set = has
    return make_optimizer(kind, flat, lr=LR, eps=EPS, betas=BETAS, momentum=MOMENTUM,
                          weight_decay=wd, look_ahead=la, look_ahead_k=LA_K,
                          look_ahead_alpha=LA_ALPHA, gradient_clip_val=CLIP if clip else 0.0,
                          accumulate_grad_batches=2 if acc else 1, nonfinite=nonfinite)


def check_guarded(name, made, opt, units, acc, clip, wd, last, track):
    from torch_scae_amd import _lib
    family = OPTIMISERS[name][2]
    A = "_acc" if acc else ""
    ranges = RANGES[last] if wd else [(0, TOTAL)]
    # -- the entry points and their order: the column sums ride in the norm launch (all but
    # the last sixteen run alone first), whatever the weight decay, tracking or not
    alone = units[:-16]
    riders = units[len(alone):]
    want = [SUMS_ALONE] if alone else []
    want.append(f"scae_grad_sq{A}_partials{'_sums' if units else ''}_f32")
    if track:
        want.append(NORMS)
    want += [f"{family}{A}_guard_step_f32"] * len(ranges)
    assert [c[0] for c in made] == want
    assert not any("_sums_step" in c[0] for c in made)       # never a _sums pass
    # -- every argument
    i = 0
    for cname, args in made:
        if cname == SUMS_ALONE:
            assert list(args) == list(alone)
            continue
        if cname == NORMS:      # of the gradient the pass consumes, acc not yet cleared
            assert args[0] is opt.flat.flat_grad and args[2] == SCALE
            assert args[1] is (opt.acc if acc else None)
            continue
        sig = _lib.SIGNATURES[cname]
        assert len(args) == len(sig), cname
        for t, a in zip(sig, args):
            t.from_param(a)
        if "_partials" in cname:      # the norm launch: the whole buffer
            off, n, first, is_last = 0, TOTAL, True, True
            fields = LAYOUT[cname].split()
        else:
            (off, n), first, is_last = ranges[i], i == 0, i == len(ranges) - 1
            i += 1
            fields = GUARD_LAYOUT[cname].split()
        vals = expected_values(opt, name, off, n, first, is_last, riders)
        vals.update(grad_sq=opt.grad_sq.data_ptr(),
                    norm_out=opt.grad_norm.data_ptr() if first else None,
                    guard_state=opt.guard_state.data_ptr() if first else None,
                    max_norm=CLIP if clip else math.inf)
        got = [plain(a) for a in args]
        assert got == [vals[f] for f in fields], (cname, fields)
        if "_partials" not in cname:
            assert fields[-3:] == ["norm_out", "guard_state", "stream"]
            assert "advance" not in fields or got[fields.index("advance")] == int(is_last)
        if acc:     # acc sits directly after grad
            at = fields.index("acc")
            assert fields[at - 1] == "grad" and plain(args[at]) == opt.acc.data_ptr() + 4 * off
    assert i == len(ranges)


MATRIX = list(itertools.product(OPTIMISERS, (False, True), (False, True), (0.0, 1e-2),
                                (0, 3, 20), (True, False)))


@pytest.mark.parametrize("name,acc,clip,wd,n_units,last", MATRIX)
def test_a_guarded_device_step_takes_the_norm_launch_then_the_guard_forms(
        calls, name, acc, clip, wd, n_units, last):
    opt = make(name, acc, clip, wd, last)
    assert opt.grad_sq is not None and opt.guard_state.tolist() == [0, -1, -1, 0]
    units = fake_units(n_units)
    opt._acc_seen = [False] * 4 if acc else None      # (a group is open)
    step(opt, units, acc)
    assert opt._acc_seen is None                      # the step ends the group
    check_guarded(name, calls, opt, units, acc, clip, wd, last, track=False)
    # the host counts nothing: the launch does
    assert opt.guard_state.tolist() == [0, -1, -1, 0]


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("name", OPTIMISERS)
def test_a_guarded_tracking_step_takes_the_norms_after_the_norm_launch(calls, name, acc, clip,
                                                                       wd):
    """As a clipping step: the sums ride in the norm launch and the tracked norms follow it,
    ahead of the pass -- a skipped step's row is written."""
    opt = make(name, acc, clip, wd, True)
    opt.track = Tracker(calls)
    units = fake_units(20)
    step(opt, units, acc)
    assert opt.track.built == 1
    check_guarded(name, calls, opt, units, acc, clip, wd, True, track=True)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", OPTIMISERS)
def test_no_active_range_launches_no_pass_and_counts_nothing(calls, name, clip):
    """Weight decay and no parameter with a gradient: the norm launch alone, as a clipping
    step's; no ``_guard`` launch, so nothing is counted (the CPU form counts nothing either)."""
    opt = make(name, True, clip, 1e-2, False)
    for p in opt.flat.params:
        p._flat_was_set = False
    opt._acc_seen = [False] * 4
    step(opt, [], True)
    assert [c[0] for c in calls] == ["scae_grad_sq_acc_partials_f32"]


@pytest.mark.parametrize("name,acc,clip,wd,n_units,last",
                         [m for m in MATRIX if m[4] != 3])
def test_an_unguarded_step_launches_what_it_launched(calls, name, acc, clip, wd, n_units, last):
    """nonfinite=None: the launch list test_optimizer_dispatch.py describes, name by name and
    argument by argument (its own checker), and no guard buffer is allocated."""
    opt = make(name, acc, clip, wd, last, nonfinite=None)
    assert opt.guard_state is None and (opt.grad_sq is None) == (not clip)
    units = fake_units(n_units)
    step(opt, units, acc)
    assert not any("_guard" in c[0] for c in calls)
    check_step(name, calls, opt, units, acc, clip, wd, last, track=False)


@pytest.mark.parametrize("clip", [False, True])
def test_an_unguarded_tracking_step_launches_what_it_launched(calls, clip):
    opt = make("adam", True, clip, 0.0, True, nonfinite=None)
    opt.track = Tracker(calls)
    units = fake_units(20)
    step(opt, units, True)
    check_step("adam", calls, opt, units, True, clip, 0.0, True, track=True)


def test_guard_state_and_norm_follow_the_device():
    """``_init_guard`` builds the counters, the norm and the partials on the flat buffers'
    device; a device type with neither form still raises."""
    from torch_scae_amd._lib import GRAD_SQ_MAX_PARTIALS, ScaeHipError
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    opt = make("adam", False, False, 0.0, True)
    dev = opt.flat.flat_param.device
    assert opt.guard_state.device == dev and opt.guard_state.dtype == torch.int64
    assert opt.grad_norm.device == dev and opt.grad_norm.dtype == torch.float32
    assert opt.grad_sq.dtype == torch.float64 and opt.grad_sq.numel() == GRAD_SQ_MAX_PARTIALS
    with pytest.raises(ScaeHipError):
        make_optimizer("adam", FlatParameters(Four().to("meta")), lr=1e-3, eps=1e-8,
                       nonfinite="skip")
