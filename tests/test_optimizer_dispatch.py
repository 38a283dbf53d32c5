"""The flat optimisers' device branch without a GPU: which entry points a step calls, in which
order, and every argument of every call (data_parallel._device_step, _launch_norm,
_riding_units).  The branch reads its tensors' addresses and sizes only, so it runs on CPU
tensors once ``_lib.call``, the stream helper and ``ops._launch_sum_units`` are replaced by
recorders; no built library is needed.  What the calls compute: test_optimizers_gpu.py,
test_grad_clip_gpu.py, test_grad_accumulate_gpu.py, test_grad_norms_gpu.py."""
import ctypes
import itertools

import pytest
import torch
import torch.nn as nn

# four parameters; the second never has a gradient, so that weight decay (which skips the
# parameters without one) gives two ranges; the last has one or not
SIZES = (7, 5, 6, 3)
TOTAL = sum(SIZES)
RANGES = {True: [(0, 7), (12, 9)], False: [(0, 7), (12, 6)]}      # by the last one's gradient

LR, EPS, MOMENTUM, ALPHA, BETAS, CLIP, SCALE = 1e-2, 1e-3, 0.75, 0.99, (0.5, 0.875), 0.25, 0.5
LA_K, LA_ALPHA = 3, 0.25
STREAM = ctypes.c_void_p(0x5EED)
N_PARTIALS = 5          # what the recorded norm launch reports
SUMS_ALONE = "scae_sum_rows_multi_f32"
NORMS = "scae_segment_norms_f32"

# the argument lists (include/scae_hip.h), by field; the accumulate forms (``_acc`` after the
# family's name) take ``acc`` directly after ``grad``.  Fields that are buffers of the flat
# layout point at the launch's range; the _sums forms take neither weight_decay nor advance
RMS = "square_avg buf n lr lr_dev alpha eps momentum"
OPT = "m v slow n lr_dev step_state kind beta1 beta2 eps"
CLIPPED = "grad_sq n_partials max_norm norm_out"
LAYOUT = {
    "scae_rmsprop_step_f32": f"param grad {RMS} weight_decay grad_scale stream",
    "scae_rmsprop_sums_step_f32": f"param grad {RMS} grad_scale jobs n_jobs stream",
    "scae_rmsprop_clip_step_f32": f"param grad {RMS} weight_decay grad_scale {CLIPPED} stream",
    "scae_flat_opt_step_f32":
        f"param grad {OPT} weight_decay grad_scale la_k la_alpha advance stream",
    "scae_flat_opt_sums_step_f32": f"param grad {OPT} grad_scale la_k la_alpha jobs n_jobs stream",
    "scae_flat_opt_clip_step_f32":
        f"param grad {OPT} weight_decay grad_scale la_k la_alpha advance {CLIPPED} stream",
    "scae_grad_sq_partials_f32": "grad n grad_sq grad_sq_len count stream",
    "scae_grad_sq_partials_sums_f32": "grad n grad_sq grad_sq_len count jobs n_jobs stream",
}
for _name, _fields in list(LAYOUT.items()):
    _fam = next(f for f in ("scae_rmsprop", "scae_flat_opt", "scae_grad_sq")
                if _name.startswith(f + "_"))
    LAYOUT[_fam + "_acc" + _name[len(_fam):]] = _fields.replace("grad ", "grad acc ", 1)

OPTIMISERS = {      # name -> (kind, LookAhead, entry-point family)
    "rmsprop": ("rmsprop", False, "scae_rmsprop"),
    "rmsprop_la": ("rmsprop", True, "scae_flat_opt"),
    "adam": ("adam", False, "scae_flat_opt"),
    "radam_la": ("radam", True, "scae_flat_opt"),
}


class Four(nn.Module):
    def __init__(self):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(torch.randn(n)) for n in SIZES])


def make(name, acc, clip, wd, last):
    from torch_scae_amd.data_parallel import FlatParameters, make_optimizer
    kind, la, _ = OPTIMISERS[name]
    flat = FlatParameters(Four())
    assert flat.offsets == [0, 7, 12, 18] and flat.numel == TOTAL
    for p, has in zip(flat.params, (True, False, True, last)):
        p._flat_was_set = has
    return make_optimizer(kind, flat, lr=LR, eps=EPS, betas=BETAS, momentum=MOMENTUM,
                          weight_decay=wd, look_ahead=la, look_ahead_k=LA_K,
                          look_ahead_alpha=LA_ALPHA, gradient_clip_val=CLIP if clip else 0.0,
                          accumulate_grad_batches=2 if acc else 1)


def fake_units(n):
    """``n`` column-sum units as ``ops._sum_rows_multi`` queues them, over CPU tensors."""
    from torch_scae_amd import _lib
    units = []
    for i in range(n):
        partial, segs = torch.zeros(2, 3), (_lib.SumSegment * 1)()
        units.append((partial, 2, 3, ctypes.cast(segs, ctypes.POINTER(_lib.SumSegment)), 1,
                      segs))
    return units


@pytest.fixture
def calls(monkeypatch):
    """The launches a step makes, as (name, args): ``_lib.call``'s, and one entry per
    ``ops._launch_sum_units`` call with the units it got."""
    from torch_scae_amd import _lib, data_parallel, ops
    made = []

    def call(name, *args):
        for a in args:
            if hasattr(a, "_obj"):      # (the norm launch's partial count, by reference)
                a._obj.value = N_PARTIALS
        made.append((name, args))

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(data_parallel, "_stream", lambda t: STREAM)
    monkeypatch.setattr(ops, "_launch_sum_units",
                        lambda units: made.append((SUMS_ALONE, tuple(units))))
    return made


class Tracker:
    """Stands in for GradNorms (whose own launch test_grad_norms_gpu.py covers): records when
    the norms are taken, and of what."""

    def __init__(self, made):
        self.made, self.built = made, 0

    def build(self, seen):
        self.built += 1

    def launch(self, x, acc, scale):
        self.made.append((NORMS, (x, acc, scale)))


def step(opt, units, acc):
    """``opt.step(SCALE, units)`` as it runs when the flat buffers are on a HIP device."""
    from torch_scae_amd import data_parallel as dp
    a = opt.acc if acc else None
    dp._device_step(opt, SCALE, dp._track_first(opt, SCALE, units, a, True), a)


def plain(a):
    """An argument as a comparable value: a pointer's address, a job array's sources."""
    if isinstance(a, ctypes.c_void_p):
        return a.value
    if isinstance(a, ctypes.Array):
        return tuple(job.src for job in a)
    return "by reference" if hasattr(a, "_obj") else a


def expected_values(opt, name, off, n, first, last, riders):
    """field -> value for the launch over [off, off + n) (``first`` / ``last`` of the step's
    ranges) with ``riders`` riding in it."""
    from torch_scae_amd import _lib
    flat = opt.flat
    rms = OPTIMISERS[name][0] == "rmsprop"
    here = dict(param=flat.flat_param, grad=flat.flat_grad, acc=opt.acc,
                square_avg=getattr(opt, "square_avg", None), buf=getattr(opt, "buf", None),
                m=opt.buf if rms else opt.exp_avg,
                v=opt.square_avg if rms else opt.exp_avg_sq,
                slow=opt.slow if OPTIMISERS[name][1] else flat.flat_param)
    vals = {k: t.data_ptr() + 4 * off for k, t in here.items() if t is not None}
    vals.update(
        n=n, lr=LR, lr_dev=opt.lr_dev.data_ptr(), alpha=ALPHA, eps=EPS, momentum=MOMENTUM,
        step_state=opt.step_state.data_ptr(), kind=dict(adam=0, radam=1, rmsprop=2)[
            OPTIMISERS[name][0]],
        beta1=MOMENTUM if rms else BETAS[0], beta2=ALPHA if rms else BETAS[1],
        weight_decay=opt.weight_decay, grad_scale=SCALE,
        la_k=LA_K if OPTIMISERS[name][1] else 0, la_alpha=LA_ALPHA, advance=int(last),
        n_partials=N_PARTIALS, max_norm=CLIP, grad_sq_len=_lib.GRAD_SQ_MAX_PARTIALS,
        count="by reference", stream=STREAM.value,
        jobs=tuple(u[0].data_ptr() for u in riders), n_jobs=len(riders))
    if opt.max_norm:
        vals.update(grad_sq=opt.grad_sq.data_ptr(),
                    norm_out=opt.grad_norm.data_ptr() if first else None)
    return vals


def check_step(name, calls, opt, units, acc, clip, wd, last, track):
    from torch_scae_amd import _lib
    family = OPTIMISERS[name][2]
    A = "_acc" if acc else ""
    ranges = RANGES[last] if wd else [(0, TOTAL)]
    # -- the entry points and their order
    ride = bool(units) and (clip or (wd == 0 and not track))
    alone = (units[:-16] if ride else units)
    riders = units[len(alone):]
    want = [SUMS_ALONE] if alone else []
    if clip:
        want.append(f"scae_grad_sq{A}_partials{'_sums' if units else ''}_f32")
    if track:
        want.append(NORMS)
    if clip:
        want += [f"{family}{A}_clip_step_f32"] * len(ranges)
    elif riders:
        want.append(f"{family}{A}_sums_step_f32")
    else:
        want += [f"{family}{A}_step_f32"] * len(ranges)
    assert [c[0] for c in calls] == want
    passes = [c for c in calls if c[0].endswith("_step_f32")]
    if riders and not clip:       # the _sums form covers the whole buffer
        ranges = [(0, TOTAL)]
    assert len(passes) == len(ranges)
    # -- every argument
    i = 0
    for cname, args in calls:
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
        else:
            (off, n), first, is_last = ranges[i], i == 0, i == len(ranges) - 1
            i += 1
        vals = expected_values(opt, name, off, n, first, is_last, riders)
        fields = LAYOUT[cname].split()
        assert [plain(a) for a in args] == [vals[f] for f in fields], (cname, fields)
        if acc:     # acc sits directly after grad
            at = fields.index("acc")
            assert fields[at - 1] == "grad" and plain(args[at]) == opt.acc.data_ptr() + 4 * off


MATRIX = list(itertools.product(OPTIMISERS, (False, True), (False, True), (0.0, 1e-2),
                                (0, 3, 20), (True, False)))


@pytest.mark.parametrize("name,acc,clip,wd,n_units,last", MATRIX)
def test_a_device_step_calls_the_parents_entry_points_with_its_arguments(
        calls, name, acc, clip, wd, n_units, last):
    opt = make(name, acc, clip, wd, last)
    units = fake_units(n_units)
    opt._acc_seen = [False] * 4 if acc else None      # (a group is open)
    step(opt, units, acc)
    assert opt._acc_seen is None                      # the step ends the group
    check_step(name, calls, opt, units, acc, clip, wd, last, track=False)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", OPTIMISERS)
def test_a_tracking_step_takes_the_norms_once_the_gradient_is_complete(calls, name, clip):
    """Without clipping all column sums run alone, then the norms, then the forms without
    riders; clipping, the sums ride in the norm launch and the norms follow it."""
    opt = make(name, True, clip, 0.0, True)
    opt.track = Tracker(calls)
    units = fake_units(20)
    step(opt, units, True)
    assert opt.track.built == 1
    check_step(name, calls, opt, units, True, clip, 0.0, True, track=True)


def test_a_parameter_seen_earlier_in_the_group_takes_the_step(calls):
    """Weight decay covers the parameters with a gradient in ANY batch of the group."""
    opt = make("adam", True, False, 1e-2, False)
    opt._acc_seen = [False, False, False, True]
    step(opt, [], True)
    assert [(a[6], plain(a[0]) - opt.flat.flat_param.data_ptr()) for _, a in calls] == \
        [(7, 0), (9, 4 * 12)]


@pytest.mark.parametrize("n_units,ride,alone", [(0, True, 0), (3, True, 0), (16, True, 0),
                                                (17, True, 1), (20, True, 4), (3, False, 3),
                                                (20, False, 20)])
def test_riding_units_are_the_last_sixteen(calls, n_units, ride, alone):
    from torch_scae_amd.data_parallel import _riding_units
    units = fake_units(n_units)
    riders = _riding_units(units, ride)
    assert (riders or []) == units[alone:]
    assert calls == ([(SUMS_ALONE, tuple(units[:alone]))] if alone else [])


@pytest.mark.parametrize("n_units", [0, 3, 20])
def test_accumulate_and_fold_on_the_device(calls, monkeypatch, n_units):
    """``accumulate`` hosts the column sums whatever the weight decay; these two dispatch on
    ``is_cuda`` themselves, so the flat gradient is made to answer like a device tensor."""
    class OnDevice(torch.Tensor):
        is_cuda = True

    opt = make("rmsprop", True, False, 1e-2, True)
    g = opt.flat.flat_grad = opt.flat.flat_grad.as_subclass(OnDevice)
    units = fake_units(n_units)
    opt.accumulate(units)
    opt.fold()
    gp, ap, st = g.data_ptr(), opt.acc.data_ptr(), STREAM.value
    riders = units[-16:]
    want = [(SUMS_ALONE, tuple(units[:-16]))] if n_units > 16 else []
    got = [(n, tuple(plain(a) for a in args)) if n != SUMS_ALONE else (n, args)
           for n, args in calls]
    if riders:
        want.append(("scae_grad_accumulate_sums_f32",
                     (ap, gp, TOTAL, tuple(u[0].data_ptr() for u in riders), len(riders), st)))
    else:
        want.append(("scae_grad_accumulate_f32", (ap, gp, TOTAL, st)))
    want.append(("scae_grad_accumulate_f32", (gp, ap, TOTAL, st)))
    assert got == want
