"""The non-finite guard on the GPU: the guarded forms of the optimiser passes
(scae_{rmsprop,flat_opt}[_acc]_guard_step_f32) launch by launch -- a finite gradient gives the
clip form's bits (the plain pass's with max_norm = +inf), a poisoned one leaves every buffer and
all of step_state alone, zeroes acc and is counted -- and TrainStep(nonfinite=...) in eager,
graph-replay and launch-list form: a skipped batch equals a run that never saw it.  Every
comparison is bit for bit, on int32 views (NaN != NaN).  No test here creates a process
group."""
import ctypes
import itertools
import math

import pytest
import torch

from tests.test_optimizers_gpu import BETAS, KIND, batches, small_step

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
NAN, INF = float("nan"), float("inf")
PAD = 8             # sentinel floats before and after every buffer (a multiple of a 16-byte line)
SENTINEL = -777.25
LR, EPS, LA_ALPHA, MAX_NORM = 1e-3, 1e-4, 0.5, 0.05
NS = (1, 5, 257, 4099, 20011)

# (entry-point family, kind, LookAhead k, steps taken t, slow made): plain RMSprop; Adam; a
# LookAhead sync step with the slow weights made (t + 1 = 10) and the first one (t + 1 = 5);
# a LookAhead step that does not sync
CONFIGS = [("scae_rmsprop", "rmsprop", 0, 0, 0), ("scae_flat_opt", "adam", 0, 3, 0),
           ("scae_flat_opt", "radam", 5, 9, 1), ("scae_flat_opt", "rmsprop", 5, 4, 0),
           ("scae_flat_opt", "adam", 5, 6, 1)]
VARIANTS = list(itertools.product(CONFIGS, (False, True), (0.0, 1e-2), (False, True)))


def stream():
    return P(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


_TEMPLATES = {}


def templates(n):
    if n not in _TEMPLATES:
        g = torch.Generator().manual_seed(100 + n)
        _TEMPLATES[n] = {k: x.cuda() for k, x in dict(
            p=torch.randn(n, generator=g), g=torch.randn(n, generator=g),
            acc=torch.randn(n, generator=g), m=torch.randn(n, generator=g) * .1,
            v=torch.rand(n, generator=g), slow=torch.randn(n, generator=g)).items()}
    return _TEMPLATES[n]


class Bufs:
    """The flat buffers of one optimiser over n elements at 4-byte phase ``phase`` of a 16-byte
    line, each between two sentinel bands, with the optimiser's small state."""

    def __init__(self, n, phase, cfg, g=None, acc=None):
        from torch_scae_amd import _lib
        self.n, self.lo = n, PAD + phase
        self.b = {}
        given = dict(g=g, acc=acc)
        for k, x in templates(n).items():
            full = torch.full((2 * PAD + phase + n,), SENTINEL, device="cuda")
            full[self.lo:self.lo + n] = x if given.get(k) is None else given[k]
            assert full.data_ptr() % 16 == 0
            self.b[k] = full
        _, _, la_k, t, made = cfg
        self.state = torch.zeros(_lib.FLAT_OPT_STATE_INTS, dtype=torch.int32, device="cuda")
        self.state[:2] = torch.tensor([t, made], dtype=torch.int32)
        self.norm = torch.full((), -1.0, device="cuda")
        self.guard = torch.tensor([0, -1, -1, 0], dtype=torch.int64, device="cuda")

    def inner(self, k):
        return self.b[k][self.lo:self.lo + self.n]

    def snap(self):
        out = {k: bits(x).clone() for k, x in self.b.items()}
        out["state"] = self.state.clone()
        return out


LR_DEV = {}


def lr_dev():
    if "t" not in LR_DEV:
        LR_DEV["t"] = torch.full((1,), LR, device="cuda")
    return LR_DEV["t"]


def norm_launch(bufs, acc, off=0, n=None):
    """The norm launch over [off, off + n) of grad (acc + grad) -> (partials, count)."""
    from torch_scae_amd import _lib
    n = bufs.n if n is None else n
    part = torch.full((_lib.GRAD_SQ_MAX_PARTIALS,), NAN, dtype=torch.float64, device="cuda")
    cnt = ctypes.c_int(0)
    at = lambda k: P(bufs.b[k].data_ptr() + 4 * (bufs.lo + off))   # noqa: E731
    if acc:
        _lib.call("scae_grad_sq_acc_partials_f32", at("g"), at("acc"), n, P(part.data_ptr()),
                  part.numel(), ctypes.byref(cnt), stream())
    else:
        _lib.call("scae_grad_sq_partials_f32", at("g"), n, P(part.data_ptr()), part.numel(),
                  ctypes.byref(cnt), stream())
    return part, cnt.value


def launch(form, bufs, cfg, acc, wd, part=None, cnt=0, max_norm=None, scale=0.5, off=0, n=None,
           advance=1, first=True):
    """One pass over [off, off + n): ``form`` "" (plain), "_clip" or "_guard"."""
    from torch_scae_amd import _lib
    family, kind, la_k, _, _ = cfg
    n = bufs.n if n is None else n
    at = lambda k: P(bufs.b[k].data_ptr() + 4 * (bufs.lo + off))   # noqa: E731
    tail = []
    if form:
        tail = [P(part.data_ptr()), cnt, max_norm, P(bufs.norm.data_ptr()) if first else None]
        if form == "_guard":
            tail.append(P(bufs.guard.data_ptr()) if first else None)
    head = [at("p"), at("g")] + ([at("acc")] if acc else [])
    name = "%s%s%s_step_f32" % (family, "_acc" if acc else "", form)
    if family == "scae_rmsprop":
        _lib.call(name, *head, at("v"), at("m"), n, LR, P(lr_dev().data_ptr()), 0.99, EPS, 0.9,
                  wd, scale, *tail, stream())
    else:
        _lib.call(name, *head, at("m"), at("v"), at("slow"), n, P(lr_dev().data_ptr()),
                  P(bufs.state.data_ptr()), KIND[kind], *BETAS[kind], EPS, wd, scale, la_k,
                  LA_ALPHA, advance, *tail, stream())


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


# -- 1. a finite gradient ------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_a_finite_step_has_the_clip_forms_bits_or_the_plain_passes(n):
    """Every variant (family and step kind, acc, weight decay, guard alone / guard + clip) at
    every 4-byte phase: all buffers with their sentinel bands and all 2112 ints of step_state
    equal the ``_clip`` form's -- guard alone (max_norm = +inf): the plain (``_acc``) pass's --,
    the norm equals the clip form's, and the step is counted as taken."""
    for phase, (cfg, acc, wd, clip) in itertools.product(range(4), VARIANTS):
        ours, ref = Bufs(n, phase, cfg), Bufs(n, phase, cfg)
        part, cnt = norm_launch(ours, acc)
        launch("_guard", ours, cfg, acc, wd, part, cnt, MAX_NORM if clip else INF)
        if clip:
            launch("_clip", ref, cfg, acc, wd, part, cnt, MAX_NORM)
        else:
            launch("", ref, cfg, acc, wd)
        what = (n, phase, cfg, acc, wd, clip)
        same(ours.snap(), ref.snap(), what)
        assert ours.guard.tolist() == [0, -1, -1, 1], what
        norm = float(ours.norm)
        assert math.isfinite(norm) and norm > 0, what
        if clip:
            assert bits(ours.norm).item() == bits(ref.norm).item(), what
        # the fp32 norm of the fp64 partials (their sum in the kernel's own order may differ
        # in the last fp64 bit: one fp32 ulp at the most)
        host = 0.5 * math.sqrt(float(part[:cnt].sum()))
        assert abs(norm - host) <= 1.2e-7 * host, what
        # a step was taken, and acc is consumed
        assert not torch.equal(ours.inner("p"), templates(n)["p"]), what
        if acc:
            assert float(ours.inner("acc").abs().max()) == 0.0, what


def test_guard_alone_writes_the_clip_forms_norm():
    """max_norm = +inf: ``norm_out`` has the bits the ``_clip`` form writes from the same
    partials."""
    for cfg, acc in itertools.product(CONFIGS, (False, True)):
        for n, phase in ((257, 1), (4099, 3)):
            ours, ref = Bufs(n, phase, cfg), Bufs(n, phase, cfg)
            part, cnt = norm_launch(ours, acc)
            launch("_guard", ours, cfg, acc, 0.0, part, cnt, INF)
            launch("_clip", ref, cfg, acc, 0.0, part, cnt, 1e30)
            assert bits(ours.norm).item() == bits(ref.norm).item(), (cfg, acc, n)


# -- 2. a poisoned gradient ----------------------------------------------------------------------
def positions(n, phase):
    """The first element, one inside the unaligned head (the first, when there is no other),
    the middle, the last element of the tail."""
    head = min((4 - phase) % 4, n)
    return [0, max(head - 1, 0), n // 2, n - 1]


POISON = list(itertools.product((NAN, INF, -INF), range(4)))


@pytest.mark.parametrize("n", NS)
def test_a_poisoned_step_writes_nothing_but_zeros_to_acc_and_is_counted(n):
    """Every variant at every phase, with one NaN / +Inf / -Inf element at one of the four
    positions -- with acc, in acc alone or in grad alone.  The (value, position, site)
    combinations rotate over the variants, so that every one of them meets every n and phase
    and every variant meets several of them.  param, the moments and slow keep their bits,
    every int of step_state its value, acc is all zero over the range, the sentinels are
    intact, the norm is NaN or +Inf and the skip is counted."""
    i = 0
    for phase, (cfg, acc, wd, clip) in itertools.product(range(4), VARIANTS):
        sites = ("acc", "g") if acc else ("g",)
        for site in sites:
            bad, where = POISON[i % len(POISON)]
            i += 5        # (coprime to 12: a rotation through every combination)
            at = positions(n, phase)[where]
            bufs = Bufs(n, phase, cfg)
            bufs.inner(site)[at] = bad
            before = bufs.snap()
            part, cnt = norm_launch(bufs, acc)
            launch("_guard", bufs, cfg, acc, wd, part, cnt, MAX_NORM if clip else INF)
            after = bufs.snap()
            what = (n, phase, cfg, acc, wd, clip, site, bad, at)
            if acc:
                assert int(bits(bufs.inner("acc")).abs().max()) == 0, what     # (+0.0)
                band = before["acc"].clone()
                band[bufs.lo:bufs.lo + n] = 0
                assert torch.equal(after.pop("acc"), band), what
                before.pop("acc")
            same(before, after, what)
            assert bufs.guard.tolist() == [1, 0, 0, 1], what
            norm = float(bufs.norm)
            assert math.isnan(norm) if math.isnan(bad) else norm == INF, what


def test_every_poison_at_every_position():
    """The full product of value x position x site at one odd size and every phase, for one
    variant of each family with acc (clipping, weight decay) and one without acc and without
    clipping (max_norm = +inf: rmsprop_guard_kernel, adam_guard_kernel alone)."""
    n = 4099
    for cfg, acc in itertools.product((CONFIGS[0], CONFIGS[2]), (True, False)):
        sites = ("acc", "g") if acc else ("g",)
        for phase, (bad, where), site in itertools.product(range(4), POISON, sites):
            bufs = Bufs(n, phase, cfg)
            bufs.inner(site)[positions(n, phase)[where]] = bad
            before = bufs.snap()
            part, cnt = norm_launch(bufs, acc)
            launch("_guard", bufs, cfg, acc, 1e-2 if acc else 0.0, part, cnt,
                   MAX_NORM if acc else INF)
            after = bufs.snap()
            what = (cfg, acc, phase, bad, where, site)
            if acc:
                assert int(bits(bufs.inner("acc")).abs().max()) == 0, what
                before.pop("acc"), after.pop("acc")
            same(before, after, what)
            assert bufs.guard.tolist() == [1, 0, 0, 1], what
            norm = float(bufs.norm)
            assert math.isnan(norm) if math.isnan(bad) else norm == INF, what


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[2]])
@pytest.mark.parametrize("acc", [False, True])
def test_two_ranges_of_one_step_both_skip_and_the_step_is_counted_once(cfg, acc):
    """Weight decay's launch per active range: the norm launch covers the whole buffer, the
    first range's launch takes norm_out and guard_state, the second NULL and ``advance``.  A
    NaN in the gap between the ranges skips both; acc is zeroed over the ranges only.  The
    same two launches on the finite gradient equal the ``_clip`` form's."""
    n, ranges = 4099, [(3, 1000), (1501, 2598)]
    for bad in (NAN, None):
        ours, ref = Bufs(n, 0, cfg), Bufs(n, 0, cfg)
        if bad is not None:
            ours.inner("g")[1200] = bad
        before = ours.snap()
        part, cnt = norm_launch(ours, acc)
        for i, (off, m) in enumerate(ranges):
            launch("_guard", ours, cfg, acc, 1e-2, part, cnt, MAX_NORM, off=off, n=m,
                   advance=i, first=i == 0)
            if bad is None:
                launch("_clip", ref, cfg, acc, 1e-2, part, cnt, MAX_NORM, off=off, n=m,
                       advance=i, first=i == 0)
        after = ours.snap()
        if bad is None:
            same(after, ref.snap(), (cfg, acc))
            assert ours.guard.tolist() == [0, -1, -1, 1]
            continue
        if acc:
            want = before.pop("acc").clone()
            for off, m in ranges:
                want[ours.lo + off:ours.lo + off + m] = 0
            assert torch.equal(after.pop("acc"), want)
        same(before, after, (cfg, acc))
        assert ours.guard.tolist() == [1, 0, 0, 1]
        assert math.isnan(float(ours.norm))


# -- 3. a finite gradient whose fp32 norm overflows ----------------------------------------------
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[1], CONFIGS[2]])
@pytest.mark.parametrize("acc", [False, True])
def test_a_norm_that_overflows_fp32_is_a_step_that_is_taken(cfg, acc):
    """Five elements of 3e38 among small ones, grad_scale 1: the fp64 sum of squares is finite
    (4.5e77), the fp32 norm is +Inf.  Guard alone: the plain pass bit for bit (coefficient the
    constant 1, not inf / inf).  With clipping: the ``_clip`` form, coefficient 0."""
    n = 257
    g = templates(n)["g"].clone()
    g[[0, 3, 100, 200, 256]] = 3e38
    a0 = templates(n)["acc"] * 1e-3
    for clip in (False, True):
        ours, ref = Bufs(n, 1, cfg, g, a0), Bufs(n, 1, cfg, g, a0)
        part, cnt = norm_launch(ours, acc)
        assert math.isfinite(float(part[:cnt].sum()))
        launch("_guard", ours, cfg, acc, 0.0, part, cnt, MAX_NORM if clip else INF, scale=1.0)
        launch("_clip" if clip else "", ref, cfg, acc, 0.0, part, cnt, MAX_NORM, scale=1.0)
        same(ours.snap(), ref.snap(), (cfg, acc, clip))
        assert ours.guard.tolist() == [0, -1, -1, 1]
        assert float(ours.norm) == INF
        assert not torch.equal(ours.inner("v"), templates(n)["v"])     # the step was taken
        if clip:      # coefficient 0: a zero gradient, yet a step
            assert bool(torch.isfinite(ours.inner("p")).all())


# -- 4. a sequence -------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("clip", [False, True])
def test_finite_nan_finite_inf_equals_the_two_finite_steps(acc, clip):
    """Adam with LookAhead k = 2 from t = 0: finite, NaN, finite, Inf.  The counters read
    {2, 1, 3, 4}; every buffer and step_state equal the two finite steps run through the
    unguarded pass (the ``_clip`` form when clipping) -- the sync falls on the second step
    TAKEN --; a second run gives the same bits."""
    n, cfg = 4099, ("scae_flat_opt", "adam", 2, 0, 0)
    gen = torch.Generator().manual_seed(77)
    grads = [torch.randn(n, generator=gen).cuda() for _ in range(4)]
    accs = [torch.randn(n, generator=gen).cuda() for _ in range(4)]
    runs = []
    for guarded in (True, True, False):
        bufs = Bufs(n, 2, cfg)
        for i, bad in enumerate((None, NAN, None, INF)):
            if bad is not None and not guarded:
                continue
            bufs.inner("g").copy_(grads[i])
            if acc:
                bufs.inner("acc").copy_(accs[i])
            if bad is not None:
                bufs.inner("acc" if acc and i == 1 else "g")[n // 3] = bad
            part, cnt = norm_launch(bufs, acc)
            form = "_guard" if guarded else "_clip" if clip else ""
            launch(form, bufs, cfg, acc, 1e-2, part, cnt, MAX_NORM if clip or not guarded
                   else INF)
        if guarded:
            assert bufs.guard.tolist() == [2, 1, 3, 4]
            assert not math.isfinite(float(bufs.norm))
        snap = bufs.snap()
        snap.pop("g")           # (the guarded runs end on the poisoned gradient)
        if not acc:
            snap.pop("acc")
        runs.append(snap)
    assert runs[2]["state"][:2].tolist() == [2, 1]
    same(runs[0], runs[1], "two runs")
    same(runs[0], runs[2], "against the unguarded steps")


# -- 5. TrainStep(nonfinite=...) -----------------------------------------------------------------
FORMS = {"eager": dict(use_graph=False), "graph": dict(), "launches": dict(replay="launches")}


def _state(step):
    opt = step.opt
    out = dict(param=step.flat.flat_param, step_state=opt.step_state,
               **dict(opt.state_buffers()))
    if opt.acc is not None:
        out["acc"] = opt.acc
    return {k: bits(v).clone() for k, v in out.items()}


_CLEAN = {}


def _clean(kind, k, form, keep):
    """An unguarded step given only the clean batches (groups) ``keep`` of six batches."""
    key = (kind, k, form, tuple(keep))
    if key not in _CLEAN:
        data = batches(6)
        _, step = small_step(noise=False, lr=1e-3, optimizer=kind,
                             accumulate_grad_batches=k, **FORMS[form])
        for i in keep:
            step(*data[i])
        torch.cuda.synchronize()
        _CLEAN[key] = (_state(step), step.optimizer_steps)
    return _CLEAN[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_a_poisoned_group_is_dropped_and_the_run_equals_a_clean_one(kind, form):
    """accumulate_grad_batches=2, six batches; a NaN written into one element of acc between
    the two batches of the second group (no forward or backward kernel sees it).  The guarded
    run ends bit for bit on the parameters, optimiser state and ``optimizer_steps - skipped``
    of an unguarded step given groups one and three only: one capture serves both outcomes.
    The skip is counted and the norm after it is non-finite."""
    data = batches(6)
    _, step = small_step(noise=False, lr=1e-3, optimizer=kind, accumulate_grad_batches=2,
                         nonfinite="skip", **FORMS[form])
    norms = []
    for i, (img, lab) in enumerate(data):
        step(img, lab)
        if i == 2:
            step.opt.acc[step.flat.numel // 2] = NAN
        if i % 2 == 1:
            norms.append(float(step.last_grad_norm()))
    torch.cuda.synchronize()
    assert math.isfinite(norms[0]) and math.isnan(norms[1]) and math.isfinite(norms[2])
    counters = step.nonfinite_steps()
    assert counters == dict(skipped=1, first=1, last=1, attempts=3)
    want, clean_steps = _clean(kind, 2, form, (0, 1, 4, 5))
    same(_state(step), want, (kind, form))
    assert step.optimizer_steps - counters["skipped"] == clean_steps == 2
    if form == "launches":
        assert step._klist, "the guarded step did not replay as a launch list"
    step.end_epoch()          # "skip" never raises


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_an_inf_class_head_weight_skips_that_step_only(kind, form):
    """k = 1: +Inf in one weight of the class head's linear layer, which feeds only the
    classification loss (its inputs are detached, and the loss tail derives no index from the
    logits but a bounded arg-max), for the second of three batches; the value is put back after
    the step.  The run equals the unguarded one given batches one and three."""
    data = batches(6)
    model, step = small_step(noise=False, lr=1e-3, optimizer=kind, nonfinite="skip",
                             **FORMS[form])
    w = model.prior_classifier[0].weight
    for i in (0, 1, 2):
        if i == 1:
            with torch.no_grad():
                old = w[1, 2].clone()
                w[1, 2] = INF
        step(*data[i])
        if i == 1:
            assert not math.isfinite(float(step.last_grad_norm()))
            with torch.no_grad():
                w[1, 2] = old
    torch.cuda.synchronize()
    counters = step.nonfinite_steps()
    assert counters == dict(skipped=1, first=1, last=1, attempts=3)
    want, clean_steps = _clean(kind, 1, form, (0, 2))
    same(_state(step), want, (kind, form))
    assert step.optimizer_steps - counters["skipped"] == clean_steps == 2
    assert math.isfinite(float(step.last_grad_norm()))


def _raised(fn):
    """``fn()`` raises NonFiniteGradientError -> (its counters, its text).  The caught exception
    is dropped here: its traceback holds the frames it passed through and the one that caught
    it, so keeping it in a local (``pytest.raises(...) as err``) ties the caller's step into a
    reference cycle -- the step, its graph and its launch list would then be freed by the
    cyclic collector at some later point, possibly in the middle of another step's capture,
    instead of by refcounting where the step is dropped."""
    from torch_scae_amd.train_step import NonFiniteGradientError
    with pytest.raises(NonFiniteGradientError) as err:
        fn()
    e = err.value
    out = (dict(skipped=e.skipped, first=e.first, last=e.last, attempts=e.attempts), str(e))
    del err, e
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_raise_reports_each_skip_once_and_restore_carries_the_counters(kind, form):
    """nonfinite="raise": ``end_epoch()`` raises NonFiniteGradientError naming the count, once
    per skip; ``optimizer_state_dict()`` reports the steps taken (the device count for Adam,
    ``optimizer_steps - skipped`` for plain RMSprop); ``snapshot()`` / ``restore()`` carry the
    counters, and the restored counters are the ones the same capture counts on from.  The
    step is freed by refcounting where the test drops it (no cycle through a caught error)."""
    import gc
    import weakref
    data = batches(6)
    model, step = small_step(noise=False, lr=1e-3, optimizer=kind, accumulate_grad_batches=2,
                             nonfinite="raise", **FORMS[form])
    step(*data[0]), step(*data[1])
    step.end_epoch()                         # nothing skipped: no error
    snap = step.snapshot()
    assert snap["guard_state"].tolist() == [0, -1, -1, 1]
    step(*data[2])
    step.opt.acc[5] = -INF
    step(*data[3])
    counters, text = _raised(step.end_epoch)
    assert counters == dict(skipped=1, first=1, last=1, attempts=2)
    assert "1 of 2" in text
    step.end_epoch()                         # reported once
    assert step.nonfinite_steps()["skipped"] == 1
    sd = step.optimizer_state_dict()
    assert {float(s["step"]) for s in sd["state"].values()} == {1.0}
    step.restore(snap)
    assert step.nonfinite_steps() == dict(skipped=0, first=-1, last=-1, attempts=1)
    step.end_epoch()                         # the restored count of reported skips: no error
    # the same capture counts on from the restored counters: a clean group, then a poisoned one
    step(*data[2]), step(*data[3])
    step(*data[4])
    step.opt.acc[7] = NAN
    step(*data[5])
    assert step.nonfinite_steps() == dict(skipped=1, first=2, last=2, attempts=3)
    assert _raised(step.check_nonfinite)[0]["skipped"] == 1
    step.check_nonfinite()                   # once
    if form == "launches":
        assert step._klist, "the guarded step did not replay as a launch list"
    assert bool(torch.isfinite(step.flat.flat_param).all())
    torch.cuda.synchronize()
    gone = weakref.ref(step)
    was = gc.isenabled()
    gc.disable()
    try:
        del step, model, snap, sd
        assert gone() is None, "the step is held by a reference cycle"
    finally:
        if was:
            gc.enable()


@pytest.mark.parametrize("kind,family", [("rmsprop", "scae_rmsprop"), ("adam", "scae_flat_opt")])
def test_construction_on_the_device_and_the_recorded_launch_lists(kind, family):
    """On ``cuda`` the guarded optimiser is built, its counters and norm in device memory.  The
    recorded launch lists, entry point by entry point: the unguarded step (nonfinite=None, and
    equally without the argument) ends in the ``_sums`` form of its pass and names no guard or
    norm launch anywhere; the guarded step's list is that list with its last entry replaced by
    the norm launch (hosting the column sums) and the ``_guard`` form -- one launch more, and
    nothing else of the step differs.  (Every argument of the optimiser's launches:
    test_nonfinite_guard_dispatch.py.)"""
    from torch_scae_amd import _lib
    data = batches(1)
    names, sizes = {}, {}
    for key, kw in (("none", dict(nonfinite=None)), ("absent", dict()),
                    ("skip", dict(nonfinite="skip"))):
        _, step = small_step(noise=False, lr=1e-3, optimizer=kind, replay="launches", **kw)
        step(*data[0])
        assert step._klist
        sizes[key] = _lib.load().scae_launch_list_size(step._klist)
        names[key] = [getattr(fn, "__name__", "") for fn, _, _ in step._cap.launches]
        assert names[key] and all(names[key])
        if key == "skip":
            assert step.opt.guard_state.is_cuda and step.opt.grad_norm.is_cuda
            assert step.opt.grad_sq.is_cuda
        else:
            assert step.opt.guard_state is None and step.opt.grad_sq is None
    assert names["none"] == names["absent"]
    plain, guarded = names["none"], names["skip"]
    assert not any("_guard" in x or "grad_sq" in x for x in plain)
    assert plain[-1] == f"{family}_sums_step_f32"
    assert guarded[-2:] == ["scae_grad_sq_partials_sums_f32", f"{family}_guard_step_f32"]
    assert guarded[:-2] == plain[:-1]
    assert sizes["skip"] == sizes["none"] + 1
