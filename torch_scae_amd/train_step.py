"""One SCAE training step = forward + SCAE.loss + backward (+ gradient
all-reduce + optimiser), optionally captured once into a HIP graph and
replayed: at B=128 the step is launch-latency bound, so
removing the per-launch host cost matters more than any single kernel.

Mirrors the semantics of the reference's BaseExperiment.training_step
(torch_scae_experiments/base_experiment.py:109-126)."""
import contextlib
import weakref

import torch

from . import ops
from . import replay as _replay   # (``replay`` is the steps' constructor argument)
from .data_parallel import (FlatParameters, GradNorms, _group_seen, accumulate_value,
                            all_reduce_gradients, broadcast_parameters, clip_value,
                            load_optimizer_state_dict, make_optimizer, nonfinite_value,
                            optimizer_state_dict, segment_norms_host, track_value, world)


class NonFiniteGradientError(ValueError):
    """``TrainStep(nonfinite="raise")``: optimiser steps were skipped because their gradient
    held a NaN or Inf element.  ``skipped``, ``first``, ``last``, ``attempts``: the guard's
    counters when it was raised."""

    def __init__(self, counters):
        self.__dict__.update(counters)
        super().__init__(
            "{skipped} of {attempts} optimiser steps had a non-finite gradient and were "
            "skipped (the first: optimiser step {first}, the last: {last}, 0-based); the "
            "parameters and the optimiser's state are those of the steps taken".format(**counters))


# the remainder step's noise generators: keyed by torch's seed XOR this (step_plan.StepPlan.
# noise_salt), so that its draws do not repeat the full step's
REMAINDER_NOISE_SALT = 0x52454D41494E4452 & ((1 << 63) - 1)

# parameters whose gradients are final once backward has come down through
# the two decoders (the object decoder's capsule MLPs alone are 66 % of the
# model): the first all-reduce bucket
EARLY_PREFIXES = ("obj_decoder.", "part_decoder.", "prior_classifier.",
                  "posterior_classifier.")


def update_batch(i, steps_in_epoch, k):
    """Lightning's rule for accumulate_grad_batches = k: the optimiser steps after batch i
    (0-based in the epoch) when (i + 1) % k == 0 or i is the epoch's last batch."""
    return (i + 1) % k == 0 or i == steps_in_epoch - 1


def update_at(view, batch, k):
    """``update_batch`` for the step ``view.take_step(batch)`` hands out next (the view is not
    advanced)."""
    last = view.steps_in_epoch(batch)
    return update_batch(view.cursor if view.cursor < last else 0, last, k)


class TrainStep:
    """collective modes (world > 1, or ``force_collective`` in a 1-rank group):

    * ``"2 buckets"`` (default when the model exposes the backward cut): the
      step is captured as TWO HIP graphs sharing one memory pool -- A: forward,
      loss, backward down to the inputs of the two decoders; B: the backward of
      the object encoder, template generator and part encoder.  The decoders'
      gradient block (flat[:n_front]) is all-reduced on RCCL's stream while B
      replays; the rest after B; then the fused RMSprop.  (Branches INSIDE one
      replayed graph serialise on this stack, DESIGN.md section 5, hence two
      graphs with the collective between them.)
    * ``"1 bucket"``: one graph, one all-reduce of the whole flat buffer after
      it (``overlap=False``, or a model without the cut).
    * ``"in graph"``: the all-reduce and the RMSprop step captured inside the
      one graph -- no host-side stream hand-off at all, nothing overlapped.
    ``collective_mode``: one of the three names (``"2 buckets"`` falls back to
    ``"1 bucket"`` for a model without the backward cut), ``"off"`` (no
    collective even with ranks: measurements only -- the ranks' parameters
    drift apart) or None (two buckets where possible).  ``bench.py`` measures
    all three on the ranks it is given and takes the fastest.

    ``optimizer``: the reference's choice (base_experiment.py:44-77) --
    ``"rmsprop"`` (RMSpropFlat, also ``True``), ``"adam"`` (AdamFlat),
    ``"radam"`` (RAdamFlat), or ``False`` / ``None`` for none; each optionally
    wrapped in LookAhead(``look_ahead_k``, ``look_ahead_alpha``) (optimizers.py:105-190),
    fused into the same pass.  eps = 1e-2 / batch_size**2 for all three
    (:46).  Every optimiser runs in every replay and collective mode.

    ``log_steps``: the capacity of the step's training log (0: no log).  Every step then
    leaves the `log` of BaseExperiment.training_step (base_experiment.py:109-126) -- the
    keys ``training_step()`` returns for this model, plus ``learning_rate`` -- as one row of
    a device ring, and adds it into an fp64 epoch accumulator.  Where the loss tail forms
    the whole scalar the row is written by the tail's batch combine (no launch and no torch
    operator more: ``step_from`` / ``replay="launches"`` keep their form); other models log
    with one launch of their own (scae_train_log_f32).  ``last_log()``,
    ``log_history()``, ``training_epoch_end()``, ``reset_log()``.  Rows are rank-local.

    A batch of 1 <= b < B (a ``drop_last=False`` loader's last batch, a view's short step)
    runs on the step's remainder step (``remainder_step(b)``): a second step of batch b,
    built on first use and cached (the last b only), that trains the same parameters with
    the same optimiser -- its moments, step count, LookAhead's slow weights, learning rate
    and the eps of THIS step's B (base_experiment.py:47) -- writes the same training log and
    counts in the same ``steps``.  It has its own input buffers, graph(s) or launch list,
    prologue and noise draws.  Not padded: the loss's between-example terms depend on the
    batch size.

    ``gradient_clip_val``: Lightning's ``Trainer(gradient_clip_val)`` -- every step clips the
    averaged gradient (after the all-reduce) to that global L2 norm before the optimiser, as
    torch.nn.utils.clip_grad_norm_ does; any value <= 0 (the default) is off, and then the
    step is exactly the unclipped one.  One launch more per step (scae_grad_sq_partials_f32:
    the gradient's sum of squares, the step's last column sums riding in it); the optimiser
    pass reads the coefficient from its partials.  ``last_grad_norm()``: the last step's norm
    before clipping, a device scalar.

    ``accumulate_grad_batches`` (k, an int >= 1): Lightning's ``Trainer(accumulate_grad_batches)``
    -- the optimiser steps once per group of k batches, on the sum of their gradients scaled
    by 1/k (the loss itself is not scaled: acc = g_1 + g_2 + ... in fp32, the 1/k rides in the
    optimiser pass).  ``step_from`` / ``train_epoch`` step after batch i of the epoch when
    (i + 1) % k == 0 or i is the epoch's last batch; ``step(image, label)`` counts groups, and
    ``end_epoch()`` first steps on a group still pending.  A batch that does not end its group
    ends in an accumulate pass instead of the optimiser (the column sums ride in it); the
    group's last batch in the accumulate form of the optimiser pass.  Each is a captured form
    of its own (captured on first use).  With a collective: no all-reduce until the group's
    last batch, then one of the accumulated gradient.  ``steps`` counts batches,
    ``optimizer_steps`` optimiser steps; k = 1 (the default) is the step as it was.

    ``track_grad_norm`` (p): Lightning's ``Trainer(track_grad_norm=p)`` -- 1, 2, ``float('inf')``
    or ``'inf'``; None, -1 or 0 (the default, Lightning's -1) is off, and then every captured
    form has exactly the launches it has without the argument.  Every OPTIMISER step (not
    every batch: the batches inside an accumulated group write nothing) leaves one row in a
    device ring of ``log_steps`` rows (1 without a log): the p-norm of the gradient the
    optimiser consumes -- after the all-reduce, with the scale the optimiser pass applies
    (1/k, 1/world), before clipping: what ``p.grad.norm(p)`` is in Lightning between backward
    and ``clip_grad_norm_`` -- per parameter that received a gradient, in ``FlatParameters``
    order (``obj_decoder.dummy_vote`` and ``posterior_classifier.*`` are absent from the default
    model, as Lightning skips ``p.grad is None``), then the p-norm of those.  ``split_capsules``
    (default True): a ``nn_ext.GroupedMLP`` stacked parameter is reported as one entry per
    capsule under the reference's per-capsule ``state_dict`` key -- which object capsules have
    stopped learning --; False: one entry per stacked tensor.  The segment table is fixed at
    the first capture (eager: the first optimiser step).  Two launches more per optimiser step
    (scae_segment_norms_f32: the chunks' fp64 partials, then the row; the cursor advances on
    the device, so a graph and a launch list replay into successive rows), after the step's
    last column sums: those no longer ride in the optimiser pass but launch on their own (with
    clipping they ride in its norm launch as before) -- the same bits either way, and the
    trained state equals the untracked step's bit for bit.  ``grad_norm_names()``,
    ``last_grad_norms()``, ``grad_norm_history()``; ``parameter_norms()`` for the weights'.  The
    remainder step and ``end_epoch``'s step on a pending group write to the same ring.

    ``nonfinite``: what an optimiser step does whose gradient -- the one the optimiser
    consumes: after the all-reduce, the group's sum when accumulating -- holds a NaN or +-Inf
    element.  None (the default): nothing special, the step is exactly the one it was (and one
    such element reaches the moments, then the parameters, then everything).  ``"skip"``: the
    form of Lightning's ``Trainer(terminate_on_nan)`` that mixed-precision harnesses carry:
    the step writes nothing -- parameters, both moment buffers, the momentum buffer,
    LookAhead's slow weights, the step count and the slow-made flag keep their bits, a
    poisoned accumulated group is dropped (acc zeroed) -- and is counted ({skipped, first,
    last, attempts}, int64, beside the optimiser's state).  The fp64 sum of squares of the
    gradient decides: finite exactly when every element is (the fp32 norm, which can overflow
    for finite gradients, does not).  A finite step has the unguarded step's bits.  With a
    collective the sum is taken after the all-reduce, so every rank decides alike.
    ``"raise"``: the same, and ``end_epoch()`` reads the counters (one read per epoch, never
    one per step) and raises ``NonFiniteGradientError`` when a step was skipped since the
    last check; ``check_nonfinite()`` does so on demand.  ``nonfinite_steps()``: the counters.
    The guard is on the GRADIENT: a non-finite loss whose gradients are all finite is not
    detected.  A tracked ``GradNorms`` row is written for a skipped step too (its total is
    non-finite: the row shows which segment blew up), and ``last_grad_norm()`` shows the NaN
    or Inf.  ``steps`` and ``optimizer_steps`` stay HOST counts of batches and of ATTEMPTED
    optimiser steps, skipped ones included; ``optimizer_state_dict()`` reports ``step`` as the
    optimiser's own count where it keeps one and as ``optimizer_steps - skipped`` for plain
    RMSprop.  ``snapshot()`` / ``restore()`` carry the counters.  On a HIP device the
    decision is taken inside the optimiser pass (the guarded forms, scae_*_guard_step_f32, on
    the partial sums of the same norm launch clipping uses: one launch more per optimiser step
    than the unguarded, unclipped step, none more than the clipped one), and the counters and
    the norm live in device memory: one captured graph or launch list serves both outcomes,
    and a replayed step reads nothing back.
    """

    MODES = ("2 buckets", "1 bucket", "in graph")

    def __init__(self, model, batch_size, image_shape, lr=3e-5, use_graph=True,
                 optimizer=True, momentum=0.9, weight_decay=0.0,
                 lr_decay_rate=0.997, autocast_dtype=None,
                 force_collective=False, overlap=True, lazy_render=True,
                 prologue=True, fuse_kernels=True, collective_mode=None,
                 replay="graph", betas=(0.9, 0.999),
                 look_ahead=False, look_ahead_k=5, look_ahead_alpha=0.5,
                 log_steps=0, gradient_clip_val=0.0, accumulate_grad_batches=1,
                 track_grad_norm=None, split_capsules=True, nonfinite=None):
        if not isinstance(log_steps, int) or isinstance(log_steps, bool) or log_steps < 0:
            raise ValueError(f"log_steps must be an int >= 0, got {log_steps!r}")
        gradient_clip_val = clip_value(gradient_clip_val)
        if gradient_clip_val and optimizer in (None, False):
            raise ValueError("gradient_clip_val needs an optimizer: clipping is part of its step")
        track_grad_norm = track_value(track_grad_norm)
        if track_grad_norm is not None and optimizer in (None, False):
            raise ValueError("track_grad_norm needs an optimizer: the norms are those of the "
                             "gradient its step consumes")
        self.nonfinite = nonfinite_value(nonfinite)
        if self.nonfinite and optimizer in (None, False):
            raise ValueError("nonfinite needs an optimizer: the guard is part of its step")
        self._guard_checked = [0]   # skips already reported by "raise" (shared with the
        #                             remainder step)
        self.accumulate_grad_batches = accumulate_value(accumulate_grad_batches)
        if self.accumulate_grad_batches > 1 and optimizer in (None, False):
            raise ValueError("accumulate_grad_batches needs an optimizer: it steps once a group")
        # batches accumulated since the last optimiser step, optimiser steps taken (one dict,
        # shared with the remainder step)
        self._acc_state = {"pending": 0, "optimizer_steps": 0}
        self._form = "update"     # the captured form the step holds in _cap (with its loss)
        self._cap = _replay.Captured()
        self._other_cap = self._other_loss = None   # ... the other one, once swapped out
        self._parent = None      # (a remainder step: the step whose state it shares)
        self._rem = None         # the cached remainder step (remainder_step)
        self.model = model
        self.device = next(model.parameters()).device
        if log_steps and self.device.type != "cuda":
            raise ValueError("log_steps needs a model on a HIP device (the log's epilogue "
                             "is a device kernel)")
        self.world = world()[1]
        if collective_mode not in (None, "off") + self.MODES:
            raise ValueError(f"collective_mode must be one of {self.MODES}, "
                             f"'off' or None, got {collective_mode!r}")
        self.collective = collective_mode != "off" and (
            self.world > 1 or (force_collective
                               and torch.distributed.is_initialized()))
        self.in_graph_collective = self.collective and use_graph and \
            collective_mode == "in graph"
        overlap = overlap and collective_mode in (None, "2 buckets")
        self.split = bool(self.collective and overlap
                          and not self.in_graph_collective
                          # the conditions under which SCAE._forward cuts
                          # the backward in two (res._phase_cut)
                          and getattr(model, "stop_grad_caps_target", False)
                          and getattr(model, "vote_type", None) == "enc"
                          and getattr(model, "presence_type", None) == "enc")
        self.flat = FlatParameters(
            model, front=(lambda n: n.startswith(EARLY_PREFIXES))
            if self.split else None)
        if self.split and self.flat.n_front in (0, self.flat.numel):
            self.split = False
        if hasattr(model, "split_backward"):
            model.split_backward = self.split
        # loss-only step: the (B, M+1, ., H, W) reconstruction tensors, which
        # neither SCAE.loss nor its backward read, render on first access.
        # Scoped to the step's own forward (_lazy): the user's model keeps
        # returning plain AttrDicts outside it
        dec = getattr(model, "part_decoder", None)
        self._lazy_dec = dec if lazy_render and hasattr(dec, "lazy_render") \
            else None
        # the step's noise draws and parameter-only folding products ride with
        # the batch hand-over in ONE launch ahead of the step (ops.StepPrologue)
        self._pro = ops.StepPrologue() if prologue and \
            self.device.type == "cuda" else None
        # this step's launch plan (step_plan.py): the only holder of its
        # parked launches, deferred column sums, prologue buffers and noise
        # generators -- nothing of a step lives in module state, so several
        # steps (models) can interleave in one process
        self.plan = ops.StepPlan("train step", prologue=self._pro)
        self.collective_mode = None if not self.collective else \
            "in graph" if self.in_graph_collective else \
            "2 buckets, the first overlapping the encoder backward" \
            if self.split else "1 bucket after the backward"
        broadcast_parameters(self.flat)
        # eps = 1e-2 / bs**2 for every optimiser (base_experiment.py:46)
        if optimizer is True:
            optimizer = "rmsprop"
        self.opt = make_optimizer(
            optimizer, self.flat, lr=lr, eps=1e-2 / float(batch_size) ** 2,
            betas=betas, momentum=momentum, weight_decay=weight_decay,
            look_ahead=look_ahead, look_ahead_k=look_ahead_k,
            look_ahead_alpha=look_ahead_alpha, gradient_clip_val=gradient_clip_val,
            accumulate_grad_batches=self.accumulate_grad_batches,
            nonfinite="skip" if self.nonfinite else None) \
            if optimizer not in (None, False) else None
        # the tracked gradient norms (data_parallel.GradNorms): on the optimiser, whose step
        # launches them -- the remainder step shares both
        if track_grad_norm is not None:
            self.opt.track = GradNorms(self.flat, model, track_grad_norm,
                                       capacity=log_steps or 1, split_capsules=split_capsules)
        self.steps = 0           # steps taken (host count, with the remainder step's; the
        #                          optimisers keep their own)
        # the training log (ops.TrainLog): ring, step counter, epoch accumulator
        self.train_log = ops.TrainLog(
            log_steps, self.device, lr=None if self.opt is None else self.opt.lr_dev) \
            if log_steps else None
        self._log_keys = None    # the log's keys, from the logged step's SCAE.loss
        self._warming = False    # a capture's warm-ups: not logged
        self.lr_decay_rate = lr_decay_rate
        # the backward's last column sums (parameter gradients only) ride in the optimiser's
        # launch: one launch less on the step's dependent chain.  Not with a collective (the
        # all-reduce reads the finished gradient buffer first) nor with weight decay.  With
        # clipping they ride in the norm launch, the optimiser's first.
        self.plan.sums_to_optimizer = bool(
            self.opt is not None and fuse_kernels and not self.collective
            and weight_decay == 0 and self.device.type == "cuda")
        # torch.bfloat16 (BASELINE.json configs[2]): the GEMM-shaped kernels --
        # K8 convolutions, K7 capsule-MLP / 1x1-conv GEMMs, forward and backward
        # -- take bf16 operands with fp32 accumulation (ops.mfma_bf16); the
        # mixture likelihood, the capsule likelihood, the fused object encoder
        # and all reductions stay fp32
        if autocast_dtype not in (None, torch.bfloat16):
            raise ValueError("autocast_dtype must be None or torch.bfloat16")
        self.autocast_dtype = autocast_dtype
        self.log = None          # device tensors of the last step's log dict
        self.image = torch.zeros(batch_size, *image_shape, device=self.device)
        self.label = torch.zeros(batch_size, dtype=torch.long,
                                 device=self.device)
        self.loss = torch.zeros((), device=self.device)
        self._one = torch.ones((), device=self.device)   # d loss / d loss
        self.use_graph = use_graph
        # how a captured step is re-issued: "graph" (hipGraphLaunch: ~10 us of host time and
        # ~8.6 us of device time between two replays, tools/graph_gap_probe.py) or "launches"
        # (the library's record of the captured launches -- replay.LaunchList.run: a
        # hipLaunchKernel each on the current stream, no per-replay device cost: 0-5 us per
        # step at cfg-2 depending on the host -- ~18 us of host time per launch leave little
        # room beside a 550 us step --, tools/launch_list_probe.py; single-rank steps only,
        # and only when the captured graph holds nothing but those launches: otherwise --
        # e.g. training_step()'s log outputs, computed by torch kernels -- the graph replays)
        if replay not in ("graph", "launches"):
            raise ValueError("replay must be 'graph' or 'launches'")
        self.replay = replay
        # independent kernels of the step sharing launches (ops.step_fusion:
        # the reconstruction likelihood rides with the object encoder's trunk)
        self.fuse_kernels = fuse_kernels
        self.skip_collective = False
        self._capturing = False
        self._stream = None
        self._with_log = False
        self._cut = None

    # the captured form in use, read-only (replay.Captured; _klist: its list's raw handle)
    graph = _replay.forwarded("graph")
    graph_b = _replay.forwarded("graph_b")
    _klist = _replay.forwarded("handle")
    _launches = _replay.forwarded("launches")
    graph_nodes = _replay.forwarded("nodes")

    @property
    def steps(self):
        return self._steps if self._parent is None else self._parent.steps

    @steps.setter
    def steps(self, value):
        if self._parent is None:
            self._steps = value
        else:
            self._parent.steps = value

    @property
    def optimizer_steps(self):
        """Optimiser steps taken (== ``steps`` without accumulation)."""
        return self._acc_state["optimizer_steps"]

    # -- the two captured forms of an accumulating step -------------------------
    def _tail_captured(self):
        return self.use_graph and not self.split and \
            (not self.collective or self.in_graph_collective)

    def _use_form(self, form):
        """Make ``form`` ("update": the optimiser ends the step; "acc": the accumulate pass)
        the one the step's graph attributes hold, stashing the other (captured lazily)."""
        if form == self._form:
            return
        if self._tail_captured():
            cap, loss = self._other_cap, self._other_loss
            if cap is None:
                cap, loss = _replay.Captured(), torch.zeros((), device=self.device)
            self._other_cap, self._other_loss = self._cap, self.loss
            self._cap, self.loss = cap, loss
        self._form = form

    def _drop_forms(self):
        """Forget both captured forms (the next step captures again)."""
        self._cap.drop()
        if self._other_cap is not None:
            self._other_cap.drop()
        self._other_cap = self._other_loss = None

    # -- the remainder step ---------------------------------------------------
    def remainder_step(self, size):
        """The step that runs this step's batches of ``size`` (1 <= size < B): built on the
        first call for that size and cached -- only the last size: another one rebuilds it.
        ``capture()`` on it builds its graph(s) ahead of the first short batch (its warm-ups
        draw from its own noise generator, as this step's do)."""
        if self._parent is not None:
            raise ValueError("a remainder step has no remainder step of its own")
        B = self.image.shape[0]
        if not (isinstance(size, int) and 1 <= size < B):
            raise ValueError(f"a remainder batch holds 1 .. {B - 1} examples, got {size!r}")
        rem = self._rem
        if rem is None or rem.image.shape[0] != size:
            if rem is not None:
                rem._drop_forms()
            self._rem = None
            rem = self._rem = self._remainder_of(size)
        if self._with_log and not rem._with_log:
            rem._with_log = True
            rem._drop_forms()
        return rem

    def _remainder_of(self, size):
        """A step of batch ``size`` sharing this step's training state: the model and its
        FlatParameters (a second one would re-home the parameters under this step's captured
        graph), the optimiser object, the training log, the host step count, the capture
        stream (autograd keeps each parameter's AccumulateGrad node with the stream it first
        ran on) and every setting.  Its own: plan, prologue, input buffers, graph(s) / launch
        list and noise generators (salted: its draws are not this step's)."""
        rem = TrainStep.__new__(TrainStep)
        rem.__dict__.update(self.__dict__)
        if self._stream is None and self.device.type == "cuda":
            self._stream = torch.cuda.Stream(self.device)
        rem._stream = self._stream
        # (a weak reference: a cycle would leave both steps to the cyclic collector, whose
        # run may then free their graphs in the middle of another step's capture)
        rem._parent, rem._rem = weakref.proxy(self), None
        rem._pro = ops.StepPrologue() if self._pro is not None else None
        rem.plan = ops.StepPlan("train step remainder", prologue=rem._pro)
        rem.plan.sums_to_optimizer = self.plan.sums_to_optimizer
        rem.plan.noise_salt = REMAINDER_NOISE_SALT
        rem.image = torch.zeros(size, *self.image.shape[1:], device=self.device)
        rem.label = torch.zeros(size, dtype=torch.long, device=self.device)
        rem.loss = torch.zeros((), device=self.device)
        rem.log = None
        rem._cap, rem._other_cap, rem._other_loss = _replay.Captured(), None, None
        rem._cut = None
        rem._capturing = rem._warming = False
        rem._form = "update"
        return rem

    def _for_batch(self, size):
        """The step that runs a batch of ``size``: this one, or its remainder step."""
        B = self.image.shape[0]
        if size == B:
            return self
        if self._parent is not None or not 1 <= size < B:
            raise ValueError(f"a step of batch {B} takes batches of 1 .. {B} examples, "
                             f"got {size}" if self._parent is None else
                             f"a remainder step takes batches of {B} only, got {size}")
        return self.remainder_step(int(size))

    @contextlib.contextmanager
    def _lazy(self):
        dec = self._lazy_dec
        if dec is None:
            yield
            return
        prev, dec.lazy_render = dec.lazy_render, True
        try:
            yield
        finally:
            dec.lazy_render = prev

    # -- the step in two parts ------------------------------------------------
    def _part_a(self):
        """forward + loss + backward (split: down to the decoders' inputs)."""
        plan = self.plan
        stale = plan.take_held_sums()
        if stale and not self._capturing:
            # (a backward nobody followed by the optimiser; inside a capture they are the
            # warm-ups' -- whose gradients nobody reads -- and are dropped: launched here they
            # would become a launch of every replay)
            ops._launch_sum_units(stale)
        self.flat.clear_grads()
        tlog = self.train_log if not self._warming else None
        if tlog is not None:
            tlog.fused = False
        with plan.active(), plan.precision(self.autocast_dtype is not None), \
                self._lazy(), plan.logging(tlog), \
                plan.fusing(self.image if self.fuse_kernels else None):
            res = self.model(self.image)
            loss, info = self.model.loss(res, self.image, self.label)
            # a resident seed: no ones_like fill per step; the column sums that
            # only produce parameter gradients wait for ONE launch at the end
            with plan.deferring():
                loss.backward(self._one)
        if tlog is not None:
            self._log_step(tlog, res, loss, info)
        self._cut = res.get("_phase_cut") if self.split else None
        self.flat.gather_grads(None if self._cut is None else 0)
        if self._capturing:
            # the captured loss tensor lives in the graph's private pool at a
            # fixed address: expose it instead of copying it out every replay
            self.loss = loss.detach()
        else:
            self.loss.copy_(loss.detach())
        if self._with_log:
            # the `log` dict of BaseExperiment.training_step (:118-125)
            acc = self.model.calculate_accuracy(res, self.label) \
                if self.model.n_classes is not None else None
            fresh = dict(loss=loss.detach(), **{k: v.detach()
                                                for k, v in info.items()})
            if acc is not None:
                fresh["accuracy"] = acc.detach()
            if self.log is None:
                self.log = {k: torch.zeros_like(v) for k, v in fresh.items()}
            for k, v in fresh.items():
                self.log[k].copy_(v)

    def _log_step(self, tlog, res, loss, info):
        """The log's keys from this step's SCAE.loss; a loss the tail did not complete logs
        with the epilogue's own launch."""
        keys = ["loss", *info.keys()]
        if self.model.n_classes is not None:
            keys.append("accuracy")
        keys.append("learning_rate")
        unknown = [k for k in keys if k not in ops.TRAIN_LOG_INDEX]
        if unknown:
            raise ValueError(f"log keys {unknown} have no place in the training log's row")
        self._log_keys = keys
        if self._parent is not None:
            self._parent._log_keys = keys
        if tlog.fused:
            return
        from .eval_step import out12_from_log
        labelled = self.model.n_classes is not None
        extra = [info.get(k) for k in ("mse", "part_caps_loss")]
        with self.plan.active():
            extra2 = None if extra == [None, None] else torch.stack(
                [torch.zeros((), device=self.device) if v is None
                 else v.detach().reshape(()).float() for v in extra])
            tlog.log_alone(loss.detach(), out12_from_log(loss, info), extra2,
                           res.prior_cls_prob.detach() if labelled else None,
                           res.posterior_cls_prob.detach() if labelled else None,
                           self.label if labelled else None)

    def _part_b(self):
        """split only: the backward below the decoders' inputs."""
        if self._cut is None:
            return
        srcs, leaves = self._cut
        self._cut = None
        keep = [(t, l.grad) for t, l in zip(srcs, leaves)
                if l.grad is not None]
        plan = self.plan
        with plan.active(), plan.precision(self.autocast_dtype is not None), \
                plan.deferring():
            torch.autograd.backward([t for t, _ in keep],
                                    [g for _, g in keep])
        self.flat.gather_grads(1)

    def _fwd_bwd(self):
        self._part_a()
        self._part_b()

    def _reduce(self, which=None, async_op=False):
        # SUM all-reduce; the 1/world scale rides in the optimiser kernel
        if self.skip_collective:      # measurement only (bench.py's comm leg)
            return None
        return all_reduce_gradients(self.flat, average=self.opt is None,
                                    which=which, async_op=async_op,
                                    force=self.collective)

    def _finish(self):
        k = self.accumulate_grad_batches
        if k > 1:
            self._finish_group()
            return
        if self.collective:
            self._reduce()
        if self.opt is not None:
            self.opt.step(grad_scale=1.0 / self.world,
                          sum_units=self.plan.take_held_sums())

    def _finish_group(self):
        """The end of an accumulating step: the accumulate pass ("acc" form), or the
        optimiser on the group's gradient -- with a collective, folded into the flat
        gradient buffer and all-reduced first."""
        if self._form == "acc":
            self.opt.accumulate(sum_units=self.plan.take_held_sums())
            return
        scale = 1.0 / (self.accumulate_grad_batches * self.world)
        if self.collective:
            self.opt.fold()
            self._reduce()
            self.opt.step(grad_scale=scale, sum_units=self.plan.take_held_sums(),
                          with_acc=False)
        else:
            self.opt.step(grad_scale=scale, sum_units=self.plan.take_held_sums())

    def _after_buckets(self):
        """What follows a split step's parts (their all-reduces included)."""
        if self.accumulate_grad_batches > 1:
            self._finish_group()
        elif self.opt is not None:
            self.opt.step(grad_scale=1.0 / self.world)

    def _run(self, part_a, part_b):
        """One step from its two parts (graph replays or eager calls)."""
        if not self.split:
            part_a()
            return
        if self.accumulate_grad_batches > 1:   # (one all-reduce after the backward: _finish_group)
            part_a()
            part_b()
            return
        part_a()
        w0 = self._reduce(0, async_op=True)     # overlaps part B
        part_b()
        w1 = self._reduce(1, async_op=True)
        for w in (w0, w1):
            if w is not None:
                w.wait()                        # stream-side wait, not a host one

    def _capture(self):
        # warm up on a side stream (allocator, lazy init), then capture; the
        # same stream for every (re-)capture: autograd keeps each parameter's
        # AccumulateGrad node, and with it the stream it first ran on
        if self._stream is None:
            self._stream = torch.cuda.Stream()
        s = self._stream
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._warming = True        # (the warm-ups' batches are not the log's)
            try:
                for _ in range(3):
                    self._refresh_prologue()
                    self._fwd_bwd()
            finally:
                self._warming = False
            self._refresh_prologue()    # what the capture below consumes
            if self.grad_norms is not None:
                # the segment table goes to the device here: the warm-ups have shown which
                # parameters receive a gradient, and the capture below cannot copy
                self.grad_norms.build(_group_seen(self.opt))
        torch.cuda.current_stream().wait_stream(s)
        # capture on the SAME stream the warm-up ran on: autograd caches each
        # parameter's AccumulateGrad node together with its stream
        self._cap.drop()
        # an accumulating step's second form shares the first one's memory pool: the two
        # never replay at once, and each rewrites its temporaries before reading them
        other = self._other_cap.graph if self._other_cap is not None else None
        self._capturing = True
        try:
            # the step replays as the library's launch list (replay.adopts) on a single rank
            # only: a collective is a node of the graph that the list does not have
            cap = _replay.capture(
                s, self._captured, keep_graph=self.replay == "launches",
                pool=None if other is None else other.pool(),
                want_list=not self.collective and not self.split and self.replay == "launches")
            if self.collective:
                cap.launches = None
            if self.split:
                # part B allocates from part A's pool: the tensors A left for it
                # (saved activations, the cut gradients) are alive across the two
                # captures, and the graphs are always replayed A, B, A, B, ...
                cap.graph_b = torch.cuda.CUDAGraph()
                with torch.cuda.graph(cap.graph_b, stream=s, pool=cap.graph.pool(),
                                      capture_error_mode=_replay.capture_error_mode()):
                    self._part_b()
            self._cap = cap
        finally:
            # (a capture that raised -- out of memory, an op that cannot be captured -- must
            # not leave the step in capture mode: eager calls would drop held column sums
            # and alias self.loss to a pool tensor)
            self._capturing = False

    def _captured(self):
        """What the step's (first) graph holds."""
        self._part_a()
        if not self.split:
            self._part_b()
            if not self.collective or self.in_graph_collective:
                self._finish()

    def capture(self):
        """Build the step's HIP graph(s) now instead of at the first call
        (no-op without ``use_graph`` or when already built).  Runs the
        forward / backward warm-ups on whatever the resident input buffers
        hold; parameters and optimiser state are not touched."""
        if self.use_graph and self.graph is None:
            self._capture()
            self._refresh_prologue()   # the capture consumed the last one

    def prepare(self, image, label):
        """Stage a batch and build the step's graph(s) WITHOUT stepping: what
        a measurement does before it snapshots the state it wants to time."""
        self._stage(image, label)
        self.capture()

    def snapshot(self):
        """The training state this step advances -- parameters, the
        optimiser's two moment buffers, its step count, LookAhead's slow weights
        and its learning rate -- as clones (a few device copies; not for use
        inside a timed region).  ``restore``
        puts it back, under an already captured graph too: the graph reads
        and writes the same flat buffers, and everything derived from the
        parameters (folding products, filter re-layouts) is recomputed by
        every step's own prologue / graph."""
        snap = {"param": self.flat.flat_param.clone(), "steps": self.steps}
        if self.accumulate_grad_batches > 1:
            snap.update(acc=self.opt.acc.clone(), acc_state=dict(self._acc_state))
        if self.opt is not None:
            snap.update({k: b.clone() for k, b in self.opt.state_buffers()},
                        lr=self.opt.lr)
            if self.opt.counts_steps:
                snap["step_state"] = self.opt.step_state.clone()
            if self.opt.slow is not None:
                snap["slow"] = self.opt.slow.clone()
            if self.opt.guard_state is not None:
                snap["guard_state"] = self.opt.guard_state.clone()
                snap["guard_checked"] = self._guard_checked[0]
        return snap

    @torch.no_grad()
    def restore(self, snap):
        self.flat.flat_param.copy_(snap["param"])
        self.steps = snap.get("steps", self.steps)
        if "acc" in snap:
            self.opt.acc.copy_(snap["acc"])
            self._acc_state.update(snap["acc_state"])
        if self.opt is not None:
            for k, b in self.opt.state_buffers():
                b.copy_(snap[k])
            if "step_state" in snap:
                self.opt.step_state.copy_(snap["step_state"])
            if "slow" in snap:
                self.opt.slow.copy_(snap["slow"])
            if "guard_state" in snap and self.opt.guard_state is not None:
                self.opt.guard_state.copy_(snap["guard_state"])
                self._guard_checked[0] = snap["guard_checked"]
            if self.opt.lr != snap["lr"]:
                self.opt.set_lr(snap["lr"])

    def optimizer_state_dict(self):
        """The optimiser's state in ``torch.optim``'s schema (state keyed by the
        parameter's index in ``model.parameters()``): loads into the matching
        stock optimiser over the model's parameters
        (data_parallel.optimizer_state_dict; with LookAhead a ``slow_state``
        keyed the same way).  ``step``: the device count for the optimisers that keep one
        (skipped steps do not advance it); for plain RMSprop the host's count of optimiser
        steps, less the guard's ``skipped`` when the guard is on (one more read)."""
        if self.opt is None:
            raise ValueError("this step has no optimiser")
        steps = self.optimizer_steps if self.accumulate_grad_batches > 1 else self.steps
        if self.nonfinite and not self.opt.counts_steps:
            steps -= self.nonfinite_steps()["skipped"]
        return optimizer_state_dict(self.opt, list(self.model.parameters()), steps=steps)

    def load_optimizer_state_dict(self, sd):
        """Load a ``torch.optim``-schema state (``optimizer_state_dict``, or a
        stock optimiser's over ``model.parameters()``); a captured graph
        replays from it.  ``steps`` and ``optimizer_steps`` become the state's step
        count; accumulating, a group in progress is dropped (acc zeroed, nothing
        pending)."""
        if self.opt is None:
            raise ValueError("this step has no optimiser")
        self.steps = load_optimizer_state_dict(
            self.opt, list(self.model.parameters()), sd)
        # the state dict holds optimiser steps and no group in progress: a group pending
        # here is dropped (acc cleared), and the batch count restarts at the step count
        self._acc_state.update(pending=0, optimizer_steps=self.steps)
        if self.opt.acc is not None:
            self.opt.acc.zero_()

    def _refresh_prologue(self):
        _replay.refresh_prologue(self.plan, self._pro, self.image)

    def _stage(self, image, label):
        """The batch into the resident input buffers (replay.stage)."""
        _replay.stage(self.plan, self._pro, self.image, self.label, image, label, self.device,
                      stage_batch=True)

    def _stage_source(self, view, epoch, position):
        """The view's batch at ``position`` of ``epoch`` gathered (replay.stage_source)."""
        _replay.stage_source(self.plan, self._pro, self.image, self.label, view, epoch, position)

    def step_from(self, view):
        """One step on the next batch of ``view`` (data.DatasetView of a
        ResidentDataset on this step's device): the batch is gathered -- order, padding
        and shifts applied -- in the step's prologue launch, with no torch operator and no
        host-to-device copy.  Advances the view's cursor and wraps to its next epoch after
        ``view.steps_in_epoch(batch)`` steps (the LR decays in ``end_epoch``); a
        ``drop_last=False`` view's short step runs on the remainder step, gathered the same
        way.  -> the loss (a device tensor the next step overwrites)."""
        B = self.image.shape[0]
        view.check(B, self.image.shape[1:])
        if self.world > 1 and (view.rank, view.world) != world():
            raise ValueError(f"view of rank {view.rank} / world {view.world} in a step "
                             f"of rank {world()[0]} / world {self.world}")
        update = update_at(view, B, self.accumulate_grad_batches) \
            if self.accumulate_grad_batches > 1 else None
        at = view.take_step(B)
        step = self._for_batch(at.size)
        step._stage_source(view, *at)
        return step._step_staged(update)

    def train_epoch(self, view):
        """The view's remaining steps of its current epoch (``step_from``: the full ones,
        then the short one of a ``drop_last=False`` view), then ``end_epoch()`` once.
        -> the last step's loss (a device tensor)."""
        B = self.image.shape[0]
        view.check(B, self.image.shape[1:])
        epoch, loss = view.epoch, None
        while view.epoch == epoch:
            loss = self.step_from(view)
        self.end_epoch()
        return loss

    def __call__(self, image, label):
        """image / label may be device tensors; copied into the static inputs.  A batch of
        1 <= b < B runs on the remainder step."""
        step = self._for_batch(image.shape[0])
        step._stage(image, label)
        return step._step_staged()

    def _step_staged(self, update=None):
        """``update``: whether this batch ends its group (accumulating; None: the host's
        count of the group's batches decides)."""
        k, acc = self.accumulate_grad_batches, self._acc_state
        if k > 1:
            if update is None:
                update = acc["pending"] + 1 >= k
            self._use_form("update" if update else "acc")
        self.steps += 1
        if self.train_log is not None:
            self.train_log.count += 1   # (the row this step writes)
        self._step_form()
        if k > 1 and not update:
            acc["pending"] += 1
        elif self.opt is not None:
            acc["pending"] = 0
            acc["optimizer_steps"] += 1
            if self.grad_norms is not None:
                self.grad_norms.count += 1   # (the row this optimiser step wrote)
        return self.loss

    def _step_form(self):
        if self.use_graph:
            self.capture()
            if self.split:
                self._run(self.graph.replay, self.graph_b.replay)
                self._after_buckets()
            else:
                if self.replay == "launches":    # (a setting read per step: bench.py flips it)
                    self._cap.replay(self.device)
                else:
                    self.graph.replay()
                if self.collective and not self.in_graph_collective:
                    self._finish()
        elif self.split:
            self._run(self._part_a, self._part_b)
            self._after_buckets()
        else:
            self._fwd_bwd()
            self._finish()

    def training_step(self, image, label):
        """-> {'loss': tensor, 'log': {...}} like BaseExperiment.training_step
        (base_experiment.py:109-126); the log values are device tensors that
        the next call overwrites.  Builds the step with the log outputs on
        first use (costs a few extra small kernels per step)."""
        if not self._with_log:
            self._with_log = True
            self._drop_forms()
        step = self._for_batch(image.shape[0])
        loss = step(image, label)
        return dict(loss=loss, log=step.log)

    def last_grad_norm(self):
        """The last step's total gradient L2 norm before clipping (the total that Lightning's
        ``track_grad_norm=2`` reports): a device scalar the next step overwrites, no read.  A
        step that clips returns the clip's own norm, a guarded one (``nonfinite``) the guard's
        -- NaN or Inf on a skipped step --; one that only tracks with p = 2 the
        tracked total (None before its first optimiser step); None otherwise."""
        opt = self.opt
        if opt is None:
            return None
        if opt.max_norm or opt.nonfinite:
            return opt.grad_norm
        if opt.track is not None and opt.track.p == 2.0:
            row = opt.track.last()
            return None if row is None else row[-1]
        return None

    # -- the non-finite guard (nonfinite) -----------------------------------------------------
    def nonfinite_steps(self):
        """-> {'skipped', 'first', 'last', 'attempts'}: the guard's counters (one host read).
        attempts: guarded optimiser steps so far; first / last: the attempts values (0-based)
        of the first and the last skipped one, -1 before any."""
        if not self.nonfinite:
            raise ValueError("this step has no non-finite guard (TrainStep(nonfinite=...))")
        vals = self.opt.guard_state.cpu().tolist()
        return dict(zip(("skipped", "first", "last", "attempts"), vals))

    def check_nonfinite(self):
        """``nonfinite="raise"``'s check, on demand (one host read): raises
        ``NonFiniteGradientError`` when an optimiser step was skipped since the last check.
        -> the counters otherwise."""
        counters = self.nonfinite_steps()
        if counters["skipped"] > self._guard_checked[0]:
            self._guard_checked[0] = counters["skipped"]
            raise NonFiniteGradientError(counters)
        return counters

    # -- tracked gradient norms (track_grad_norm) ---------------------------------------------
    @property
    def grad_norms(self):
        """The step's ``data_parallel.GradNorms`` (None: not tracking)."""
        return None if self.opt is None else self.opt.track

    def _need_norms(self, built=True):
        trk = self.grad_norms
        if trk is None:
            raise ValueError("this step tracks no gradient norms (TrainStep(track_grad_norm=...))")
        if built and trk.segments is None:
            raise ValueError("the tracked segments are fixed by the first capture or optimiser "
                             "step: take a step (or capture()) first")
        return trk

    def grad_norm_names(self, prefix=""):
        """The names of a row's entries: ``f"grad_{float(p)}_norm_{prefix}{key}"`` per tracked
        segment (key: the parameter's ``state_dict`` name, per capsule with
        ``split_capsules``), then ``f"grad_{float(p)}_norm_total"``.  Modelled on the
        ``grad_norm`` dict of Lightning 0.9's ``track_grad_norm``; the spelling is this
        library's and has not been checked against Lightning, and Lightning's rounding of the
        values to 3 decimals is not reproduced."""
        return self._need_norms().names(prefix)

    def last_grad_norms(self):
        """The newest row -- the tracked norms of the last optimiser step, in
        ``grad_norm_names()`` order -- as a device view (a later step overwrites it once the
        ring wraps), no read.  None before the first optimiser step."""
        return self._need_norms(built=False).last()

    def grad_norm_history(self, prefix=""):
        """-> ({name: host tensor (n,)}, optimiser steps): the last n = min(optimiser steps,
        capacity) rows in step order and those steps' numbers (0-based).  One read of the
        ring."""
        trk = self._need_norms(built=False)
        slots, steps = ops.ring_order(trk.count, trk.capacity)
        if not slots:
            return {}, []
        rows = trk.ring.cpu()[slots]
        return {k: rows[:, i] for i, k in enumerate(trk.names(prefix))}, steps

    @torch.no_grad()
    def parameter_norms(self, p=2):
        """The p-norms of the parameters over the tracked segments (``grad_norm_names()``
        order, then the total): one eager call of the gradient norms' kernel on the flat
        parameter buffer -> a fresh device row.  With ``last_grad_norms()`` (times the learning
        rate) it gives the update-to-weight ratio."""
        p = track_value(p)
        if p is None:
            raise ValueError("parameter_norms needs p = 1, 2 or inf")
        trk = self._need_norms()
        w = self.flat.flat_param
        if not w.is_cuda:
            return segment_norms_host(w, [(off, n) for _, off, n in trk.segments], p)
        row = torch.empty(1, len(trk.segments) + 1, device=w.device)
        trk.launch(w, None, 1.0, p=p, into=row)
        return row[0]

    # -- the training log (log_steps) ---------------------------------------------
    def _need_log(self):
        if self.train_log is None:
            raise ValueError("this step keeps no training log (TrainStep(log_steps=...))")
        return self.train_log

    def last_log(self):
        """-> {'loss', 'log'} of the newest logged step, as ``training_step()`` returns them
        for this model plus ``log['learning_rate']``: device views of the ring's row (a
        later step overwrites it once the ring wraps), no read.  None before the first
        step."""
        tlog = self._need_log()
        if tlog.count == 0:
            return None
        row = tlog.rows[(tlog.count - 1) % tlog.capacity]
        return dict(loss=row[0], log={k: row[ops.TRAIN_LOG_INDEX[k]] for k in self._log_keys})

    def log_history(self):
        """-> ({key: host tensor (n,)}, steps): the last n = min(steps logged, capacity)
        rows in step order and their step numbers (0-based since the last ``reset_log``).
        One read of the ring."""
        tlog = self._need_log()
        slots, steps = ops.ring_order(tlog.count, tlog.capacity)
        if not slots:
            return {}, []
        rows = tlog.rows.cpu()[slots]
        return {k: rows[:, ops.TRAIN_LOG_INDEX[k]] for k in self._log_keys}, steps

    def training_epoch_end(self, all_ranks=False):
        """-> the means of the steps logged since the last call ({key: fp32 mean, 'batches':
        n}, eval_step.means: the unweighted mean over steps), then clears the accumulator.
        ``all_ranks``: summed over the ranks first (data_parallel.all_reduce_sums, outside
        any graph); else this rank's."""
        from .data_parallel import all_reduce_sums
        from .eval_step import means
        tlog = self._need_log()
        sums = tlog.acc
        if all_ranks:
            sums = sums.clone()
            all_reduce_sums(sums)
        out = means(sums)
        tlog.acc.zero_()
        return out

    def reset_log(self):
        """Empty ring, step counter 0, accumulator cleared."""
        self._need_log().reset()

    def end_epoch(self):
        """Per-epoch ExponentialLR step (base_experiment.py:73-76); accumulating, a group
        still pending (``step(image, label)`` batches short of k) first steps the optimiser
        on what it has: one eager pass over acc alone (guarded like any step).  With
        ``nonfinite="raise"``: then ``check_nonfinite()``, after the learning rate's decay --
        the one read of the epoch."""
        acc = self._acc_state
        if self.accumulate_grad_batches > 1 and acc["pending"]:
            scale = 1.0 / (self.accumulate_grad_batches * self.world)
            if self.collective:
                self.flat.flat_grad.zero_()
                self.opt.fold()
                self._reduce()
                self.opt.step(grad_scale=scale, with_acc=False)
            else:
                self.opt.flush(scale)
            acc["pending"] = 0
            acc["optimizer_steps"] += 1
            if self.grad_norms is not None:
                self.grad_norms.count += 1
        if self.opt is not None and self.lr_decay_rate:
            self.opt.decay_lr(self.lr_decay_rate)
        if self.nonfinite == "raise":
            self.check_nonfinite()
