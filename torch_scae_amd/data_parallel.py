"""Data-parallel SCAE training over one node: one process per GPU, the model
replicated, the batch sharded, and ONE collective per step -- an all-reduce of
a single flat fp32 gradient buffer over RCCL/xGMI.

The reference has no distributed code at all (it would inherit Lightning's
DDP); this is the MI355X-native equivalent: gradients are views into one
contiguous buffer (one multi-tensor pack per step), parameters that get no
gradient in a given configuration (``obj_decoder.dummy_vote``,
``posterior_classifier.*`` by default) simply stay zero in it, and the
reduction is a single large message -- the right shape for xGMI's per-link
bound rings.
"""
import ctypes
import math
import numbers

import torch
import torch.distributed as dist


class GradSlot:
    """Where a parameter's gradient lives in the flat buffer.  The HIP ops'
    backward passes ask for it (``ops._grad_out``) and write the gradient
    there directly; autograd then adopts that view as ``p.grad`` and the
    per-step pack has nothing to copy for this parameter.  One taker per
    step: a second gradient of the same parameter gets a fresh buffer
    (``ops._grad_out`` first flushes any column sum still waiting to be
    written into the slot) and autograd accumulates it as usual."""

    def __init__(self, flat_grad, offset, shape):
        self.flat_grad, self.offset, self.shape = flat_grad, offset, shape
        self.numel = 1
        for d in shape:
            self.numel *= d
        self.taken = False

    def take(self):
        if self.taken:
            return None
        self.taken = True
        # a fresh tensor object every time: autograd only adopts a gradient
        # nobody else holds a reference to
        return self.flat_grad[self.offset:self.offset + self.numel] \
            .view(self.shape)


class FlatParameters:
    """Re-homes every parameter (and its gradient) of ``module`` into two flat
    fp32 buffers.  ``param.data`` / ``param.grad`` become views, so optimisers,
    autograd and checkpoints keep working unchanged."""

    def __init__(self, module, front=None):
        """``front``: optional predicate on parameter names; the parameters it
        selects are laid out first, as one contiguous block ``[0, n_front)``
        (the bucket whose gradients are final earliest in backward), the rest
        starts on a 16-byte boundary behind it."""
        named = [(n, p) for n, p in module.named_parameters()
                 if p.requires_grad]
        params = [p for _, p in named]
        if not params:
            raise ValueError("module has no trainable parameters")
        first_back = None
        if front is not None:
            head = [p for n, p in named if front(n)]
            back = [p for n, p in named if not front(n)]
            params = head + back
            first_back = back[0] if head and back else None
        # modules may ask for groups of parameters to lie back to back (in
        # the layout one of their kernels reads): move each group, in order,
        # to the position of its first member
        aligned = set()      # group heads start on a 16-byte boundary
        for m in module.modules():
            for group in getattr(m, "_flat_param_groups", lambda: [])():
                ids = {id(p) for p in group}
                if len(ids) != len(group) or \
                        not ids <= {id(p) for p in params}:
                    continue
                first = min(i for i, p in enumerate(params) if id(p) in ids)
                rest = [p for p in params if id(p) not in ids]
                params = rest[:first] + list(group) + rest[first:]
                aligned.add(id(group[0]))
        if first_back is not None:
            head_ids = {id(q) for q in head}
            flags = [id(p) in head_ids for p in params]
            n_head = sum(flags)
            if not all(flags[:n_head]):
                raise ValueError("a parameter group straddles the front block")
            first_back = params[n_head]
            aligned.add(id(first_back))
        dev, dt = params[0].device, params[0].dtype
        for p in params:
            if p.device != dev or p.dtype != dt:
                raise ValueError("all parameters must share device and dtype")
        self.params = params
        # offsets (in elements); the few padding elements in front of an
        # aligned group stay zero in both buffers
        self.offsets, off = [], 0
        for p in params:
            if id(p) in aligned:
                off = (off + 3) // 4 * 4
            self.offsets.append(off)
            off += p.numel()
        total = off
        self.flat_param = torch.zeros(total, device=dev, dtype=dt)
        self.flat_grad = torch.zeros(total, device=dev, dtype=dt)
        with torch.no_grad():
            for p, off in zip(params, self.offsets):
                n = p.numel()
                self.flat_param[off:off + n].copy_(p.reshape(-1))
                p.data = self.flat_param[off:off + n].view(p.shape)
                p.grad = None
                p._scae_grad_slot = GradSlot(self.flat_grad, off, tuple(p.shape))
        self.numel = total
        self._views = None
        # element offset where the second block starts (== numel without one)
        self.n_front = self.offsets[[id(p) for p in params].index(
            id(first_back))] if first_back is not None else total
        self.front_count = sum(1 for p, off in zip(params, self.offsets)
                               if off < self.n_front)

    def grad_views(self):
        if self._views is None:
            self._views = [self.flat_grad[off:off + p.numel()].view(p.shape)
                           for p, off in zip(self.params, self.offsets)]
        return self._views

    def clear_grads(self):
        """Drop every ``p.grad`` so that backward ASSIGNS fresh gradients
        instead of launching one accumulate-add kernel per parameter."""
        for p in self.params:
            p.grad = None
            p._scae_grad_slot.taken = False

    def block(self, which):
        """(first, last) parameter index of a block: 0 = the front block,
        1 = the rest, None = everything."""
        if which is None:
            return 0, len(self.params)
        return (0, self.front_count) if which == 0 else \
            (self.front_count, len(self.params))

    def block_grad(self, which):
        """The contiguous slice of the flat gradient buffer of a block."""
        if which is None:
            return self.flat_grad
        return self.flat_grad[:self.n_front] if which == 0 else \
            self.flat_grad[self.n_front:]

    @torch.no_grad()
    def gather_grads(self, which=None):
        """Pack the gradients backward produced into the flat buffer with one
        multi-tensor copy.  Parameters that received no gradient
        (``obj_decoder.dummy_vote``, ``posterior_classifier.*`` in the default
        SCAE config) keep zeros in their slice.  ``which``: only the
        parameters of that block (see ``block``)."""
        lo, hi = self.block(which)
        views, params = self.grad_views()[lo:hi], self.params[lo:hi]
        pairs = [(v, p.grad) for v, p in zip(views, params)
                 if p.grad is not None
                 # written in place by the op that produced it (GradSlot)
                 and p.grad.data_ptr() != v.data_ptr()]
        if pairs:
            torch._foreach_copy_([v for v, _ in pairs], [g for _, g in pairs])
        for v, p in zip(views, params):
            if p.grad is None and getattr(p, "_flat_was_set", False):
                v.zero_()
            p._flat_was_set = p.grad is not None

    def active_ranges(self, also=None):
        """[(offset, numel)] of the maximal runs of parameters that received a
        gradient in the last backward (torch optimisers skip ``grad is None``
        parameters altogether -- it matters with weight decay).  ``also``: a flag
        per parameter that counts it in too (a gradient in an earlier batch of an
        accumulated group)."""
        runs = []
        for i, (p, off) in enumerate(zip(self.params, self.offsets)):
            n = p.numel()
            if getattr(p, "_flat_was_set", True) or (also is not None and also[i]):
                if runs and runs[-1][0] + runs[-1][1] == off:
                    runs[-1][1] += n
                else:
                    runs.append([off, n])
        return [tuple(r) for r in runs]


def world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def all_reduce_sums(buf, group=None):
    """``buf`` <- its sum over the ranks, in place: one all-reduce of a small buffer (an
    evaluation step's fp64 accumulator, eval_step.EvalStep) outside any graph.  A no-op
    with one rank.  gloo reduces a host copy."""
    if world()[1] <= 1:
        return buf
    if buf.is_cuda and dist.get_backend(group) == "gloo":
        host = buf.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        buf.copy_(host)
    else:
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    return buf


def broadcast_parameters(flat: FlatParameters, src=0):
    """Make every rank start from rank ``src``'s weights."""
    if world()[1] > 1:
        dist.broadcast(flat.flat_param, src=src)


def all_reduce_gradients(flat: FlatParameters, async_op=False, average=True,
                         which=None, force=False):
    """grad <- mean over ranks (``average=False``: the sum, for an optimiser
    step that folds the 1/world scale in), one all-reduce of the flat buffer
    (``which``: of one of its two blocks).  ``force``: issue the collective
    even in a 1-rank group (tests of the collective path on one GPU)."""
    _, n = world()
    if n == 1 and not (force and dist.is_initialized()):
        return None
    g = flat.block_grad(which)
    if average and n > 1:
        g.div_(n)
    return dist.all_reduce(g, op=dist.ReduceOp.SUM, async_op=async_op)


def _stream(t):
    """The current stream of ``t``'s device: a launcher's last argument."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _riding_units(sum_units, ride):
    """The column-sum units (``ops._sum_rows_multi``) that ride in the coming launch: at most
    the last 16, the rest are launched now; None when none ride (``ride`` false: the launch
    hosts none, all are launched now)."""
    if not sum_units:
        return None
    from . import ops
    early = sum_units[:-16] if ride else sum_units
    if early:
        ops._launch_sum_units(early)
    return sum_units[len(early):] or None


class _FlatOptimizer:
    """What the flat optimisers share: the learning rate in device memory, so that
    ``decay_lr`` (the per-epoch ExponentialLR of base_experiment.py:73-76) takes effect inside
    an already captured HIP graph; ``step``, one driver for every pass and its CPU form
    (``_device_step`` / ``_cpu_step``; a class supplies ``_device_form`` and
    ``_cpu_update``); and gradient accumulation over k batches (Lightning's
    Trainer(accumulate_grad_batches=k)): ``acc``, a buffer laid out like ``flat_grad`` (None
    for k = 1), collects the gradients of a group's batches (``accumulate``: acc += g, in
    batch order, fp32); the group's last batch steps through the accumulate forms of the
    passes, which read g_eff = grad_scale (acc + g) and leave acc = 0.  The caller folds 1/k
    into ``grad_scale``.  Weight decay applies to the parameters that had a gradient in ANY
    batch of the group (torch skips only ``grad is None`` parameters)."""

    def _init_shared(self, look_ahead, look_ahead_k, look_ahead_alpha, gradient_clip_val,
                     accumulate_grad_batches, nonfinite):
        """The state beside the moments (``flat`` and ``lr`` are set)."""
        p = self.flat.flat_param
        self.lr_dev = torch.full((1,), self.lr, device=p.device, dtype=p.dtype)
        _init_look_ahead(self, look_ahead, look_ahead_k, look_ahead_alpha)
        _init_clip(self, gradient_clip_val)
        _init_guard(self, nonfinite)
        _init_track(self)
        _init_accumulate(self, accumulate_grad_batches)

    def set_lr(self, lr):
        self.lr = float(lr)
        self.lr_dev.fill_(self.lr)

    def decay_lr(self, gamma):
        """One ExponentialLR step (call once per epoch, gamma = decay_rate)."""
        self.set_lr(self.lr * gamma)

    @torch.no_grad()
    def step(self, grad_scale=1.0, sum_units=None, with_acc=True):
        """``grad_scale`` multiplies the gradient on the fly (1/world after a SUM
        all-reduce).  ``sum_units``: column-sum units (``ops._sum_rows_multi``) whose outputs
        are slots of the flat gradient buffer and which have NOT been launched yet: they ride
        in this step's launch (the ``_sums`` forms: the sum workgroups update the elements
        they produce), bit for bit the two launches' result.  Accumulating (``acc``, unless
        ``with_acc`` is False): the gradient is acc + g, and acc is 0 afterwards."""
        acc = self.acc if with_acc else None
        device = self.flat.flat_grad.is_cuda
        sum_units = _track_first(self, grad_scale, sum_units, acc, device)
        (_device_step if device else _cpu_step)(self, grad_scale, sum_units, acc)

    @torch.no_grad()
    def accumulate(self, sum_units=None):
        """acc <- acc + g (HIP: scae_grad_accumulate_f32; ``sum_units``, the step's column
        sums not launched yet, ride in the launch: scae_grad_accumulate_sums_f32)."""
        if self.acc is None:
            raise ValueError("this optimiser does not accumulate (accumulate_grad_batches=1)")
        g = self.flat.flat_grad
        self._acc_seen = _group_seen(self)
        sum_units = _riding_units(sum_units, g.is_cuda)
        if not g.is_cuda:
            self.acc.add_(g)
            return
        from . import _lib, ops
        P = ctypes.c_void_p
        if sum_units:
            _lib.call("scae_grad_accumulate_sums_f32", P(self.acc.data_ptr()), P(g.data_ptr()),
                      g.numel(), ops._sum_job_array(sum_units), len(sum_units), _stream(g))
        else:
            _lib.call("scae_grad_accumulate_f32", P(self.acc.data_ptr()), P(g.data_ptr()),
                      g.numel(), _stream(g))

    @torch.no_grad()
    def fold(self):
        """g <- g + acc, acc <- 0: the group's gradient in the flat gradient buffer, for an
        all-reduce of that buffer and the plain pass (``step(with_acc=False)``)."""
        g = self.flat.flat_grad
        if g.is_cuda:
            from . import _lib
            P = ctypes.c_void_p
            _lib.call("scae_grad_accumulate_f32", P(g.data_ptr()), P(self.acc.data_ptr()),
                      g.numel(), _stream(g))
        else:
            g.add_(self.acc)
        self.acc.zero_()

    @torch.no_grad()
    def flush(self, grad_scale):
        """One step on acc alone (a group that ended before its k-th batch): the flat
        gradient buffer zeroed, then the accumulate form."""
        self.flat.flat_grad.zero_()
        self.step(grad_scale=grad_scale)


def accumulate_value(v):
    """``accumulate_grad_batches`` as an int >= 1; a bool, another type (a per-epoch dict
    schedule included) or a value < 1 is an error."""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or int(v) < 1:
        raise ValueError(f"accumulate_grad_batches must be an int >= 1, got {v!r}")
    return int(v)


def _init_accumulate(opt, k):
    opt.accumulate_grad_batches = accumulate_value(k)
    opt.acc = torch.zeros_like(opt.flat.flat_grad) if opt.accumulate_grad_batches > 1 \
        else None
    opt._acc_seen = None     # per parameter: a gradient in an earlier batch of the group


def _group_seen(opt):
    """Per parameter: a gradient in the last backward or an earlier batch of the group."""
    now = [getattr(p, "_flat_was_set", True) for p in opt.flat.params]
    seen = getattr(opt, "_acc_seen", None)
    return now if seen is None else [a or b for a, b in zip(now, seen)]


def _take_ranges(opt):
    """The ranges an optimiser step updates (with weight decay: the parameters with a
    gradient, in the group when accumulating; else the whole buffer); ends the group."""
    g = opt.flat.flat_grad
    seen = getattr(opt, "_acc_seen", None)
    opt._acc_seen = None
    if opt.weight_decay == 0:
        return [(0, g.numel())]
    return opt.flat.active_ranges(also=seen)


class RMSpropFlat(_FlatOptimizer):
    """RMSprop with momentum on the flat buffers -- the reference's default
    optimiser (torch.optim.RMSprop(lr, momentum=0.9, eps=1e-2/bs**2,
    weight_decay), base_experiment.py:44-77) as ONE fused pass over the flat
    buffers on a HIP device (a handful of whole-buffer ops on CPU tensors, which
    only the host-logic tests use)."""

    kind = 2      # scae_flat_opt_step_f32's kind (with LookAhead)

    def __init__(self, flat: FlatParameters, lr=3e-5, alpha=0.99, eps=1e-8,
                 momentum=0.9, weight_decay=0.0, look_ahead=False,
                 look_ahead_k=5, look_ahead_alpha=0.5, gradient_clip_val=0.0,
                 accumulate_grad_batches=1, nonfinite=None):
        self.flat = flat
        self.lr, self.alpha, self.eps, self.momentum = lr, alpha, eps, momentum
        self.weight_decay = weight_decay
        self.square_avg = torch.zeros_like(flat.flat_param)
        self.buf = torch.zeros_like(flat.flat_param)
        self._init_shared(look_ahead, look_ahead_k, look_ahead_alpha, gradient_clip_val,
                          accumulate_grad_batches, nonfinite)

    def _device_form(self):
        if self.look_ahead_k:     # (the fused family: it counts the steps)
            return _flat_opt_form(self, self.buf, self.square_avg,
                                  (self.momentum, self.alpha))
        return ("scae_rmsprop", (self.square_avg, self.buf),
                (self.lr, ctypes.c_void_p(self.lr_dev.data_ptr()), self.alpha, self.eps,
                 self.momentum))

    def _cpu_update(self, g, t):
        """The CPU form of the update (torch.optim.RMSprop's arithmetic) on
        whole buffers; ``g`` already scaled."""
        if self.weight_decay != 0:
            g = g.add(self.flat.flat_param, alpha=self.weight_decay)
        self.square_avg.mul_(self.alpha).addcmul_(g, g, value=1 - self.alpha)
        avg = self.square_avg.sqrt().add_(self.eps)
        if self.momentum > 0:
            self.buf.mul_(self.momentum).addcdiv_(g, avg)
            self.flat.flat_param.add_(self.buf, alpha=-self.lr)
        else:
            self.flat.flat_param.addcdiv_(g, avg, value=-self.lr)

    @property
    def counts_steps(self):
        """The device step count is kept (only LookAhead needs one here)."""
        return bool(self.look_ahead_k)

    def state_buffers(self):
        """(torch.optim.RMSprop's state key, flat buffer) pairs."""
        return [("square_avg", self.square_avg), ("momentum_buffer", self.buf)]

    def hyper_parameters(self):
        return dict(lr=self.lr, momentum=self.momentum, alpha=self.alpha,
                    eps=self.eps, weight_decay=self.weight_decay,
                    centered=False)


def _init_look_ahead(opt, look_ahead, k, alpha):
    """The state every flat optimiser shares beside its moments: the step count
    in device memory and LookAhead's slow buffer (torch_scae/optimizers.py:105-190)."""
    flat = opt.flat
    if look_ahead and (int(k) < 1 or not 0.0 <= float(alpha) <= 1.0):
        raise ValueError(f"LookAhead needs k >= 1 and 0 <= alpha <= 1, got "
                         f"k={k}, alpha={alpha}")
    opt.look_ahead_k = int(k) if look_ahead else 0
    opt.look_ahead_alpha = float(alpha)
    # [0] steps taken, [1] the slow buffer has been made (LookAhead's first
    # sync), the rest the kernel's arrival counters (0 between launches).  Read
    # by the kernel at every step, so a captured graph follows it; the host
    # reads it back only for state_dict()
    from ._lib import FLAT_OPT_STATE_INTS
    opt.step_state = torch.zeros(FLAT_OPT_STATE_INTS, dtype=torch.int32,
                                 device=flat.flat_param.device)
    opt.slow = torch.zeros_like(flat.flat_param) if opt.look_ahead_k else None


def clip_value(v):
    """``gradient_clip_val`` as Lightning 0.9 reads it: any value <= 0 is off (-> 0.0); a
    non-numeric or non-finite value is an error."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(float(v)):
        raise ValueError(f"gradient_clip_val must be a finite number, got {v!r}")
    return float(v) if v > 0 else 0.0


def _init_clip(opt, gradient_clip_val):
    """Clipping by global norm (torch.nn.utils.clip_grad_norm_, which Lightning's
    Trainer(gradient_clip_val) applies before every optimiser step): ``max_norm`` (0.0: off),
    the norm launch's fp64 partial sums and the last norm before clipping, both in device
    memory (read by a captured step's launches, never by the host)."""
    opt.max_norm = clip_value(gradient_clip_val)
    dev = opt.flat.flat_param.device
    opt.grad_sq = opt.grad_norm = None
    if opt.max_norm:
        from ._lib import GRAD_SQ_MAX_PARTIALS
        opt.grad_sq = torch.zeros(GRAD_SQ_MAX_PARTIALS, dtype=torch.float64, device=dev)
        opt.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)


def nonfinite_value(v):
    """``nonfinite`` -> None (off), "skip" or "raise"; anything else is an error."""
    if v is None:
        return None
    if isinstance(v, str) and v.lower() in ("skip", "raise"):
        return v.lower()
    raise ValueError(f"nonfinite must be None, 'skip' or 'raise', got {v!r}")


def _init_guard(opt, nonfinite):
    """The non-finite guard (``nonfinite="skip"``; off by default): an optimiser step whose
    gradient -- the one the step consumes: acc + g when accumulating, after the all-reduce --
    holds a NaN or +-Inf element writes nothing.  Parameters, moments, LookAhead's slow
    weights and ``step_state`` keep their bits, acc is zeroed (the group is dropped), and the
    skip is counted in ``guard_state``, int64 {skipped, first, last, attempts}: attempts
    counts guarded optimiser steps, first / last are the attempts values (0-based) of the
    first and last skipped one, -1 before any.  The rule: the fp64 sum of squares is finite
    exactly when every element is (the fp32 norm may overflow for finite gradients and does
    not decide).  A finite step has the unguarded step's bits; ``grad_norm`` is written either
    way, and a tracking optimiser's ``GradNorms`` row is still written for a skipped step.
    On a HIP device the step takes the guarded forms of the passes (``_device_step``:
    scae_*_guard_step_f32), which decide on the norm launch's partials: ``grad_sq`` is
    allocated as clipping allocates it, and ``guard_state`` and ``grad_norm`` live in device
    memory -- a replayed step reads nothing back.  Any other device type raises (nothing falls
    back to an unguarded step)."""
    if nonfinite not in (None, "skip"):
        raise ValueError(f"an optimiser's nonfinite must be None or 'skip', got {nonfinite!r}")
    opt.nonfinite = nonfinite
    opt.guard_state = None
    if nonfinite:
        dev = opt.flat.flat_param.device
        if dev.type not in ("cpu", "cuda"):
            from ._lib import ScaeHipError
            raise ScaeHipError(f"nonfinite='skip' has a CPU form and a HIP device form, none for "
                               f"a {dev.type!r} device, and the step does not run unguarded")
        if opt.grad_norm is None:
            opt.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        if opt.grad_sq is None:       # (as _init_clip: the CPU forms do not read it)
            from ._lib import GRAD_SQ_MAX_PARTIALS
            opt.grad_sq = torch.zeros(GRAD_SQ_MAX_PARTIALS, dtype=torch.float64, device=dev)
        opt.guard_state = torch.tensor([0, -1, -1, 0], dtype=torch.int64, device=dev)


def _cpu_guard_skips(opt, g, grad_scale):
    """(CPU forms) The guard's decision on ``g`` (acc already folded in and zeroed), counted
    in ``guard_state``; on a skip, or without clipping, the norm into ``grad_norm``."""
    sq = g.double().square().sum()
    skip = not bool(torch.isfinite(sq))
    gs = opt.guard_state
    t = int(gs[3])
    if skip:
        gs[0] += 1
        if int(gs[1]) < 0:
            gs[1] = t
        gs[2] = t
    gs[3] = t + 1
    if skip or not opt.max_norm:
        opt.grad_norm.copy_((float(grad_scale) * sq.sqrt()).float())
    return skip


def _cpu_effective_grad(opt, g, grad_scale, seen=None):
    """(CPU forms) The gradient the update consumes -- scaled, clipped when clipping -- or
    None when the guard skips the step."""
    if opt.nonfinite and _cpu_guard_skips(opt, g, grad_scale):
        return None
    if opt.max_norm:
        return _cpu_clipped_grad(opt, g, grad_scale, seen)
    return g * grad_scale if grad_scale != 1.0 else g


def track_value(v):
    """``track_grad_norm`` as Lightning's Trainer reads it: 1, 2, ``float('inf')`` or ``'inf'``
    -> the norm's p as a float; None, -1 or 0 -> None (off, Lightning's default -1); a bool,
    another string or any other number is an error."""
    if v is None:
        return None
    if isinstance(v, str):
        if v == "inf":
            return math.inf
    elif not isinstance(v, bool) and isinstance(v, numbers.Real):
        v = float(v)
        if v in (-1.0, 0.0):
            return None
        if v in (1.0, 2.0, math.inf):
            return v
    raise ValueError(f"track_grad_norm must be 1, 2 or 'inf' (None, -1 or 0: off), got {v!r}")


def norm_segments(flat, model, split_capsules=True, seen=None):
    """[(key, offset, length)]: the segments of ``flat``'s buffers whose norms are tracked, in
    flat order -- the parameters that received a gradient (``seen``: a flag per parameter of
    ``flat.params``; default: in the last backward), keyed by their ``model.state_dict()``
    names.  ``split_capsules``: a ``nn_ext.GroupedMLP`` stacked parameter gives one segment per
    capsule slice under the reference's per-capsule key (the mapping of
    ``GroupedMLP._save_to_state_dict``); else one segment under the stacked parameter's own
    name."""
    from .nn_ext import GroupedMLP
    names, slices = {}, {}
    for name, p in model.named_parameters():
        names.setdefault(id(p), name)
    if split_capsules:
        for mod_name, mod in model.named_modules():
            if not isinstance(mod, GroupedMLP):
                continue
            prefix = mod_name + "." if mod_name else ""
            for j in range(mod.n_layers):
                for kind, stacked in (("weight", mod.weights[j]),
                                      ("bias", mod.biases[j] if mod.has_bias else None)):
                    if stacked is not None:
                        slices[id(stacked)] = [f"{prefix}{g}.{2 * j}.{kind}"
                                               for g in range(mod.n_groups)]
    if seen is None:
        seen = [getattr(p, "_flat_was_set", True) for p in flat.params]
    out = []
    for p, off, s in zip(flat.params, flat.offsets, seen):
        n = p.numel()
        if not s or n == 0:
            continue
        keys = slices.get(id(p))
        if keys is None:
            out.append((names[id(p)], off, n))
            continue
        per = n // len(keys)
        out.extend((key, off + g * per, per) for g, key in enumerate(keys))
    return out


def norm_chunk_table(segments, n, chunk=None, group_chunks=None):
    """The work division of scae_segment_norms_f32 for ``segments`` [(offset, length)] of a
    buffer of ``n`` elements -> (chunks, group_first, seg_first): chunks [(first element,
    length)] of at most ``chunk`` elements of one segment each, ascending; ``group_first``: the
    first chunk of every workgroup's run of chunks (at most ``group_chunks`` chunks and four
    chunks' worth of elements: small segments share a workgroup), then the chunk count;
    ``seg_first``: every segment's first chunk, then the chunk count.  Segments must be
    ascending, disjoint, non-empty and inside [0, n)."""
    from ._lib import NORM_CHUNK, NORM_GROUP_CHUNKS
    chunk = NORM_CHUNK if chunk is None else int(chunk)
    group_chunks = NORM_GROUP_CHUNKS if group_chunks is None else int(group_chunks)
    chunks, seg_first, end = [], [], 0
    for off, length in segments:
        off, length = int(off), int(length)
        if length < 1 or off < end or off + length > n:
            raise ValueError(f"segment ({off}, {length}) is empty, overlaps the one before it or "
                             f"leaves the buffer of {n} elements")
        end = off + length
        seg_first.append(len(chunks))
        chunks.extend((b, min(chunk, end - b)) for b in range(off, end, chunk))
    if not chunks:
        raise ValueError("no segments")
    seg_first.append(len(chunks))
    group_first, load, count = [0], 0, 0
    for i, (_, length) in enumerate(chunks):
        if count and (count >= group_chunks or load + length > 4 * chunk):
            group_first.append(i)
            load = count = 0
        load, count = load + length, count + 1
    group_first.append(len(chunks))
    return chunks, group_first, seg_first


def segment_norms_host(x, segments, p, scale=1.0):
    """The row scae_segment_norms_f32 writes, in torch on the host: fp32 (len(segments) + 1) of
    fp32(scale) * ||x[offset:offset + length]||_p per segment [(offset, length)], taken in fp64,
    then the p-norm of those (fp64, before rounding).  The CPU form of a tracking step and
    the tests' yardstick."""
    x = x.detach().double()
    vals = [torch.linalg.vector_norm(x[off:off + n], p) for off, n in segments]
    vals.append(torch.linalg.vector_norm(torch.stack(vals), p) if vals else x.new_zeros(()))
    scale = float(torch.tensor(float(scale), dtype=torch.float32))
    return (torch.stack(vals) * scale).float()


class GradNorms:
    """Per-parameter norms of the gradient an optimiser step consumes (Lightning's
    ``Trainer(track_grad_norm=p)``): one row per optimiser step -- a norm per segment
    (``norm_segments``), then the total -- in a device ring of ``capacity`` rows whose cursor
    the launch itself advances (scae_segment_norms_f32; on CPU tensors ``segment_norms_host``).
    The segment table is fixed by the first ``build``: after a backward, outside any capture.
    ``count``: the host's mirror of the cursor (the step that owns the optimiser counts).
    A step the non-finite guard skips (``_init_guard``) still writes its row, ahead of the pass:
    the row shows which segment blew up, and its total is non-finite."""

    def __init__(self, flat, model, p, capacity=1, split_capsules=True):
        self.flat, self.model, self.p = flat, model, float(p)
        self.capacity = max(1, int(capacity))
        self.split_capsules = bool(split_capsules)
        self.segments = None
        self.ring = self.cursor = self.partials = self.tables = None
        self.count = 0

    def build(self, seen=None):
        if self.segments is not None:
            return
        flat = self.flat
        segs = norm_segments(flat, self.model, self.split_capsules, seen)
        if not segs:
            raise ValueError("no parameter received a gradient: nothing to track")
        dev = flat.flat_grad.device
        self.ring = torch.zeros(self.capacity, len(segs) + 1, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        if dev.type == "cuda":
            chunks, group_first, seg_first = norm_chunk_table(
                [(off, n) for _, off, n in segs], flat.numel)
            self.tables = tuple(torch.tensor(t, dtype=torch.int32).to(dev)
                                for t in (chunks, group_first, seg_first))
            self.partials = torch.zeros(len(chunks), dtype=torch.float64, device=dev)
        self.segments = segs

    def names(self, prefix=""):
        return [f"grad_{self.p}_norm_{prefix}{key}" for key, _, _ in self.segments] + \
            [f"grad_{self.p}_norm_total"]

    @torch.no_grad()
    def launch(self, x, acc, scale, p=None, into=None):
        """One row of the norms of ``x`` (or ``acc + x``), scaled.  ``into``: a (1, n + 1) row
        of the caller's instead of the ring's next one (the cursor stays)."""
        p = self.p if p is None else p
        ring, cursor = (self.ring, self.cursor) if into is None else (into, None)
        if not x.is_cuda:
            if acc is not None:
                x = acc + x
            row = segment_norms_host(x, [(off, n) for _, off, n in self.segments], p, scale)
            if cursor is None:
                ring[0].copy_(row)
            else:
                ring[int(cursor) % self.capacity].copy_(row)
                cursor += 1
            return
        from . import _lib
        P = ctypes.c_void_p
        chunks, group_first, seg_first = self.tables
        partials = self.partials if into is None else torch.empty_like(self.partials)
        _lib.call("scae_segment_norms_f32", P(x.data_ptr()),
                  None if acc is None else P(acc.data_ptr()), x.numel(),
                  P(chunks.data_ptr()), chunks.shape[0], P(group_first.data_ptr()),
                  group_first.numel() - 1, P(seg_first.data_ptr()), len(self.segments),
                  _lib.NORM_INF if math.isinf(p) else int(p), float(scale),
                  P(partials.data_ptr()), P(ring.data_ptr()),
                  None if cursor is None else P(cursor.data_ptr()),
                  self.capacity if into is None else 1, _stream(x))

    def last(self):
        """The newest row (a device view, no read); None before the first one."""
        return None if self.count == 0 else self.ring[(self.count - 1) % self.capacity]


def _init_track(opt):
    """``opt.track``: the ``GradNorms`` of a step that tracks (train_step.TrainStep attaches
    it), else None."""
    opt.track = None


def _track_first(opt, grad_scale, sum_units, acc, device):
    """A tracking optimiser's step, before its pass: the norms of the gradient the pass
    consumes.  The flat gradient is complete only once the step's last column sums
    (``sum_units``) have run, so they are launched on their own here -- the same bits as riding
    in the pass -- and the norms after them; -> the units still to launch.  A clipping or
    guarded step on the device (``device``: the step takes ``_device_step``) keeps them: they
    ride in its norm launch, and the norms follow that (``_track_after_norm``)."""
    trk = opt.track
    if trk is None or (device and (opt.max_norm or opt.nonfinite)):
        return sum_units
    _riding_units(sum_units, False)
    trk.build(_group_seen(opt))
    trk.launch(opt.flat.flat_grad, acc, grad_scale)
    return None


def _track_after_norm(opt, grad_scale, acc):
    """... of a clipping or guarded step on the device: after the norm launch, which hosts the
    column sums, and before the pass (whose accumulate form clears acc; a step the guard
    skips has its row written here)."""
    trk = opt.track
    if trk is not None:
        trk.build(_group_seen(opt))
        trk.launch(opt.flat.flat_grad, acc, grad_scale)


def _launch_norm(opt, g, sum_units, st, acc=None):
    """The gradient's fp64 partial sums of squares into ``opt.grad_sq`` (column-sum units ride
    in the launch: ``_riding_units``); -> the partial count.  ``acc``: of acc + g (the
    accumulate forms, which take acc right after grad)."""
    from . import _lib, ops
    P = ctypes.c_void_p
    cnt = ctypes.c_int(0)
    sum_units = _riding_units(sum_units, True)
    args = [P(g.data_ptr())] + ([] if acc is None else [P(acc.data_ptr())]) + \
        [g.numel(), P(opt.grad_sq.data_ptr()), opt.grad_sq.numel(), ctypes.byref(cnt)]
    if sum_units:
        args += [ops._sum_job_array(sum_units), len(sum_units)]
    _lib.call("scae_grad_sq%s_partials%s_f32" % ("" if acc is None else "_acc",
                                                 "_sums" if sum_units else ""), *args, st)
    return cnt.value


def _cpu_clipped_grad(opt, g, grad_scale, seen=None):
    """The CPU form: torch.nn.utils.clip_grad_norm_'s arithmetic on the (scaled) gradients of
    the parameters that have one (a norm per parameter, then the norm of those), applied to
    the whole flat gradient; the norm into ``opt.grad_norm``.  ``seen``: which parameters
    have one (default: a gradient in the last backward)."""
    if grad_scale != 1.0:
        g = g * grad_scale
    flat = opt.flat
    if seen is None:
        seen = [getattr(p, "_flat_was_set", True) for p in flat.params]
    norms = [torch.linalg.vector_norm(g[off:off + p.numel()])
             for p, off, s in zip(flat.params, flat.offsets, seen) if s]
    total = torch.linalg.vector_norm(torch.stack(norms)) if norms else g.new_zeros(())
    opt.grad_norm.copy_(total)
    coef = torch.clamp(opt.max_norm / (total + 1e-6), max=1.0)
    return g * coef


def _keep_inactive(opt, ranges, bufs):
    """(CPU forms) what ``_restore_inactive`` needs to put back the elements outside
    ``ranges`` -- parameters without a gradient, which torch.optim skips; None when the
    ranges cover the whole buffer."""
    g = opt.flat.flat_grad
    if ranges == [(0, g.numel())]:
        return None
    keep = torch.zeros_like(g, dtype=torch.bool)
    for off, n in ranges:
        keep[off:off + n] = True
    return keep, [(b, b.clone()) for b in bufs]


def _restore_inactive(saved):
    if saved is None:
        return
    keep, pairs = saved
    for cur, old in pairs:
        cur.copy_(torch.where(keep, cur, old))


def _flat_opt_form(opt, m, v, betas):
    """``_device_form`` of the scae_flat_opt family (Adam, RAdam, RMSprop with LookAhead): its
    buffers after grad -- both moments and LookAhead's slow weights (without LookAhead the
    parameters stand in) -- and its fixed argument run."""
    P = ctypes.c_void_p
    slow = opt.slow if opt.slow is not None else opt.flat.flat_param
    return ("scae_flat_opt", (m, v, slow),
            (P(opt.lr_dev.data_ptr()), P(opt.step_state.data_ptr()), opt.kind,
             float(betas[0]), float(betas[1]), float(opt.eps)))


def _device_step(opt, grad_scale, sum_units, acc):
    """One optimiser step on a HIP device, through
    scae_{family}[_acc][_sums|_clip|_guard]_step_f32 (``opt._device_form()`` -> family, buffers,
    fixed arguments).  Clipping: the norm launch (the column sums ride in it), the tracked
    norms, then the ``_clip`` form over each active range.  Guarded (``_init_guard``): the same
    path whether it clips or not, through the ``_guard`` form -- max_norm +inf when it does
    not clip; the first range's launch writes the norm and counts in ``guard_state``, every
    range's launch takes the same decision.  Else the column sums ride in the pass when there
    is no weight decay (the ``_sums`` form, over the whole buffer: the sum workgroups update
    the elements they produce), and
    otherwise the plain form runs over each active range: parameters without a gradient are
    left alone, like torch.optim does; without weight decay a zero gradient already is a
    no-op (zero moments stay zero, LookAhead's slow copy of such a parameter equals it).
    ``acc``: the accumulate forms (the gradient is acc + g, acc -> 0).  Reads the tensors'
    addresses and sizes only."""
    from . import _lib, ops
    P = ctypes.c_void_p
    flat = opt.flat
    g = flat.flat_grad
    st = _stream(g)
    family, bufs, fixed = opt._device_form()
    counts = family == "scae_flat_opt"     # (this family counts steps and syncs LookAhead)
    guard = bool(opt.nonfinite)
    clip = bool(opt.max_norm) or guard      # (the forms that follow a norm launch)
    if clip:
        n_partials = _launch_norm(opt, g, sum_units, st, acc)
        _track_after_norm(opt, grad_scale, acc)
        sum_units = None
    else:
        sum_units = _riding_units(sum_units, opt.weight_decay == 0)
    ranges = _take_ranges(opt)
    if sum_units:
        ranges = [(0, g.numel())]
    name = "%s%s%s_step_f32" % (family, "" if acc is None else "_acc",
                                "_guard" if guard else "_clip" if clip else
                                "_sums" if sum_units else "")
    for i, (off, n) in enumerate(ranges):
        ptr = lambda t: P(t.data_ptr() + 4 * off)   # noqa: E731
        # the accumulate forms take acc right after grad
        args = [ptr(flat.flat_param), ptr(g)] + ([] if acc is None else [ptr(acc)]) + \
            [ptr(b) for b in bufs] + [n, *fixed]
        if not sum_units:
            args.append(float(opt.weight_decay))
        args.append(float(grad_scale))
        if counts:
            args += [opt.look_ahead_k, opt.look_ahead_alpha]
            if not sum_units:
                # (one launch per step advances the count: the last, so that every range
                # reads the same t)
                args.append(int(i == len(ranges) - 1))
        if clip:
            args += [P(opt.grad_sq.data_ptr()), n_partials, opt.max_norm or math.inf,
                     P(opt.grad_norm.data_ptr()) if i == 0 else None]
            if guard:
                args.append(P(opt.guard_state.data_ptr()) if i == 0 else None)
        elif sum_units:
            args += [ops._sum_job_array(sum_units), len(sum_units)]
        _lib.call(name, *args, st)


def _cpu_step(opt, grad_scale, sum_units, acc):
    """One optimiser step on CPU tensors (the host-logic tests), in whole-buffer torch ops:
    the guard (``_init_guard``) decides first, then the clip, ``opt._cpu_update(g, t)`` and,
    where the optimiser counts steps, LookAhead's sync; parameters without a gradient are
    put back afterwards.  When no parameter takes the step (weight decay, no gradient at
    all) nothing is counted or written beyond acc -> 0, as on the device, which launches no
    pass then."""
    _riding_units(sum_units, False)
    flat = opt.flat
    g = flat.flat_grad
    seen = _group_seen(opt)
    ranges = _take_ranges(opt)
    if acc is not None:
        g = acc + g
        acc.zero_()
    if not ranges:
        return
    g = _cpu_effective_grad(opt, g, grad_scale, seen)
    if g is None:      # (the guard: nothing is written, the step count stays)
        return
    saved = _keep_inactive(opt, ranges, [flat.flat_param] + [b for _, b in opt.state_buffers()]
                           + ([opt.slow] if opt.slow is not None else []))
    t = int(opt.step_state[0]) + 1 if opt.counts_steps else None
    opt._cpu_update(g, t)
    k = opt.look_ahead_k
    if k and t % k == 0:        # optimizers.py:118-128, 136-142
        p = flat.flat_param
        if int(opt.step_state[1]):
            opt.slow.add_(p - opt.slow, alpha=opt.look_ahead_alpha)
            p.copy_(opt.slow)
        else:
            opt.slow.copy_(p)
        opt.step_state[1] = 1
    if t is not None:
        opt.step_state[0] = t
    _restore_inactive(saved)


class _FlatAdamBase(_FlatOptimizer):
    """What AdamFlat and RAdamFlat share: two moment buffers, the step count in device
    memory and optionally LookAhead(k, alpha) fused into the same pass."""

    kind = None
    counts_steps = True

    def __init__(self, flat: FlatParameters, lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, weight_decay=0.0, look_ahead=False, look_ahead_k=5,
                 look_ahead_alpha=0.5, gradient_clip_val=0.0, accumulate_grad_batches=1,
                 nonfinite=None):
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {betas}")
        self.flat = flat
        self.lr, self.betas, self.eps = float(lr), (b1, b2), float(eps)
        self.weight_decay = float(weight_decay)
        self.exp_avg = torch.zeros_like(flat.flat_param)
        self.exp_avg_sq = torch.zeros_like(flat.flat_param)
        self._init_shared(look_ahead, look_ahead_k, look_ahead_alpha, gradient_clip_val,
                          accumulate_grad_batches, nonfinite)

    def _device_form(self):
        return _flat_opt_form(self, self.exp_avg, self.exp_avg_sq, self.betas)

    def state_buffers(self):
        """(torch.optim's state key, flat buffer) pairs."""
        return [("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)]

    def hyper_parameters(self):
        return dict(lr=self.lr, betas=self.betas, eps=self.eps,
                    weight_decay=self.weight_decay)


class AdamFlat(_FlatAdamBase):
    """torch.optim.Adam(lr, betas, eps, weight_decay) -- the reference's
    ``optimizer.type: Adam`` (base_experiment.py:56-60) -- as ONE fused pass
    over the flat buffers (scae_flat_opt_step_f32, kind 0): coupled L2 weight
    decay, eps added after the bias correction of sqrt(v)."""

    kind = 0

    def _cpu_update(self, g, t):
        b1, b2 = self.betas
        if self.weight_decay != 0:
            g = g.add(self.flat.flat_param, alpha=self.weight_decay)
        self.exp_avg.lerp_(g, 1 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (self.exp_avg_sq.sqrt() / math.sqrt(1 - b2 ** t)).add_(self.eps)
        self.flat.flat_param.addcdiv_(self.exp_avg, denom,
                                      value=-self.lr / (1 - b1 ** t))


class RAdamFlat(_FlatAdamBase):
    """The reference's RAdam (torch_scae/optimizers.py:36-102,
    ``degenerated_to_sgd=True``; ``optimizer.type: RAdam``) as ONE fused pass
    over the flat buffers (scae_flat_opt_step_f32, kind 1): decoupled weight
    decay (p -= wd lr p), eps added to the raw sqrt(v), and the variance
    rectification from the step N_sma = N_max - 2t b2^t / (1 - b2^t) reaches 5
    on (t = 6 at b2 = 0.999); before that, SGD with momentum.
    torch.optim.RAdam(decoupled_weight_decay=True) has the same arithmetic."""

    kind = 1

    def _cpu_update(self, g, t):
        b1, b2 = self.betas
        m, v, p = self.exp_avg, self.exp_avg_sq, self.flat.flat_param
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        m.mul_(b1).add_(g, alpha=1 - b1)
        b2t = b2 ** t
        n_max = 2 / (1 - b2) - 1
        n_sma = n_max - 2 * t * b2t / (1 - b2t)
        if self.weight_decay != 0:
            p.add_(p, alpha=-self.weight_decay * self.lr)
        if n_sma >= 5:
            size = math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2)
                             / n_sma * n_max / (n_max - 2)) / (1 - b1 ** t)
            p.addcdiv_(m, v.sqrt().add_(self.eps), value=-size * self.lr)
        else:
            p.add_(m, alpha=-self.lr / (1 - b1 ** t))


def make_optimizer(kind, flat, lr, eps, betas=(0.9, 0.999), momentum=0.9,
                   weight_decay=0.0, look_ahead=False, look_ahead_k=5,
                   look_ahead_alpha=0.5, gradient_clip_val=0.0, accumulate_grad_batches=1,
                   nonfinite=None):
    """``kind``: "rmsprop" | "adam" | "radam" (any case) -> the flat optimiser.
    ``gradient_clip_val`` > 0: every step clips the gradient to that global norm first.
    ``accumulate_grad_batches`` > 1: the optimiser keeps an accumulator (``accumulate``).
    ``nonfinite="skip"``: a step whose gradient holds a NaN or Inf writes nothing and is
    counted (``_init_guard``; on a HIP device through the guarded forms of the passes); None
    (the default): the step as it was."""
    name = str(kind).lower()
    la = dict(look_ahead=look_ahead, look_ahead_k=look_ahead_k,
              look_ahead_alpha=look_ahead_alpha, gradient_clip_val=gradient_clip_val,
              accumulate_grad_batches=accumulate_grad_batches, nonfinite=nonfinite)
    if name == "rmsprop":
        return RMSpropFlat(flat, lr=lr, momentum=momentum, eps=eps,
                           weight_decay=weight_decay, **la)
    if name in ("adam", "radam"):
        cls = AdamFlat if name == "adam" else RAdamFlat
        return cls(flat, lr=lr, betas=betas, eps=eps,
                   weight_decay=weight_decay, **la)
    raise ValueError(f"unknown optimizer {kind!r}: expected 'rmsprop', 'adam' "
                     "or 'radam'")


def optimizer_state_dict(opt, params, steps=None):
    """``opt``'s state in ``torch.optim``'s schema: ``state`` keyed by the
    parameter's index in ``params`` (``model.parameters()``), with ``step`` and
    the optimiser's own buffers (``exp_avg`` / ``exp_avg_sq``; ``square_avg`` /
    ``momentum_buffer``), one ``param_groups`` entry.  Loads into the matching
    stock optimiser built on ``params``.  ``steps``: the step count when ``opt``
    keeps none (RMSprop without LookAhead).  With LookAhead, ``slow_state``
    {index: {'slow_buffer': tensor}} once the slow weights exist, and the
    group carries ``lookahead_k`` / ``lookahead_alpha`` / ``lookahead_step``
    (the reference's LookAhead.state_dict keys its slow state by Python id()
    instead, optimizers.py:169-182, which no other process can map back)."""
    flat = opt.flat
    where = {id(p): off for p, off in zip(flat.params, flat.offsets)}
    t = int(opt.step_state[0]) if opt.counts_steps or steps is None \
        else int(steps)
    made = opt.slow is not None and bool(int(opt.step_state[1]))
    bufs = [(k, b) for k, b in opt.state_buffers()
            if not (k == "momentum_buffer" and opt.momentum <= 0)]
    state, slow_state = {}, {}
    for i, p in enumerate(params):
        off = where.get(id(p))
        if off is None:
            continue
        sl = slice(off, off + p.numel())
        state[i] = dict(step=torch.tensor(float(t)),
                        **{k: b[sl].view(p.shape).detach().cpu().clone()
                           for k, b in bufs})
        if made:
            slow_state[i] = dict(
                slow_buffer=opt.slow[sl].view(p.shape).detach().cpu().clone())
    group = dict(opt.hyper_parameters(), params=list(range(len(params))))
    out = dict(state=state, param_groups=[group])
    if opt.look_ahead_k:
        group.update(lookahead_k=opt.look_ahead_k,
                     lookahead_alpha=opt.look_ahead_alpha, lookahead_step=t)
        out["slow_state"] = slow_state
    return out


@torch.no_grad()
def load_optimizer_state_dict(opt, params, sd):
    """The inverse of ``optimizer_state_dict``: ``sd`` in ``torch.optim``'s
    schema (e.g. a stock optimiser's ``state_dict()`` over ``params``).  The
    learning rate is taken over; the other hyper-parameters must equal
    ``opt``'s (a captured step holds them).  A parameter without state starts
    from zero moments; LookAhead's slow weights come from ``slow_state`` (when
    it is missing or empty the next sync creates them, as the reference
    does).  Returns the step count."""
    groups = sd["param_groups"]
    if len(groups) != 1:
        raise ValueError("one parameter group expected, got %d" % len(groups))
    group = groups[0]
    mine = opt.hyper_parameters()
    for key, val in mine.items():
        if key == "lr" or key not in group:
            continue
        a = val if isinstance(val, tuple) else (val,)
        b = tuple(group[key]) if isinstance(group[key], (tuple, list)) \
            else (group[key],)
        if len(a) != len(b) or not all(
                math.isclose(float(x), float(y), rel_tol=1e-6, abs_tol=0.0)
                for x, y in zip(a, b)):
            raise ValueError(f"{key}={group[key]!r} in the state dict, the "
                             f"optimiser has {val!r}")
    flat = opt.flat
    where = {id(p): off for p, off in zip(flat.params, flat.offsets)}
    bufs = [(k, b) for k, b in opt.state_buffers()
            if not (k == "momentum_buffer" and opt.momentum <= 0)]
    state = sd["state"]
    slow_state = sd.get("slow_state") or {}
    steps = set()
    for i, p in enumerate(params):
        off = where.get(id(p))
        if off is None:
            continue
        sl = slice(off, off + p.numel())
        st = state.get(i, state.get(str(i)))
        for k, b in bufs:
            if st is None:
                b[sl].zero_()
            else:
                b[sl].copy_(st[k].reshape(-1))
        if st is not None:
            steps.add(int(float(st["step"])))
        if opt.slow is not None:
            ss = slow_state.get(i, slow_state.get(str(i)))
            # (a parameter without slow weights: the reference would create
            # them from the fast ones at its first sync with a gradient)
            opt.slow[sl].copy_(ss["slow_buffer"].reshape(-1) if ss is not None
                               else p.detach().reshape(-1))
    if len(steps) > 1:
        raise ValueError(f"one step count for all parameters, got {sorted(steps)}")
    t = steps.pop() if steps else 0
    opt.set_lr(group["lr"])
    opt.step_state[:2].copy_(torch.tensor([t, int(bool(slow_state))],
                                          dtype=torch.int32))
    return t
