"""One SCAE evaluation batch = forward + SCAE.loss + SCAE.calculate_accuracy under
``model.eval()`` and ``no_grad``, optionally captured once into a HIP graph and replayed,
with the epoch's means kept in a device-resident fp64 accumulator: a whole epoch is N
replays and one read at its end.

Mirrors the semantics of the reference's BaseExperiment.validation_step /
validation_epoch_end / test_step / test_epoch_end
(torch_scae_experiments/base_experiment.py:128-202)."""
import contextlib

import torch

from . import ops
from . import replay as _replay   # (``replay`` is the steps' constructor argument)
from .data_parallel import all_reduce_sums, world

# the accumulator (include/scae_hip.h, SCAE_EVAL_ACC_DOUBLES): [0] batches, then the sums
# of these keys ([5] is the 12-vector's loss entry, the same value as [1]: not a key)
ACC_KEYS = {"loss": 1, "accuracy": 2, "prior_accuracy": 3, "posterior_accuracy": 4,
            "log_prob": 6, "prior_within_sparsity_loss": 7,
            "prior_between_sparsity_loss": 8, "posterior_within_sparsity_loss": 9,
            "posterior_between_sparsity_loss": 10, "prior_cls_xe": 11,
            "posterior_cls_xe": 12, "rec_ll": 13, "rec_ll_loss": 14, "log_prob_loss": 15,
            "cpr_dynamic_reg_loss": 16}
ACC_DOUBLES = 17

# the evaluation steps' noise generators: keyed by torch's seed XOR these (step_plan.StepPlan.
# noise_salt).  Unsalted, validation batch i would draw the (seed, launch i) stream training
# step i draws, and evaluate()'s tail batch the stream of one of its full batches.
EVAL_NOISE_SALT = 0x4556414C53544550 & ((1 << 63) - 1)
EVAL_TAIL_NOISE_SALT = 0x4556414C5441494C & ((1 << 63) - 1)

# one row of predict()'s records (include/scae_hip.h, SCAE_EVAL_RECORD_FLOATS)
RECORD_FLOATS = 9
RECORD_COLUMNS = {"label": 0, "prior_class": 1, "posterior_class": 2, "prior_conf": 3,
                  "posterior_conf": 4, "prior_label_prob": 5, "posterior_label_prob": 6,
                  "rec_ll": 7, "log_prob": 8}


def means(sums):
    """{key: fp32 mean} of an accumulator (fp64, any device): sum / number of batches --
    the reference's unweighted mean over batches.  Empty (no batch) -> NaN means."""
    s = sums.detach().to("cpu", torch.float64)
    n = float(s[0])
    out = {k: (s[i] / n if n else torch.tensor(float("nan"), dtype=torch.float64))
           .to(torch.float32) for k, i in ACC_KEYS.items()}
    out["batches"] = int(n)
    return out


def out12_from_log(loss, log):
    """The loss tail's 12-vector (ops.loss_tail_scalar) from SCAE.loss's log dict, for a
    loss the fused tail did not complete; entries the model does not log are zero."""
    z = torch.zeros((), device=loss.device, dtype=loss.dtype)

    def get(k):
        v = log.get(k)
        return z if v is None else v.detach().reshape(()).to(loss.dtype)
    rec_loss, lp_loss = get("rec_ll_loss"), get("log_prob_loss")
    return torch.stack([loss.detach().reshape(()), -lp_loss,
                        get("prior_within_sparsity_loss"), get("prior_between_sparsity_loss"),
                        get("posterior_within_sparsity_loss"),
                        get("posterior_between_sparsity_loss"), get("prior_cls_xe"),
                        get("posterior_cls_xe"), -rec_loss, rec_loss, lp_loss,
                        get("cpr_dynamic_reg_loss")])


def records_host(res, image, label, labelled=True):
    """The records of one batch (csrc/eval_tail.hip, records_body) for a model on the CPU, in
    torch: (B, RECORD_FLOATS).  ``res`` gives the class probabilities (or neither), the
    reconstruction mixture ``rec.pdf`` and ``_log_prob_per_point`` where the model has them."""
    B = image.shape[0]
    rows = torch.zeros(B, RECORD_FLOATS)
    rows[:, 0:3] = -1.0
    prior, post = getattr(res, "prior_cls_prob", None), getattr(res, "posterior_cls_prob", None)
    labelled = labelled and label is not None
    if labelled:
        rows[:, 0] = label.to(torch.float32)
    if prior is not None and post is not None:
        ncls = prior.shape[-1]
        for j, p in enumerate((prior.detach().float(), post.detach().float())):
            cls = p.argmax(-1)
            rows[:, 1 + j] = cls.to(torch.float32)
            rows[:, 3 + j] = p.gather(1, cls[:, None])[:, 0]
            if labelled:
                ok = (label >= 0) & (label < ncls)
                at = p.gather(1, label.clamp(0, ncls - 1)[:, None])[:, 0]
                rows[:, 5 + j] = torch.where(ok, at, torch.zeros_like(at))
    rec = getattr(res, "rec", None)
    if rec is not None:
        rows[:, 7] = rec.pdf.log_prob(image).detach().reshape(B, -1).sum(-1)
    lpp = getattr(res, "_log_prob_per_point", None)
    if lpp is not None:
        rows[:, 8] = lpp.detach().sum(-1)
    return rows


def confusion_of(records, ncls):
    """(2, ncls, ncls) int64 [head, label, predicted] counts of ``records``' rows (any device);
    rows whose label lies outside [0, ncls) are not counted."""
    lab = records[:, 0].to(torch.int64)
    ok = (lab >= 0) & (lab < ncls)
    out = []
    for j in (1, 2):
        cell = lab[ok] * ncls + records[ok, j].to(torch.int64)
        out.append(torch.bincount(cell, minlength=ncls * ncls).view(ncls, ncls))
    return torch.stack(out)


def classification_report(confusion):
    """Per-class support, recall and precision and the example-weighted accuracy of each head,
    from a (2, ncls, ncls) [head, label, predicted] matrix (one read when it is on a device):
    {"support" (ncls,) int64, "recall" (2, ncls), "precision" (2, ncls), "accuracy" (2,),
    "predicted" (2, ncls) int64}, fp64 on the host.  A class without examples has recall 0, a
    class never predicted precision 0, an empty matrix accuracy 0: no NaN."""
    c = confusion.detach().to("cpu", torch.float64)
    if c.dim() != 3 or c.shape[0] != 2 or c.shape[1] != c.shape[2]:
        raise ValueError(f"confusion must be (2, ncls, ncls), got {tuple(confusion.shape)}")
    hit = c.diagonal(dim1=1, dim2=2)
    support, predicted = c.sum(2), c.sum(1)
    recall = torch.where(support > 0, hit / support.clamp(min=1), torch.zeros_like(hit))
    precision = torch.where(predicted > 0, hit / predicted.clamp(min=1), torch.zeros_like(hit))
    total = support.sum(1)
    accuracy = torch.where(total > 0, hit.sum(1) / total.clamp(min=1), torch.zeros_like(total))
    return {"support": support[0].to(torch.int64), "recall": recall, "precision": precision,
            "accuracy": accuracy, "predicted": predicted.to(torch.int64)}


def accumulate_host(acc, loss, out12, prior, post, label):
    """The epilogue's accumulation (csrc/eval_tail.hip) for a model on the CPU: the same
    sums, in torch.  Returns the batch's (accuracy, prior, posterior) accuracies."""
    pa = qa = torch.zeros((), dtype=torch.float32)
    if label is not None:
        B = label.shape[0]
        pa = (prior.argmax(-1) == label).sum().to(torch.float32) / B
        qa = (post.argmax(-1) == label).sum().to(torch.float32) / B
    best = torch.maximum(pa, qa)
    acc[0] += 1.0
    acc[1] += loss.detach().double().reshape(())
    acc[2] += best.double()
    acc[3] += pa.double()
    acc[4] += qa.double()
    acc[5:17] += out12.detach().double().cpu()
    return torch.stack([best, pa, qa])


class EvalStep:
    """``EvalStep(model, batch_size, image_shape)``: ``step(image, label)`` runs one
    evaluation batch and returns its loss (a device tensor the next call overwrites); the
    batch is added to the step's fp64 accumulator, ``epoch_means()`` reads it.

    Inside the step's plan the forward takes the training step's fused launches under
    ``no_grad`` (image layer and folding products in the prologue, coloured templates in
    the part-capsule head, the reconstruction likelihood in the object encoder's trunk,
    the class probabilities in the loss tail's per-image launch), and the loss tail ends
    in the evaluation epilogue (csrc/eval_tail.hip) instead of its batch combine.  A model
    the fused tail does not complete (``recon_mse_weight`` > 0,
    ``part_caps_sparsity_weight`` > 0, more than 32 classes, ``fuse_kernels=False``) takes
    its own loss launches and then the epilogue's accumulation alone.

    The step runs its warm-ups, capture and eager calls with ``model.eval()`` (the part
    encoder draws no noise; the object decoder's uniform noise comes from the step's own
    device generator) and restores ``model.training``.  It has its own plan, prologue and
    noise generator (salted: its draws are neither a training step's nor, for ``evaluate()``'s
    tail step, the full batches') and writes no gradients and no optimiser state.
    Parameters re-homed after the capture (a ``TrainStep`` built later moves them into flat
    buffers) are detected by a pointer check and the step recaptures; in-place updates need
    nothing.
    With a process group of world > 1 ``*_epoch_end`` / ``epoch_means`` sum the
    accumulators of all ranks first (data_parallel.all_reduce_sums).

    ``replay``: "graph" (hipGraphLaunch) or "launches" (the recorded launch list, when the
    captured graph holds only library launches; else the graph).  ``autocast_dtype``:
    torch.bfloat16 takes the training step's bf16 operand paths."""

    def __init__(self, model, batch_size, image_shape, use_graph=True, replay="graph",
                 autocast_dtype=None, lazy_render=True, prologue=True, fuse_kernels=True):
        if not isinstance(batch_size, int) or isinstance(batch_size, bool) \
                or batch_size <= 0:
            raise ValueError(f"batch_size must be a positive int, got {batch_size!r}")
        image_shape = tuple(image_shape)
        if len(image_shape) != 3 or not all(isinstance(d, int) and d > 0
                                            for d in image_shape):
            raise ValueError(f"image_shape must be (C, H, W), got {image_shape!r}")
        if replay not in ("graph", "launches"):
            raise ValueError("replay must be 'graph' or 'launches'")
        if autocast_dtype not in (None, torch.bfloat16):
            raise ValueError("autocast_dtype must be None or torch.bfloat16")
        self.model = model
        self._params = [p for p in model.parameters()]
        if not self._params:
            raise ValueError("model has no parameters")
        self.device = self._params[0].device
        self.batch_size, self.image_shape = batch_size, image_shape
        self.cuda = self.device.type == "cuda"
        self.use_graph = use_graph and self.cuda
        self.replay, self.autocast_dtype = replay, autocast_dtype
        self.lazy_render, self.prologue, self.fuse_kernels = lazy_render, prologue, \
            fuse_kernels
        dec = getattr(model, "part_decoder", None)
        self._lazy_dec = dec if lazy_render and hasattr(dec, "lazy_render") else None
        self._pro = ops.StepPrologue() if prologue and self.cuda else None
        # this step's plan: its prologue, parked launches and noise generator
        self.plan = ops.StepPlan("eval step", prologue=self._pro)
        self.plan.noise_salt = EVAL_NOISE_SALT
        self.epi = ops.EvalEpilogue(self.device) if self.cuda else None
        self.acc = self.epi.acc if self.cuda else \
            torch.zeros(ACC_DOUBLES, dtype=torch.float64)
        self.batch_acc = self.epi.batch3 if self.cuda else torch.zeros(3)
        self.image = torch.zeros(batch_size, *image_shape, device=self.device)
        self.label = torch.zeros(batch_size, dtype=torch.long, device=self.device)
        self.loss = torch.zeros((), device=self.device)
        self._cap = _replay.Captured()
        self.fused = None        # the captured batch ends in the fused epilogue
        self._stream = None
        self._home = None        # parameter storage the capture read
        self._tail_step = None   # evaluate()'s remainder batch
        self._cap_desc = (None, None)   # the (sink, records) the captured launches carry
        self._cpu_collect = None    # collecting on the CPU: (a batch's rows, the batches' rows)
        self._zero_labels = None

    # the captured batch, read-only (replay.Captured; _klist: its list's raw handle)
    graph = _replay.forwarded("graph")
    _klist = _replay.forwarded("handle")
    _launches = _replay.forwarded("launches")
    graph_nodes = _replay.forwarded("nodes")

    # -- the batch ----------------------------------------------------------
    def _storage(self):
        ps = self._params
        return (ps[0].data_ptr(), ps[-1].data_ptr())

    @contextlib.contextmanager
    def _eval_mode(self):
        was = self.model.training
        self.model.eval()
        prev = None
        if self._lazy_dec is not None:
            prev, self._lazy_dec.lazy_render = self._lazy_dec.lazy_render, True
        try:
            with torch.no_grad():
                yield
        finally:
            if self._lazy_dec is not None:
                self._lazy_dec.lazy_render = prev
            self.model.train(was)

    def _label_arg(self):
        return self.label if getattr(self.model, "n_classes", None) is not None else None

    def _batch(self):
        """forward + loss + epilogue on the resident buffers (eval mode, no_grad)."""
        model, label = self.model, self._label_arg()
        if not self.cuda:
            res = model(self.image)
            loss, log = model.loss(res, self.image, label)
            if self._cpu_collect is not None:
                rows_of, rows = self._cpu_collect
                rows.append(rows_of(res, self.image, label))
            probs = (res.prior_cls_prob, res.posterior_cls_prob) if label is not None \
                else (None, None)
            self.batch_acc.copy_(accumulate_host(self.acc, loss, out12_from_log(loss, log),
                                                 *probs, label))
            self.loss.copy_(loss.detach())
            return
        plan, epi = self.plan, self.epi
        epi.fused = epi.sink_written = False
        with plan.active(), plan.precision(self.autocast_dtype is not None), \
                plan.fusing(self.image if self.fuse_kernels else None), \
                plan.evaluating(epi):
            res = model(self.image)
            loss, log = model.loss(res, self.image, label)
        self.fused = epi.fused
        if not epi.fused:
            with plan.active():
                probs = (res.prior_cls_prob, res.posterior_cls_prob) \
                    if label is not None else (None, None)
                epi.accumulate(loss.detach(), out12_from_log(loss, log), *probs, label)
        if epi.sink is not None and not epi.sink_written:
            # (the class probabilities did not ride in the loss tail: the rows on their own)
            with plan.active():
                epi.sink.launch_alone(res.caps_presence, res["_posterior_full"])
        if epi.records is not None and not epi.fused:
            # (no fused epilogue to write them: the records' own launch, the reconstruction
            # term from the decoder's tile sums or, without compact inputs, its per-pixel map)
            with plan.active():
                probs = (res.prior_cls_prob, res.posterior_cls_prob) \
                    if label is not None else (None, None)
                sums = res.rec.pdf.log_prob_tile_sums(self.image)
                pixels = res.rec.pdf.log_prob(self.image) if sums is None else None
                epi.records.launch_alone(*probs, label, res["_log_prob_per_point"],
                                         rec_sums=sums, rec_pixels=pixels)
            epi.records_alone = True
        if torch.cuda.is_current_stream_capturing():
            # the captured loss lives in the graph's pool at a fixed address
            self.loss = loss.detach()
        else:
            self.loss.copy_(loss.detach())

    def _refresh_prologue(self):
        _replay.refresh_prologue(self.plan, self._pro, self.image)

    def _stage(self, image, label):
        """The batch into the resident buffers (replay.stage)."""
        if tuple(image.shape) != tuple(self.image.shape) or \
                tuple(label.shape) != tuple(self.label.shape):
            raise ValueError(f"batch of shape {tuple(image.shape)} / {tuple(label.shape)}; "
                             f"this step takes {tuple(self.image.shape)} / "
                             f"{tuple(self.label.shape)}")
        _replay.stage(self.plan, self._pro, self.image, self.label, image, label, self.device)

    def _stage_source(self, view, epoch, position, rank=None, standalone=False):
        """The view's batch at ``position`` of ``epoch`` gathered (replay.stage_source)."""
        _replay.stage_source(self.plan, self._pro, self.image, self.label, view, epoch,
                             position, rank=rank, standalone=standalone)

    # -- capture / replay ---------------------------------------------------
    def _capture(self):
        # parameters re-homed since the last capture: the prologue's registered layer
        # inputs point at the old storage -- a fresh prologue (the generator state lives
        # in the plan and continues)
        if self._home is not None and self._pro is not None:
            self._pro = ops.StepPrologue()
            self.plan.prologue = self._pro
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.device)
        s = self._stream
        s.wait_stream(torch.cuda.current_stream(self.device))
        with self._eval_mode():
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._refresh_prologue()
                    self._batch()
                self._refresh_prologue()    # what the capture below consumes
            torch.cuda.current_stream(self.device).wait_stream(s)
            # the warm-ups' batches are not the epoch's
            self.acc.zero_()
            # (keep_graph: the captured graph stays readable -- graph_nodes, always read)
            self._cap = _replay.capture(s, self._batch, keep_graph=True, census_always=True,
                                        want_list=self.replay == "launches")
        self._home = self._storage()
        self._cap_desc = (self.epi.sink, self.epi.records)
        self._refresh_prologue()

    def capture(self):
        """Build the step's graph now (or again, when the parameters have been re-homed
        since the last capture).  The accumulator is left cleared."""
        if self.use_graph and self._stale():
            self._cap.drop()
            self._capture()

    def _stale(self):
        return self.graph is None or self._home != self._storage() or \
            self._cap_desc[0] is not self.epi.sink or \
            self._cap_desc[1] is not self.epi.records

    def __call__(self, image, label):
        """One evaluation batch: stage, run (replay), accumulate.  -> the batch loss."""
        return self._run(lambda: self._stage(image, label))

    def _run(self, stage):
        stage()
        if self.use_graph:
            if self._stale():
                # (a capture runs warm-up batches: keep what the epoch has so far)
                kept = self.acc.clone()
                self.capture()
                self.acc.copy_(kept)
                stage()
            self._cap.replay(self.device)
        else:
            with self._eval_mode():
                self._batch()
        return self.loss

    # -- the reference's hooks ----------------------------------------------
    def _eager_result(self):
        """One eager no_grad forward of the staged batch (not replayed): the ``result``
        for image logging (validation_epoch_end, base_experiment.py:145-184)."""
        with self._eval_mode():
            return self.model(self.image.clone())

    def validation_images(self, result=None, n=8):
        """The three image sheets validation_epoch_end logs (base_experiment.py:152-182),
        each a (3, Hs, Ws) fp32 device tensor for ``add_image``:

        'recons': rows of the first ``min(batch_size, n)`` images -- the input, the mode of
          ``rec`` and, on a model built with ``reconstruct_alternatives``, of ``bottom_up_rec``
          and ``top_down_rec``;
        'templates': the M templates of image 0, ``int(sqrt(M))`` per row;
        'transformed_templates': the M + 1 rendered components of image 0, same layout.

        ``result``: a forward result of the staged batch (``validation_step(...,
        batch_idx=0)['result']``); default: one eager forward of the staged batch.  The modes
        come from the fused render-and-mode kernel for the ``n`` images alone and the one
        image's components from a descriptor of that image: nothing of the size of the batch's
        (B, M+1, C, H, W) tensors is made, and ``result`` stays unrendered.  Neither the
        accumulator nor the captured step is touched.

        The one-image render picks its kernel form from its own descriptor (B = 1).  Where
        the batch's render cannot take the quad-store form (its LDS bound: three-channel
        templates at B >= 512), 'transformed_templates' can differ in the last bit from
        ``result.transformed_templates[0]``; the other two sheets do not depend on B."""
        if not self.cuda:
            raise ops.ScaeHipError("validation_images runs on the library's kernels: the "
                                   "model is on the CPU")
        if not isinstance(n, int) or isinstance(n, bool) or n <= 0:
            raise ValueError(f"n must be a positive int, got {n!r}")
        res = self._eager_result() if result is None else result
        n = min(self.batch_size, n)
        with torch.no_grad():
            # (the reference's validation_step stores the batch as result.image)
            image = dict.get(res, "image")
            rows = [(self.image if image is None else image)[:n]]
            recs = [res["rec"]]
            if getattr(self.model, "reconstruct_alternatives", False):
                recs += [res["bottom_up_rec"], res["top_down_rec"]]
            for rec in recs:
                inputs = rec.pdf._decoder_inputs
                rows.append(ops.render_gmm_mode(inputs, first=0, count=n))
            sheets = {"recons": ops.image_sheet(rows, nrow=n, padding=1, pad_value=0.0)}
            templates = res["templates"][0].detach()
            nrow = int(templates.shape[0] ** 0.5)
            sheets["templates"] = ops.image_sheet([templates], nrow=nrow, padding=1,
                                                  pad_value=0.0)
            inputs = res["rec"].pdf._decoder_inputs
            one = ops.DecoderInputs(inputs.output_size, **{
                f: (getattr(inputs, f)[:1] if f in ("templates", "pose", "presence", "bg_image")
                    and getattr(inputs, f) is not None else getattr(inputs, f))
                for f in ops.DecoderInputs.FIELDS})
            components = ops.render_templates(one)[0][0]
            sheets["transformed_templates"] = ops.image_sheet([components], nrow=nrow,
                                                              padding=1, pad_value=0.0)
        return sheets

    def segmentation_images(self, result=None, n=8):
        """Two more sheets for ``add_image``, the image decomposed into its parts
        (torch_scae_amd.segment), each a (3, Hs, Ws) fp32 device tensor of the first
        ``min(batch_size, n)`` images:

        'parts': rows input, mode of ``rec``, every pixel painted with its owning part's
          colour times the part's value there (background pixels stay grey);
        'capsules': the same with the colour of the object capsule that owns the part
          (``segment.part_owner``).

        ``result`` as for ``validation_images``, whose first two 'recons' rows these sheets
        repeat.  The owners are the posterior given the staged batch, from the fused E-step
        kernel for the ``n`` images alone; ``result`` stays unrendered, the accumulator and
        the captured step untouched."""
        if not self.cuda:
            raise ops.ScaeHipError("segmentation_images runs on the library's kernels: the "
                                   "model is on the CPU")
        if not isinstance(n, int) or isinstance(n, bool) or n <= 0:
            raise ValueError(f"n must be a positive int, got {n!r}")
        from . import segment
        res = self._eager_result() if result is None else result
        n = min(self.batch_size, n)
        with torch.no_grad():
            image = dict.get(res, "image")
            image = self.image if image is None else image
            inputs = res["rec"].pdf._decoder_inputs
            # (the sheet kernel takes one channel count for all its sources)
            rgb = lambda t: t.expand(-1, 3, -1, -1) if t.shape[1] == 1 else t  # noqa: E731
            rows = [rgb(image[:n]), rgb(ops.render_gmm_mode(inputs, first=0, count=n))]
            seg = segment.segment(res, image, first=0, count=n)
            return {key: ops.image_sheet(rows + [painted], nrow=n, padding=1, pad_value=0.0)
                    for key, painted in (("parts", seg.rgb_part),
                                         ("capsules", seg.rgb_group))}

    def validation_step(self, image, label, batch_idx=None):
        """-> {'val_loss', 'accuracy'} as device tensors the next call overwrites
        (base_experiment.py:128-143); with ``batch_idx == 0`` also 'result'."""
        loss = self(image, label)
        out = {"val_loss": loss, "accuracy": self.batch_acc[0]}
        if batch_idx == 0:
            out["result"] = self._eager_result()
        return out

    def test_step(self, image, label, batch_idx=None):
        """-> {'test_loss', 'accuracy'} (base_experiment.py:186-195).  The reference's
        test_step stores the ``(loss, info)`` tuple of SCAE.loss as 'test_loss', which its
        test_epoch_end's ``torch.stack`` cannot take; this returns the loss tensor."""
        loss = self(image, label)
        out = {"test_loss": loss, "accuracy": self.batch_acc[0]}
        if batch_idx == 0:
            out["result"] = self._eager_result()
        return out

    def _global_sums(self):
        sums = self.acc.clone()
        if world()[1] > 1:
            all_reduce_sums(sums)
        return sums

    def epoch_means(self):
        """{key: fp32 mean over the batches so far} (one read; across ranks when a process
        group of world > 1 is up), plus 'batches'."""
        return means(self._global_sums())

    def reset(self):
        self.acc.zero_()

    def _epoch_end(self, prefix):
        m = self.epoch_means()
        self.reset()
        return {f"{prefix}_loss": m["loss"],
                "log": {f"{prefix}_loss": m["loss"], f"{prefix}_accuracy": m["accuracy"]}}

    def validation_epoch_end(self, outputs=None):
        """-> {'val_loss', 'log': {'val_loss', 'val_accuracy'}} (base_experiment.py:145-184:
        the unweighted means over the epoch's batches); clears the accumulator."""
        return self._epoch_end("val")

    def test_epoch_end(self, outputs=None):
        """-> {'test_loss', 'log': {'test_loss', 'test_accuracy'}} (:197-202)."""
        return self._epoch_end("test")

    def _tail(self, rem):
        tail = self._tail_step
        if tail is None or tail.batch_size != rem:
            tail = self._tail_step = EvalStep(
                self.model, rem, self.image_shape, use_graph=self.use_graph,
                replay=self.replay, autocast_dtype=self.autocast_dtype,
                lazy_render=self.lazy_render, prologue=self.prologue,
                fuse_kernels=self.fuse_kernels)
            tail.plan.noise_salt = EVAL_TAIL_NOISE_SALT     # (before its first draw)
        tail.reset()
        return tail

    # -- a whole split: evaluate / encode / predict ---------------------------------------------
    def _split(self, what, images, labels, need_labels=False, any_world=False):
        """The one argument check of ``what`` ("evaluate", "encode", "predict"), before anything
        is touched.  -> (view or None, N, full, rem): the examples of the split and this rank's
        full batches and remainder."""
        from .data import DatasetView
        B = self.batch_size
        if not any_world and world()[1] > 1:
            raise ValueError(f"{what} gathers one process's rows: world > 1 is not supported")
        if isinstance(images, DatasetView):
            view, ds = images, images.dataset
            if not self.cuda:
                raise ValueError(f"{what} of a device-resident dataset needs a device step")
            if (ds.C, ds.H, ds.W) != self.image_shape:
                raise ValueError(f"the view gives ({ds.C}, {ds.H}, {ds.W}) images, the step "
                                 f"takes {self.image_shape}")
            full = view.steps_per_epoch(B)
            rem = view.n - full * view.world * B if view.rank == 0 else 0
            return view, view.n, full, rem
        N = images.shape[0]
        if N == 0 or (labels is None and need_labels) or \
                (labels is not None and labels.shape[0] != N):
            raise ValueError("images and labels must hold the same number (> 0) of examples")
        return (None, N) + divmod(N, B)

    def _out_rows(self, out, N, shape):
        """The (R, *shape) fp32 buffer the rows go to: ``out`` checked, or N rows."""
        if out is None:
            return torch.empty(N, *shape, device=self.device)
        if tuple(out.shape[1:]) != shape or out.dtype != torch.float32 or \
                out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous (R, {', '.join(map(str, shape))}) fp32 "
                             f"tensor on {self.device}")
        return out

    def _labels_for(self, labels, lo, hi):
        if labels is not None:
            return labels[lo:hi]
        n = hi - lo
        if self._zero_labels is None or self._zero_labels.shape[0] != n:
            self._zero_labels = torch.zeros(n, dtype=torch.long, device=self.device)
        return self._zero_labels

    def _walk(self, split, images, labels, collect=None):
        """Run a checked split (``_split``): every full batch replayed, the remainder through
        a second step of the remainder's size (``_tail``: captured once, cached by size; not
        padded -- the between-example terms depend on the batch size).  Both accumulators are
        cleared on entry and on exit.  -> (this step's fp64 sums, the tail step's or None,
        ``_collecting``'s dict).

        Tensors are staged batch by batch, missing labels as cached zeros.  A data.DatasetView
        gives its examples in the order and with the shifts of its current epoch
        (``view.materialise()``): the full batches gathered in the step's prologue launch, the
        remainder by the stand-alone gather into the tail step.  With ``view.world`` > 1 rank r
        takes slots [r*B, (r+1)*B) of each global batch of world*B and rank 0 alone the
        remainder.  The view moves on to its next epoch once every batch has run.

        ``collect``: ``_collecting``'s arguments after the steps -- the rows the batches write
        on the way."""
        view, N, full, rem = split
        B = self.batch_size
        tail = self._tail(rem) if rem else None
        steps = [self] + ([tail] if tail is not None else [])
        rows = self._collecting(steps, *collect) if collect else contextlib.nullcontext({})
        with rows as got:
            self.reset()
            if view is not None:
                epoch, stride = view.epoch, view.world * B
                for i in range(full):
                    self._run(lambda: self._stage_source(view, epoch, i * stride))
                if tail is not None:
                    tail._run(lambda: tail._stage_source(view, epoch, full * stride, rank=0,
                                                         standalone=True))
                view.epoch, view.cursor = epoch + 1, 0
            else:
                for i in range(full):
                    self(images[i * B:(i + 1) * B], self._labels_for(labels, i * B,
                                                                     (i + 1) * B))
                if tail is not None:
                    tail(images[full * B:], self._labels_for(labels, full * B, N))
            sums, tail_sums = self.acc.clone(), None
            if tail is not None:
                tail_sums = tail.acc.clone()
                tail.reset()
            self.reset()
        return sums, tail_sums, got

    def _attach(self, field, desc):
        """Aim this step's batches at ``desc``, the epilogue's ``field`` ("sink", "records");
        off while the capture's warm-ups run."""
        setattr(self.epi, field, desc)
        if self.use_graph:
            self.capture()

    @contextlib.contextmanager
    def _collecting(self, steps, out, field, make, rows_of, aim=()):
        """The rows ``steps``' batches write on the way, into ``out``.  -> a dict that holds
        "rows" (rows written) and "overflow" on exit.  On the device through the epilogue's
        descriptor ``field`` (made by ``make`` once, attached to every step -- a step whose
        descriptor changed recaptures, ``_stale`` -- aimed by ``point(out, *aim)``, read once,
        and off again whatever happens: it stays attached with capacity 0, so later calls
        replay the same graphs).  On the CPU each batch appends ``rows_of(res, image, label)``
        and the rows that fit are copied."""
        if self.cuda:
            desc = getattr(self.epi, field)
            if desc is None:
                desc = make(self.device)
            desc.off()
            for st in steps:
                st._attach(field, desc)
            desc.point(out, *aim)
        else:
            for st in steps:
                st._cpu_collect = (rows_of, [])
        got = {}
        try:
            yield got
            if self.cuda:
                cursor, overflow = desc.status()
            else:
                rows = torch.cat([r for st in steps for r in st._cpu_collect[1]])
                cursor, overflow = rows.shape[0], rows.shape[0] > out.shape[0]
            written = min(cursor, out.shape[0])
            if not self.cuda:
                out[:written].copy_(rows[:written])
            got.update(rows=written, overflow=overflow)
        finally:
            if self.cuda:
                desc.off()
            else:
                for st in steps:
                    st._cpu_collect = None

    def evaluate(self, images, labels=None):
        """A whole split (``_walk``; ``images`` may be a data.DatasetView instead of (images,
        labels)).  -> ``epoch_means()`` of the split: the unweighted mean over its batches, as
        the reference's loop (and a ``drop_last=False`` loader) gives."""
        split = self._split("evaluate", images, labels, need_labels=True, any_world=True)
        sums, tail_sums, _ = self._walk(split, images, labels)
        reduce = world()[1] > 1
        if reduce and split[0] is None and tail_sums is not None:
            # tensors: the two steps' sums are reduced each on its own and then added, a view's
            # are added and then reduced.  The two orders can differ in the last fp64 bit, so
            # each stays as it was
            all_reduce_sums(sums)
            all_reduce_sums(tail_sums)
            reduce = False
        if tail_sums is not None:
            sums += tail_sums
        if reduce:
            all_reduce_sums(sums)
        return means(sums)

    def encode(self, images, labels=None, out=None):
        """The object-capsule features of a whole split (``_walk``; ``images`` may be a
        data.DatasetView), with its evaluation means: each image's two classifier inputs --
        ``caps_presence`` and the posterior mass ``posterior_mixing_prob.sum(-1)`` -- stored
        into a device sink on the way (by the loss tail's per-image launch where SCAE.forward's
        class probabilities ride in it, else by one launch of its own per batch).

        -> {"prior" (N, O), "posterior" (N, O), "label" (N,) int64 or None, "means"
        (``evaluate``'s), "rows" (rows written), "overflow"}.  ``out``: an (R, 2, O) fp32
        device buffer to write into (default: N rows); rows at or beyond R are dropped and
        ``overflow`` is True.  Without labels the step's loss sees zeros and the accuracies
        in ``means`` mean nothing."""
        split = self._split("encode", images, labels)
        view, N = split[:2]
        O = self.model.obj_decoder.n_obj_capsules
        out = self._out_rows(out, N, (2, O))
        if view is not None:
            ds = view.dataset
            rows, _ = view.rows_and_shifts(view.epoch, torch.arange(N))
            label = ds.labels[rows.to(ds.device)].to(torch.int64)
        else:
            label = None if labels is None else labels.to(self.device, torch.int64)
        sums, tail_sums, got = self._walk(split, images, labels, (
            out, "sink", ops.EvalSink, lambda res, image, lab: torch.stack(
                [res.caps_presence, res.posterior_mixing_prob.sum(-1)], 1)))
        if tail_sums is not None:
            sums += tail_sums
        feats = out[:got["rows"]]
        return {"prior": feats[:, 0], "posterior": feats[:, 1], "label": label,
                "means": means(sums), **got, "features": feats}

    def predict(self, images, labels=None, out=None):
        """One record per image of a whole split (``_walk``; ``images`` may be a
        data.DatasetView), both heads' confusion matrices and the split's evaluation means:
        the records written on the way by the launch that ends each batch (the fused
        epilogue's combine workgroup; for a model outside the fused tail one launch of its own
        per batch).

        -> {"records": (N, 9) fp32 device tensor, one row per image --
              [0] label (-1 without labels)
              [1] prior-head class  [2] posterior-head class (``torch.argmax``'s rule)
              [3] [4] the heads' probability of their own predicted class
              [5] [6] the heads' probability of the label's class (0 without labels)
              [7] the image's reconstruction log-likelihood (``rec_ll``'s per-image term)
              [8] the image's capsule log-likelihood (``log_prob``'s per-image term);
            "label", "prior_class", "posterior_class", "prior_conf", "posterior_conf",
            "prior_label_prob", "posterior_label_prob", "rec_ll", "log_prob": views of those
            columns; "label_int", "prior_class_int", "posterior_class_int": the three as int64;
            "confusion": (2, ncls, ncls) int64 device tensor indexed [head, label, predicted],
            head 0 the prior and 1 the posterior (``classification_report`` reads it);
            "means" (``evaluate``'s); "rows" (rows written); "overflow"}.
        ``out``: an (R, 9) fp32 device buffer to write into (default: N rows); rows at or beyond
        R are dropped, are not counted in ``confusion`` either, and ``overflow`` is True.
        Without labels the step's loss sees zeros: the accuracies in ``means`` mean nothing,
        ``confusion`` stays zero and means nothing either.  A model without classes gives
        classes -1, probabilities 0 and an empty ``confusion``."""
        split = self._split("predict", images, labels)
        view, N = split[:2]
        ncls = getattr(self.model, "n_classes", None) or 0
        labelled = view is not None or labels is not None
        out = self._out_rows(out, N, (RECORD_FLOATS,))
        confusion = torch.zeros(2, ncls, ncls, dtype=torch.int64, device=self.device)
        sums, tail_sums, got = self._walk(split, images, labels, (
            out, "records", ops.EvalRecords,
            lambda res, image, label: records_host(res, image, label, labelled),
            (confusion, labelled)))
        if tail_sums is not None:
            sums += tail_sums
        rows = out[:got["rows"]]
        if not self.cuda and labelled and ncls:
            confusion = confusion_of(rows, ncls)
        res = {"records": rows, "confusion": confusion, "means": means(sums), **got}
        for name, j in RECORD_COLUMNS.items():
            res[name] = rows[:, j]
        for name in ("label", "prior_class", "posterior_class"):
            res[name + "_int"] = res[name].to(torch.int64)
        return res
