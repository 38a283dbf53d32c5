"""Host logic of ``EvalStep.predict`` on CPU: the records' rows, their order, the remainder
batch, overflow, the means (``evaluate``'s), the confusion matrix against a bincount of the
records, ``classification_report`` on a hand-made matrix, and argument validation of the new C
entry points, which reject bad arguments before any HIP call."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn


class _Pdf:
    def __init__(self, mean):
        self.mean = mean

    def log_prob(self, x):
        return -(x - self.mean) ** 2


class StubModel(nn.Module):
    """A CPU stand-in with SCAE's evaluation surface (tests/test_eval_step.py's), plus what
    the records read: a reconstruction mixture with a per-pixel ``log_prob`` and the
    per-point capsule log-likelihood."""

    n_classes = 3

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(1))

    def forward(self, image):
        x = image.flatten(1)[:, :3] * self.w
        return SimpleNamespace(prior_cls_prob=torch.softmax(x, -1),
                               posterior_cls_prob=torch.softmax(-x, -1),
                               rec=SimpleNamespace(pdf=_Pdf(0.25 * self.w)),
                               _log_prob_per_point=-image.flatten(1) * 2.0)

    def loss(self, res, image, label):
        lp = image.mean() * image.shape[0]
        loss = lp + res.prior_cls_prob[:, 0].mean()
        return loss, dict(log_prob_loss=lp, rec_ll_loss=loss - lp,
                          cpr_dynamic_reg_loss=torch.zeros(()))


def _split(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 1, 2, 2, generator=g), torch.randint(0, 3, (n,), generator=g)


def _hand_records(model, images, labels):
    """Row by row, from the definitions (no batching: the stub's rows do not depend on it)."""
    with torch.no_grad():
        res = model(images)
    rows = []
    for b in range(images.shape[0]):
        p, q = res.prior_cls_prob[b], res.posterior_cls_prob[b]
        lab = -1 if labels is None else int(labels[b])
        pc, qc = int(p.argmax()), int(q.argmax())
        rows.append([float(lab), float(pc), float(qc), float(p[pc]), float(q[qc]),
                     float(p[lab]) if lab >= 0 else 0.0, float(q[lab]) if lab >= 0 else 0.0,
                     float((-(images[b] - 0.25) ** 2).sum()),
                     float((-images[b].flatten() * 2.0).sum())])
    return torch.tensor(rows)


def test_predict_rows_order_remainder_means_and_confusion():
    from torch_scae_amd import EvalStep, eval_step
    torch.manual_seed(0)
    model = StubModel().train()
    images, labels = _split(10, 1)
    step = EvalStep(model, 4, (1, 2, 2))
    got = step.predict(images, labels)
    assert got["rows"] == 10 and not got["overflow"]
    assert step._tail_step.batch_size == 2              # the remainder: its own step
    rec = got["records"]
    assert rec.shape == (10, eval_step.RECORD_FLOATS) and rec.dtype == torch.float32
    want = _hand_records(model, images, labels)
    assert torch.equal(rec[:, :3], want[:, :3])         # label and classes, in input order
    assert torch.allclose(rec[:, 3:], want[:, 3:], rtol=1e-6, atol=1e-6)
    # the named views and their int64 forms
    for name, j in eval_step.RECORD_COLUMNS.items():
        assert torch.equal(got[name], rec[:, j]), name
    assert got["label_int"].dtype == torch.int64
    assert torch.equal(got["label_int"], labels)
    assert torch.equal(got["prior_class_int"], want[:, 1].long())
    assert torch.equal(got["posterior_class_int"], want[:, 2].long())
    # means: evaluate's
    m = step.evaluate(images, labels)
    assert set(m) == set(got["means"]) and m["batches"] == got["means"]["batches"] == 3
    for k in eval_step.ACC_KEYS:
        assert float(m[k]) == float(got["means"][k]), k
    # confusion == bincount of the records, [head, label, predicted]
    conf = got["confusion"]
    assert conf.shape == (2, 3, 3) and conf.dtype == torch.int64
    for h in (0, 1):
        cells = rec[:, 0].long() * 3 + rec[:, 1 + h].long()
        assert torch.equal(conf[h].flatten(), torch.bincount(cells, minlength=9))
        assert int(conf[h].sum()) == 10
    assert model.training and float(step.acc.abs().sum()) == 0.0
    # accuracy from the matrix == the split's example-weighted accuracy
    rep = eval_step.classification_report(conf)
    assert float(rep["accuracy"][0]) == pytest.approx(
        float((rec[:, 1] == rec[:, 0]).double().mean()))


def test_predict_overflow_and_no_labels():
    from torch_scae_amd import EvalStep, eval_step
    model = StubModel()
    images, labels = _split(10, 2)
    step = EvalStep(model, 4, (1, 2, 2))
    full = step.predict(images, labels)["records"].clone()
    out = torch.full((6, eval_step.RECORD_FLOATS), 7.0)
    got = step.predict(images, labels, out=out)
    assert got["rows"] == 6 and got["overflow"]
    assert got["records"].data_ptr() == out.data_ptr()
    assert torch.equal(out, full[:6])
    assert int(got["confusion"].sum()) == 2 * 6          # the rows written, per head
    big = torch.full((12, eval_step.RECORD_FLOATS), 7.0)
    got = step.predict(images, labels, out=big)
    assert got["rows"] == 10 and not got["overflow"]
    assert torch.equal(big[:10], full) and float(big[10:].min()) == 7.0
    # without labels: label -1, no label probabilities, an all-zero confusion
    nol = step.predict(images)
    assert torch.equal(nol["records"][:, 0], torch.full((10,), -1.0))
    assert float(nol["records"][:, 5:7].abs().sum()) == 0.0
    assert torch.equal(nol["records"][:, [1, 2, 3, 4, 7, 8]], full[:, [1, 2, 3, 4, 7, 8]])
    assert int(nol["confusion"].abs().sum()) == 0
    for bad in (torch.zeros(6, 8), torch.zeros(6, 9, dtype=torch.float64),
                torch.zeros(9, 6).t()):
        with pytest.raises(ValueError):
            step.predict(images, labels, out=bad)
    with pytest.raises(ValueError):
        step.predict(images, labels[:5])


def test_classification_report_on_a_hand_made_matrix():
    from torch_scae_amd import eval_step
    # 3 classes, class 2 has no examples; head 1 never predicts class 0
    prior = [[3, 1, 0],
             [2, 4, 0],
             [0, 0, 0]]
    post = [[0, 2, 2],
            [0, 5, 1],
            [0, 0, 0]]
    rep = eval_step.classification_report(torch.tensor([prior, post]))
    assert rep["support"].tolist() == [4, 6, 0]
    assert rep["predicted"].tolist() == [[5, 5, 0], [0, 7, 3]]
    assert rep["recall"].tolist() == [[3 / 4, 4 / 6, 0.0], [0.0, 5 / 6, 0.0]]
    assert rep["precision"].tolist() == [[3 / 5, 4 / 5, 0.0], [0.0, 5 / 7, 0.0]]
    assert rep["accuracy"].tolist() == [7 / 10, 5 / 10]
    empty = eval_step.classification_report(torch.zeros(2, 3, 3, dtype=torch.int64))
    assert empty["accuracy"].tolist() == [0.0, 0.0]
    assert not any(torch.isnan(v.double()).any() for v in empty.values())
    with pytest.raises(ValueError):
        eval_step.classification_report(torch.zeros(3, 3))


def test_records_entry_points_reject_bad_arguments_without_a_gpu():
    from torch_scae_amd import _lib
    lib = _lib.load()
    P = 0x1000          # (never dereferenced: validation comes first)
    rec = P
    # scae_eval_records_f32(prior, post, label, lpp, rec_sums, rec_pixels, B, ncls, M, n_rec,
    #                       records, stream)
    f = lib.scae_eval_records_f32
    assert f(P, P, P, P, P, None, 4, 10, 4, 4, None, None) == -1     # no records
    assert f(P, P, P, P, P, None, 0, 10, 4, 4, rec, None) == -1      # B = 0
    assert f(P, P, P, P, P, None, -4, 10, 4, 4, rec, None) == -1     # B < 0
    assert f(P, P, P, P, P, None, 4, -1, 4, 4, rec, None) == -1      # ncls < 0
    assert f(None, P, P, P, P, None, 4, 10, 4, 4, rec, None) == -1   # classes, no probs
    assert f(P, None, P, P, P, None, 4, 10, 4, 4, rec, None) == -1
    assert f(P, P, P, P, P, None, 4, 10, 0, 4, rec, None) == -1      # lpp, M = 0
    assert f(P, P, P, P, P, None, 4, 10, 4, 0, rec, None) == -1      # tile sums, none of them
    assert f(P, P, P, P, None, P, 4, 10, 4, -3, rec, None) == -1     # a map of no pixels
    assert f(P, P, P, P, P, None, 4, _lib.EVAL_RECORDS_MAX_CLASSES + 1, 4, 4, rec,
             None) == -2                                             # beyond the LDS histograms
    w5 = (_lib.c_float * 5)(1, 0, 0, 0, 0)
    g = lib.scae_eval_tail_records_f32
    tail = [P, P, P, None, None, None, None, P, P]
    assert g(*tail, 4, 4, 4, 0, 0, 0, 0, 0, w5, 0.0, None, None, None, None, None, rec,
             None) == -1                                             # no accumulator
    assert g(*tail, 4, 5000, 4, 0, 0, 0, 0, 0, w5, 0.0, None, None, P, None, None, rec,
             None) == -2                                             # O beyond the tail
    assert g(*tail, 0, 4, 4, 0, 0, 0, 0, 0, w5, 0.0, None, None, P, None, None, rec,
             None) == -1                                             # B = 0
    lab = [P, P, P, P, P, P, None, P, P]
    assert g(*lab, 4, 4, 4, 40, 40, 0, 0, 0, w5, 0.0, P, P, P, None, None, rec,
             None) == -2                                             # > 32 classes
    assert g(*lab, 4, 4, 4, 10, 10, 0, 0, 0, w5, 0.0, None, None, P, None, None, rec,
             None) == -1                                             # label, no probs
    ex = _lib.LossExtras()
    ex.rec_sums, ex.n_rec = P, 7                                     # 7 sums for 4 images
    bad = [P, P, P, P, P, P, _lib.ctypes.byref(ex), P, P]
    assert g(*bad, 4, 4, 4, 10, 10, 0, 0, 0, w5, 0.0, P, P, P, None, None, rec,
             None) == -1
    # without records it is scae_eval_tail_sink_f32: the same validation
    assert g(*tail, 4, 4, 4, 0, 0, 0, 0, 0, w5, 0.0, None, None, None, None, None, None,
             None) == -1
    assert _lib.EVAL_RECORDS_INT64S == 7 and _lib.EVAL_RECORD_FLOATS == 9
