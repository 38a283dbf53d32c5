"""Host logic of the evaluation step on CPU: the epoch means (unweighted over batches, a
remainder batch through its own step), the cross-rank reduction of the accumulator
(gloo, world size 2) and argument validation -- of EvalStep and of the epilogue's C entry
points, which reject bad arguments before any HIP call."""
import os
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn


class StubModel(nn.Module):
    """A CPU stand-in with SCAE's evaluation surface: class probabilities from the
    image's per-class means, a loss that depends on the batch size (as SCAE's
    between-example terms do) and a log dict with some of SCAE.loss's keys."""

    n_classes = 3

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(1))

    def forward(self, image):
        x = image.flatten(1)[:, :3] * self.w
        return SimpleNamespace(prior_cls_prob=torch.softmax(x, -1),
                               posterior_cls_prob=torch.softmax(-x, -1))

    def loss(self, res, image, label):
        lp = image.mean() * image.shape[0]
        loss = lp + res.prior_cls_prob[:, 0].mean()
        return loss, dict(log_prob_loss=lp, rec_ll_loss=loss - lp,
                          cpr_dynamic_reg_loss=torch.zeros(()))


def _batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 1, 2, 2, generator=g), torch.randint(0, 3, (n,), generator=g)


def _hand(model, images, labels, B):
    """The reference's loop: per batch forward + loss + calculate_accuracy, then the plain
    mean over the batches' values."""
    losses, accs = [], []
    with torch.no_grad():
        return _hand_loop(model, images, labels, B, losses, accs)


def _hand_loop(model, images, labels, B, losses, accs):
    for i in range(0, images.shape[0], B):
        x, y = images[i:i + B], labels[i:i + B]
        res = model(x)
        loss, _ = model.loss(res, x, y)
        a = (res.prior_cls_prob.argmax(-1) == y).float().mean()
        b = (res.posterior_cls_prob.argmax(-1) == y).float().mean()
        losses.append(float(loss))
        accs.append(float(torch.max(a, b)))
    return sum(losses) / len(losses), sum(accs) / len(accs), len(losses)


def test_epoch_means_are_unweighted_over_batches_with_a_remainder():
    from torch_scae_amd import EvalStep
    torch.manual_seed(0)
    model = StubModel()
    model.train()
    images, labels = _batches(10, 1)
    step = EvalStep(model, 4, (1, 2, 2))
    m = step.evaluate(images, labels)
    loss, acc, n = _hand(model, images, labels, 4)
    assert m["batches"] == n == 3
    assert abs(float(m["loss"]) - loss) <= 1e-6 * abs(loss)
    assert abs(float(m["accuracy"]) - acc) <= 1e-6
    # a weighted mean would differ: the remainder batch has half the images
    w = sum(float(model.loss(model(images[i:i + 4]), images[i:i + 4], None)[0])
            * images[i:i + 4].shape[0] for i in range(0, 10, 4)) / 10
    assert abs(w - loss) > 1e-3
    assert model.training                       # restored
    assert float(step.acc.abs().sum()) == 0.0   # evaluate leaves it cleared
    assert step._tail_step.batch_size == 2
    # the reference's hooks: per-batch values, then the epoch's means
    outs = [step.validation_step(images[i:i + 4], labels[i:i + 4], i) for i in (0, 4)]
    assert "result" in outs[0] and "result" not in outs[1]
    end = step.validation_epoch_end(outs)
    loss2, acc2, _ = _hand(model, images[:8], labels[:8], 4)
    assert abs(float(end["val_loss"]) - loss2) <= 1e-6 * abs(loss2)
    assert abs(float(end["log"]["val_accuracy"]) - acc2) <= 1e-6
    assert float(step.acc.abs().sum()) == 0.0   # *_epoch_end resets
    step.test_step(images[:4], labels[:4])
    end = step.test_epoch_end()
    assert set(end) == {"test_loss", "log"} and set(end["log"]) == {"test_loss",
                                                                    "test_accuracy"}


class CapsStub(StubModel):
    """StubModel with the object-capsule surface ``encode`` reads as well."""

    def __init__(self):
        super().__init__()
        self.obj_decoder = SimpleNamespace(n_obj_capsules=2)

    def forward(self, image):
        res = super().forward(image)
        x = image.flatten(1) * self.w
        res.caps_presence, res.posterior_mixing_prob = x[:, :2], x.view(-1, 2, 2)
        return res


@pytest.mark.parametrize("N", [10, 8])
def test_evaluate_encode_and_predict_give_the_same_means(N):
    """The three walk the split alike: identical means, with a remainder batch (N = 10) and
    without (N = 8), and again on the same step (the tail step reused, accumulators cleared)."""
    from torch_scae_amd import EvalStep
    model = CapsStub()
    images, labels = _batches(N, 3)
    step = EvalStep(model, 4, (1, 2, 2))
    rounds = []
    for _ in range(2):
        m = step.evaluate(images, labels)
        assert m["batches"] == -(-N // 4)
        for other in (step.encode(images, labels)["means"],
                      step.predict(images, labels)["means"]):
            assert set(other) == set(m)
            for k in m:
                assert torch.equal(torch.as_tensor(m[k]), torch.as_tensor(other[k])), k
        for s in (step, step._tail_step):
            assert s is None or float(s.acc.abs().sum()) == 0.0
        rounds.append(m)
    assert (step._tail_step is None) == (N % 4 == 0)
    for k in rounds[0]:
        assert torch.equal(torch.as_tensor(rounds[0][k]), torch.as_tensor(rounds[1][k])), k


def test_epoch_means_keep_every_key_and_count():
    from torch_scae_amd import eval_step
    acc = torch.zeros(eval_step.ACC_DOUBLES, dtype=torch.float64)
    for v in (1.0, 2.0, 4.0):
        out12 = torch.arange(12, dtype=torch.float32) * v
        eval_step.accumulate_host(acc, torch.tensor(v), out12, None, None, None)
    m = eval_step.means(acc)
    assert m["batches"] == 3
    assert float(m["loss"]) == pytest.approx(7 / 3)
    assert float(m["log_prob"]) == pytest.approx(7 / 3)           # out12[1]
    assert float(m["cpr_dynamic_reg_loss"]) == pytest.approx(11 * 7 / 3)
    assert m["loss"].dtype == torch.float32
    assert set(eval_step.ACC_KEYS) <= set(m)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from torch_scae_amd import EvalStep
    from torch_scae_amd.data_parallel import all_reduce_sums
    buf = torch.tensor([1.0, rank + 0.5], dtype=torch.float64)
    all_reduce_sums(buf)
    torch.manual_seed(0)
    model = StubModel()
    step = EvalStep(model, 4, (1, 2, 2))
    images, labels = _batches(8, 10 + rank)     # each rank its own two batches
    for i in (0, 4):
        step.validation_step(images[i:i + 4], labels[i:i + 4], i)
    end = step.validation_epoch_end()
    out[rank] = (buf, float(end["val_loss"]), float(end["log"]["val_accuracy"]))
    dist.destroy_process_group()


def test_two_rank_epoch_means_are_global():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    (b0, l0, a0), (b1, l1, a1) = out[0], out[1]
    assert torch.equal(b0, b1) and b0.tolist() == [2.0, 2.0]
    assert l0 == l1 and a0 == a1
    torch.manual_seed(0)
    model = StubModel()
    imgs, labs = zip(*(_batches(8, 10 + r) for r in range(world)))
    loss, acc, n = _hand(model, torch.cat(imgs), torch.cat(labs), 4)
    assert n == 4
    assert abs(l0 - loss) <= 1e-6 * abs(loss) and abs(a0 - acc) <= 1e-6


def test_eval_step_rejects_bad_arguments():
    from torch_scae_amd import EvalStep
    model = StubModel()
    for bad in (0, -4, 2.0, True):
        with pytest.raises(ValueError):
            EvalStep(model, bad, (1, 2, 2))
    with pytest.raises(ValueError):
        EvalStep(model, 4, (2, 2))
    with pytest.raises(ValueError):
        EvalStep(model, 4, (1, 2, 2), replay="stream")
    with pytest.raises(ValueError):
        EvalStep(model, 4, (1, 2, 2), autocast_dtype=torch.float16)
    step = EvalStep(model, 4, (1, 2, 2))
    images, labels = _batches(6, 0)
    with pytest.raises(ValueError):            # a batch of another size
        step(images, labels)
    with pytest.raises(ValueError):
        step.evaluate(images, labels[:5])


def test_epilogue_entry_points_reject_bad_arguments_without_a_gpu():
    from torch_scae_amd import _lib
    lib = _lib.load()
    P = 0x1000          # (never dereferenced: validation comes first)
    acc = P
    assert lib.scae_eval_accumulate_f32(None, None, None, None, None, 4, 0, acc, None,
                                        None) == -1                      # no loss
    assert lib.scae_eval_accumulate_f32(P, None, None, None, None, 4, 0, None, None,
                                        None) == -1                      # no accumulator
    assert lib.scae_eval_accumulate_f32(P, None, None, None, None, 0, 0, acc, None,
                                        None) == -1                      # B = 0
    assert lib.scae_eval_accumulate_f32(P, None, None, None, P, 4, 10, acc, None,
                                        None) == -1                      # label, no probs
    assert lib.scae_eval_accumulate_f32(P, None, P, P, P, 4, 0, acc, None,
                                        None) == -1                      # label, 0 classes
    w5 = (_lib.c_float * 5)(1, 0, 0, 0, 0)
    tail = [P, P, P, None, None, None, None, P, P]
    assert lib.scae_eval_tail_f32(*tail, 4, 4, 4, 0, 0, 0, 0, 0, w5, 0.0, None, None, None,
                                  None, None) == -1                      # no accumulator
    assert lib.scae_eval_tail_f32(*tail, 4, 5000, 4, 0, 0, 0, 0, 0, w5, 0.0, None, None,
                                  acc, None, None) == -2                 # O beyond the tail
    lab = [P, P, P, P, P, P, None, P, P]
    assert lib.scae_eval_tail_f32(*lab, 4, 4, 4, 40, 40, 0, 0, 0, w5, 0.0, P, P, acc, None,
                                  None) == -2                            # > 32 classes
    assert lib.scae_eval_tail_f32(*lab, 4, 4, 4, 10, 10, 0, 0, 0, w5, 0.0, None, None,
                                  acc, None, None) == -1                 # label, no probs
