"""Tracked gradient norms (Lightning's Trainer(track_grad_norm=p)) without a GPU: the setting's
parsing and factory.make_train_step's reading of ``trainer.track_grad_norm``; the host
yardstick ``segment_norms_host`` against torch.linalg.vector_norm; the rows' names (per-capsule
keys, gradient-less parameters absent, total last); the chunk table scae_segment_norms_f32
works from; and a CPU TrainStep whose rows are the norms of the per-parameter ``.grad``s, with
and without accumulation.  The kernel and the replayed step: test_grad_norms_gpu.py."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.test_optimizers import REF_CFG, YAML
from tests.test_train_remainder import SMALL

ULP = 2.0 ** -23     # one fp32 ulp, relative (at most)


# -- the setting --------------------------------------------------------------------------------
@pytest.mark.parametrize("given,p", [(1, 1.0), (2, 2.0), (2.0, 2.0), (float("inf"), math.inf),
                                     ("inf", math.inf), (None, None), (-1, None), (0, None)])
def test_track_value_reads_lightnings_values(given, p):
    from torch_scae_amd.data_parallel import track_value
    assert track_value(given) == p


@pytest.mark.parametrize("bad", [3, 1.5, -2, True, "2", "INF", float("nan"), -math.inf, [2]])
def test_track_value_refuses_everything_else(bad):
    from torch_scae_amd.data_parallel import track_value
    with pytest.raises(ValueError):
        track_value(bad)


def test_train_step_validates_the_setting_and_needs_an_optimizer():
    from torch_scae_amd.train_step import TrainStep
    with pytest.raises(ValueError):
        TrainStep(Toy(), 4, (1, 4, 4), track_grad_norm=3)
    with pytest.raises(ValueError):
        TrainStep(Toy(), 4, (1, 4, 4), optimizer=None, track_grad_norm=2)
    off = TrainStep(Toy(), 4, (1, 4, 4))
    assert off.grad_norms is None and off.last_grad_norm() is None
    for call in (off.grad_norm_names, off.last_grad_norms, off.grad_norm_history,
                 off.parameter_norms):
        with pytest.raises(ValueError):
            call()
    assert TrainStep(Toy(), 4, (1, 4, 4), track_grad_norm=-1).grad_norms is None
    assert TrainStep(Toy(), 4, (1, 4, 4), track_grad_norm="inf").grad_norms.p == math.inf


@pytest.mark.parametrize("given,p", [(2, 2.0), ("inf", math.inf), (-1, None), (None, None)])
def test_factory_reads_trainer_track_grad_norm(given, p):
    from torch_scae_amd import factory
    cfg = dict(REF_CFG, optimizer=YAML["adam"], trainer=dict(max_epochs=3))
    if given is not None:
        cfg["trainer"]["track_grad_norm"] = given
    step = factory.make_train_step(Toy(), cfg)
    assert (step.grad_norms.p if p is not None else step.grad_norms) == p
    with pytest.raises(ValueError):
        factory.make_train_step(Toy(), dict(cfg, trainer=dict(track_grad_norm=3)))
    assert factory.make_train_step(Toy(), dict(REF_CFG, optimizer=YAML["adam"])).grad_norms is None


# -- the host yardstick ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, math.inf])
def test_segment_norms_host_is_vector_norm_per_segment(p):
    from torch_scae_amd.data_parallel import segment_norms_host
    x = torch.randn(40, generator=torch.Generator().manual_seed(3))
    segs = [(1, 1), (2, 5), (9, 7), (30, 10)]
    row = segment_norms_host(x, segs, p, scale=0.25)
    assert row.dtype == torch.float32 and row.shape == (5,)
    ref = [0.25 * float(torch.linalg.vector_norm(x[o:o + n].double(), p)) for o, n in segs]
    ref.append(float(torch.linalg.vector_norm(torch.tensor(ref, dtype=torch.float64), p)))
    assert np.allclose(row.double().numpy(), ref, rtol=ULP, atol=0)
    x[10] = float("nan")
    row = segment_norms_host(x, segs, p)
    assert [bool(v) for v in torch.isnan(row)] == [False, False, True, False, True]


# -- names ------------------------------------------------------------------------------------------
def _small_step(**kw):
    from torch_scae_amd import factory
    from torch_scae_amd.train_step import TrainStep
    torch.manual_seed(0)
    model = factory.make_scae(SMALL)
    step = TrainStep(model, 4, (1, 16, 16), use_graph=False, **kw)
    seen = [not n.startswith(("obj_decoder.dummy_vote", "posterior_classifier."))
            for n in _names_in_flat_order(step)]
    assert not all(seen)
    step.grad_norms.build(seen)
    return step, seen


def _names_in_flat_order(step):
    name = {id(p): n for n, p in step.model.named_parameters()}
    return [name[id(p)] for p in step.flat.params]


def test_names_skip_gradient_less_parameters_and_end_in_the_total():
    step, seen = _small_step(track_grad_norm=2, split_capsules=False)
    names = step.grad_norm_names()
    kept = [n for n, s in zip(_names_in_flat_order(step), seen) if s]
    assert names == [f"grad_2.0_norm_{n}" for n in kept] + ["grad_2.0_norm_total"]
    assert not any("dummy_vote" in n or "posterior_classifier" in n for n in names)
    assert step.grad_norm_names("ocae/")[0] == f"grad_2.0_norm_ocae/{kept[0]}"
    assert _small_step(track_grad_norm="inf")[0].grad_norm_names()[-1] == "grad_inf_norm_total"


def test_split_capsules_names_the_state_dicts_per_capsule_keys_in_flat_order():
    from torch_scae_amd.nn_ext import GroupedMLP
    step, seen = _small_step(track_grad_norm=1)
    trk, model = step.grad_norms, step.model
    stacked = {id(p) for m in model.modules() if isinstance(m, GroupedMLP)
               for p in m.parameters()}
    assert stacked
    plain = {n for n, p in model.named_parameters() if id(p) not in stacked}
    capsule_keys = [k for k in model.state_dict() if k not in plain]
    got = [k for k, _, _ in trk.segments if k not in plain]
    assert sorted(got) == sorted(capsule_keys) and len(set(got)) == len(got)
    # every key covers exactly its slice of the flat buffer, segments ascending
    sd = model.state_dict()
    base = step.flat.flat_param.data_ptr()
    for key, off, n in trk.segments:
        assert sd[key].numel() == n and sd[key].data_ptr() == base + 4 * off, key
    offs = [off for _, off, _ in trk.segments]
    assert offs == sorted(offs)
    assert trk.names()[-1] == "grad_1.0_norm_total" and len(trk.names()) == len(offs) + 1
    # and one entry per stacked tensor without the split
    one = _small_step(track_grad_norm=1, split_capsules=False)[0].grad_norms
    assert len(one.segments) == len(offs) - len(got) + len(stacked)


# -- the chunk table ------------------------------------------------------------------------------
def _check_table(segs, n):
    from torch_scae_amd import _lib
    from torch_scae_amd.data_parallel import norm_chunk_table
    CH, GC = _lib.NORM_CHUNK, _lib.NORM_GROUP_CHUNKS
    chunks, group_first, seg_first = norm_chunk_table(segs, n)
    cover = np.zeros(n, dtype=np.int64)
    owner = np.full(n, -1, dtype=np.int64)
    for s, (off, length) in enumerate(segs):
        owner[off:off + length] = s
    assert len(seg_first) == len(segs) + 1 and seg_first[0] == 0 and seg_first[-1] == len(chunks)
    for s in range(len(segs)):
        assert seg_first[s] < seg_first[s + 1]
        for b, length in chunks[seg_first[s]:seg_first[s + 1]]:
            assert 1 <= length <= CH
            cover[b:b + length] += 1
            assert (owner[b:b + length] == s).all()      # no chunk crosses its segment
    assert (cover[owner >= 0] == 1).all() and (cover[owner < 0] == 0).all()
    assert [b for b, _ in chunks] == sorted(b for b, _ in chunks)
    assert group_first[0] == 0 and group_first[-1] == len(chunks)
    for a, b in zip(group_first, group_first[1:]):
        assert 1 <= b - a <= GC
        assert b - a == 1 or sum(length for _, length in chunks[a:b]) <= 4 * CH
    return chunks, group_first


def test_chunk_table_around_the_chunk_size():
    from torch_scae_amd import _lib
    CH = _lib.NORM_CHUNK
    assert _lib.load().scae_segment_norms_chunk() == CH
    lengths = [1, 2, 3, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 1, 3 * CH + 7, 1, 1]
    segs, off = [], 3
    for i, length in enumerate(lengths):
        segs.append((off, length))
        off += length + (i % 3)          # gaps of 0, 1, 2 elements
    chunks, group_first = _check_table(segs, off + 5)
    assert len(chunks) == sum(-(-length // CH) for length in lengths)
    assert len(group_first) - 1 < len(chunks)            # small chunks share workgroups
    _check_table([(0, 1)], 1)
    _check_table([(0, 40 * CH)], 40 * CH)
    _check_table([(i, 1) for i in range(0, 200, 2)], 200)


def test_chunk_table_refuses_bad_segments():
    from torch_scae_amd.data_parallel import norm_chunk_table
    for bad in ([(0, 0)], [(0, 4), (3, 2)], [(5, 2), (0, 2)], [(0, 11)], [(-1, 2)], []):
        with pytest.raises(ValueError):
            norm_chunk_table(bad, 10)


def test_chunk_table_of_the_cfg2_layout():
    """cfg-2's model on the host: ~2.4 M parameters; with the capsule split every element of
    every tracked parameter lies in exactly one chunk."""
    from torch_scae_amd import factory
    from torch_scae_amd.data_parallel import FlatParameters, norm_segments
    from tests.test_train_remainder_gpu import CFG2
    torch.manual_seed(0)
    model = factory.make_scae(CFG2)
    flat = FlatParameters(model)
    names = {id(p): n for n, p in model.named_parameters()}
    seen = [not names[id(p)].startswith(("obj_decoder.dummy_vote", "posterior_classifier."))
            for p in flat.params]
    segs = norm_segments(flat, model, True, seen)
    assert len(segs) > len(flat.params)
    tracked = sum(p.numel() for p, s in zip(flat.params, seen) if s)
    assert sum(n for _, _, n in segs) == tracked
    _check_table([(off, n) for _, off, n in segs], flat.numel)


def test_launcher_refuses_bad_arguments():
    """Every call here is refused before a HIP call."""
    from torch_scae_amd import _lib
    lib = _lib.load()
    import ctypes
    P = ctypes.c_void_p
    fake = P(0x1000)
    ok = [fake, None, 100, fake, 3, fake, 2, fake, 2, 2, 1.0, fake, fake, None, 1, None]
    for i, v in ((0, None), (2, 0), (2, 1 << 31), (4, 0), (6, 0), (6, 4), (8, 0), (8, 4),
                 (9, 3), (10, -1.0), (10, math.nan), (11, None), (12, None), (14, 0),
                 (1, P(0x1004)), (3, P(0x1004))):
        args = list(ok)
        args[i] = v
        assert lib.scae_segment_norms_f32(*args) == -1, (i, v)


# -- a CPU step -----------------------------------------------------------------------------------
class Toy(nn.Module):
    """What TrainStep needs of a model, on the host: a linear layer, three capsules' stacked
    weights (a GroupedMLP's parameters, used through einsum: its own forward is a HIP kernel)
    and a parameter that never gets a gradient."""
    n_classes = None

    def __init__(self):
        super().__init__()
        from torch_scae_amd.nn_ext import GroupedMLP
        torch.manual_seed(0)
        self.body = nn.Linear(16, 4)
        self.caps = GroupedMLP(3, [4, 5])
        self.unused = nn.Parameter(torch.randn(3))

    def forward(self, image):
        h = torch.tanh(self.body(image.flatten(1)))
        out = torch.einsum("bi,goi->bgo", h, self.caps.stacked_weight_0) + self.caps.stacked_bias_0
        return dict(out=out)

    def loss(self, res, image, label):
        scale = torch.arange(1, 4, dtype=torch.float32).view(1, 3, 1)
        return (res["out"] ** 2 * scale).sum(), {}


def _batch(it):
    g = torch.Generator().manual_seed(50 + it)
    return torch.randn(4, 1, 4, 4, generator=g), torch.zeros(4, dtype=torch.long)


def _by_hand(model, grads, p, scale):
    """{key: fp64 norm} of per-key gradients {key: tensor} scaled by fp32(scale), and the total."""
    scale = float(np.float32(scale))
    out = {k: scale * float(torch.linalg.vector_norm(g.double().reshape(-1), p))
           for k, g in grads.items() if g is not None}
    total = float(torch.linalg.vector_norm(torch.tensor(list(out.values()),
                                                        dtype=torch.float64), p))
    return out, total


@pytest.mark.parametrize("p", [1, 2, "inf"])
@pytest.mark.parametrize("kind,clip", [("rmsprop", 0.0), ("adam", 0.0), ("rmsprop", 0.05)])
def test_cpu_step_rows_are_the_parameters_grad_norms(p, kind, clip):
    from torch_scae_amd import nn_ext
    from torch_scae_amd.train_step import TrainStep
    model = Toy()
    step = TrainStep(model, 4, (1, 4, 4), use_graph=False, optimizer=kind, lr=1e-2,
                     gradient_clip_val=clip, track_grad_norm=p)
    assert step.last_grad_norms() is None
    pf = float(p)
    for it in range(3):
        step(*_batch(it))
        ref, total = _by_hand(model, nn_ext.named_reference_grads(model), pf, 1.0)
        names = step.grad_norm_names()
        assert names[-1] == f"grad_{pf}_norm_total" and len(names) == len(ref) + 1
        assert not any("unused" in n for n in names)
        assert sum("caps." in n for n in names) == 6
        row = step.last_grad_norms().double()
        for n, v in zip(names[:-1], row):
            key = n[len(f"grad_{pf}_norm_"):]
            assert abs(float(v) - ref[key]) <= ULP * ref[key], (it, key)
        assert abs(float(row[-1]) - total) <= ULP * total
        if clip:
            assert total > clip
        if pf == 2.0:      # the clip's norm when clipping, else the tracked total
            assert abs(float(step.last_grad_norm()) - total) <= 2e-6 * total
        else:
            assert (step.last_grad_norm() is None) == (not clip)
        hist, steps = step.grad_norm_history()
        assert steps == [it] and float(hist[names[-1]][0]) == float(row[-1].float())
    w = step.parameter_norms(2)
    assert w.shape == row.shape
    sd = model.state_dict()
    key = step.grad_norms.segments[0][0]
    assert abs(float(w[0]) - float(sd[key].double().norm())) <= ULP * float(w[0])


def test_cpu_step_accumulating_writes_one_row_per_optimiser_step():
    """k = 2 over 5 batches and end_epoch(): rows for batches (0, 1), (2, 3) and the pending
    (4,), each of fp32(1/2) * (g_1 + g_2) -- the sum in fp32, as the accumulator holds it."""
    from torch_scae_amd import nn_ext
    from torch_scae_amd.train_step import TrainStep
    model = Toy()
    step = TrainStep(model, 4, (1, 4, 4), use_graph=False, optimizer="adam", lr=1e-2,
                     accumulate_grad_batches=2, track_grad_norm=2)
    rows, sums = [], None
    for it in range(5):
        step(*_batch(it))
        g = {k: v.clone() for k, v in nn_ext.named_reference_grads(model).items()
             if v is not None}
        sums = g if sums is None else {k: sums[k] + g[k] for k in g}
        if it % 2 == 1:
            assert step.optimizer_steps == step.grad_norms.count == (it + 1) // 2
            rows.append((step.last_grad_norms().clone(), sums))
            sums = None
        else:
            assert step.grad_norms.count == it // 2       # nothing written inside a group
    step.end_epoch()
    assert step.optimizer_steps == step.grad_norms.count == 3
    rows.append((step.last_grad_norms().clone(), sums))
    names = step.grad_norm_names()
    for row, grads in rows:
        ref, total = _by_hand(model, grads, 2.0, 0.5)
        for n, v in zip(names[:-1], row.double()):
            key = n[len("grad_2.0_norm_"):]
            assert abs(float(v) - ref[key]) <= ULP * ref[key], key
        assert abs(float(row[-1]) - total) <= ULP * total
