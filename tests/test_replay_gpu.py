"""The captured forms of a step on the GPU (torch_scae_amd/replay.py): each form of an
accumulating TrainStep and its remainder step owns a launch list of its own, the census of
every captured graph equals the list, and dropped forms capture again."""
import pytest
import torch

from tests.test_hip_model import full_size_params
from tests.test_timed_path import build_step

pytestmark = pytest.mark.gpu


def _only_launches(nodes):
    work, kernels, recorded = nodes
    return work == kernels == recorded > 0


def test_every_captured_form_owns_its_launch_list():
    from torch_scae_amd import EvalStep, _lib
    cfg, B, sd, g = full_size_params("cfg2_bs32")
    images = torch.rand(5, B, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, cfg["n_classes"], (5, B), generator=g).cuda()
    model, step = build_step(cfg, B, sd, replay="launches", accumulate_grad_batches=2)
    rem = step.remainder_step(8)
    # the accumulate form, the update form, the remainder's accumulate form, the update form
    # again (a replay)
    for i, n in enumerate((B, B, 8, B)):
        step(images[i, :n], labels[i, :n])
    torch.cuda.synchronize()
    assert step._rem is rem and step._form == "update" and rem._form == "acc"
    handles = [step._klist, step._other_cap.handle, rem._klist]
    assert all(handles) and len(set(handles)) == 3, handles
    size = _lib.load().scae_launch_list_size
    for nodes, handle in zip((step.graph_nodes, step._other_cap.nodes, rem.graph_nodes), handles):
        assert _only_launches(nodes) and size(handle) == nodes[2], nodes
    step._drop_forms()
    assert not step._klist and step._other_cap is None
    assert step.graph is None and step.graph_nodes is None
    assert rem._klist == handles[2]               # (the remainder step keeps its own)
    # both forms capture again as lists, then the accumulate form's list replays: it is what
    # ran when the state the form writes (the gradient sum; the parameters) has changed
    lists = {}
    for i, form in ((4, "acc"), (0, "update"), (1, "acc")):
        acc, param = step.opt.acc.clone(), step.flat.flat_param.clone()
        step(images[i], labels[i])
        torch.cuda.synchronize()
        assert step._form == form and step._klist and _only_launches(step.graph_nodes)
        assert lists.setdefault(form, step._klist) == step._klist
        if form == "acc":
            assert not torch.equal(step.opt.acc, acc) and torch.equal(step.flat.flat_param, param)
        else:
            assert not torch.equal(step.flat.flat_param, param)
        assert bool(torch.isfinite(step.loss))
    assert lists["acc"] != lists["update"]
    ev = EvalStep(model, B, cfg["image_shape"], replay="launches")
    ev(images[0], labels[0])
    torch.cuda.synchronize()
    assert ev._klist and _only_launches(ev.graph_nodes), ev.graph_nodes
    assert size(ev._klist) == ev.graph_nodes[2]
