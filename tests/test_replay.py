"""torch_scae_amd/replay.py on the host: who frees a launch list and how often, when a capture
replays as its list, what a capture that raises leaves behind, and the nine clauses of
``is_direct`` -- against a stub of the library that counts begin / end / free / run per handle,
with the graph context stubbed (no device)."""
import contextlib
import gc
import types
from collections import Counter

import pytest
import torch

from torch_scae_amd import replay

STREAM = types.SimpleNamespace(cuda_stream=0x1000)


class StubLib:
    """scae_launch_list_* with the calls counted per handle; ``handles``: what successive
    ``begin``s return (0: the library could not begin a list)."""

    def __init__(self, handles=(101, 102, 103, 104), size=5):
        self.handles, self.sizes = list(handles), size
        self.calls = Counter()

    def scae_launch_list_begin(self, stream):
        h = self.handles.pop(0)
        self.calls["begin", h] += 1
        return h

    def scae_launch_list_end(self, h):
        self.calls["end", h] += 1
        return 0

    def scae_launch_list_size(self, h):
        return self.sizes

    def scae_launch_list_run(self, h, stream):
        self.calls["run", h] += 1
        return 0

    def scae_launch_list_free(self, h):
        self.calls["free", h] += 1

    def of(self, h):
        return {k: n for (k, hh), n in self.calls.items() if hh == h}


@pytest.fixture
def lib(monkeypatch):
    stub = StubLib()
    monkeypatch.setattr(replay._lib, "load", lambda: stub)
    return stub


class FakeGraph:
    def __init__(self, keep_graph=False):
        self.keep_graph, self.replays = keep_graph, 0

    def replay(self):
        self.replays += 1


@pytest.fixture
def no_device(monkeypatch):
    """torch.cuda.CUDAGraph / torch.cuda.graph / current_stream stubbed: a capture just runs
    its body."""
    monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", lambda g, **kw: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: STREAM)


# -- LaunchList ------------------------------------------------------------------------------
def test_free_twice_frees_once(lib):
    kl = replay.LaunchList.begin(STREAM)
    assert kl and kl.handle == 101
    kl.end()
    kl.run(STREAM)
    kl.free()
    assert not kl and kl.handle is None
    kl.free()
    del kl
    gc.collect()
    assert lib.of(101) == {"begin": 1, "end": 1, "run": 1, "free": 1}


def test_a_freed_list_does_not_run(lib):
    kl = replay.LaunchList.begin(STREAM)
    kl.free()
    with pytest.raises(replay._lib.ScaeHipError):
        kl.run(STREAM)
    assert "run" not in lib.of(101)


@pytest.mark.parametrize("falsy", [0, None])
def test_a_falsy_handle_is_never_ended_run_or_freed(lib, falsy):
    lib.handles = [falsy]
    kl = replay.LaunchList.begin(STREAM)
    assert not kl
    kl.end()
    with pytest.raises(replay._lib.ScaeHipError):
        kl.run(STREAM)
    kl.free()
    del kl
    gc.collect()
    assert lib.of(falsy) == {"begin": 1}


def test_del_frees_a_live_handle(lib):
    kl = replay.LaunchList.begin(STREAM)
    del kl
    gc.collect()
    assert lib.of(101) == {"begin": 1, "free": 1}


# -- Captured --------------------------------------------------------------------------------
def _captured(lib):
    cap = replay.Captured()
    cap.graph, cap.klist = FakeGraph(), replay.LaunchList.begin(STREAM)
    cap.launches, cap.nodes = [], (5, 5, 5)
    return cap


def test_drop_frees_the_list_once_and_forgets_everything(lib, no_device):
    cap = _captured(lib)
    assert cap.handle == 101
    graph = cap.graph
    cap.replay("cuda")
    assert lib.of(101)["run"] == 1 and graph.replays == 0
    cap.drop()
    cap.drop()
    assert cap.handle is None and not cap.klist
    assert (cap.graph, cap.graph_b, cap.launches, cap.nodes) == (None,) * 4
    del cap
    gc.collect()
    assert lib.of(101) == {"begin": 1, "run": 1, "free": 1}


def test_a_form_without_a_list_replays_its_graph(lib, no_device):
    cap = replay.Captured()
    cap.graph = FakeGraph()
    cap.replay("cuda")
    assert cap.graph.replays == 1 and not lib.calls


def test_swapped_forms_each_free_their_list_once(lib):
    """TrainStep._use_form: the two forms change places as whole objects."""
    step = types.SimpleNamespace(_cap=_captured(lib), _other_cap=_captured(lib))
    first, second = step._cap.handle, step._other_cap.handle
    assert (first, second) == (101, 102)
    for _ in range(3):
        step._cap, step._other_cap = step._other_cap, step._cap
    assert (step._cap.handle, step._other_cap.handle) == (second, first)
    step._cap.drop()
    step._other_cap.drop()
    del step
    gc.collect()
    assert lib.of(101) == lib.of(102) == {"begin": 1, "free": 1}


# -- the adopt / reject rule -------------------------------------------------------------------
N = 5
RULE = [((N, N), N, True, True),
        (None, N, True, False),            # a graph that could not be read
        ((N + 1, N), N, True, False),      # another work node
        ((N, N), N + 1, True, False),      # kernels != size
        ((N - 1, N - 1), N, True, False),
        ((N, N), N, False, False)]         # nobody asked for the list


@pytest.mark.parametrize("census,size,want_list,adopted", RULE)
def test_adopt_rule(census, size, want_list, adopted):
    assert replay.adopts(census, size, want_list) is adopted


@pytest.mark.parametrize("census,size,want_list,adopted", RULE)
def test_capture_adopts_or_frees_once(lib, no_device, monkeypatch, census, size, want_list,
                                      adopted):
    lib.sizes = size
    monkeypatch.setattr(replay, "graph_census", lambda graph: census)
    ran = []
    cap = replay.capture(STREAM, lambda: ran.append(1), keep_graph=True, want_list=want_list,
                         census_always=True)
    assert ran == [1] and isinstance(cap.graph, FakeGraph) and cap.launches == []
    assert cap.nodes == (None if census is None else (*census, size))
    if adopted:
        assert cap.handle == 101 and lib.of(101) == {"begin": 1, "end": 1}
        cap.drop()
    else:
        assert cap.klist is None and cap.handle is None
    del cap
    gc.collect()
    assert lib.of(101) == {"begin": 1, "end": 1, "free": 1}


def test_census_is_taken_only_when_asked_for(lib, no_device, monkeypatch):
    """The training step reads the graph only for a list it wants; the evaluation step always,
    with -1 recorded launches when no list could be begun."""
    seen = []
    monkeypatch.setattr(replay, "graph_census", lambda graph: seen.append(1) or (N, N))
    cap = replay.capture(STREAM, lambda: None, keep_graph=False, want_list=False)
    assert not seen and cap.nodes is None and cap.klist is None
    assert cap.graph.keep_graph is False
    lib.handles = [0]
    cap = replay.capture(STREAM, lambda: None, keep_graph=True, want_list=True,
                         census_always=True)
    assert seen == [1] and cap.nodes == (N, N, -1) and cap.klist is None
    assert lib.of(0) == {"begin": 1}


def test_a_body_that_raises_frees_the_list_and_propagates(lib, no_device, monkeypatch):
    monkeypatch.setattr(replay, "graph_census", lambda graph: (N, N))

    def body():
        raise ValueError("inside the capture")
    with pytest.raises(ValueError, match="inside the capture"):
        replay.capture(STREAM, body, keep_graph=True, want_list=True, census_always=True)
    gc.collect()
    assert lib.of(101) == {"begin": 1, "free": 1}
    assert replay._lib._RECORDER is None


# -- is_direct ---------------------------------------------------------------------------------
class OnDevice:
    """A CPU tensor that says it lives on a HIP device (``is_direct`` reads attributes only)."""

    def __init__(self, t, device="cuda:0"):
        self.t, self.is_cuda, self.device = t, True, torch.device(device)
        self.dtype, self.shape = t.dtype, t.shape

    def is_contiguous(self):
        return self.t.is_contiguous()


def test_is_direct_clause_by_clause():
    dev = torch.device("cuda:0")
    dst_image, dst_label = torch.zeros(4, 1, 6, 6), torch.zeros(4, dtype=torch.long)
    image, label = OnDevice(torch.rand(4, 1, 6, 6)), OnDevice(torch.zeros(4, dtype=torch.long))

    def direct(im=image, lb=label, device=dev):
        return bool(replay.is_direct(dst_image, dst_label, im, lb, device))
    assert direct()
    not_direct = {
        "image on the host": dict(im=torch.rand(4, 1, 6, 6)),
        "label on the host": dict(lb=torch.zeros(4, dtype=torch.long)),
        "image on meta": dict(im=torch.empty(4, 1, 6, 6, device="meta")),
        "image dtype": dict(im=OnDevice(torch.rand(4, 1, 6, 6).double())),
        "label dtype": dict(lb=OnDevice(torch.zeros(4, dtype=torch.int32))),
        "image strides": dict(im=OnDevice(torch.rand(4, 1, 6, 12)[..., ::2])),
        "label strides": dict(lb=OnDevice(torch.zeros(8, dtype=torch.long)[::2])),
        "image shape": dict(im=OnDevice(torch.rand(3, 1, 6, 6))),
        "label shape": dict(lb=OnDevice(torch.zeros(3, dtype=torch.long))),
        "image on another device": dict(im=OnDevice(torch.rand(4, 1, 6, 6), "cuda:1")),
        "label on another device": dict(lb=OnDevice(torch.zeros(4, dtype=torch.long), "cuda:1")),
        "step on another device": dict(device=torch.device("cuda:1")),
    }
    for what, kw in not_direct.items():
        assert not direct(**kw), what
    # (the strided cases have the buffers' shapes: only their layout differs)
    assert not_direct["image strides"]["im"].shape == dst_image.shape
    assert not_direct["label strides"]["lb"].shape == dst_label.shape
