"""What TrainStep and EvalStep share: capturing a step into a HIP graph with the library's
record of its launches beside it, replaying either, and staging a batch into a step's buffers.

Ownership: a ``LaunchList`` is the only holder of a ``scae_launch_list_*`` handle (an owning C
pointer) and frees it once; a ``Captured`` is one captured form of a step and owns its list; a
step holds ``Captured`` objects, never a raw handle (``step._klist`` only reads it)."""
import ctypes

import torch
import torch.distributed as dist

from . import _lib
from .ops import _p, _stream


def graph_census(graph):
    """(work nodes, kernel nodes) of a captured ``torch.cuda.CUDAGraph``, or None for anything
    that cannot be verified (no ``raw_cuda_graph`` in this torch build, no HIP runtime handle,
    a HIP error).  Empty / WaitEvent / EventRecord nodes carry no work and are not counted:
    with every kernel node one of the list's launches, all recorded in order on the capturing
    stream, that order already holds the edges they stand for.  (EvalStep.graph_nodes[0] used
    to count them; no graph the tests capture holds any.)"""
    try:
        raw = ctypes.c_void_p(graph.raw_cuda_graph())
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_size_t(0)
        if hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) != 0:
            return None
        nodes = (ctypes.c_void_p * max(1, n.value))()
        if hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) != 0:
            return None
        kernels = other = 0
        for i in range(n.value):
            t = ctypes.c_int(-1)
            if hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t)) != 0:
                return None
            kernels += t.value == 0                  # hipGraphNodeTypeKernel
            other += t.value not in (0, 5, 6, 7)     # ... Empty, WaitEvent, EventRecord
        return kernels + other, kernels
    except Exception:
        return None


def adopts(census, size, want_list):
    """Whether a capture replays as its launch list of ``size`` launches: only when the graph
    holds exactly those -- ``size`` kernel nodes and no other work node.  A captured torch
    kernel (training_step's accuracy and log copies), a memset inside a launcher or a
    collective is a node the list does not have, and replaying the list would silently drop
    it; a graph that cannot be read (``census`` None) counts as a mismatch."""
    return bool(want_list) and census is not None and tuple(census) == (size, size)


class LaunchList:
    """The library's record of the kernel launches made on one stream between ``begin`` and
    ``end`` (include/scae_hip.h, launch lists: kernel, grid, block, LDS, argument bytes), which
    ``run`` re-issues with one hipLaunchKernel each.  False once freed, or when the library
    could not begin one."""

    def __init__(self, handle=None):
        self.handle = handle or None

    @classmethod
    def begin(cls, stream):
        """Bound to ``stream``: another step's (or an eager forward's) launches on other
        streams are not in it."""
        return cls(_lib.load().scae_launch_list_begin(ctypes.c_void_p(stream.cuda_stream)))

    def __bool__(self):
        return self.handle is not None

    def end(self):
        if self:
            _lib.load().scae_launch_list_end(self.handle)

    def size(self):
        return _lib.load().scae_launch_list_size(self.handle)

    def run(self, stream):
        if not self:
            raise _lib.ScaeHipError("this launch list has been freed")
        _lib.check(_lib.load().scae_launch_list_run(
            self.handle, ctypes.c_void_p(stream.cuda_stream)), "scae_launch_list_run")

    def free(self):
        handle, self.handle = self.handle, None
        if handle is not None:
            _lib.load().scae_launch_list_free(handle)

    def __del__(self):
        try:
            self.free()
        except Exception:      # (interpreter shutdown)
            pass


class Captured:
    """One captured form of a step: its graph (``graph_b``: the second one of a split training
    step), the launch list when the step replays as one (else None), the recorded C-ABI calls
    (``launches``: their ctypes arguments keep the buffers the list points into alive) and
    ``nodes`` = (work nodes, kernel nodes, recorded launches) when the graph was read."""

    def __init__(self):
        self.graph = self.graph_b = self.klist = self.launches = self.nodes = None

    @property
    def handle(self):
        """The list's raw handle (None without a list): to read it, never to free it."""
        return self.klist.handle if self.klist else None

    def replay(self, device):
        """On ``device``'s current stream: launch by launch (no per-replay graph cost on the
        device, one C call on the host) or as a graph replay."""
        if self.klist:
            self.klist.run(torch.cuda.current_stream(device))
        else:
            self.graph.replay()

    def drop(self):
        """Free the list and forget the graphs."""
        if self.klist is not None:
            self.klist.free()
        self.graph = self.graph_b = self.klist = self.launches = self.nodes = None


def forwarded(name):
    """A read-only property of a step: ``name`` of the captured form it holds in ``_cap``."""
    return property(lambda step: getattr(step._cap, name))


def capture_error_mode():
    """With a process group alive its watchdog thread polls HIP events at any time; under the
    default "global" capture mode such a poll during the capture is an error that aborts the
    process.  Then (and only then) the check is narrowed to the capturing thread."""
    return "thread_local" if dist.is_available() and dist.is_initialized() else "global"


def capture(stream, body, *, keep_graph, want_list, pool=None, census_always=False):
    """``body()`` captured on ``stream`` (the one its warm-ups ran on) -> a ``Captured``.
    ``keep_graph``: the captured hipGraph_t stays readable (``graph_census``; a torch without
    it replays graphs only); ``pool``: the memory pool of a graph that never replays at the
    same time; ``want_list``: take the launch list when ``adopts`` allows it; ``census_always``:
    read the graph's nodes also when the list is not wanted (``nodes[2]`` is -1 when no list
    could be begun).  A ``body`` that raises leaves nothing behind: the list is freed and the
    exception propagates."""
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=keep_graph)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    klist = LaunchList.begin(stream)
    try:
        with torch.cuda.graph(graph, pool=pool, stream=stream,
                              capture_error_mode=capture_error_mode()), \
                _lib.recorder() as launches:
            body()
        klist.end()
        cap = Captured()
        cap.graph, cap.launches = graph, launches
        recorded = klist.size() if klist else -1
        census = graph_census(graph) if census_always or (want_list and klist) else None
        if census is not None:
            cap.nodes = (*census, recorded)
        if klist and adopts(census, recorded, want_list):
            cap.klist = klist
        else:
            klist.free()
        return cap
    except BaseException:
        klist.free()
        raise


# -- staging a batch into a step's resident buffers ------------------------------------------
def is_direct(dst_image, dst_label, image, label, device):
    """The batch already lives on ``device`` in the resident buffers' layout."""
    return image.is_cuda and label.is_cuda \
        and image.dtype == dst_image.dtype and label.dtype == dst_label.dtype \
        and image.is_contiguous() and label.is_contiguous() \
        and image.shape == dst_image.shape and label.shape == dst_label.shape \
        and image.device == device == label.device


def refresh_prologue(plan, pro, image):
    """Noise + folding products for the next forward (no batch)."""
    if pro is not None:
        with plan.active():
            pro.launch(stream_ref=image)


def stage(plan, pro, dst_image, dst_label, image, label, device, stage_batch=False):
    """The batch into the resident buffers: one launch when it ``is_direct`` -- the prologue's
    when there is one, else (``stage_batch``) scae_stage_batch --, otherwise plain copies and
    a refresh of the prologue."""
    if is_direct(dst_image, dst_label, image, label, device):
        if pro is not None:
            with plan.active():
                pro.launch(dst_image, image, dst_label, label)
            return
        if stage_batch:
            _lib.call("scae_stage_batch", _p(dst_image), _p(image), image.numel(),
                      _p(dst_label), _p(label), label.numel(), _stream(image))
            return
    dst_image.copy_(image, non_blocking=True)
    dst_label.copy_(label, non_blocking=True)
    refresh_prologue(plan, pro, dst_image)


def stage_source(plan, pro, dst_image, dst_label, view, epoch, position, rank=None,
                 standalone=False):
    """The batch at ``position`` of ``epoch`` gathered from a device-resident dataset
    (data.DatasetView) into the resident buffers: the prologue's source mode, or
    (``standalone``, or no prologue) the view's own gather and a refresh of the prologue.
    That gather launches on the current stream of the dataset's device, which is the step's
    whenever the dataset lives where the step's buffers do -- the only arrangement in use."""
    if pro is not None and not standalone:
        with plan.active():
            pro.launch(dst_image, None, dst_label, source=view.desc(epoch, position, rank))
        return
    view.gather(dst_image.shape[0], epoch, image=dst_image, label=dst_label, rank=rank,
                position=position)
    refresh_prologue(plan, pro, dst_image)
