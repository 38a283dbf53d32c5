"""K8r (csrc/conv_resident.hip) with the staged pixels held as three bf16 planes: the
staging splits every pixel once (bf16x6.h ``split3``), writes hi / mid / lo side by side per
8-channel unit, swizzled by a key of the pixel, and the main loop reads the planes back --
the eight waves of two column tiles from one staged image where Cout % 64 == 0.

What can go wrong there -- a lost or swapped plane, a unit at the wrong offset, a swizzle key
the staging and the fragment reads compute differently, a read past the images -- changes bits
of a result that must be an input value itself, so everything here is checked with
``torch.equal``: no tolerance.
"""
import ctypes

import pytest
import torch

from tests import x6_emulate as E

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else P(t.data_ptr())


def _lib():
    from torch_scae_amd import _lib
    return _lib


def _planes(w):
    """-> (wf, wp): the relayout's buffer (alive while wp is used) and its fragment-major planes."""
    L = _lib()
    Co, Ci = w.shape[:2]
    wf = torch.empty(L.load().scae_conv3x3_wf_floats(Co, Ci), device="cuda")
    wd = torch.empty(Ci, 9, Co, device="cuda")
    L.call("scae_conv3x3_relayout_f32", _p(w.contiguous().cuda()), _p(wf), _p(wd), Co, Ci, _st())
    return wf, P(wf.data_ptr() + 4 * Co * 9 * Ci)


def _inputs(g, B, IH, Ci):
    """full 24-bit mantissas (all three planes nonzero), mixed signs, and exact zeros."""
    x = E.full_mantissa(g, (B, IH, IH, Ci))
    x = torch.where(torch.rand(x.shape, generator=g) < 0.1, torch.zeros(()), x)
    hi, mid, lo = E.split3(x)
    live = x != 0
    assert bool(((hi != 0) & (mid != 0) & (lo != 0))[live].all()) and bool((x < 0).any())
    return x


def _run(xd, wp, bias, B, IH, Ci, Co, s, group, pbd=None):
    OH = (IH - 3) // s + 1
    out = torch.full((B, OH, OH, Co), float("nan"), device="cuda")
    outp = torch.full((B, OH, OH, Co), float("nan"), device="cuda") if pbd is not None else None
    _lib().call("scae_conv3x3_fwd_res_f32", _p(xd), wp, _p(bias), _p(out), _p(pbd), _p(outp),
                B, IH, IH, Ci, Co, s, group, _st())
    torch.cuda.synchronize()
    return out, outp


SHAPES = [
    (3, 9, 128, 128, 1, 0),    # MI = 2, the encoder's third layer (two column tiles a workgroup)
    (3, 7, 128, 128, 1, 0),    # MI = 1, NS = 3: its fourth
    (5, 7, 128, 64, 1, 2),     # ragged last group: its second image lies past the batch
    (2, 9, 256, 256, 2, 1),    # stride 2, two channel blocks per wave and tap
    (3, 7, 128, 96, 1, 0),     # Cout % 64 != 0: one column tile a workgroup, four waves
]


@pytest.mark.parametrize("B,IH,Ci,Co,s,group", SHAPES)
def test_one_hot_filter_returns_the_input_pixels_bitwise(B, IH, Ci, Co, s, group):
    """For each of the nine taps a filter that is 1.0 (and -1.0) at that tap from channel
    perm(co) and 0 elsewhere: out = relu(+-x) at the pixel under the tap -- every plane of every
    channel of every staged pixel comes back through hi + (mid + lo), bit for bit.  The last tap's
    run also checks the embedding-bias output as out + post_bias."""
    g = torch.Generator().manual_seed(B * 1000 + IH * 10 + Co)
    x = _inputs(g, B, IH, Ci)
    xd = x.cuda()
    OH = (IH - 3) // s + 1
    span = (OH - 1) * s + 1
    zero = torch.zeros(Co, device="cuda")
    pb = E.full_mantissa(g, (Co, OH, OH), 4)
    pbd = pb.cuda()
    co = torch.arange(Co)
    seen = torch.zeros(Ci, dtype=torch.bool)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        ci = (co * 5 + 3 + 17 * tap) % Ci            # a fixed injection co -> ci, moved by the tap
        seen[ci] = True
        for sign in (1.0, -1.0):
            w = torch.zeros(Co, Ci, 3, 3)
            w[co, ci, kh, kw] = sign
            wf, wp = _planes(w)
            post = tap == 8 and sign > 0
            out, outp = _run(xd, wp, zero, B, IH, Ci, Co, s, group, pbd if post else None)
            want = torch.relu(sign * x[:, kh:kh + span:s, kw:kw + span:s, :][..., ci])
            assert torch.equal(out.cpu(), want), (tap, sign)
            if post:
                assert torch.equal(outp.cpu(), want + pb.permute(1, 2, 0)), tap
    assert Co < Ci or bool(seen.all())


def test_nothing_past_the_batch_reaches_a_result():
    """The ragged-group case with its input as the first B images of a buffer of B + G images
    whose tail is NaN: the last workgroup's second image lies in that tail and must be staged
    as zero planes, not read."""
    B, IH, Ci, Co, s, group = SHAPES[2]
    g = torch.Generator().manual_seed(77)
    x = _inputs(g, B, IH, Ci)
    w = E.full_mantissa(g, (Co, Ci, 3, 3), 2)
    bias = E.full_mantissa(g, (Co,), 2).cuda()
    wf, wp = _planes(w)
    big = torch.full((B + group, IH, IH, Ci), float("nan"), device="cuda")
    big[:B] = x.cuda()
    exact, _ = _run(x.cuda(), wp, bias, B, IH, Ci, Co, s, group)
    tail, _ = _run(big, wp, bias, B, IH, Ci, Co, s, group)
    assert bool(torch.isfinite(tail).all())
    assert torch.equal(tail, exact)
    assert bool((exact > 0).any())


def test_plan_counts_the_planes():
    """Two workgroups per CU stay resident: at most 80 KiB of planes (6 bytes per element)
    per workgroup when the launcher chooses the group."""
    lib = _lib().load()
    ok = lib.scae_conv3x3_fwd_res_supported
    assert ok(128, 9, 9, 128, 128, 1) == 1
    assert ok(128, 7, 7, 128, 128, 1) == 1
    assert ok(256, 7, 7, 128, 128, 1) == 1
    assert ok(128, 19, 19, 128, 128, 2) == 0     # 277 KB of planes
    assert ok(128, 7, 7, 64, 128, 1) == 0        # Cin % 128
    assert ok(128, 7, 7, 128, 48, 1) == 0        # Cout % 32
    assert ok(128, 11, 11, 128, 128, 1) == 0     # 90.75 KiB of planes (its fp32 image was 60.5)
