"""The kernel-form selectors of the C ABI (scae_gemm_desc.form, the dgrad_forms argument of
the convolution's backward pair) are the only levers: the environment variables that used to
pick a form are not read any more, and a selector outside its set is SCAE_ERR_BAD_ARG before
anything is launched.  Shapes: the smallest of test_x6_kernels_vs_fp64.py at which the forms
differ in their bits (asserted there)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p

# every variable the library once read, at the value that switched its default form off
OLD_KNOBS = {"SCAE_GEMM_KSPLIT": "0", "SCAE_K8_DGX": "1", "SCAE_K8_DGK": "0",
             "SCAE_FUSE_K1_K4_BWD": "0", "SCAE_ST_WAVE": "0", "SCAE_FUSE_TRUNK_LOGPROB": "0"}


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


def _gemm_pair(g, form=0):
    """the 1 x 1 attention convolution's backward at (B, HW, C, AP, gsz) = (64, 9, 128, 160, 32)
    -> (the two descriptors, their outputs, what keeps the operands alive)"""
    from torch_scae_amd import ops
    B, HW, C, AP, gsz = 64, 9, 128, 160, 32
    S, kper, slab = B // gsz, HW * gsz, AP * C + AP
    dy, w, x, gate = (torch.randn(*s, generator=g).cuda()
                      for s in ((B * HW, AP), (AP, C), (B * HW, C), (B * HW, C)))
    part = torch.full((S * slab,), 7.0, device="cuda")
    dx, raw = torch.full((B * HW * C,), 7.0, device="cuda"), torch.full((B * HW * C,), 7.0,
                                                                        device="cuda")
    dgrad = ops._gemm_desc(ops._p(dy), ops._p(w), ops._p(dx), 1, B * HW, C, AP, True, AP, 0,
                           False, C, 0, C, 0)
    dgrad.mask, dgrad.ldmask, dgrad.c_nomask = gate.data_ptr(), C, raw.data_ptr()
    wgrad = ops._gemm_desc(ops._p(dy), ops._p(x), ops._p(part), S, AP, C, kper, False, AP,
                           kper * AP, False, C, kper * C, C, slab, asum=ops._off(part, AP * C),
                           asum_b=slab)
    wgrad.form = dgrad.form = form
    return (wgrad, dgrad), (dx, raw, part), (dy, w, x, gate)


def _conv_pair(g, B, IH, IW, Ci, Co, s):
    """-> (the arguments of scae_conv3x3_bwd_pair_f32 up to stride, its outputs, the operands)"""
    from torch_scae_amd import _lib
    OH, OW = (IH - 3) // s + 1, (IW - 3) // s + 1
    x = torch.relu(torch.randn(B, IH, IW, Ci, generator=g)).cuda()
    wd = (torch.randn(Ci, 9, Co, generator=g) * 0.05).cuda()
    dpre = torch.randn(B, OH, OW, Co, generator=g).cuda()
    splits = _lib.load().scae_conv3x3_wgrad_splits(B, OH, OW, Ci, Co)
    din = torch.full((B, IH, IW, Ci), 7.0, device="cuda")
    part = torch.full((splits * (9 * Co * Ci + Co),), 7.0, device="cuda")
    args = (P(dpre.data_ptr()), P(wd.data_ptr()), P(x.data_ptr()), P(din.data_ptr()),
            P(part.data_ptr()), B, IH, IW, Ci, Co, s)
    return args, (din, part), (x, wd, dpre)


CONV_SHAPES = [(2, 10, 12, 256, 64, 2), (3, 9, 11, 128, 64, 2)]


def test_the_old_environment_variables_do_nothing(monkeypatch):
    """scae_gemm_pair_f32 and scae_conv3x3_bwd_pair_f32 with all six old variables set to
    their non-default values: every output bit-equal to a run with none set."""
    from torch_scae_amd import _lib
    runs = {}
    for mode in ("unset", "set"):
        for k, v in OLD_KNOBS.items():
            if mode == "set":
                monkeypatch.setenv(k, v)
            else:
                monkeypatch.delenv(k, raising=False)
        g = torch.Generator().manual_seed(11)
        (wgrad, dgrad), outs, keep = _gemm_pair(g)
        _lib.call("scae_gemm_pair_f32", ctypes.byref(wgrad), ctypes.byref(dgrad), _st())
        for shape in CONV_SHAPES:
            args, o, k = _conv_pair(g, *shape)
            _lib.call("scae_conv3x3_bwd_pair_f32", *args, _st())
            outs, keep = outs + o, keep + k
        torch.cuda.synchronize()
        runs[mode] = outs
    assert len(runs["set"]) == 3 + 2 * len(CONV_SHAPES)
    for i, (a, b) in enumerate(zip(runs["unset"], runs["set"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i


def _rejected_without_a_launch(fn, *args):
    """rc of fn(*args, stream) and the number of launches a recording around it saw"""
    from torch_scae_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lst = lib.scae_launch_list_begin(_st())
    assert lst
    try:
        rc = getattr(lib, fn)(*args, _st())
        assert lib.scae_launch_list_end(P(lst)) == 0
        return rc, lib.scae_launch_list_size(P(lst))
    finally:
        lib.scae_launch_list_free(P(lst))


def test_a_gemm_form_outside_its_set_is_an_error_and_nothing_is_launched():
    from torch_scae_amd import _lib
    (wgrad, dgrad), outs, keep = _gemm_pair(torch.Generator().manual_seed(12), form=2)
    pair = (ctypes.byref(wgrad), ctypes.byref(dgrad))
    assert _rejected_without_a_launch("scae_gemm_pair_f32", *pair) == (_lib.ERR_BAD_ARG, 0)
    dgrad.form = _lib.GEMM_TILES            # one bad descriptor is enough
    assert _rejected_without_a_launch("scae_gemm_pair_f32", *pair) == (_lib.ERR_BAD_ARG, 0)
    descs = (_lib.GemmDesc * 2)(wgrad, dgrad)
    assert _rejected_without_a_launch("scae_gemm_multi_f32", descs, 2) == (_lib.ERR_BAD_ARG, 0)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)
    wgrad.form = _lib.GEMM_TILES            # the same arguments with a selector of the set
    assert _rejected_without_a_launch("scae_gemm_pair_f32", *pair) == (0, 1)


@pytest.mark.parametrize("forms", [5, 8], ids=["TILE|NO_TILE", "unknown bit"])
def test_dgrad_forms_outside_their_set_are_an_error_and_nothing_is_launched(forms):
    from torch_scae_amd import _lib
    assert forms in (_lib.DGRAD_TILE | _lib.DGRAD_NO_TILE, 8)
    assert 8 & (_lib.DGRAD_TILE | _lib.DGRAD_NO_TILE | _lib.DGRAD_NO_KSPLIT) == 0
    args, outs, keep = _conv_pair(torch.Generator().manual_seed(13), *CONV_SHAPES[1])
    assert _rejected_without_a_launch("scae_conv3x3_bwd_pair_forms_f32", *args, forms) == \
        (_lib.ERR_BAD_ARG, 0)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)
    assert _rejected_without_a_launch("scae_conv3x3_bwd_pair_forms_f32", *args,
                                      _lib.DGRAD_TILE) == (0, 1)
