"""The object encoder's backward in one launch (csrc/seed_bwd_gemm.hip,
``scae_object_encoder_bwd_gemm_*``): the output attention's backward, the
trunk's backward of the same set behind it in the same workgroup, and the
capsule MLPs' weight-gradient GEMM tiles as the tail of the grid.

Same kernels' bodies on the same inputs, the gradient handed over in registers
instead of through memory: everything is held to the launches it replaces BIT
FOR BIT -- at the C ABI on the smallest shapes that take every path (both trunk
tile counts, a tile with one valid row, no / one / several blocks, LayerNorm
on / off, presence absent / with exact zeros, null segment gradients, narrow and
wide inputs, both precisions), and in a training step (``RIDES['trunk_bwd']``).
"""
import ctypes

import pytest
import torch

D = 16
WIDE = (6, 1, 16, 121)          # cfg-2's four input segments


def test_predicate_on_the_host():
    """One set per workgroup (B <= 512), N and O within two tiles, the trunk
    without fc2: decided on the host, no device needed."""
    from torch_scae_amd import _lib
    ok = _lib.load().scae_object_encoder_bwd_supported
    # (B, N, O, C, D, Din, Dout, L, layer_norm)
    assert ok(128, 24, 24, 256, 16, 144, 0, 3, 1)
    assert ok(512, 24, 24, 256, 16, 144, 0, 3, 1)
    assert ok(256, 32, 32, 256, 16, 144, 0, 3, 1)
    assert ok(1, 1, 1, 64, 16, 7, 0, 0, 0)
    assert not ok(513, 24, 24, 256, 16, 144, 0, 3, 1)
    assert not ok(128, 33, 24, 256, 16, 144, 0, 3, 1)
    assert not ok(128, 24, 33, 256, 16, 144, 0, 3, 1)
    assert not ok(128, 24, 24, 256, 16, 144, 16, 3, 1)     # Dout > 0
    assert not ok(128, 24, 24, 256, 8, 144, 0, 3, 1)       # D != 16: no wave kernels
    assert not ok(128, 24, 24, 200, 16, 144, 0, 3, 1)      # C not a multiple of 64
    assert not ok(0, 24, 24, 256, 16, 144, 0, 3, 1)


# (B, N, O, L, layer_norm, presence, segment widths, gradient flags, C)
CASES = [
    (1, 1, 1, 0, 1, False, (7,), (True,), 64),
    (3, 15, 16, 1, 1, True, WIDE, (True, False, True, True), 256),
    (5, 16, 17, 3, 0, True, WIDE, (False, True, False, True), 64),
    (3, 17, 24, 3, 1, True, WIDE, (True, True, True, True), 256),
    (5, 24, 24, 3, 1, True, WIDE, (True, False, True, True), 256),
    (1, 32, 32, 1, 0, False, WIDE, (False, False, False, False), 64),
    (3, 32, 1, 0, 1, True, (7,), (False,), 256),
    (5, 1, 32, 3, 1, True, (7,), (True,), 64),
    (3, 24, 17, 1, 0, False, WIDE, (True, True, False, False), 64),
    (5, 17, 16, 0, 0, True, WIDE, (False, False, True, True), 256),
]


def _problem(case, bf16):
    """Inputs of one case on the device; the trunk's forward has run (hsave, z)."""
    from torch_scae_amd import _lib, ops
    B, N, O, L, ln, with_presence, widths, flags, C = case
    g = torch.Generator().manual_seed(1000 * B + 10 * N + O + L)
    rnd = lambda *shape: torch.randn(*shape, generator=g).cuda()  # noqa: E731
    lib = _lib.load()
    Din = sum(widths)
    segs = [rnd(B, N, w) for w in widths]
    params = rnd(lib.scae_set_encoder_param_count(D, Din, 0, L, ln)) * 0.1
    presence = None
    if with_presence:
        presence = torch.rand(B, N, generator=g)
        presence[torch.rand(B, N, generator=g) < 0.25] = 0.0   # exact zeros
        presence = presence.cuda()
    z = torch.empty(B, N, D, device="cuda")
    hsave = torch.empty(B, L + 1, N, D, device="cuda")
    seg_args = ops._seg_arrays(segs)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sfx = "bf16" if bf16 else "f32"
    _lib.call("scae_set_encoder_fwd_" + sfx, len(segs), *seg_args,
              ops._p(presence), ops._p(params), ops._p(z), ops._p(hsave), B, N,
              D, Din, 0, L, ln, st)
    q, wk, wv = rnd(O, C) / C ** .5, rnd(C, D) * .3, rnd(C, D) * .3
    gout = rnd(B, O, C)
    # four weight-gradient problems gW[g] (n x k) = gpre[g]^T x[g] over G groups
    G, rows = 3, 37
    gemms = [(rnd(G, rows, n), rnd(G, rows, k), n, k)
             for n, k in ((32, 48), (50, 33), (16, 20), (40, 17))]
    return dict(segs=segs, seg_args=seg_args, params=params, presence=presence,
                z=z, hsave=hsave, q=q, wk=wk, wv=wv, gout=gout, gemms=gemms,
                G=G, rows=rows, Din=Din, st=st, sfx=sfx)


def _run(case, p, merged):
    from torch_scae_amd import _lib, ops
    B, N, O, L, ln, _, widths, flags, C = case
    lib = _lib.load()
    # (a sentinel, not NaN: what neither form writes compares equal)
    new = lambda *shape: torch.full(shape, 7.0, device="cuda")  # noqa: E731
    gh = new(B, N, D)
    apart = new(lib.scae_seed_attention_mfma_rows(B), O * D + C * D + C)
    gws = [new(p["G"], n, k) for _, _, n, k in p["gemms"]]
    tpart = new(lib.scae_set_encoder_grid(B), p["params"].numel())
    gsegs = [new(B, N, w) if f else None for w, f in zip(widths, flags)]
    gptrs = (ctypes.c_void_p * len(widths))(
        *[None if t is None else t.data_ptr() for t in gsegs])
    descs = (_lib.GemmDesc * len(gws))()
    G, rows = p["G"], p["rows"]
    for i, ((gpre, x, n, k), gw) in enumerate(zip(p["gemms"], gws)):
        descs[i] = ops._gemm_desc(ops._p(gpre), ops._p(x), ops._p(gw), G, n, k,
                                  rows, False, n, rows * n, False, k, rows * k,
                                  k, n * k)
    att = (ops._p(p["z"]), ops._p(p["q"]), ops._p(p["wk"]), ops._p(p["wv"]),
           ops._p(p["presence"]), ops._p(p["gout"]), ops._p(gh), ops._p(apart),
           B, N, O, C, descs, len(gws))
    trunk = (len(widths), *p["seg_args"], gptrs, ops._p(p["presence"]),
             ops._p(p["params"]), ops._p(p["hsave"]))
    dims = (B, N, D, p["Din"], 0, L, ln)
    if merged:
        _lib.call("scae_object_encoder_bwd_gemm_" + p["sfx"], *att, *trunk,
                  ops._p(tpart), *dims, p["st"])
    else:
        _lib.call("scae_seed_attention_mfma_bwd_gemm_" + p["sfx"], *att, p["st"])
        _lib.call("scae_set_encoder_bwd_" + p["sfx"], *trunk, ops._p(gh),
                  ops._p(tpart), *dims, p["st"])
    torch.cuda.synchronize()
    named = [("gh", gh), ("attention partial", apart), ("trunk partial", tpart)]
    named += [("gW%d" % i, t) for i, t in enumerate(gws)]
    named += [("gseg%d" % i, t) for i, t in enumerate(gsegs) if t is not None]
    return named


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-N%d-O%d-L%d" % c[:4])
def test_one_launch_equals_the_two_it_replaces_bitwise(case, bf16):
    from torch_scae_amd import _lib
    B, N, O, L, ln, _, widths, _, C = case
    assert _lib.load().scae_object_encoder_bwd_supported(
        B, N, O, C, D, sum(widths), 0, L, ln)
    p = _problem(case, bf16)
    two, one = _run(case, p, False), _run(case, p, True)
    assert [n for n, _ in two] == [n for n, _ in one]
    for (name, a), (_, b) in zip(two, one):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    # ... and it computed something: the gradient of a wanted segment is not
    # the sentinel, the trunk's partial rows are not all zero
    assert float(dict(two)["trunk partial"].abs().max()) > 0
    for name, t in two:
        if name.startswith("gseg"):
            assert not bool((t == 7.0).all()), name


@pytest.mark.gpu
def test_shapes_outside_the_predicate_launch_nothing():
    """N = 40 (hydra's 40 / 32) keeps its two launches: the launcher declines."""
    from torch_scae_amd import _lib, ops
    case = (2, 24, 24, 1, 1, True, WIDE, (True,) * 4, 64)
    p = _problem(case, False)
    lib = _lib.load()
    assert not lib.scae_object_encoder_bwd_supported(2, 40, 32, 64, D, 144, 0, 1, 1)
    B, N, O, L, ln, _, widths, flags, C = case
    descs = (_lib.GemmDesc * 1)()
    gpre, x, n, k = p["gemms"][0]
    gw = torch.empty(p["G"], n, k, device="cuda")
    descs[0] = ops._gemm_desc(ops._p(gpre), ops._p(x), ops._p(gw), p["G"], n, k,
                              p["rows"], False, n, p["rows"] * n, False, k,
                              p["rows"] * k, k, n * k)
    gh = torch.zeros(B, N, D, device="cuda")
    apart = torch.zeros(B, O * D + C * D + C, device="cuda")
    tpart = torch.zeros(B, p["params"].numel(), device="cuda")
    gptrs = (ctypes.c_void_p * 4)(None, None, None, None)
    # the trunk with fc2 (Dout = 16): ERR_UNSUPPORTED, nothing written
    rc = lib.scae_object_encoder_bwd_gemm_f32(
        ops._p(p["z"]), ops._p(p["q"]), ops._p(p["wk"]), ops._p(p["wv"]),
        ops._p(p["presence"]), ops._p(p["gout"]), ops._p(gh), ops._p(apart), B, N,
        O, C, descs, 1, 4, *p["seg_args"], gptrs, ops._p(p["presence"]),
        ops._p(p["params"]), ops._p(p["hsave"]), ops._p(tpart), B, N, D, 144, 16,
        L, ln, p["st"])
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED
    assert float(gh.abs().max()) == 0 and float(tpart.abs().max()) == 0


# --------------------------------------------------------------------------
# In a training step: RIDES['trunk_bwd']
# --------------------------------------------------------------------------
def _small_step(carry, use_graph):
    from tests.test_hip_model import full_size_params
    from tests.test_timed_path import build_step
    cfg, _, sd, g = full_size_params("cfg2")
    B = 8
    model, step = build_step(cfg, B, sd, use_graph=use_graph)
    step.plan.carry_trunk_bwd = carry
    images = torch.rand(3, B, *cfg["image_shape"], generator=g).cuda()
    labels = torch.randint(0, 10, (3, B), generator=g).cuda()
    return step, images, labels


def _names(launches):
    return [getattr(fn, "__name__", "?") for fn, _, _ in launches]


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "replayed"])
def test_carried_trunk_backward_changes_nothing_in_a_training_step(use_graph):
    """cfg-2's model at B = 8, two steps from one seed, one of them with
    ``plan.carry_trunk_bwd = False``: after three steps loss, every parameter
    and every gradient agree bit for bit, and the carried step has one launch
    fewer -- the merged one instead of the attention's and the trunk's."""
    from torch_scae_amd import _lib
    from tests.test_timed_path import _set_counter
    out, names = {}, {}
    for carry in (True, False):
        step, images, labels = _small_step(carry, use_graph)
        if use_graph:
            step.capture()
            names[carry] = _names(step._launches)
        else:
            step._fwd_bwd()       # establishes the prologue's buffers
        _set_counter(step, 1000)
        losses = []
        for i in range(3):
            if use_graph:
                losses.append(float(step(images[i], labels[i])))
            else:
                with _lib.recorder() as launches:
                    losses.append(float(step(images[i], labels[i])))
                names[carry] = _names(launches)
        torch.cuda.synchronize()
        out[carry] = (losses, step.flat.flat_param.clone(),
                      step.flat.flat_grad.clone())
    merged = "scae_object_encoder_bwd_gemm_f32"
    assert merged in names[True], names[True]
    assert "scae_set_encoder_bwd_f32" not in names[True]
    assert "scae_seed_attention_mfma_bwd_gemm_f32" not in names[True]
    assert merged not in names[False]
    assert "scae_set_encoder_bwd_f32" in names[False]
    assert "scae_seed_attention_mfma_bwd_gemm_f32" in names[False]
    assert len(names[True]) == len(names[False]) - 1, (names[True], names[False])
    (l1, p1, g1), (l0, p0, g0) = out[True], out[False]
    assert l1 == l0, (l1, l0)
    assert torch.equal(p1, p0) and torch.equal(g1, g0)
    assert float(g0.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("second_consumer", [False, True])
def test_trunk_output_with_a_second_consumer_keeps_the_two_launch_gradients(
        second_consumer):
    """The carried result is used only when autograd hands the attention's own
    ``gh`` on to the trunk.  With ``h.sum()`` added to the loss the trunk's
    gradient is a sum: the trunk launches again on it and overwrites the
    carried buffers -- the gradients of the two-launch path, bit for bit."""
    from torch_scae_amd import _lib, ops, step_plan
    B, N, O, C, L = 5, 24, 24, 64, 2
    g = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=g).cuda()  # noqa: E731
    lib = _lib.load()
    seg_vals = [rnd(B, N, w) for w in WIDE]
    packed0 = rnd(lib.scae_set_encoder_param_count(D, sum(WIDE), 0, L, 1)) * 0.1
    presence = torch.rand(B, N, generator=g).cuda()
    att0 = [rnd(O, C) / C ** .5, rnd(C, D) * .3, rnd(C), rnd(C, D) * .3, rnd(C)]
    weight = rnd(B, O, C)
    G, rows, n, k = 3, 37, 32, 48
    gpre, x = rnd(G, rows, n), rnd(G, rows, k)
    res = {}
    for carry in (True, False):
        plan = step_plan.StepPlan("test")
        plan.carry_trunk_bwd = carry
        segs = [t.clone().requires_grad_() for t in seg_vals]
        packed = packed0.clone().requires_grad_()
        att = [t.clone().requires_grad_() for t in att0]
        gw = torch.full((G, n, k), 7.0, device="cuda")
        descs = (_lib.GemmDesc * 1)()
        descs[0] = ops._gemm_desc(ops._p(gpre), ops._p(x), ops._p(gw), G, n, k,
                                  rows, False, n, rows * n, False, k, rows * k,
                                  k, n * k)
        with plan.active(), plan.fusing(weight):
            h = ops.set_encoder(segs, presence, packed, D, 0, L, True)
            out = ops.seed_attention(h, *att, presence)
            loss = (out * weight).sum()
            if second_consumer:
                loss = loss + h.sum()
            with plan.deferring(), _lib.recorder() as launches:
                # (what the capsule MLPs' backward leaves for the attention's)
                plan.park("wgrads", ops._PendingWeightGemms(descs, 1, (gpre, x),
                                                            gpre))
                loss.backward()
        torch.cuda.synchronize()
        names = _names(launches)
        if carry:
            assert "scae_object_encoder_bwd_gemm_f32" in names, names
            # a second consumer: the trunk's own launch follows on the sum
            assert ("scae_set_encoder_bwd_f32" in names) == second_consumer, names
        else:
            assert "scae_object_encoder_bwd_gemm_f32" not in names, names
            assert "scae_set_encoder_bwd_f32" in names, names
        res[carry] = [t.grad.clone() for t in segs + [packed] + att] + [gw]
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    assert all(float(t.abs().max()) > 0 for t in res[False][:5])
    assert not bool((res[True][-1] == 7.0).all())
