"""Eval-mode BatchNorm (+ residual, + ReLU) folded into the epilogues of the fp32 forward convolutions (config.fold_eval_bn,
diga_conv2d_nhwc_f32_infer / diga_conv2d_winograd_f32_infer, include/diga_hip.h: diga_infer_epilogue_t).

The unfused eval path computes, per element, o = fmaf(y, a[c], b[c]); o += skip; o = fmaxf(o, 0) on the fp32 value the conv stored
(norm.hip, affine_apply_kernel); the epilogue applies the same expressions to the same accumulator value, so every comparison against
the path that exists without the fold is torch.equal, not a tolerance.  Each kernel-level case is additionally held to float64 at the
bounds tests/test_gpu_conv.py and conftest.WINO_TOL use for the convolution in front, so that two equally wrong results cannot pass:
with e_conv <= tol * max|conv| the error of fma(y, a, b) (+ skip, ReLU: 1-Lipschitz) is <= max|a| * e_conv plus the fp32 rounding
of the two or three operations behind it (<= 3 * 2^-24 of the largest intermediate, taken as 1e-6 of the output scale + 1e-5 relative).

Inputs come from local torch.Generators; torch's global RNG state is not touched.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import WINO_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5

# (with a residual?, with ReLU?)
FORMS = [(False, False), (False, True), (True, True)]
FORM_IDS = ["affine", "affine_relu", "affine_residual_relu"]


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """The models, blocks and references of this file are shared between its tests and dropped with it: the scratch buffers the
    library's host side grew meanwhile go back to the ones it held before, and the caching allocator returns what became free, so
    that the memory-accounting tests that run later in the same process start from pools this file has not shaped."""
    import gc
    from diga_amd import _lib
    saved = dict(_lib._workspaces)
    prev_math = _lib.get_conv_math()
    _lib.set_conv_math(0)                 # the fold is an fp32 feature: the cases below state the arithmetic they run in
    yield
    _lib.set_conv_math(prev_math)
    _block.cache_clear()
    _model.cache_clear()
    _lib._workspaces.clear()
    _lib._workspaces.update(saved)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _tag():
    from diga_amd import _lib
    return _lib.PROF_TAGS.index("conv_fwd")


def _bn_params(c, g):
    """gamma (a few negative), beta, running_mean, running_var -- none of them trivial."""
    gamma = 0.5 + torch.rand(c, generator=g)
    gamma[torch.randperm(c, generator=g)[: max(2, c // 8)]] *= -1.0
    beta = 0.3 * torch.randn(c, generator=g)
    mean = 0.2 * torch.randn(c, generator=g)
    var = 0.5 + 1.5 * torch.rand(c, generator=g)
    return tuple(t.to(DEV) for t in (gamma, beta, mean, var))


def _coefficients(bn):
    from diga_amd import _lib
    gamma, beta, mean, var = bn
    ab = torch.empty(2 * gamma.numel(), dtype=torch.float32, device=DEV)
    _lib.call("diga_bn_eval_coefficients", _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(ab), gamma.numel(), EPS,
              _lib.stream())
    return ab


def _bn_eval(y, bn, residual, relu):
    """diga_bn_fwd(training = 0) on y [..., C] (dense): the unfused path."""
    from diga_amd import _lib
    gamma, beta, mean, var = bn
    c = y.shape[-1]
    m = y.numel() // c
    out = torch.empty_like(y)
    sm, si = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    ws = torch.empty(_lib.lib.diga_norm_workspace_bytes(m, 1, c), dtype=torch.uint8, device=DEV)
    _lib.call("diga_bn_fwd", _lib.ptr(y), c, _lib.ptr(out), c, _lib.ptr(residual), c, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(mean),
              _lib.ptr(var), _lib.ptr(sm), _lib.ptr(si), None, m, c, 0, 1 if relu else 0, 0, None, 0.1, EPS, _lib.ptr(ws), ws.numel(),
              _lib.stream())
    return out


def _epilogue(ab, residual, relu, residual_ld=None):
    from diga_amd import _lib
    e = _lib.InferEpilogue()
    e.ab = _lib.ptr(ab)
    e.residual = _lib.ptr(residual)
    e.residual_ld = 0 if residual is None else (residual_ld or residual.shape[-1])
    e.relu = 1 if relu else 0
    return e


def _direct(x, w, bias, stride, pad, dil, epi=None, raw=False):
    """x [N,H,W,Cin], w [Cout,R,S,Cin] -> [N,Ho,Wo,Cout] on diga_conv2d_nhwc_f32 (epi None) / _infer.  raw: return the status code."""
    from diga_amd import _lib
    n, h, wd, cin = x.shape
    cout, r, s, _ = w.shape
    ho = (h + 2 * pad - dil * (r - 1) - 1) // stride + 1
    wo = (wd + 2 * pad - dil * (s - 1) - 1) // stride + 1
    out = torch.full((n, ho, wo, cout), float("nan"), dtype=torch.float32, device=DEV)
    args = [_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), n, h, wd, cin, cin, ho, wo, cout, cout, r, s, stride, stride, -pad, -pad,
            dil, dil]
    if epi is None:
        _lib.call("diga_conv2d_nhwc_f32", *args, None, _tag(), _lib.stream())
        return out
    if raw:
        return _lib.lib.diga_conv2d_nhwc_f32_infer(*args, ctypes.byref(epi), _tag(), _lib.stream()), out
    _lib.call("diga_conv2d_nhwc_f32_infer", *args, ctypes.byref(epi), _tag(), _lib.stream())
    return out


def _winograd(x, w, bias, d, tile, epi=None):
    from diga_amd import _lib
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    out = torch.full((n, h, wd, cout), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(_lib.lib.diga_conv2d_winograd_workspace_bytes(n, h, wd, cin, cout, d, tile), dtype=torch.uint8, device=DEV)
    head = [_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(ws), ws.numel(), n, h, wd, cin, cin, cout, cout, d, tile]
    if epi is None:
        _lib.call("diga_conv2d_winograd_f32", *head, 0, None, None, _tag(), _lib.stream())
    else:
        _lib.call("diga_conv2d_winograd_f32_infer", *head, ctypes.byref(epi), None, _tag(), _lib.stream())
    return out


def _conv_f64(x, w, bias, stride, pad, dil):
    """float64 convolution of NHWC x with [Cout,R,S,Cin] weights on the device (tap by tap: a matrix product per tap)."""
    n, h, wd, cin = x.shape
    cout, r, s, _ = w.shape
    ho = (h + 2 * pad - dil * (r - 1) - 1) // stride + 1
    wo = (wd + 2 * pad - dil * (s - 1) - 1) // stride + 1
    xp = torch.zeros((n, h + 2 * pad, wd + 2 * pad, cin), dtype=torch.float64, device=x.device)
    xp[:, pad:pad + h, pad:pad + wd] = x.double()
    out = torch.zeros((n, ho, wo, cout), dtype=torch.float64, device=x.device)
    for i in range(r):
        for j in range(s):
            sl = xp[:, i * dil: i * dil + (ho - 1) * stride + 1: stride, j * dil: j * dil + (wo - 1) * stride + 1: stride]
            out += sl @ w[:, i, j].double().t()
    return out if bias is None else out + bias.double()


def _check_forms(name, conv, y64, bn, residual, conv_tol):
    """conv(epi) runs the convolution: epi None = the plain entry point, else the `_infer` one.  All forms x {bias handled by caller}."""
    gamma, beta, mean, var = (t.double() for t in bn)
    a64 = gamma / torch.sqrt(var + EPS)
    b64 = beta - mean * a64
    ab = _coefficients(bn)
    raw = conv(None)
    assert not bool(torch.isnan(raw).any()), name
    e_conv = conv_tol * float(y64.abs().max()) * float(a64.abs().max())
    for (with_res, relu), fid in zip(FORMS, FORM_IDS):
        res = residual if with_res else None
        want = _bn_eval(raw, bn, res, relu)
        got = conv(_epilogue(ab, res, relu))
        assert torch.equal(got, want), (name, fid, int((got != want).sum()))
        ref = y64 * a64 + b64
        if with_res:
            ref = ref + res.double()
        if relu:
            ref = ref.clamp_min(0.0)
        err = (got.double() - ref).abs()
        bound = e_conv + 1e-6 * float(ref.abs().max()) + 1e-5 * ref.abs()
        worst = float((err - bound).max())
        print(f"{name} {fid}: max err {float(err.max()):.3g} (conv bound {e_conv:.3g})")
        assert worst <= 0.0, (name, fid, float(err.max()), e_conv)


def _inputs(seed, xshape, wshape):
    g = torch.Generator().manual_seed(seed)
    cout = wshape[0]
    fan = wshape[1] * wshape[2] * wshape[3]
    x = (torch.randn(xshape, generator=g) + 0.25).to(DEV)
    w = (torch.randn(wshape, generator=g) * (2.0 / fan) ** 0.5).to(DEV)
    bias = torch.randn(cout, generator=g).to(DEV)
    bn = _bn_params(cout, g)
    return g, x, w, bias, bn


# ---------------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("k", [32, 64])
def test_persistent_gemm_infer_epilogue(k, with_bias):
    """gemm_f32_persistent_kernel: M = 256 * 512 - 240 rows as one-pixel images (512 row tiles, the last one holds 16 rows)."""
    from diga_amd import _lib
    m, cout = 256 * 512 - 240, 128
    assert _lib.lib.diga_conv2d_stats_chunk_rows(m, 1, 1, k, 1, 1, cout, 1, 1, 1, 1, 0, 0, 0) == 64       # = the persistent kernel's shape rule
    g, x, w, bias, bn = _inputs(100 + k, (m, 1, 1, k), (cout, 1, 1, k))
    res = torch.randn((m, 1, 1, cout), generator=g).to(DEV)
    b = bias if with_bias else None
    _check_forms(f"persistent K{k}", lambda e: _direct(x, w, b, 1, 0, 1, e), _conv_f64(x, w, b, 1, 0, 1), bn, res, 1e-5)


# name, x shape (NHWC), weight shape, stride, pad, dilation
DIRECT = [
    ("dma_M777_K256_C256", (777, 1, 1, 256), (256, 1, 1, 256), 1, 0, 1),          # conv_fwd_dma_kernel, ragged last 256-row tile
    ("tn2_1x1s2_64_256", (2, 17, 19, 64), (256, 1, 1, 64), 2, 0, 1),              # conv_fwd_kernel<2>, stride 2
    ("tn1_3x3_64_64", (2, 13, 11, 64), (64, 3, 3, 64), 1, 1, 1),                  # conv_fwd_kernel<1>
    ("tn1_3x3_64_20", (2, 13, 11, 64), (20, 3, 3, 64), 1, 1, 1),                  # ... ragged column-quad group
]


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", DIRECT, ids=[c[0] for c in DIRECT])
def test_direct_kernels_infer_epilogue(case, with_bias):
    name, xs, wsh, stride, pad, dil = case
    g, x, w, bias, bn = _inputs(len(name) * 7 + wsh[0], xs, wsh)
    b = bias if with_bias else None
    y64 = _conv_f64(x, w, b, stride, pad, dil)
    res = torch.randn(tuple(y64.shape), generator=g).to(DEV)
    _check_forms(name, lambda e: _direct(x, w, b, stride, pad, dil, e), y64, bn, res, 1e-5)


WINO = [(tile, d, 64, 128) for tile in (4, 6) for d in (1, 2, 4)] + [(4, 2, 96, 160), (6, 1, 96, 160)]


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", WINO, ids=[f"tile{t}_d{d}_{ci}_{co}" for t, d, ci, co in WINO])
def test_winograd_output_transform_infer_epilogue(case, with_bias):
    tile, d, cin, cout = case
    g, x, w, bias, bn = _inputs(10 * tile + d + cin, (2, 33, 31, cin), (cout, 3, 3, cin))
    b = bias if with_bias else None
    y64 = _conv_f64(x, w, b, 1, d, d)
    res = torch.randn(tuple(y64.shape), generator=g).to(DEV)
    _check_forms(f"winograd tile {tile} d {d} {cin}->{cout}", lambda e: _winograd(x, w, b, d, tile, e), y64, bn, res, WINO_TOL[tile][0])


def test_stem_im2col_gemm_through_the_module():
    """The stem's im2col GEMM (3 -> 64, 7x7 / 2) through DigaConv2d(..., infer=) against conv module + eval-mode BatchNorm module."""
    from diga_amd import config
    from diga_amd.model import conv as dc
    from diga_amd.model import norm as dn
    g = torch.Generator().manual_seed(5)
    conv = dc.DigaConv2d(3, 64, 7, stride=2, padding=3, bias=False)
    bn = dn.DigaBatchNorm2d(64)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / 147) ** 0.5)
    _fill_bn(bn, g)
    for p in bn.parameters():
        p.requires_grad = False
    conv, bn = conv.to(DEV), bn.to(DEV).eval()
    x = torch.randn((2, 3, 37, 41), generator=g).to(DEV)
    with torch.no_grad():
        want = bn(conv(x), relu=True)
        assert not conv.folds_eval_bn(x, bn)                      # (the default configuration leaves the fold off)
        with config.override(fold_eval_bn=True):
            assert conv.folds_eval_bn(x, bn)
            dc.path_log = {}
            try:
                got = conv(x, infer=(bn, None, True))
                log = dc.path_log
            finally:
                dc.path_log = None
    assert log == {("fwd", "f32+bn"): 1}, log
    assert torch.equal(got, want)
    a = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    ref = torch.nn.functional.conv2d(x.double(), conv.weight.detach().double(), None, 2, 3)
    e_conv = 1e-5 * float(ref.abs().max()) * float(a.abs().max())
    ref = (ref * a[None, :, None, None] + (bn.bias.double() - bn.running_mean.double() * a)[None, :, None, None]).clamp_min(0.0)
    err = (got.double() - ref).abs()
    assert bool((err <= e_conv + 1e-6 * float(ref.abs().max()) + 1e-5 * ref.abs()).all()), float(err.max())


def test_argument_errors_return_a_code_and_launch_nothing():
    from diga_amd import _lib
    g, x, w, bias, bn = _inputs(3, (2, 9, 9, 64), (64, 1, 1, 64))
    ab = _coefficients(bn)
    res = torch.randn((2 * 9 * 9 * 64 + 4,), generator=g).to(DEV)
    ok = _epilogue(ab, res[:-4].view(2, 9, 9, 64), True)
    rc, out = _direct(x, w, None, 1, 0, 1, ok, raw=True)
    assert rc == 0 and not bool(torch.isnan(out).any())
    null_ab = _epilogue(None, None, True)
    misaligned = _epilogue(ab, res[1:-3].view(2, 9, 9, 64), True)            # 4 bytes off a 16-byte boundary
    assert res[1:].data_ptr() % 16 == 4
    for what, e, ww in (("null ab", null_ab, w), ("misaligned residual", misaligned, w), ("Cout % 4", ok, w[:18].contiguous())):
        rc, out = _direct(x, ww, None, 1, 0, 1, e, raw=True)
        assert rc == -1, (what, rc)                                           # DIGA_EINVAL
        assert _lib.last_error() != ""
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), what                             # nothing ran
    # Winograd: tile 2 has no inference epilogue, and the same descriptor checks
    xw = torch.randn((1, 12, 12, 64), generator=g).to(DEV)
    ww = torch.randn((128, 3, 3, 64), generator=g).to(DEV)
    ab128 = _coefficients(_bn_params(128, g))
    for tile, e in ((2, _epilogue(ab128, None, False)), (4, _epilogue(None, None, False))):
        with pytest.raises(RuntimeError, match="code -1"):
            _winograd(xw, ww, None, 1, tile, e)


# ---------------------------------------------------------------------------------------------------------------- module level
def _fill_bn(bn, g):
    with torch.no_grad():
        c = bn.num_features
        gamma = 0.5 + torch.rand(c, generator=g)
        gamma[torch.randperm(c, generator=g)[: max(2, c // 8)]] *= -1.0
        bn.weight.copy_(gamma)
        bn.bias.copy_(0.3 * torch.randn(c, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(c, generator=g))
        bn.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g))


def _fill(module, g):
    """Deterministic, non-trivial weights: He-scaled convolutions, BatchNorms as _fill_bn."""
    from diga_amd.model import norm as dn
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            with torch.no_grad():
                fan = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan) ** 0.5)
        elif isinstance(m, dn.DigaBatchNorm2d):
            _fill_bn(m, g)


# name, inplanes, planes, stride, dilation, downsample?, input N, H, W
BLOCKS = {
    "s1_plain": (256, 64, 1, 1, False, 2, 17, 19),
    "s2_down": (256, 128, 2, 1, True, 2, 17, 19),
    "d2_down": (512, 256, 1, 2, True, 1, 17, 19),
    "p512_33x31": (2048, 512, 1, 4, False, 1, 33, 31),
}


@functools.lru_cache(maxsize=None)
def _block(name):
    """(block in eval mode, input, unfused output): built once per shape and shared by the tests below, which leave it unchanged."""
    from diga_amd.model import conv as dc
    from diga_amd.model import seg_model_noaux as sm
    inpl, planes, stride, dil, down, n, h, w = BLOCKS[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    ds = None
    if down:
        ds = nn.Sequential(dc.DigaConv2d(inpl, planes * 4, 1, stride=stride, bias=False), sm._frozen_bn(planes * 4))
    blk = sm.Bottleneck(inpl, planes, stride, dilation=dil, downsample=ds)
    _fill(blk, g)
    blk = blk.to(DEV).eval()
    x = torch.randn((n, inpl, h, w), generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = blk(x)
    return blk, x, want


def _run(blk, x, fold, grad=False, **cfg):
    """(output, path_log) of blk(x) under config.override(fold_eval_bn=fold, **cfg)."""
    from diga_amd import config
    from diga_amd.model import conv as dc
    dc.path_log = {}
    try:
        with config.override(fold_eval_bn=fold, **cfg), torch.set_grad_enabled(grad):
            y = blk(x)
        return y.detach(), dc.path_log
    finally:
        dc.path_log = None


def _bn_entries(log):
    return {k: v for k, v in log.items() if k[1].endswith("+bn")}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_bottleneck_folded_equals_unfolded(name):
    blk, x, want = _block(name)
    off, log_off = _run(blk, x, False)
    on, log_on = _run(blk, x, True)
    assert torch.equal(off, want) and not _bn_entries(log_off)
    assert torch.equal(on, want), int((on != want).sum())
    sites = 4 if blk.downsample is not None else 3
    assert set(log_on) <= {("fwd", "f32+bn"), ("fwd", "winograd+bn")} and sum(log_on.values()) == sites, log_on
    planes = BLOCKS[name][1]
    assert (("fwd", "winograd+bn") in log_on) == (planes >= 128), log_on          # conv2 of the wide blocks runs through Winograd
    # a steady pass computes no coefficients: the cached tensor is the one the first folded pass made
    ab = blk.bn1.__dict__["_diga_eval_ab"][1]
    _run(blk, x, True)
    assert blk.bn1.__dict__["_diga_eval_ab"][1] is ab


def test_fallbacks_run_unfolded_and_bit_identical():
    import copy
    from diga_amd import _lib
    blk0, x, want = _block("s2_down")
    # grad enabled with an input that requires grad: nothing folds
    xg = x.clone().requires_grad_()
    y, log = _run(blk0, xg, True, grad=True)
    assert torch.equal(y, want) and not _bn_entries(log), log
    # Winograd capped at 2x2 tiles: conv2 keeps its BatchNorm, the other three sites fold
    y, log = _run(blk0, x, True, winograd_max_tile=2)
    y_off, _ = _run(blk0, x, False, winograd_max_tile=2)
    assert torch.equal(y, y_off) and log == {("fwd", "winograd"): 1, ("fwd", "f32+bn"): 3}, log
    # split-bf16 arithmetic: no layer folds
    prev = _lib.get_conv_math()
    try:
        _lib.set_conv_math(1)
        y, log = _run(blk0, x, True)
        y_off, _ = _run(blk0, x, False)
    finally:
        _lib.set_conv_math(prev)
    assert torch.equal(y, y_off) and not _bn_entries(log), log
    # a forward hook on bn1: that site stays two modules and the hook receives bn1's output
    blk = copy.deepcopy(blk0)
    seen = []
    handle = blk.bn1.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().clone()))
    y, log = _run(blk, x, True)
    assert torch.equal(y, want) and log == {("fwd", "f32"): 1, ("fwd", "f32+bn"): 2, ("fwd", "winograd+bn"): 1}, log
    y_off, _ = _run(blk, x, False)
    handle.remove()
    assert len(seen) == 2 and torch.equal(seen[0], seen[1]) and tuple(seen[0].shape) == (2, 128, 9, 10)
    # train mode: batch statistics, nothing folds (the copy's running statistics move; the shared block is left alone)
    blk.train()
    y, log = _run(blk, x, True)
    y_off, _ = _run(blk, x, False)
    assert torch.equal(y, y_off) and not _bn_entries(log), log


def test_coefficient_cache_follows_the_state_dict():
    import copy
    blk0, x, want = _block("s1_plain")
    blk = copy.deepcopy(blk0)
    y, _ = _run(blk, x, True)
    assert torch.equal(y, want)
    g = torch.Generator().manual_seed(99)
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g).to(DEV)
        elif k.endswith("running_var"):
            sd[k] = sd[k] * (0.5 + torch.rand(sd[k].shape, generator=g).to(DEV))
    blk.load_state_dict(sd)
    y_off, _ = _run(blk, x, False)
    y_on, log = _run(blk, x, True)
    assert not torch.equal(y_off, want)
    assert torch.equal(y_on, y_off) and sum(_bn_entries(log).values()) == 3
    # a train-mode pass in between updates the running statistics inside the kernel: the next folded pass follows
    blk.train()
    _run(blk, x, True)
    blk.eval()
    y_off, _ = _run(blk, x, False)
    y_on, _ = _run(blk, x, True)
    assert torch.equal(y_on, y_off)


# ---------------------------------------------------------------------------------------------------------------- model level
@functools.lru_cache(maxsize=None)
def _model(which):
    from diga_amd.model import seg_model_noaux as sm
    from diga_amd.model.model_noaux import SegModel
    from oracle import deeplab as od
    from oracle import detweights
    arch, oarch = (sm.TINY, od.TINY) if which == "tiny" else (sm.RESNET101, od.RESNET101)
    sd = detweights.state_dict(oarch)
    m = SegModel(arch=arch)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


@pytest.mark.parametrize("which,shape", [("tiny", (2, 3, 128, 192)), ("resnet101", (1, 3, 257, 385))], ids=["tiny", "resnet101"])
def test_segmodel_outputs_equal_fold_on_and_off(which, shape):
    from diga_amd import config
    from diga_amd.model import conv as dc
    m, _ = _model(which)
    x = (torch.rand(shape, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)
    with torch.no_grad():
        off = m(x)
        dc.path_log = {}
        try:
            with config.override(fold_eval_bn=True):
                on = m(x)
            log = dc.path_log
        finally:
            dc.path_log = None
    for a, b, what in zip(on, off, ("shallow", "deep", "out", "feat")):
        assert torch.equal(a, b), (which, what, int((a != b).sum()))
    folded = sum(_bn_entries(log).values())
    print(f"{which}: {log}")
    if which == "resnet101":
        assert folded == 1 + 3 * 33 + 4, log            # stem + 33 bottlenecks x 3 + 4 downsample branches: every trunk BatchNorm
    else:
        assert folded >= 1, log                         # (16-channel layers: Cout % 4 == 0 holds; Winograd needs >= 128 channels)


def test_offline_passes_fold_on_and_off_and_vs_oracle():
    from diga_amd import evaluate as ev
    from diga_amd.util.metrics import runningScore
    from oracle import deeplab as od
    from oracle import evaluate as oe
    from oracle import synth
    m, sd = _model("tiny")
    g = synth.gen(22)
    images = torch.rand((2, 3, 128, 192), generator=g) * 2 - 1
    labels = synth.block_labels(g, 2, 128, 192, block=16, ignore_frac=0.05)
    rs_on, rs_off = runningScore(19, verbose=False), runningScore(19, verbose=False)
    on = ev.evaluate_two_scale(m, images.to(DEV), labels.to(DEV), rs_on, want_pred=True, fold_bn=True)
    off = ev.evaluate_two_scale(m, images.to(DEV), labels.to(DEV), rs_off, want_pred=True, fold_bn=False)
    assert torch.equal(on, off)
    rs_on.get_scores(), rs_off.get_scores()
    assert np.array_equal(rs_on.confusion_matrix, rs_off.confusion_matrix) and rs_on.confusion_matrix.sum() > 0
    # ... and the folded pass against the CPU oracle, at the tolerance of tests/test_gpu_evaluate.py
    with torch.no_grad():
        want, want_hist, fused = oe.evaluate_two_scale(lambda x: od.forward(sd, x, od.TINY, training=False)[2], images, labels)
    top2 = fused.topk(2, dim=1)[0]
    safe = (top2[:, 0] - top2[:, 1]) > 1e-3 * float(fused.abs().max())
    assert float(safe.float().mean()) > 0.95
    assert bool((on.cpu() == want)[safe].all())
    diff = np.abs(rs_on.confusion_matrix - want_hist).sum() / want_hist.sum()
    assert diff < 2.5 * float((~safe).float().mean()) + 1e-9
    pl_on = ev.generate_pseudo_labels(m, images.to(DEV), fold_bn=True)
    pl_off = ev.generate_pseudo_labels(m, images.to(DEV), fold_bn=False)
    assert pl_on.dtype == torch.uint8 and torch.equal(pl_on, pl_off)
    c_on = ev.initial_centroids(m, [images.to(DEV)], epochs=1, fold_bn=True)
    c_off = ev.initial_centroids(m, [images.to(DEV)], epochs=1, fold_bn=False)
    assert torch.equal(c_on.objective_vectors, c_off.objective_vectors)
