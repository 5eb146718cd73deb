"""GPU tests of bf16x6 for multi-tap convolutions and the stem (config.x6_taps under conv_math = 2; csrc/conv_bf16x6.h: the TAPS
instantiations of conv_fwd_x6_kernel, conv_wgrad_x6_kernel<256, 128, true> with R * S > 1; model/conv.py: the "x6rs" family).

  1. forward / backward-data bit for bit against the POINTWISE kernel on the torch-built im2col of the same input;
  2. the weight gradient bit for bit, tap by tap, against the pointwise weight gradient on the tap-shifted input;
  3. the per-layer error table against float64, next to the direct fp32 kernels on the same inputs;
  4. a layer1-width bottleneck chain (statistics, fused backward epilogues, every gradient);
  5. the whole small model: no launch left on the fp32 matrix pipe, and the switch off = the switch absent;
  6. the inference fold;
  7. the switch changed between forward and backward.
`conv.path_log` is asserted everywhere: a layer that silently fell back to the fp32 kernels fails its test."""
import ctypes
import dataclasses

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from diga_amd import config

from conftest import assert_close
from oracle import deeplab as od
from oracle import detweights, synth
from test_gpu_conv import CASES
from test_gpu_conv_bf16x6 import FWD_TOL_F32, _block_state, _inputs, _make_block, _Mode

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _leave_global_rng_and_arithmetic_untouched():
    """As tests/test_gpu_conv_bf16x6.py: layer constructors draw from torch's global generators and later tests are sensitive to the
    draw, so every test hands the generators -- and the process-wide conv arithmetic -- back as it found them."""
    from diga_amd import _lib
    cpu, gpu = torch.get_rng_state(), (torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    math = _lib.get_conv_math()
    yield
    _lib.join_side()
    _lib.set_conv_math(math)
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max()) / float(ref.detach().abs().max())


def _tags():
    from diga_amd import _lib
    return _lib.PROF_TAGS.index("conv_fwd"), _lib.PROF_TAGS.index("conv_bwd_data")


# ------------------------------------------------------------------------------------------------ entry-point helpers
def _image(w):
    """diga_split_bf16x6_image of [K,R,S,C] weights (tap-major K-steps)."""
    from diga_amd import _lib
    k, r, s, c = w.shape
    img = torch.empty(_lib.lib.diga_split_bf16x6_image_bytes(k, r * s, c), dtype=torch.uint8, device=DEV)
    _lib.call("diga_split_bf16x6_image", _lib.ptr(w), _lib.ptr(img), k, r * s, c, _lib.stream())
    return img


def _im2col(x, r, s, stride, off0, doff, ho, wo):
    """x [N,Hi,Wi,C] -> [N,Ho,Wo,R*S,C]: tap (i, j) of output pixel (y, x) = input pixel (y * stride + off0 + i * doff, ...), exact
    zeros where that falls outside the image.  Copies only (torch.where), so every element is the input's bits or +0."""
    n, hi, wi, c = x.shape
    ys = torch.arange(ho, device=x.device) * stride[0] + off0[0]
    xs = torch.arange(wo, device=x.device) * stride[1] + off0[1]
    taps = []
    for i in range(r):
        iy = ys + i * doff[0]
        oky = (iy >= 0) & (iy < hi)
        for j in range(s):
            ix = xs + j * doff[1]
            okx = (ix >= 0) & (ix < wi)
            g = x[:, iy.clamp(0, hi - 1)][:, :, ix.clamp(0, wi - 1)]
            ok = (oky[:, None] & okx[None, :])[None, :, :, None]
            taps.append(torch.where(ok, g, torch.zeros((), device=x.device)))
    return torch.stack(taps, dim=3).contiguous()


def _conv_entry(name, x, w, bias, ho, wo, stride, off0, doff, tail, tag, stats=False):
    """One call of a forward entry point of the loader form: x [N,Hi,Wi,C] fp32, w [K,R,S,C].  -> (out, statistics or None)."""
    from diga_amd import _lib
    n, hi, wi, c = x.shape
    k, r, s, _ = w.shape
    out = torch.full((n, ho, wo, k), float("nan"), dtype=torch.float32, device=DEV)
    st = torch.zeros(_lib.lib.diga_conv2d_stats_floats(n, ho, wo, k), dtype=torch.float32, device=DEV) if stats else None
    img = _image(w)
    lead = [_lib.ptr(x), x.stride(2), _lib.ptr(img)] + ([] if name.endswith("_epi") else [_lib.ptr(bias)]) + [_lib.ptr(out)]
    _lib.call(name, *lead, n, hi, wi, c, ho, wo, k, k, r, s, stride[0], stride[1], off0[0], off0[1], doff[0], doff[1],
              tail if tail is not None else _lib.ptr(st), tag, _lib.stream())
    return out, st


# name, N, Cin, H, W, Cout, k, stride, pad, dilation, bias: the multi-tap rows of test_gpu_conv.CASES ...
TAP_NAMES = ["3x3_dil1", "3x3_dil2", "3x3_dil4", "aspp_dil12_bias", "aspp_dil24_bias", "bottleneck_1280", "wide_ragged_cout"]
TAP_CASES = [c for c in CASES if c[0] in TAP_NAMES]
assert [c[0] for c in TAP_CASES] == TAP_NAMES
# ... and the geometries they leave out: a strided 3x3 with ONE 32-channel chunk per tap, 49 taps, a 256-row tile that holds all of
# image 1 and parts of images 0 and 2 (3 x 99 pixels), and R = S = 1 through the new entry point
EXTRA_CASES = [("3x3_stride2_c32", 2, 32, 17, 19, 64, 3, 2, 1, 1, False),
               ("7x7_c32", 1, 32, 20, 20, 64, 7, 1, 3, 1, True),
               ("straddle_3_images", 3, 64, 11, 9, 128, 3, 1, 1, 1, False),
               ("1x1_new_entry", 2, 64, 13, 11, 96, 1, 1, 0, 1, True)]
FWD_CASES = TAP_CASES + EXTRA_CASES
_DATA = {}


def _data(case):
    """Seeded NHWC input, [K,R,S,C] weights, bias, output gradient and the float64 references of one case: built once, shared by
    tests 1 and 2, never modified."""
    name, n, cin, h, w, cout, k, stride, pad, dil, bias = case
    if name not in _DATA:
        x, wt, b, probe, yr, dxr, dwr, _ = _inputs(case)
        _DATA[name] = dict(x=x.permute(0, 2, 3, 1).contiguous().to(DEV), w=wt.permute(0, 2, 3, 1).contiguous().to(DEV),
                           b=None if b is None else b.to(DEV), dy=probe.permute(0, 2, 3, 1).contiguous().to(DEV),
                           yr=yr.permute(0, 2, 3, 1), dxr=dxr.permute(0, 2, 3, 1), dwr=dwr.permute(0, 2, 3, 1))
    return _DATA[name]


# ------------------------------------------------------------------------------------------------ 1. forward / backward-data
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c[0])
def test_forward_equals_pointwise_kernel_on_im2col(case):
    """diga_conv_taps_bf16x6_f32in against diga_conv2d_nhwc_bf16x6_f32in on the im2col rows [M][RS * Cin] (tap-major) with the weights
    reshaped to [K][1][RS * Cin]: the same weight image (asserted byte for byte), the same K-step sequence; a dead tap the new kernel
    skips only ever added exact zeros to an accumulator that starts at +0 -- so torch.equal, output and BatchNorm partial sums.  Any
    wrong offset, dilation, stride, padding or image boundary breaks it.  Also held to float64 at test_conv_fwd_bwd's 2e-6 of scale."""
    name, n, cin, h, w, cout, k, stride, pad, dil, bias = case
    d = _data(case)
    x, wt, b = d["x"], d["w"], d["b"]
    ho, wo = d["yr"].shape[1:3]
    fwd, _ = _tags()
    geom = ((stride, stride), (-pad, -pad), (dil, dil))
    cols = _im2col(x, k, k, *geom, ho, wo).reshape(n, ho, wo, k * k * cin)
    w1 = wt.reshape(cout, 1, 1, k * k * cin)
    assert torch.equal(_image(wt), _image(w1)), "the weight image of (K, RS, C) is that of (K, 1, RS * C)"
    got, st_got = _conv_entry("diga_conv_taps_bf16x6_f32in", x, wt, b, ho, wo, *geom, None, fwd, stats=True)
    want, st_want = _conv_entry("diga_conv2d_nhwc_bf16x6_f32in", cols, w1, b, ho, wo, (1, 1), (0, 0), (1, 1), None, fwd, stats=True)
    torch.cuda.synchronize()
    assert not torch.isnan(got).any()
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} outputs differ, worst {float((got - want).abs().max()):.3e}"
    assert torch.equal(st_got, st_want), f"{name}: statistics"
    assert_close(got, d["yr"], 1e-5, 2e-6 * float(d["yr"].abs().max()), f"{name} forward vs float64")


def _bwd_geometry(case):
    name, n, cin, h, w, cout, k, stride, pad, dil, bias = case
    return (1, 1), (pad, pad), (-dil, -dil)


BWD_CASES = [c for c in FWD_CASES if c[7] == 1]          # (strided multi-tap backward-data is not built)


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c[0])
def test_backward_data_equals_pointwise_kernel_on_im2col(case):
    """The backward-data geometry -- dy read at offsets +padding - i * dilation, the [C][R][S][K] transpose as weights -- the same way,
    plain and with the backward epilogue (residual-branch addend, ReLU mask of a BatchNorm with residual, BatchNorm-backward partial
    sums): torch.equal on dx and on the partial sums; the plain dx also against float64 at 3e-6 of scale."""
    from diga_amd import _lib
    name, n, cin, h, w, cout, k, stride, pad, dil, bias = case
    d = _data(case)
    dy, wt = d["dy"], d["w"]
    _, tag = _tags()
    wT = wt.permute(3, 1, 2, 0).contiguous()                                       # [C][R][S][K]
    geom = _bwd_geometry(case)
    cols = _im2col(dy, k, k, *geom, h, w).reshape(n, h, w, k * k * cout)
    w1 = wT.reshape(cin, 1, 1, k * k * cout)
    got, _ = _conv_entry("diga_conv_taps_bf16x6_f32in", dy, wT, None, h, w, *geom, None, tag)
    want, _ = _conv_entry("diga_conv2d_nhwc_bf16x6_f32in", cols, w1, None, h, w, (1, 1), (0, 0), (1, 1), None, tag)
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} gradients differ"
    assert_close(got, d["dxr"], 1e-5, 3e-6 * float(d["dxr"].abs().max()), f"{name} grad input vs float64")

    g = synth.gen(len(name) + 17)
    m = n * h * w
    addend = torch.randn((m, cin), generator=g).to(DEV)
    mask_y = torch.randn((m, cin), generator=g).to(DEV)
    xbn = torch.randn((m, cin), generator=g).to(DEV)
    mean, invstd = torch.randn(cin, generator=g).to(DEV), (torch.rand(cin, generator=g) + 0.5).to(DEV)

    def run(entry, inp, wgt, gm):
        part = torch.zeros(((m + 63) // 64) * 2 * cin, dtype=torch.float32, device=DEV)
        e = _lib.BwdEpilogue()
        e.addend, e.addend_ld = _lib.ptr(addend), cin
        e.mask_y, e.mask_ld = _lib.ptr(mask_y), cin
        e.x, e.x_ld = _lib.ptr(xbn), cin
        e.mean, e.invstd, e.partials = _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(part)
        out, _ = _conv_entry(entry, inp, wgt, None, h, w, *gm, ctypes.byref(e), tag)
        torch.cuda.synchronize()
        return out, part

    got_e, part_got = run("diga_conv_taps_bf16x6_f32in_epi", dy, wT, geom)
    want_e, part_want = run("diga_conv2d_nhwc_bf16x6_f32in_epi", cols, w1, ((1, 1), (0, 0), (1, 1)))
    assert torch.equal(got_e, want_e), f"{name}: epilogue dx"
    assert torch.equal(part_got, part_want), f"{name}: epilogue partial sums"
    ref = torch.where(mask_y.reshape(got.shape) > 0, got + addend.reshape(got.shape), torch.zeros((), device=DEV))
    assert_close(got_e, ref.cpu().double(), 1e-6, 1e-6 * float(ref.abs().max()), f"{name} epilogue vs its definition")


# ------------------------------------------------------------------------------------------------ 2. weight gradient
def _x6_splits(m, cout, cin, rs):
    """plan_wgrad_x6 (csrc/conv_bf16x6.h): (splits, K-steps per split, whether the 8-K-step floor decided)."""
    tiles = -(-cout // 256) * -(-cin // 128) * rs
    ksteps = -(-m // 32)
    want, floor = -(-512 // tiles), max(ksteps // 8, 1)
    per = -(-ksteps // min(want, floor, 512))
    return -(-ksteps // per), per, floor <= want


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c[0])
def test_weight_gradient_equals_pointwise_kernel_per_tap(case):
    """dw[:, tap, :] of diga_conv_taps_wgrad_bf16x6_f32in against diga_conv2d_wgrad_bf16x6_f32in on dy and the tap-shifted, zero-padded
    copy of x (column `tap` of the im2col), torch.equal.  Both calls cut the pixels into the same ranges: on these shapes the floor of 8
    K-steps (256 pixels) per block decides the split count with the taps counted among the tiles and without -- ceil(512 / tiles) is at
    least K-steps // 8 for tiles = channel tiles x RS <= 64 here (asserted below) -- so a tap's block sees the LDS bytes of the
    pointwise block, range by range, and the slabs are added in the same fixed order.  3x3_dil1 (4 ranges) and aspp_dil12_bias (8) have
    several ranges, the rest one.  Every shape is also held to float64 at test_conv_fwd_bwd's 3e-6 of scale."""
    from diga_amd import _lib
    name, n, cin, h, w, cout, k, stride, pad, dil, bias = case
    d = _data(case)
    x, dy = d["x"], d["dy"]
    ho, wo = dy.shape[1:3]
    m, rs = n * ho * wo, k * k
    s_taps, s_one = _x6_splits(m, cout, cin, rs), _x6_splits(m, cout, cin, 1)
    assert s_taps[2] and s_one[2] and s_taps[:2] == s_one[:2], (s_taps, s_one)
    if name in ("3x3_dil1", "aspp_dil12_bias"):
        assert s_taps[0] > 1
    q = _lib.lib.diga_conv_taps_wgrad_bf16x6_workspace_bytes(n, ho, wo, cout, cin, k, k)
    assert q > 0
    ws = torch.empty(q, dtype=torch.uint8, device=DEV)
    dw = torch.full((cout, k, k, cin), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("diga_conv_taps_wgrad_bf16x6_f32in", _lib.ptr(dy), cout, _lib.ptr(x), cin, _lib.ptr(dw), _lib.ptr(ws), ws.numel(), n, h, w, cin,
              ho, wo, cout, k, k, stride, stride, -pad, -pad, dil, dil, _lib.stream())
    cols = _im2col(x, k, k, (stride, stride), (-pad, -pad), (dil, dil), ho, wo)     # [N,Ho,Wo,RS,C]
    ws1 = torch.empty(_lib.lib.diga_conv2d_wgrad_bf16x6_workspace_bytes(n, ho, wo, cout, cin, 1, 1), dtype=torch.uint8, device=DEV)
    for tap in sorted({0, rs // 2, rs - 1, (rs * 2) // 3}) if rs > 9 else range(rs):
        xt = cols[:, :, :, tap, :].contiguous()
        dw1 = torch.full((cout, 1, 1, cin), float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("diga_conv2d_wgrad_bf16x6_f32in", _lib.ptr(dy), cout, _lib.ptr(xt), cin, _lib.ptr(dw1), _lib.ptr(ws1), ws1.numel(), n, ho, wo,
                  cin, ho, wo, cout, 1, 1, 1, 1, 0, 0, 1, 1, _lib.stream())
        torch.cuda.synchronize()
        assert torch.equal(dw[:, tap // k, tap % k, :], dw1[:, 0, 0, :]), f"{name}: tap {tap}"
    assert_close(dw, d["dwr"], 1e-5, 3e-6 * float(d["dwr"].abs().max()), f"{name} grad weight vs float64")


# ------------------------------------------------------------------------------------------------ 3. error table
def _run_layer(case, math, x, wt, b, probe, **cfg):
    """tests/test_gpu_conv_bf16x6.py::_run_layer under config.override(**cfg)."""
    from diga_amd.model.conv import DigaConv2d
    name, n, cin, h, w, cout, k, stride, pad, dil, bias = case
    m = DigaConv2d(cin, cout, k, stride=stride, padding=pad, dilation=dil, bias=bias)
    with torch.no_grad():
        m.weight.copy_(wt)
        if bias:
            m.bias.copy_(b)
    m = m.to(DEV)
    need_dx = cin >= 8 and (stride == 1 or k == 1)
    xd = x.to(DEV).requires_grad_(need_dx)
    with config.override(**cfg), _Mode(math) as log:
        y = m(xd)
        (y * probe.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        log = dict(log)
    return y.detach(), (xd.grad if need_dx else None), m.weight.grad, (m.bias.grad if bias else None), log


TABLE_CASES = TAP_CASES + [c for c in CASES if c[0] == "stem_7x7"]


@pytest.mark.parametrize("case", TABLE_CASES, ids=lambda c: c[0])
def test_per_layer_error_against_float64_and_direct_fp32(case):
    """The form and the criterion of test_gpu_conv_bf16x6.py::test_per_layer_error_against_float64_and_exact_fp32 for the multi-tap rows
    of test_gpu_conv.CASES and the stem: y, dx, dw in mode 0 on the DIRECT fp32 kernels (winograd = False) and in mode 2 + x6_taps, each
    against F.conv2d in float64 (max |t - t64| / max |t64|):
      (a) mode 2 + x6_taps meets the bounds test_gpu_conv.py::test_conv_fwd_bwd holds the direct kernels to, unchanged: 2e-6 / 3e-6 /
          3e-6 of scale;
      (b) per tensor err_x6 <= 1.5 * err_f32 (1.5 = the noise of a max statistic, not room for a worse arithmetic);
      (c) path_log: all passes on "bf16x6/taps" (the stem: forward and weight gradient on "bf16x6/ls"), none in mode 0."""
    name = case[0]
    stem = name == "stem_7x7"
    x, wt, b, probe, yr, dxr, dwr, dbr = _inputs(case)
    y0, dx0, dw0, _, log0 = _run_layer(case, 0, x, wt, b, probe, winograd=False)
    y2, dx2, dw2, db2, log2 = _run_layer(case, 2, x, wt, b, probe, winograd=False, x6_taps=True)
    e0 = [_rel(y0, yr), None if stem else _rel(dx0, dxr), _rel(dw0, dwr)]
    e2 = [_rel(y2, yr), None if stem else _rel(dx2, dxr), _rel(dw2, dwr)]
    cell = lambda i: "      -      " if e0[i] is None else f"f32 {e0[i]:.2e} x6 {e2[i]:.2e} ratio {e2[i] / e0[i]:.2f}"
    print(f"\n[bf16x6 taps table] {name:18s} K={case[2] * case[6] ** 2:5d} | y {cell(0)} | dx {cell(1)} | dw {cell(2)}")
    if stem:
        assert log2 == {("fwd", "bf16x6/ls"): 1, ("wgrad", "bf16x6/ls"): 1}, log2
        assert log0 == {("fwd", "f32"): 1, ("wgrad", "f32"): 1}, log0
    else:
        assert log2 == {("fwd", "bf16x6/taps"): 1, ("dgrad", "bf16x6/taps"): 1, ("wgrad", "bf16x6/taps"): 1}, log2
        assert log0 == {("fwd", "f32"): 1, ("dgrad", "f32"): 1, ("wgrad", "f32"): 1}, log0
    assert_close(y2, yr, 1e-5, 2e-6 * float(yr.abs().max()), f"{name} forward")
    if not stem:
        assert_close(dx2, dxr, 1e-5, 3e-6 * float(dxr.abs().max()), f"{name} grad input")
    assert_close(dw2, dwr, 1e-5, 3e-6 * float(dwr.abs().max()), f"{name} grad weight")
    if dbr is not None:
        assert_close(db2, dbr, 1e-5, 1e-5 * float(dbr.abs().max()), f"{name} grad bias")
    for what, a0, a2 in zip(("y", "dx", "dw"), e0, e2):
        assert a0 is None or a2 <= 1.5 * a0, f"{name} {what}: bf16x6 {a2:.2e} vs direct fp32 {a0:.2e} of scale"


# ------------------------------------------------------------------------------------------------ 4. bottleneck chain
def test_layer1_width_bottleneck_chain(monkeypatch):
    """The construction of test_gpu_conv_bf16x6.py::test_residual_junction_epilogues_and_forward_statistics -- three bottlenecks of
    layer1's widths (256 -> 64 -> 64 -> 256, identity residuals, train-mode BatchNorm, fuse_bwd on) -- in mode 2 with x6_taps: conv2
    (64 -> 64, 3x3) runs forward with BatchNorm statistics, backward-data WITH the epilogue that finishes bn1's gradient, and its weight
    gradient on "bf16x6/taps".  y, dx and every weight gradient against the float64 oracle with the device's ReLU patterns pinned, at
    that test's 2e-5 of scale; the forward statistics the epilogues hand bn1 / bn2 / bn3 of the first block against a float64 two-pass
    mean / variance of the conv's own output: no further from it than 2 x what mode 0 shows on the same inputs."""
    from diga_amd import _lib
    from diga_amd.model import norm as dn
    planes, inpl, dil, n, h, w = 64, 256, 1, 2, 31, 29
    names = [f"junction{planes}.b{i}" for i in range(3)]
    sds = [_block_state(nm, inpl, planes) for nm in names]
    blocks = [_make_block(sd, nm, inpl, planes, dil) for sd, nm in zip(sds, names)]
    g = synth.gen(planes + 5)
    x = torch.randn((n, inpl, h, w), generator=g).relu_() + 0.1 * torch.randn((n, inpl, h, w), generator=g)
    probe = torch.randn((n, inpl, h, w), generator=g)
    blocks[0].bn1.momentum = blocks[0].bn2.momentum = blocks[0].bn3.momentum = 1.0
    assert config.active().fuse_bwd and dn.fuse_backward_enabled()
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])

    def run(math, **cfg):
        for b in blocks:
            for p in b.parameters():
                p.grad = None
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
        seen, hooks = {}, []
        for i, b in enumerate(blocks):
            hooks.append(b.bn1.register_forward_hook(lambda m, a, o, i=i: seen.__setitem__((i, 1), (o.detach() > 0).cpu().double())))
            hooks.append(b.bn2.register_forward_hook(lambda m, a, o, i=i: seen.__setitem__((i, 2), (o.detach() > 0).cpu().double())))
            hooks.append(b.register_forward_hook(lambda m, a, o, i=i: seen.__setitem__((i, 3), (o.detach() > 0).cpu().double())))
        for key, conv in (("c1", blocks[0].conv1), ("c2", blocks[0].conv2), ("c3", blocks[0].conv3)):
            hooks.append(conv.register_forward_hook(lambda m, a, o, key=key: seen.__setitem__(key, o.detach().cpu().double())))
        calls.clear()
        with config.override(**cfg), _Mode(math) as log:
            y = xd
            for b in blocks:
                y = b(y)
            (y * probe.to(DEV)).sum().backward()
            torch.cuda.synchronize()
            log = dict(log)
        for hk in hooks:
            hk.remove()
        stats = {}
        for key, bn in (("c1", blocks[0].bn1), ("c2", blocks[0].bn2), ("c3", blocks[0].bn3)):
            yd = seen[key]
            cnt = yd.numel() // yd.shape[1]
            mean, var = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
            got_mean, got_var = bn.running_mean.double().cpu(), bn.running_var.double().cpu() * (cnt - 1) / cnt
            stats[key] = (float((got_mean - mean).abs().max() / mean.abs().max()), float((got_var - var).abs().max() / var.max()))
        grads = {f"{i}.{k}": p.grad.clone() for i, b in enumerate(blocks) for k, p in b.named_parameters() if p.grad is not None}
        return y.detach().clone(), xd.grad.clone(), grads, seen, stats, log, list(calls)

    _, _, _, _, stats0, log0, _ = run(0)
    y2, dx2, gr2, masks, stats2, log2, calls2 = run(2, x6_split="loader", x6_taps=True)
    assert not any(a.startswith("bf16x6") for _, a in log0), log0
    # conv2 of three blocks on the multi-tap kernels in all three passes, conv1 / conv3 on the pointwise ones: nothing on fp32
    assert log2 == {(p, a): c for p in ("fwd", "dgrad", "wgrad") for a, c in (("bf16x6/taps", 3), ("bf16x6/ls", 6))}, log2
    # conv2's backward-data finishes bn1's gradient in every block
    assert calls2.count("diga_conv_taps_bf16x6_f32in_epi") == 3 and calls2.count("diga_conv_taps_bf16x6_f32in") == 3, calls2
    assert calls2.count("diga_conv_taps_wgrad_bf16x6_f32in") == 3

    sd64 = {}
    for sd in sds:
        sd64.update({k: v.double().requires_grad_(v.dim() == 4) for k, v in sd.items()})
    xr = x.double().requires_grad_()
    yr = xr
    for i, nm in enumerate(names):
        yr = od.bottleneck_fixed_masks(sd64, nm, yr, 1, dil, False, (masks[(i, 1)], masks[(i, 2)], masks[(i, 3)]))
    (yr * probe.double()).sum().backward()
    errs = {"y": _rel(y2, yr), "dx": _rel(dx2, xr.grad)}
    for k in gr2:
        i, nm = k.split(".", 1)
        errs[k] = _rel(gr2[k], sd64[f"{names[int(i)]}.{nm}"].grad)
    print(f"\n[bf16x6 taps junction] worst error / scale vs float64: {max(errs.values()):.1e} ({max(errs, key=errs.get)})")
    assert len(gr2) == 9
    for k, v in errs.items():
        assert v < 2e-5, f"{k}: {v:.2e} of scale"
    for key in ("c1", "c2", "c3"):
        print(f"[bf16x6 taps statistics] {key}: mean f32 {stats0[key][0]:.2e} x6 {stats2[key][0]:.2e} | var f32 {stats0[key][1]:.2e} x6 {stats2[key][1]:.2e}")
    for key in ("c1", "c2", "c3"):
        assert stats2[key][0] <= 2 * stats0[key][0], (key, "mean", stats2[key], stats0[key])
        assert stats2[key][1] <= 2 * stats0[key][1], (key, "var", stats2[key], stats0[key])


# ------------------------------------------------------------------------------------------------ 5. whole small model
def test_whole_small_model_leaves_nothing_on_the_fp32_pipe_and_switch_off_is_switch_absent():
    """The construction of test_gpu_conv_bf16x6.py::test_whole_model_gradients_vs_float64_with_pinned_switches for the small backbone at
    96 x 128, in mode 2 with x6_split = "loader", x6_winograd and x6_taps, at that test's mode-2 bounds (logits within 8e-5 of scale,
    every parameter gradient within 5e-5): every launch path_log counts is on "bf16x6/ls", "winograd/x6" or "bf16x6/taps".  Then the same
    model without x6_taps: one run that does not name the field and one under config.override(x6_taps=False) -- equal, bit for bit, in
    logits, features, every gradient and path_log, and neither knows the new arithmetic."""
    from diga_amd.model import seg_model_noaux as sm
    from diga_amd.model.model_noaux import SegModel
    from diga_amd.model.norm import DigaBatchNorm2d, DigaGroupNorm
    arch_d, arch_o, hw = sm.TINY, od.TINY, (96, 128)
    sd32 = detweights.state_dict(arch_o)
    m = SegModel(arch=arch_d)
    m.load_state_dict(sd32)
    m = m.to(DEV).train()
    m.final.head[0].p = 0.0
    g = synth.gen(4242)
    x = torch.rand((2, 3) + hw, generator=g) * 2 - 1
    xd = x.to(DEV)
    named = dict(m.named_parameters())
    with config.override(x6_split="loader", x6_winograd=True, x6_taps=True), _Mode(2) as log:
        seen, hooks = {}, []
        names = {mod: n for n, mod in m.named_modules()}
        for mod in m.modules():
            if isinstance(mod, DigaBatchNorm2d) or (isinstance(mod, DigaGroupNorm) and ".conv2d_list." in names[mod]):
                hooks.append(mod.register_forward_hook(lambda mo, i, o, n=names[mod]: seen.__setitem__(n, (o.detach() > 0).cpu().double())))
        hooks.append(m.layer0[3].register_forward_hook(lambda mo, i, o: seen.__setitem__("pool_in", i[0].detach().cpu().double())))
        hooks.append(m.final.bottleneck[0].se[1].register_forward_hook(lambda mo, i, o: seen.__setitem__("se", (o.detach() > 0).cpu().double())))
        try:
            with torch.no_grad():
                out_plain = m(xd)[2]
        finally:
            for h in hooks:
                h.remove()
        masks = {"layer0": seen["layer0.1"], "se": seen["se"],
                 "pool_idx": F.max_pool2d(seen["pool_in"], 3, 2, 1, ceil_mode=True, return_indices=True)[1]}
        for li in range(4):
            for bi in range(arch_o.layers[li]):
                for k in (1, 2, 3):
                    masks[f"layer{li + 1}.{bi}.{k}"] = seen[f"layer{li + 1}.{bi}.bn{k}"]
        for b in range(5):
            masks[f"aspp.{b}"] = seen[f"final.conv2d_list.{b}.1"]
        trainable = [k for k, (_, kind) in od.state_shapes(arch_o).items() if kind in ("conv", "bias", "gn_w", "gn_b", "lin", "head")]
        sd64 = {k: (v.double().requires_grad_() if k in trainable else v.double()) for k, v in sd32.items()}
        _, _, out_r, feat_r = od.forward_fixed_masks(sd64, x.double(), dataclasses.replace(arch_o, droprate=0.0), masks,
                                                     keep_mask=torch.ones(2, arch_o.aspp_width))
        probe = torch.randn(out_r.shape, generator=g)
        probe_f = 0.1 * torch.randn(feat_r.shape, generator=g)
        ((out_r * probe.double()).sum() + (feat_r * probe_f.double()).sum()).backward()
        log.clear()
        _, _, out, feat = m(xd)
        assert torch.equal(out.detach(), out_plain)
        e_fwd = _rel(out, out_r)
        print(f"\n[bf16x6 taps model] TINY: logits within {e_fwd:.1e} of scale of the float64 oracle")
        assert e_fwd < FWD_TOL_F32
        ((out * probe.to(DEV)).sum() + (feat * probe_f.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        log = dict(log)
    assert {a for _, a in log} <= {"bf16x6/ls", "winograd/x6", "bf16x6/taps"}, log
    assert all(log.get((p, "bf16x6/taps"), 0) > 0 and log.get((p, "bf16x6/ls"), 0) > 0 for p in ("fwd", "dgrad", "wgrad")), log
    worst, worst_k = 0.0, None
    for k in trainable:
        ref = sd64[k].grad
        e = float((named[k].grad.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        if e > worst:
            worst, worst_k = e, k
        assert e < 5e-5, (k, e)
    print(f"[bf16x6 taps model] TINY: all {len(trainable)} parameter gradients within {worst:.1e} of scale (worst: {worst_k}); paths {log}")

    def plain_run(**cfg):
        for p in m.parameters():
            p.grad = None
        with config.override(x6_split="loader", x6_winograd=True, **cfg), _Mode(2) as lg:
            _, _, o, f = m(xd)
            ((o * probe.to(DEV)).sum() + (f * probe_f.to(DEV)).sum()).backward()
            torch.cuda.synchronize()
            lg = dict(lg)
        return o.detach().clone(), f.detach().clone(), {k: p.grad.clone() for k, p in named.items() if p.grad is not None}, lg

    assert config.active().x6_taps is False, "this test expects the process default of the switch (off)"
    o_a, f_a, g_a, log_a = plain_run()
    o_b, f_b, g_b, log_b = plain_run(x6_taps=False)
    assert log_a == log_b and not any(a == "bf16x6/taps" for _, a in log_a), (log_a, log_b)
    assert any(a == "f32" for _, a in log_a), log_a                         # (what the switch is for)
    assert torch.equal(o_a, o_b) and torch.equal(f_a, f_b) and g_a.keys() == g_b.keys()
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), k


# ------------------------------------------------------------------------------------------------ 6. inference fold
def _eval_block_and_stem():
    """A strided layer1-width bottleneck with a downsample branch (conv2: 64 -> 64, 3x3) and a stem conv + BatchNorm, in eval mode."""
    from diga_amd.model import conv as dc
    from diga_amd.model import seg_model_noaux as sm
    from test_gpu_infer_fold import _fill
    g = torch.Generator().manual_seed(1406)
    ds = nn.Sequential(dc.DigaConv2d(256, 256, 1, stride=2, bias=False), sm._frozen_bn(256))
    blk = sm.Bottleneck(256, 64, 2, dilation=1, downsample=ds)
    _fill(blk, g)
    stem = nn.Sequential(dc.DigaConv2d(3, 64, 7, stride=2, padding=3, bias=False), sm._frozen_bn(64))
    _fill(stem, g)
    xb = torch.randn((2, 256, 19, 17), generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    xs = torch.randn((2, 3, 37, 41), generator=g).to(DEV)
    return blk.to(DEV).eval(), xb, stem.to(DEV).eval(), xs


def _stem_forward(stem, x):
    """ResNet.stem of seg_model_noaux.py without the pooling."""
    conv, bn = stem[0], stem[1]
    if conv.folds_eval_bn(x, bn):
        return conv(x, infer=(bn, None, True))
    return bn(conv(x), relu=True)


def test_inference_fold_equals_unfolded():
    """fold_eval_bn + fold_eval_bn_x6 + x6_taps: the eval forward of a bottleneck with a 64-channel conv2, and of the stem, equals the
    unfolded run under the same switches bit for bit, on "bf16x6/taps+bn" / "bf16x6/ls+bn"; with fold_eval_bn_x6 off those sites do not
    fold (the multi-tap kernels' inference epilogue is that switch's) and the result is equal too."""
    from diga_amd.model import conv as dc
    blk, xb, stem, xs = _eval_block_and_stem()

    def run(fn, fold, fold_x6):
        dc.path_log = {}
        try:
            with config.override(conv_math=2, x6_split="loader", x6_taps=True, fold_eval_bn=fold, fold_eval_bn_x6=fold_x6), torch.no_grad():
                y = fn()
            torch.cuda.synchronize()
            return y, dc.path_log
        finally:
            dc.path_log = None

    off, log_off = run(lambda: blk(xb), False, True)
    assert log_off == {("fwd", "bf16x6/ls"): 3, ("fwd", "bf16x6/taps"): 1}, log_off
    on, log_on = run(lambda: blk(xb), True, True)
    assert log_on == {("fwd", "bf16x6/ls+bn"): 3, ("fwd", "bf16x6/taps+bn"): 1}, log_on
    assert torch.equal(on, off), int((on != off).sum())
    half, log_half = run(lambda: blk(xb), True, False)
    assert log_half == log_off and torch.equal(half, off), log_half

    s_off, slog_off = run(lambda: _stem_forward(stem, xs), False, True)
    assert slog_off == {("fwd", "bf16x6/ls"): 1}, slog_off
    s_on, slog_on = run(lambda: _stem_forward(stem, xs), True, True)
    assert slog_on == {("fwd", "bf16x6/ls+bn"): 1}, slog_on
    assert torch.equal(s_on, s_off), int((s_on != s_off).sum())
    s_half, slog_half = run(lambda: _stem_forward(stem, xs), True, False)
    assert slog_half == slog_off and torch.equal(s_half, s_off), slog_half


# ------------------------------------------------------------------------------------------------ 7. switch changed inside a graph
@pytest.mark.parametrize("fwd_on,bwd_on", [(True, False), (False, True)], ids=["on_off", "off_on"])
def test_switch_changed_between_forward_and_backward(fwd_on, bwd_on):
    """The switch is read per call and the family saves nothing of its own (fp32 x and weights, as the direct kernels): 3x3_dil1 with the
    forward under one setting and the backward under the other raises nothing and gives, bit for bit, the output of the forward's
    kernel and the gradients of the backward's kernels."""
    from diga_amd.model.conv import DigaConv2d
    case = next(c for c in CASES if c[0] == "3x3_dil1")
    name, n, cin, h, w, cout, k, stride, pad, dil, bias = case
    x, wt, b, probe = _inputs(case)[:4]
    m = DigaConv2d(cin, cout, k, stride=stride, padding=pad, dilation=dil, bias=bias)
    with torch.no_grad():
        m.weight.copy_(wt)
    m = m.to(DEV)

    def run(f_on, b_on):
        m.weight.grad = None
        xd = x.to(DEV).requires_grad_()
        with _Mode(2) as log:
            with config.override(x6_taps=f_on):
                y = m(xd)
            with config.override(x6_taps=b_on):
                (y * probe.to(DEV)).sum().backward()
                torch.cuda.synchronize()
            log = dict(log)
        return y.detach(), xd.grad, m.weight.grad.clone(), log

    tag = lambda on: "bf16x6/taps" if on else "f32"
    y, dx, dw, log = run(fwd_on, bwd_on)
    assert log == {("fwd", tag(fwd_on)): 1, ("dgrad", tag(bwd_on)): 1, ("wgrad", tag(bwd_on)): 1}, log
    y_f, _, _, _ = run(fwd_on, fwd_on)
    _, dx_b, dw_b, _ = run(bwd_on, bwd_on)
    assert torch.equal(y, y_f) and torch.equal(dx, dx_b) and torch.equal(dw, dw_b)
