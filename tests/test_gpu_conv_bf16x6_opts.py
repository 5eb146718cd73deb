"""GPU tests of bf16x6 for convolutions with a folded input map / activation (config.x6_opts under conv_math = 2; csrc/conv_bf16x6.h: the
OPT instantiations of conv_fwd_x6_kernel; csrc/winograd.hip: diga_conv_winograd_bf16x6_opts; model/conv.py: ("x6rs", "opts") and the
bf16x6 form of "winograd_reflect").

  5. the loader's map bit for bit: diga_conv_taps_bf16x6_f32in_opts on the source tensor against diga_conv_taps_bf16x6_f32in on the
     explicitly upsampled and padded image;
  6. tanh against float64 tanh of the same kernel's pre-activation, next to the fp32 `_opts` kernel's deviation;
  7. the reflect-padded Winograd layers with their products on bf16x6 against float64 and against the fp32 form;
  8. the frozen translator: no launch left on the fp32 matrix pipe, the switch off = the switch absent, flipped in both directions."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from diga_amd import config

from conftest import WINO_TOL, assert_close
from oracle import synth
from test_translator import _filled

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _leave_global_rng_and_arithmetic_untouched():
    """As tests/test_gpu_conv_bf16x6.py: every test hands torch's generators, the conv arithmetic and conv.path_log back as it found
    them."""
    from diga_amd import _lib
    from diga_amd.model import conv as dc
    cpu, gpu = torch.get_rng_state(), (torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    math, log = _lib.get_conv_math(), dc.path_log
    yield
    _lib.join_side()
    _lib.set_conv_math(math)
    dc.path_log = log
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _fwd_tag():
    from diga_amd import _lib
    return _lib.PROF_TAGS.index("conv_fwd")


def _image(w):
    """diga_split_bf16x6_image of [K,R,S,C] weights (tap-major K-steps)."""
    from diga_amd import _lib
    k, r, s, c = w.shape
    img = torch.empty(_lib.lib.diga_split_bf16x6_image_bytes(k, r * s, c), dtype=torch.uint8, device=DEV)
    _lib.call("diga_split_bf16x6_image", _lib.ptr(w), _lib.ptr(img), k, r * s, c, _lib.stream())
    return img


def _taps(x, w, bias, ho, wo, stride, off0, dil, opts=None, out_ld=None):
    """diga_conv_taps_bf16x6_f32in (opts None) or its `_opts` form on x [N,Hi,Wi,C] (dense, or a channel slice of a wider NHWC buffer)
    and w [K,R,S,C] -> out [N,Ho,Wo,K], a slice of a NaN-filled buffer of pitch out_ld."""
    from diga_amd import _lib
    n, hi, wi, c = x.shape
    k, r, s, _ = w.shape
    out_ld = k if out_ld is None else out_ld
    buf = torch.full((n, ho, wo, out_ld), float("nan"), dtype=torch.float32, device=DEV)
    img = _image(w)
    name = "diga_conv_taps_bf16x6_f32in" + ("" if opts is None else "_opts")
    tail = [None] + ([] if opts is None else [ctypes.byref(_lib.ConvOptions(*opts))])
    _lib.call(name, _lib.ptr(x), x.stride(2), _lib.ptr(img), _lib.ptr(bias), _lib.ptr(buf), n, hi, wi, c, ho, wo, k, out_ld, r, s, stride,
              stride, off0, off0, dil, dil, *tail, _fwd_tag(), _lib.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[..., k:]).all()), "the kernel wrote past Cout"
    return buf[..., :k]


def _explicit(x, shift, pad, reflect):
    """The image the folded kernel reads, built with torch: nearest upsampling by 2^shift, then the padding.  x NHWC -> NHWC, copies only."""
    t = x.permute(0, 3, 1, 2)
    if shift:
        t = F.interpolate(t, scale_factor=float(1 << shift), mode="nearest")
    t = F.pad(t, (pad, pad, pad, pad), mode="reflect" if reflect else "constant")
    return t.permute(0, 2, 3, 1).contiguous()


# name, N, source H, W, Cin, Cout, k, stride, pad, dilation, reflect, shift, bias, out_ld, in_ld: M = N * Ho * Wo is more than one 256-row
# tile, (the 8 x 8 case apart) no multiple of 256, and a tile straddles two images wherever an image's rows are no multiple of 256
MAP_CASES = [
    ("4x4_stride2_reflect", 3, 25, 21, 64, 128, 4, 2, 1, 1, 1, 0, True, None, None),          # 3 x 12 x 10 = 360 rows
    ("5x5_reflect_up1", 2, 9, 11, 64, 32, 5, 1, 2, 1, 1, 1, True, None, None),                # 2 x 18 x 22 = 792
    ("7x7_reflect_cout3_pitch7", 3, 13, 10, 64, 3, 7, 1, 3, 1, 1, 0, True, 7, None),          # 3 x 130 = 390, ragged channel tile
    ("3x3_reflect_up2", 2, 9, 11, 32, 64, 3, 1, 1, 1, 1, 2, False, None, None),               # 2 x 36 x 44 = 3168
    ("3x3_dil6_zero_up1_8x8", 3, 8, 8, 64, 64, 3, 1, 6, 6, 0, 1, False, None, None),          # 3 x 16 x 16: one image per tile
    ("3x3_dil8_zero_up1_dead_taps", 3, 8, 20, 64, 64, 3, 1, 8, 8, 0, 1, True, None, None),    # 3 x 16 x 40 = 1920: 6-row tiles, dead taps
    ("5x5_reflect_up1_channel_slice", 2, 11, 9, 64, 32, 5, 1, 2, 1, 1, 1, False, None, 96),   # in_ld 96 > Cin
    ("3x3_all_options_zero", 2, 13, 10, 32, 64, 3, 1, 1, 1, 0, 0, True, None, None),          # plain zero padding through the map
]
_DATA = {}


def _data(case):
    """Seeded source tensor (NHWC, possibly a channel slice), [K,R,S,C] weights and bias of one case: built once, never modified."""
    name, n, h, w, cin, cout, k, stride, pad, dil, reflect, shift, bias, out_ld, in_ld = case
    if name not in _DATA:
        g = synth.gen(1800 + len(_DATA))
        wide = torch.randn((n, h, w, in_ld or cin), generator=g).to(DEV)
        x = wide[..., 16:16 + cin] if in_ld else wide
        wt = (torch.randn((cout, k, k, cin), generator=g) / (k * k * cin) ** 0.5).to(DEV)
        b = torch.randn(cout, generator=g).to(DEV) if bias else None
        _DATA[name] = (x, wt, b)
    return _DATA[name]


# ------------------------------------------------------------------------------------------------ 5. the loader's map, bit for bit
@pytest.mark.parametrize("case", MAP_CASES, ids=lambda c: c[0])
def test_folded_map_equals_plain_kernel_on_explicit_image(case):
    """The `_opts` kernel on the source tensor against the plain multi-tap kernel (offsets 0) on interpolate(nearest) + pad(reflect |
    constant) of it: same weight image, same row tiles, same live-tap K-step sequence (a tap that is dead for a tile reads explicit
    zeros in the reference: exact zeros added to an accumulator that starts at +0), same drain -- so torch.equal.  A wrong mirror, shift,
    extent or source pixel moves O(1) of the border outputs."""
    name, n, h, w, cin, cout, k, stride, pad, dil, reflect, shift, bias, out_ld, in_ld = case
    x, wt, b = _data(case)
    if in_ld:
        assert x.stride(2) == in_ld > cin and not x.is_contiguous()
    big = _explicit(x, shift, pad, reflect)
    hl, wl = h << shift, w << shift
    assert tuple(big.shape) == (n, hl + 2 * pad, wl + 2 * pad, cin)
    ho = (hl + 2 * pad - dil * (k - 1) - 1) // stride + 1
    wo = (wl + 2 * pad - dil * (k - 1) - 1) // stride + 1
    m = n * ho * wo
    assert m > 256 and (m % 256 != 0 or name.endswith("8x8"))
    want = _taps(big, wt, b, ho, wo, stride, 0, dil, out_ld=out_ld)
    got = _taps(x, wt, b, ho, wo, stride, -pad, dil, opts=(reflect, shift, 0), out_ld=out_ld)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} elements differ, worst " \
                                   f"{float((got - want).abs().max()):.3g}"
    # and the reference itself is the convolution: float64 on the explicit image, at the multi-tap kernels' 2e-6 of scale
    ref = F.conv2d(big.permute(0, 3, 1, 2).double().cpu(), wt.permute(0, 3, 1, 2).double().cpu(), None if b is None else b.double().cpu(),
                   stride=stride, dilation=dil).permute(0, 2, 3, 1)
    err = float((got.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"{name}: M {m}, error against float64 {err:.2e} of scale")
    assert err < 2e-6, err


# ------------------------------------------------------------------------------------------------ 6. tanh
def test_tanh_epilogue_against_float64_and_the_fp32_kernel():
    """activation = 1 against float64 tanh of the SAME entry point's activation = 0 output, for the new kernel and for
    diga_conv2d_nhwc_f32_opts (the same tanhf in the same drain_stage: the yardstick).  The two pre-activations differ in their last
    bits, so the new kernel's deviation may be at most twice the fp32 kernel's.  Measured: 5.8e-8 against 7.0e-8."""
    from diga_amd import _lib
    case = MAP_CASES[2]
    name, n, h, w, cin, cout, k, stride, pad, dil, reflect, shift, bias, out_ld, in_ld = case
    x, wt, b = _data(case)

    def f32(act):
        buf = torch.full((n, h, w, out_ld), float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("diga_conv2d_nhwc_f32_opts", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(b), _lib.ptr(buf), n, h, w, cin, x.stride(2), h, w, cout,
                  out_ld, k, k, 1, 1, -pad, -pad, 1, 1, ctypes.byref(_lib.ConvOptions(reflect, 0, act)), _fwd_tag(), _lib.stream())
        torch.cuda.synchronize()
        return buf[..., :cout]

    def dev(run):
        pre, post = run(0), run(1)
        assert float(pre.abs().max()) > 1.0                       # (the pre-activations reach tanh's curved part)
        return float((post.cpu().double() - torch.tanh(pre.cpu().double())).abs().max())

    d_new = dev(lambda act: _taps(x, wt, b, h, w, 1, -pad, 1, opts=(reflect, 0, act), out_ld=out_ld))
    d_f32 = dev(f32)
    print(f"tanh deviation from float64 tanh of the kernel's own pre-activation: bf16x6 `_opts` {d_new:.3e}, fp32 `_opts` {d_f32:.3e}")
    assert d_new <= 2.0 * d_f32, (d_new, d_f32)
    assert d_new < 1e-6                                           # (absolute: a few ulp of a value in (-1, 1))


# ------------------------------------------------------------------------------------------------ 7. Winograd with reflection
def _spy(monkeypatch):
    from diga_amd import _lib
    calls, orig = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    return calls


_WINO = {}


def _wino_data(cin, d):
    """Input, weights, bias and the float64 reference on the explicitly mirrored input: once per (Cin, dilation)."""
    if (cin, d) not in _WINO:
        g = synth.gen(1870 + cin + d)
        x = torch.randn((2, cin, 11, 17), generator=g)
        w = torch.randn((256, cin, 3, 3), generator=g) / (9 * cin) ** 0.5
        b = torch.randn(256, generator=g)
        ref = F.conv2d(F.pad(x.double(), (d, d, d, d), mode="reflect"), w.double(), b.double(), dilation=d)
        _WINO[(cin, d)] = (x, w, b, ref)
    return _WINO[(cin, d)]


@pytest.mark.parametrize("tile", [4, 6], ids=["F4x4", "F6x6"])
@pytest.mark.parametrize("d", [1, 2], ids=["pad1", "pad2"])
@pytest.mark.parametrize("cin", [256, 128])
def test_winograd_reflect_on_bf16x6(cin, d, tile, monkeypatch):
    """A reflect-padded 3x3 layer (Cin -> 256, 2 x 11 x 17: ragged tiles on both axes) with winograd_max_tile forcing the tile: the
    products on bf16x6 (x6_opts on) within WINO_TOL of float64 and no further from it than diga_conv2d_winograd_f32_opts (x6_opts off)
    on the same inputs.  A kernel that ignored the mirror would miss the border by O(1).  Measured: 0.36 - 0.46 x the fp32 form's error
    on the eight cases (has the table)."""
    from diga_amd.model import conv as dc
    from diga_amd.model.conv import DigaConv2d
    x, w, b, ref = _wino_data(cin, d)
    m = DigaConv2d(cin, 256, 3, 1, padding=d, dilation=d, bias=True)
    m.load_state_dict({"weight": w, "bias": b})
    m = m.to(DEV).eval()
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    calls = _spy(monkeypatch)
    errs = {}
    for on in (False, True):
        with config.override(conv_math=2, x6_split="loader", x6_winograd=True, x6_opts=on, winograd_max_tile=tile), torch.no_grad():
            dc.path_log = {}
            del calls[:]
            y = m(xd, opts=(1, 0, 0))
            torch.cuda.synchronize()
            assert dc._plan(2, 11, 17, cin, 256, 3, 3, (1, 1), (-d, -d), (d, d), 11, 17, opts=(1, 0, 0)).tile == tile
            assert dc.path_log == {("fwd", "winograd/x6" if on else "winograd"): 1}, dc.path_log
            assert ("diga_conv_winograd_bf16x6_opts" if on else "diga_conv2d_winograd_f32_opts") in calls, calls
        errs[on] = float((y.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"winograd_reflect {cin} -> 256, pad {d}, F({tile}x{tile}): bf16x6 {errs[True]:.2e}, fp32 {errs[False]:.2e} of scale, "
          f"ratio {errs[True] / errs[False]:.2f}")
    assert errs[True] < WINO_TOL[tile][0], errs
    assert errs[True] <= errs[False], errs


# ------------------------------------------------------------------------------------------------ 8. the layer and the translator
X6 = dict(conv_math=2, x6_split="loader", x6_taps=True, x6_winograd=True)


def _translate(enc, dec, x, **cfg):
    """dec(enc(x)) under no_grad and `cfg` -> (feat, rec, path_log, entry points called)."""
    from diga_amd import _lib
    from diga_amd.model import conv as dc
    calls, orig = [], _lib.call
    _lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        with config.override(**cfg), torch.no_grad():
            dc.path_log = {}
            feat = enc(x)
            rec = dec(feat)
            torch.cuda.synchronize()
            log = dict(dc.path_log)
    finally:
        _lib.call = orig
        dc.path_log = None
    # (the Winograd tile table of a geometry is built by the first call that needs it and kept: not part of a pass)
    return feat, rec, log, [c for c in calls if c != "diga_conv2d_winograd_tile_table"]


def test_translator_runs_on_bf16x6(golden):
    from diga_amd.model.model_noaux import ImgDecoder, ImgEncoder
    g = golden("translator")
    enc, dec = _filled(ImgEncoder, "enc").to(DEV), _filled(ImgDecoder, "dec").to(DEV)
    x = g.t("x").to(DEV)
    feat, rec, log, calls = _translate(enc, dec, x, **X6, x6_opts=True)
    assert list(feat.shape) == g["feat_shape"].tolist()
    assert synth.checksum(feat.detach().cpu()) == pytest.approx(float(g["feat_sum"]), rel=1e-3, abs=1e-2)
    assert_close(rec, g.t("rec"), 1e-3, 1e-4, "translated image")
    # nothing left on the fp32 matrix pipe: the stem on the loader form, 5 multi-tap layers, 16 ResBlock convs through Winograd
    assert log == {("fwd", "bf16x6/ls"): 1, ("fwd", "bf16x6/taps"): 5, ("fwd", "winograd/x6"): 16}, log
    opts = [c for c in calls if c.endswith("_opts")]
    assert len(opts) == 21 and opts.count("diga_conv_taps_bf16x6_f32in_opts") == 5 and opts.count("diga_conv_winograd_bf16x6_opts") == 16, opts
    assert calls.count("diga_gn_fwd") == 21

    # the switch off = the switch absent: same launches, same bits
    feat0, rec0, log0, calls0 = _translate(enc, dec, x, **X6)
    feat1, rec1, log1, calls1 = _translate(enc, dec, x, **X6, x6_opts=False)
    assert not config.DEFAULTS.x6_opts or log0 == log                                       # (unless the environment turned it on)
    assert log1 == {("fwd", "bf16x6/ls"): 1, ("fwd", "f32"): 5, ("fwd", "winograd"): 16}, log1
    if not config.DEFAULTS.x6_opts:
        assert log0 == log1 and calls0 == calls1 and torch.equal(rec0, rec1) and torch.equal(feat0, feat1)
    assert_close(rec1, g.t("rec"), 1e-3, 1e-4, "translated image, x6_opts off")
    assert not torch.equal(rec1, rec)                                                       # (the switch does select other arithmetic)

    # flipped between passes of one model, in both directions: each pass is the pass of its setting
    _, rec_on, log_on, calls_on = _translate(enc, dec, x, **X6, x6_opts=True)
    _, rec_off, log_off, calls_off = _translate(enc, dec, x, **X6, x6_opts=False)
    assert log_on == log and calls_on == calls and torch.equal(rec_on, rec)
    assert log_off == log1 and calls_off == calls1 and torch.equal(rec_off, rec1)
    # and outside conv_math = 2 the switch selects nothing
    _, rec_f0, log_f0, calls_f0 = _translate(enc, dec, x, conv_math=0)
    _, rec_f1, log_f1, calls_f1 = _translate(enc, dec, x, conv_math=0, x6_taps=True, x6_winograd=True, x6_opts=True)
    assert log_f0 == log_f1 and calls_f0 == calls_f1 and torch.equal(rec_f0, rec_f1)
    assert all(k[1] in ("f32", "winograd") for k in log_f0), log_f0
    print(f"translator: rec error against the capture {float((rec.cpu() - g.t('rec')).abs().max()):.2e} (x6_opts on), "
          f"{float((rec1.cpu() - g.t('rec')).abs().max()):.2e} (off), {float((rec_f0.cpu() - g.t('rec')).abs().max()):.2e} (mode 0)")
