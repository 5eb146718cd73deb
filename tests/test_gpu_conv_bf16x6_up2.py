"""GPU tests of the bf16x6 upsample + conv on phase-collapsed weights (config.x6_up2 under conv_math = 2 with x6_taps, x6_opts and x6_window;
csrc/conv_bf16x6.h: conv_up2_x6_kernel, the ring form of conv_win_x6_kernel, diga_collapse_up2_weights, diga_conv_up2_bf16x6_f32in;
model/conv.py: the "x6up2" family).

  7. the collapsed weights: torch.equal to the host's double-sum-then-round (tools/bf16x6_emulation.py);
  8. bits: the entry point's output is torch.equal to a composite -- ring tiles from diga_conv_window_bf16x6_f32in with the same options
     and image, interior pixels of phase (fy, fx) from diga_conv_window_bf16x6_f32in on the SOURCE tensor with that phase's collapsed
     weights, no options, first tap at (a_y(fy, 0), a_x(fx, 0)), read at (Y >> 1, X >> 1);
  9. error against float64 on the explicit interpolate + pad image, next to the window form and the exact-fp32 `_opts` kernel;
 10. the frozen translator on the golden input: paths, error, the switch off = absent, flipped in both directions.

Every input lies inside a NaN-filled allocation with guard pixels in front and behind (once as a channel slice of pitch 96), every output
is a slice of a NaN-filled buffer with guard pixels of its own: a read outside the image shows up as a NaN in the result, a write outside
the slice as a number there."""
import ctypes
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from diga_amd import config

from conftest import assert_close
from oracle import synth
from test_translator import _filled

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # NaN pixels in front of and behind every input and output
TH, TW = 8, 16                   # the window kernel's output tile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emulation():
    spec = importlib.util.spec_from_file_location("bf16x6_emulation", os.path.join(ROOT, "tools", "bf16x6_emulation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(autouse=True)
def _leave_global_rng_and_arithmetic_untouched():
    """As tests/test_gpu_conv_bf16x6_window.py: every test hands torch's generators, the conv arithmetic and conv.path_log back as it
    found them."""
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


def _out(n, ho, wo, k, out_ld):
    """(whole NaN-filled allocation, its [n, ho, wo, out_ld] body behind GUARD pixels)."""
    ld = out_ld or k
    buf = torch.full(((n * ho * wo + 2 * GUARD) * ld,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[GUARD * ld:(GUARD + n * ho * wo) * ld].view(n, ho, wo, ld)


def _result(buf, body, k):
    torch.cuda.synchronize()
    ld = body.shape[3]
    assert bool(torch.isnan(buf[:GUARD * ld]).all()) and bool(torch.isnan(buf[-GUARD * ld:]).all()), "the kernel wrote outside the output tensor"
    assert bool(torch.isnan(body[..., k:]).all()), "the kernel wrote past Cout"
    assert not bool(torch.isnan(body[..., :k]).any()), "NaN in the result: a read outside the image, or an output never written"
    return body[..., :k]


def _window(x, w, bias, ho, wo, off0, opts=None, out_ld=None):
    """diga_conv_window_bf16x6_f32in at unit dilation on x [N,Hi,Wi,C] (dense, or a channel slice) and w [K,R,S,C] -> out [N,Ho,Wo,K]."""
    from diga_amd import _lib
    n, hi, wi, c = x.shape
    k, r, s, _ = w.shape
    (buf, body), img = _out(n, ho, wo, k, out_ld), _image(w)
    _lib.call("diga_conv_window_bf16x6_f32in", _lib.ptr(x), x.stride(2), _lib.ptr(img), _lib.ptr(bias), _lib.ptr(body), n, hi, wi, c, ho, wo, k,
              body.stride(2), r, s, off0[0], off0[1], 1, 1, None if opts is None else ctypes.byref(_lib.ConvOptions(*opts)), _fwd_tag(),
              _lib.stream())
    return _result(buf, body, k)


def _collapse(w, off0):
    """diga_collapse_up2_weights -> wc [2,2,K,R',S',C] (fp32, on the device)."""
    from diga_amd import _lib
    em = _emulation()
    k, r, s, c = w.shape
    wc = torch.full((2, 2, k, em.up2_taps(r, off0[0]), em.up2_taps(s, off0[1]), c), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("diga_collapse_up2_weights", _lib.ptr(w), _lib.ptr(wc), k, r, s, c, off0[0], off0[1], _lib.stream())
    return wc


def _up2(x, w, bias, ho, wo, off0, opts, out_ld=None):
    """diga_conv_up2_bf16x6_f32in: the layer's image, the four phase images of the collapsed weights, one call."""
    from diga_amd import _lib
    n, hi, wi, c = x.shape
    k, r, s, _ = w.shape
    rc, sc = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.lib.diga_conv_up2_bf16x6_plan(hi, wi, c, k, ho, wo, r, s, off0[0], off0[1], 1, 1, opts[1], opts[0], ctypes.byref(rc),
                                              ctypes.byref(sc)) == 1
    wc = _collapse(w, off0)
    assert tuple(wc.shape[3:5]) == (rc.value, sc.value)
    phases = torch.cat([_image(wc[fy, fx]) for fy in (0, 1) for fx in (0, 1)])
    assert phases.numel() == 4 * _lib.lib.diga_split_bf16x6_image_bytes(k, rc.value * sc.value, c)
    (buf, body), img = _out(n, ho, wo, k, out_ld), _image(w)
    _lib.call("diga_conv_up2_bf16x6_f32in", _lib.ptr(x), x.stride(2), _lib.ptr(img), _lib.ptr(phases), _lib.ptr(bias), _lib.ptr(body), n, hi, wi,
              c, ho, wo, k, body.stride(2), r, s, off0[0], off0[1], ctypes.byref(_lib.ConvOptions(*opts)), _fwd_tag(), _lib.stream())
    return _result(buf, body, k)


def _f32(x, w, bias, ho, wo, off0, opts, out_ld=None):
    """The exact-fp32 kernel with the folded map: diga_conv2d_nhwc_f32_opts."""
    from diga_amd import _lib
    n, hi, wi, c = x.shape
    k, r, s, _ = w.shape
    buf, body = _out(n, ho, wo, k, out_ld)
    _lib.call("diga_conv2d_nhwc_f32_opts", _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(body), n, hi, wi, c, x.stride(2), ho, wo, k,
              body.stride(2), r, s, 1, 1, off0[0], off0[1], 1, 1, ctypes.byref(_lib.ConvOptions(*opts)), _fwd_tag(), _lib.stream())
    return _result(buf, body, k)


# name: N, source H, W, Cin, Cout, R, S, pad_y, pad_x, reflect, bias, out_ld, in_ld.  Output tiles are 8 x 16; the interior blocks are 8 x 16
# SOURCE pixels of one phase, anchored at source pixel (4, 8).
CASES = {c[0]: c for c in [
    ("5x5_reflect_32to64", 1, 12, 24, 32, 64, 5, 5, 2, 2, 1, False, None, None),            # one interior tile: a partly filled interior block
    ("5x5_reflect_128to64", 2, 20, 40, 128, 64, 5, 5, 2, 2, 1, True, None, None),           # four chunks, 3 x 3 interior tiles, ragged interior blocks
    ("5x5_reflect_64to32_slice", 2, 13, 21, 64, 32, 5, 5, 2, 2, 1, False, 40, 96),          # in_ld 96, output pitch 40, odd sizes, ragged ring tiles
    ("5x5_zero_32to64_bias", 1, 12, 24, 32, 64, 5, 5, 2, 2, 0, True, None, None),           # zero padding
    ("5x5_reflect_256to128", 1, 12, 24, 256, 128, 5, 5, 2, 2, 1, False, None, None),        # two column tiles
    ("3x3_reflect_32to80", 1, 16, 24, 32, 80, 3, 3, 1, 1, 1, True, None, None),             # 2 x 2 collapsed taps, ragged column tile
    ("4x4_reflect_32to64", 1, 12, 24, 32, 64, 4, 4, 1, 1, 1, False, None, None),            # phases with different tap counts (3 and 2)
]}
_DATA = {}


def _data(name):
    """Seeded source tensor (NHWC inside its NaN-filled, guarded allocation; possibly a channel slice), [K,R,S,C] weights, bias and the
    geometry of one case: built once, never modified."""
    _, n, h, w, cin, cout, r, s, py, px, reflect, bias, out_ld, in_ld = CASES[name]
    if name not in _DATA:
        g = synth.gen(2000 + sorted(CASES).index(name))
        ld = in_ld or cin
        buf = torch.full(((n * h * w + 2 * GUARD) * ld,), float("nan"), dtype=torch.float32, device=DEV)
        body = buf[GUARD * ld:(GUARD + n * h * w) * ld].view(n, h, w, ld)
        x = body[..., 16:16 + cin] if in_ld else body
        x.copy_(torch.randn((n, h, w, cin), generator=g).to(DEV))
        wt = (torch.randn((cout, r, s, cin), generator=g) / (r * s * cin) ** 0.5).to(DEV)
        b = torch.randn(cout, generator=g).to(DEV) if bias else None
        assert x.data_ptr() % 16 == 0 and x.stride(2) == ld and bool(torch.isnan(buf[:GUARD * ld]).all())
        _DATA[name] = (x, wt, b, buf)
    x, wt, b, _ = _DATA[name]
    ho, wo = 2 * h + 2 * py - r + 1, 2 * w + 2 * px - s + 1
    return x, wt, b, ho, wo, (-py, -px), (reflect, 1, 0), out_ld


# ------------------------------------------------------------------------------------------------ 7. the collapsed weights
@pytest.mark.parametrize("r,s,py,px", [(5, 5, 2, 2), (3, 3, 1, 1), (4, 4, 1, 1), (5, 3, 2, 1)])
def test_collapsed_weights_equal_the_host_sum(r, s, py, px):
    em = _emulation()
    g = synth.gen(2050 + 10 * r + s)
    w = torch.randn((80, r, s, 32), generator=g) * torch.logspace(-3, 3, 32)             # (magnitudes that make the rounding visible)
    want, first = em.collapse_up2(w, -py, -px)
    got = _collapse(w.to(DEV), (-py, -px))
    torch.cuda.synchronize()
    assert got.shape == want.shape and first[0][0] == ((-py) // 2, (-px) // 2)
    assert torch.equal(got.cpu(), want), f"{int((got.cpu() != want).sum())} of {want.numel()} collapsed weights differ"
    if r == 4:                                                    # phase 1 has two taps: its third stays zero
        assert bool((got[1, :, :, 2] == 0).all()) and bool((got[:, 1, :, :, 2] == 0).all()) and not bool((got[0, 0, :, 2, 2] == 0).all())


# ------------------------------------------------------------------------------------------------ 8. bits
def _composite(name):
    """The output the new entry point must give, bit for bit, built from the window form alone."""
    em = _emulation()
    x, wt, b, ho, wo, off0, opts, out_ld = _data(name)
    n, hi, wi, _ = x.shape
    want = _window(x, wt, b, ho, wo, off0, opts, out_ld).clone()   # the ring tiles (and, for now, the interior)
    ty, tx = -(-ho // TH), -(-wo // TW)
    assert ty >= 3 and tx >= 3
    wc = _collapse(wt, off0)
    ys, xs = torch.arange(TH, (ty - 1) * TH, device=DEV), torch.arange(TW, (tx - 1) * TW, device=DEV)
    for fy in (0, 1):
        for fx in (0, 1):
            first = (em.up2_rows(wt.shape[1], off0[0], fy)[0], em.up2_rows(wt.shape[2], off0[1], fx)[0])
            src = _window(x, wc[fy, fx].contiguous(), b, hi, wi, first, None, out_ld)      # a stride-1 conv of the source image
            yy, xx = ys[(ys & 1) == fy], xs[(xs & 1) == fx]
            want[:, yy[:, None], xx[None, :]] = src[:, (yy >> 1)[:, None], (xx >> 1)[None, :]]
    return want


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_the_composite_of_window_calls(name):
    """Ring tiles run the window walk on the layer's own image: the window form's bits.  An interior pixel runs the window form's K-step
    sequence (chunk-major, the taps inside, the same six products and fold add) on its phase's collapsed weights and the same source
    pixels; a padded zero tap adds an exact zero.  So torch.equal, at every Cin."""
    x, wt, b, ho, wo, off0, opts, out_ld = _data(name)
    if CASES[name][13]:
        assert x.stride(2) == 96 > x.shape[3] and not x.is_contiguous()
    got = _up2(x, wt, b, ho, wo, off0, opts, out_ld)
    want = _composite(name)
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} elements differ, worst " \
                                   f"{float((got - want).abs().max()):.3g}"
    # the interior is not the window form's own interior (other products), or the test would prove nothing
    assert not torch.equal(got, _window(x, wt, b, ho, wo, off0, opts, out_ld))
    # deterministic
    assert torch.equal(got, _up2(x, wt, b, ho, wo, off0, opts, out_ld))


# ------------------------------------------------------------------------------------------------ 9. error
def _err(t, ref):
    return float((t.cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_error_against_float64(name):
    """The yardstick is float64 on the explicit interpolate + pad image; the form must meet the project's definition of fp32-equivalent:
    under 2e-6 of scale and within 1.5 x the error of the exact-fp32 `_opts` kernel on the same inputs.  Measured, up2 / x6win / fp32 of
    scale on the whole output (and on the interior tiles alone):
    5x5_reflect_32to64 3.32e-07 / 3.32e-07 / 8.53e-07 (1.53e-07 / 2.66e-07 / 8.30e-07);
    5x5_reflect_128to64 7.19e-07 / 7.19e-07 / 1.73e-06 (3.49e-07 / 6.95e-07 / 1.51e-06);
    5x5_reflect_64to32_slice 6.01e-07 / 6.01e-07 / 1.53e-06 (3.21e-07 / 4.39e-07 / 1.32e-06);
    5x5_zero_32to64_bias 2.64e-07 / 2.64e-07 / 7.91e-07 (1.17e-07 / 2.33e-07 / 6.55e-07);
    5x5_reflect_256to128 1.64e-06 / 1.64e-06 / 3.04e-06 (6.79e-07 / 9.82e-07 / 2.24e-06);
    3x3_reflect_32to80 1.76e-07 / 1.76e-07 / 5.62e-07 (1.03e-07 / 1.53e-07 / 5.62e-07);
    4x4_reflect_32to64 3.14e-07 / 3.14e-07 / 8.96e-07 (1.53e-07 / 3.14e-07 / 7.95e-07).
    The whole-output maxima of up2 and x6win coincide where the worst pixel lies in the ring, which both compute alike."""
    x, wt, b, ho, wo, off0, opts, out_ld = _data(name)
    _, n, h, w, cin, cout, r, s, py, px, reflect, *_ = CASES[name]
    t = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    t = F.pad(t, (px, px, py, py), mode="reflect" if reflect else "constant")
    ref = F.conv2d(t.double().cpu(), wt.permute(0, 3, 1, 2).double().cpu(), None if b is None else b.double().cpu()).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (n, ho, wo, cout)
    t_up2, t_win, t_f32 = (f(x, wt, b, ho, wo, off0, opts, out_ld) for f in (_up2, _window, _f32))
    e_up2, e_win, e_f32 = _err(t_up2, ref), _err(t_win, ref), _err(t_f32, ref)
    # ... and on the interior tiles alone (the pixels the collapsed weights compute), of the same scale
    inter = (slice(None), slice(TH, (-(-ho // TH) - 1) * TH), slice(TW, (-(-wo // TW) - 1) * TW))
    i_up2, i_win, i_f32 = (float((t[inter].cpu().double() - ref[inter]).abs().max() / ref.abs().max()) for t in (t_up2, t_win, t_f32))
    print(f"{name}: error against float64, of scale: up2 {e_up2:.2e}, x6win {e_win:.2e}, fp32 {e_f32:.2e}; "
          f"interior tiles alone: up2 {i_up2:.2e}, x6win {i_win:.2e}, fp32 {i_f32:.2e}")
    assert e_up2 <= 2e-6, e_up2
    assert e_up2 <= 1.5 * e_f32, (e_up2, e_f32)


# ------------------------------------------------------------------------------------------------ 10. the translator
X6 = dict(conv_math=2, x6_split="loader", x6_taps=True, x6_winograd=True, x6_opts=True, x6_window=True)


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


def test_translator_decoder_runs_on_the_collapsed_form(golden):
    from diga_amd.model.model_noaux import ImgDecoder, ImgEncoder
    g = golden("translator")
    enc, dec = _filled(ImgEncoder, "enc").to(DEV), _filled(ImgDecoder, "dec").to(DEV)
    x = g.t("x").to(DEV)
    feat, rec, log, calls = _translate(enc, dec, x, **X6, x6_up2=True)
    assert list(feat.shape) == g["feat_shape"].tolist()
    assert_close(rec, g.t("rec"), 1e-3, 1e-4, "translated image")
    # the two upsampled 5x5 decoder layers on the collapsed form; the 7x7 on the window form, the stem, the two strided 4x4 layers and the
    # 16 ResBlock convs where they were
    assert log == {("fwd", "bf16x6/up2"): 2, ("fwd", "bf16x6/window"): 1, ("fwd", "bf16x6/taps"): 2, ("fwd", "bf16x6/ls"): 1,
                   ("fwd", "winograd/x6"): 16}, log
    assert calls.count("diga_conv_up2_bf16x6_f32in") == 2 and calls.count("diga_conv_window_bf16x6_f32in") == 1, calls
    assert calls.count("diga_collapse_up2_weights") == 2 and calls.count("diga_conv_taps_bf16x6_f32in_opts") == 2

    # the switch off = the switch absent: same launches, same bits
    feat0, rec0, log0, calls0 = _translate(enc, dec, x, **X6)
    feat1, rec1, log1, calls1 = _translate(enc, dec, x, **X6, x6_up2=False)
    assert log1 == {("fwd", "bf16x6/ls"): 1, ("fwd", "bf16x6/taps"): 2, ("fwd", "bf16x6/window"): 3, ("fwd", "winograd/x6"): 16}, log1
    assert "diga_conv_up2_bf16x6_f32in" not in calls1 and "diga_collapse_up2_weights" not in calls1
    if not config.DEFAULTS.x6_up2:
        assert log0 == log1 and calls0 == calls1 and torch.equal(rec0, rec1) and torch.equal(feat0, feat1)
    assert_close(rec1, g.t("rec"), 1e-3, 1e-4, "translated image, x6_up2 off")
    assert torch.equal(feat1, feat)                               # (the encoder has no admitted layer)
    assert not torch.equal(rec1, rec)                             # (the switch does select other products)

    # flipped between passes of one model, in both directions: each pass is the pass of its setting
    _, rec_on, log_on, calls_on = _translate(enc, dec, x, **X6, x6_up2=True)
    _, rec_off, log_off, calls_off = _translate(enc, dec, x, **X6, x6_up2=False)
    assert log_on == log and calls_on == calls and torch.equal(rec_on, rec)
    assert log_off == log1 and calls_off == calls1 and torch.equal(rec_off, rec1)
    # and outside conv_math = 2 the switch selects nothing
    _, rec_f0, log_f0, calls_f0 = _translate(enc, dec, x, conv_math=0)
    _, rec_f1, log_f1, calls_f1 = _translate(enc, dec, x, conv_math=0, x6_taps=True, x6_opts=True, x6_window=True, x6_up2=True)
    assert log_f0 == log_f1 and calls_f0 == calls_f1 and torch.equal(rec_f0, rec_f1)
    print(f"translator: rec error against the capture {float((rec.cpu() - g.t('rec')).abs().max()):.2e} (x6_up2 on), "
          f"{float((rec1.cpu() - g.t('rec')).abs().max()):.2e} (off)")
