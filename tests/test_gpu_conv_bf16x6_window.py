"""GPU tests of the window form of the multi-tap bf16x6 forward (config.x6_window under conv_math = 2 with x6_taps; csrc/conv_bf16x6.h:
conv_win_x6_kernel, diga_conv_window_bf16x6_f32in; model/conv.py: the "x6win" family).

  6. Cin = 32, where the chunk-major K-step order is the tap-major one: torch.equal to diga_conv_taps_bf16x6_f32in[_opts];
  7. several chunks: against float64 next to the existing multi-tap bf16x6 kernel and the exact-fp32 `_opts` kernel;
  8. tanh against float64 tanh of the kernel's own pre-activation;
  9. through DigaConv2d and the frozen translator: the paths taken, the switch off = the switch absent, flipped in both directions.

Every input lies inside a NaN-filled allocation with guard pixels in front and behind (once as a channel slice of pitch 96), every output
is a slice of a NaN-filled buffer: a read outside the image shows up as a NaN in the result, a write outside the slice as a number there."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from diga_amd import config

from conftest import assert_close
from oracle import synth
from test_translator import _filled

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                       # NaN pixels in front of and behind every input


@pytest.fixture(autouse=True)
def _leave_global_rng_and_arithmetic_untouched():
    """As tests/test_gpu_conv_bf16x6_opts.py: every test hands torch's generators, the conv arithmetic and conv.path_log back as it
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
    return torch.full((n, ho, wo, out_ld or k), float("nan"), dtype=torch.float32, device=DEV)


def _result(buf, k):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[..., k:]).all()), "the kernel wrote past Cout"
    assert not bool(torch.isnan(buf[..., :k]).any()), "NaN in the result: a read outside the image, or an output never written"
    return buf[..., :k]


def _window(x, w, bias, ho, wo, off0, dil, opts=None, out_ld=None):
    """diga_conv_window_bf16x6_f32in on x [N,Hi,Wi,C] (dense, or a channel slice) and w [K,R,S,C] -> out [N,Ho,Wo,K]."""
    from diga_amd import _lib
    n, hi, wi, c = x.shape
    k, r, s, _ = w.shape
    buf, img = _out(n, ho, wo, k, out_ld), _image(w)
    _lib.call("diga_conv_window_bf16x6_f32in", _lib.ptr(x), x.stride(2), _lib.ptr(img), _lib.ptr(bias), _lib.ptr(buf), n, hi, wi, c, ho, wo, k,
              buf.stride(2), r, s, off0, off0, dil, dil, None if opts is None else ctypes.byref(_lib.ConvOptions(*opts)), _fwd_tag(),
              _lib.stream())
    return _result(buf, k)


def _taps(x, w, bias, ho, wo, off0, dil, opts=None, out_ld=None):
    """The existing multi-tap kernel: diga_conv_taps_bf16x6_f32in (opts None) or its `_opts` form, stride 1."""
    from diga_amd import _lib
    n, hi, wi, c = x.shape
    k, r, s, _ = w.shape
    buf, img = _out(n, ho, wo, k, out_ld), _image(w)
    name = "diga_conv_taps_bf16x6_f32in" + ("" if opts is None else "_opts")
    tail = [None] + ([] if opts is None else [ctypes.byref(_lib.ConvOptions(*opts))])
    _lib.call(name, _lib.ptr(x), x.stride(2), _lib.ptr(img), _lib.ptr(bias), _lib.ptr(buf), n, hi, wi, c, ho, wo, k, buf.stride(2), r, s, 1, 1,
              off0, off0, dil, dil, *tail, _fwd_tag(), _lib.stream())
    return _result(buf, k)


def _f32(x, w, bias, ho, wo, off0, dil, opts, out_ld=None):
    """The exact-fp32 kernel with the folded map: diga_conv2d_nhwc_f32_opts."""
    from diga_amd import _lib
    n, hi, wi, c = x.shape
    k, r, s, _ = w.shape
    buf = _out(n, ho, wo, k, out_ld)
    _lib.call("diga_conv2d_nhwc_f32_opts", _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(buf), n, hi, wi, c, x.stride(2), ho, wo, k,
              buf.stride(2), r, s, 1, 1, off0, off0, dil, dil, ctypes.byref(_lib.ConvOptions(*opts)), _fwd_tag(), _lib.stream())
    return _result(buf, k)


def _explicit(x, shift, pad, reflect):
    """The image the folded kernel reads, built with torch: nearest upsampling by 2^shift, then the padding.  x NHWC -> NHWC, copies only."""
    t = x.permute(0, 3, 1, 2)
    if shift:
        t = F.interpolate(t, scale_factor=float(1 << shift), mode="nearest")
    t = F.pad(t, (pad, pad, pad, pad), mode="reflect" if reflect else "constant")
    return t.permute(0, 2, 3, 1).contiguous()


# name, N, source H, W, Cin, Cout, k, pad, dilation, reflect, shift, bias, out_ld, in_ld, options given.  The tile is 8 x 16 output pixels:
# every case but the 4 x 5 one has more than one tile in both directions and ragged last tiles in both (no output extent is a multiple
# of 8, so the last tiles are ragged for any tile of 128 or 256 pixels), 2 or 3 images but one, and under reflection both mirrors
CASES = {c[0]: c for c in [
    # 6. Cin = 32: one chunk, so chunk-major = tap-major
    ("7x7_reflect_32to3_pitch7", 2, 13, 37, 32, 3, 7, 3, 1, 1, 0, True, 7, None, True),
    ("5x5_reflect_up1_32to64", 2, 9, 11, 32, 64, 5, 2, 1, 1, 1, True, None, None, True),                 # logical 18 x 22
    ("3x3_zero_dil2_32to16_bias", 3, 17, 35, 32, 16, 3, 2, 2, 0, 0, True, None, None, False),            # no options: against `_f32in`
    ("3x3_reflect_32to80_4x5", 1, 4, 5, 32, 80, 3, 1, 1, 1, 0, True, None, None, True),                  # two column tiles; both mirrors in one tile
    ("3x3_all_options_zero", 2, 13, 21, 32, 64, 3, 1, 1, 0, 0, True, None, None, True),
    ("5x5_zero_up1_32to16_slice", 2, 9, 11, 32, 16, 5, 2, 1, 0, 1, False, 20, 96, True),                  # zero padding through the map, in_ld 96
    # 7. several chunks
    ("7x7_reflect_64to3", 3, 19, 21, 64, 3, 7, 3, 1, 1, 0, True, None, None, True),
    ("5x5_reflect_up1_128to64", 2, 9, 11, 128, 64, 5, 2, 1, 1, 1, True, None, None, True),
    ("5x5_reflect_up1_256to128", 1, 7, 9, 256, 128, 5, 2, 1, 1, 1, True, None, None, True),
    ("5x5_reflect_up1_64to32_slice", 2, 11, 9, 64, 32, 5, 2, 1, 1, 1, False, None, 96, True),            # in_ld 96 > Cin
]}
ONE_CHUNK = [n for n, c in CASES.items() if c[4] == 32]
CHUNKS = [n for n, c in CASES.items() if c[4] > 32]
_DATA = {}


def _data(name):
    """Seeded source tensor (NHWC inside its NaN-filled, guarded allocation; possibly a channel slice), [K,R,S,C] weights, bias and the
    geometry of one case: built once, never modified."""
    _, n, h, w, cin, cout, k, pad, dil, reflect, shift, bias, out_ld, in_ld, with_opts = CASES[name]
    if name not in _DATA:
        g = synth.gen(1900 + len(_DATA))
        ld = in_ld or cin
        buf = torch.full(((n * h * w + 2 * GUARD) * ld,), float("nan"), dtype=torch.float32, device=DEV)
        body = buf[GUARD * ld:(GUARD + n * h * w) * ld].view(n, h, w, ld)
        x = body[..., 16:16 + cin] if in_ld else body
        x.copy_(torch.randn((n, h, w, cin), generator=g).to(DEV))
        wt = (torch.randn((cout, k, k, cin), generator=g) / (k * k * cin) ** 0.5).to(DEV)
        b = torch.randn(cout, generator=g).to(DEV) if bias else None
        assert x.data_ptr() % 16 == 0 and x.stride(2) == ld and bool(torch.isnan(buf[:GUARD * ld]).all())
        _DATA[name] = (x, wt, b, buf)
    x, wt, b, _ = _DATA[name]
    ho, wo = (((v << shift) + 2 * pad - dil * (k - 1) - 1) + 1 for v in (h, w))
    return x, wt, b, ho, wo, -pad, dil, ((reflect, shift, 0) if with_opts else None), out_ld


# ------------------------------------------------------------------------------------------------ 6. one chunk: bit for bit
@pytest.mark.parametrize("name", ONE_CHUNK)
def test_one_chunk_equals_the_multi_tap_kernel(name):
    """At Cin = 32 a 16 x 16 sub-tile of the window form sees the fragments and the MFMA sequence of conv_fwd_x6_kernel<..., TAPS>: same
    weight image, same planes (split3x4 of the same pixels), K-steps in tap order, the fold add per K-step, the same drain expressions;
    taps that kernel steps over for a tile add exact zeros to a +0 start here.  So torch.equal -- on the same tensors."""
    x, wt, b, ho, wo, off0, dil, opts, out_ld = _data(name)
    n = x.shape[0]
    if name != "3x3_reflect_32to80_4x5":
        assert ho > 8 and wo > 16 and ho % 8 and wo % 8 and n > 1, (ho, wo)
    want = _taps(x, wt, b, ho, wo, off0, dil, opts, out_ld)
    got = _window(x, wt, b, ho, wo, off0, dil, opts, out_ld)
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} elements differ, worst " \
                                   f"{float((got - want).abs().max()):.3g}"
    if opts is not None and not any(opts):                        # all options zero = no options
        assert torch.equal(got, _window(x, wt, b, ho, wo, off0, dil, None, out_ld))


# ------------------------------------------------------------------------------------------------ 7. several chunks
def _err(t, ref):
    return float((t.cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("name", CHUNKS)
def test_several_chunks_against_float64(name):
    """Chunk-major K-steps reassociate the sum across chunks, so the yardstick is float64 on the explicit interpolate + pad image: the
    window form stays under the multi-tap bound of tests/test_gpu_conv_bf16x6_opts.py (2e-6 of scale) and within 1.5 x the error of the
    exact-fp32 kernel on the same inputs (VERDICT item 1's "fp32-equivalent").  Measured, window / x6rs / fp32 (of scale):
    7x7 64 -> 3: 5.97e-7 / 6.31e-7 / 1.69e-6; 5x5 128 -> 64: 1.11e-6 / 6.89e-7 / 1.74e-6; 5x5 256 -> 128: 1.04e-6 / 1.07e-6 / 2.08e-6;
    5x5 64 -> 32 as a channel slice: 6.19e-7 / 5.47e-7 / 1.50e-6."""
    x, wt, b, ho, wo, off0, dil, opts, out_ld = _data(name)
    _, n, h, w, cin, cout, k, pad, _, reflect, shift, *_ = CASES[name]
    if CASES[name][13]:
        assert x.stride(2) == 96 > cin and not x.is_contiguous()
    big = _explicit(x, shift, pad, reflect)
    ref = F.conv2d(big.permute(0, 3, 1, 2).double().cpu(), wt.permute(0, 3, 1, 2).double().cpu(), None if b is None else b.double().cpu(),
                   dilation=dil).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (n, ho, wo, cout)
    e_win = _err(_window(x, wt, b, ho, wo, off0, dil, opts, out_ld), ref)
    e_taps = _err(_taps(x, wt, b, ho, wo, off0, dil, opts, out_ld), ref)
    e_f32 = _err(_f32(x, wt, b, ho, wo, off0, dil, opts, out_ld), ref)
    print(f"{name}: error against float64, of scale: window {e_win:.2e}, x6rs {e_taps:.2e}, fp32 {e_f32:.2e}")
    assert e_win < 2e-6, e_win
    assert e_win <= 1.5 * e_f32, (e_win, e_f32)


# ------------------------------------------------------------------------------------------------ 8. tanh
def test_tanh_against_float64_and_the_fp32_kernel():
    """activation = 1 against float64 tanh of the SAME entry point's activation = 0 output, for the window form and for
    diga_conv2d_nhwc_f32_opts (the same tanhf expression: the yardstick).  The pre-activations differ in their last bits, so the window
    form's deviation may be at most twice the fp32 kernel's: the criterion of tests/test_gpu_conv_bf16x6_opts.py."""
    x, wt, b, ho, wo, off0, dil, opts, out_ld = _data("7x7_reflect_64to3")

    def dev(run):
        pre, post = run(0), run(1)
        assert float(pre.abs().max()) > 1.0                       # (the pre-activations reach tanh's curved part)
        return float((post.cpu().double() - torch.tanh(pre.cpu().double())).abs().max())

    d_win = dev(lambda act: _window(x, wt, b, ho, wo, off0, dil, (opts[0], opts[1], act), out_ld))
    d_f32 = dev(lambda act: _f32(x, wt, b, ho, wo, off0, dil, (opts[0], opts[1], act), out_ld))
    print(f"tanh deviation from float64 tanh of the kernel's own pre-activation: window {d_win:.3e}, fp32 `_opts` {d_f32:.3e}")
    assert d_win <= 2.0 * d_f32, (d_win, d_f32)


# ------------------------------------------------------------------------------------------------ 9. the layer and the translator
X6 = dict(conv_math=2, x6_split="loader", x6_taps=True, x6_winograd=True, x6_opts=True)


def test_layer_logs_the_window_path_and_equals_the_entry_point():
    from diga_amd.model import conv as dc
    from diga_amd.model.conv import DigaConv2d
    g = synth.gen(1990)
    x = torch.randn((2, 64, 13, 21), generator=g)
    w = torch.randn((3, 64, 7, 7), generator=g) / (49 * 64) ** 0.5
    b = torch.randn(3, generator=g)
    m = DigaConv2d(64, 3, 7, 1, padding=3, bias=True)
    m.load_state_dict({"weight": w, "bias": b})
    m = m.to(DEV).eval()
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    outs = {}
    for on in (True, False):
        with config.override(**X6, x6_window=on), torch.no_grad():
            dc.path_log = {}
            outs[on] = m(xd, opts=(1, 0, 1))
            torch.cuda.synchronize()
            assert dc.path_log == {("fwd", "bf16x6/window" if on else "bf16x6/taps"): 1}, dc.path_log
    direct = _window(xd.permute(0, 2, 3, 1), w.permute(0, 2, 3, 1).contiguous().to(DEV), b.to(DEV), 13, 21, -3, 1, (1, 0, 1))
    assert torch.equal(outs[True].permute(0, 2, 3, 1), direct)
    assert not torch.equal(outs[True], outs[False])               # (two chunks: another summation order)


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


def test_translator_decoder_runs_on_the_window_form(golden):
    from diga_amd.model.model_noaux import ImgDecoder, ImgEncoder
    g = golden("translator")
    enc, dec = _filled(ImgEncoder, "enc").to(DEV), _filled(ImgDecoder, "dec").to(DEV)
    x = g.t("x").to(DEV)
    feat, rec, log, calls = _translate(enc, dec, x, **X6, x6_window=True)
    assert list(feat.shape) == g["feat_shape"].tolist()
    assert synth.checksum(feat.detach().cpu()) == pytest.approx(float(g["feat_sum"]), rel=1e-3, abs=1e-2)
    assert_close(rec, g.t("rec"), 1e-3, 1e-4, "translated image")
    # the three stride-1 multi-tap decoder layers on the window form; the stem, the two strided 4x4 layers and the 16 ResBlock convs
    # where they were
    assert log == {("fwd", "bf16x6/ls"): 1, ("fwd", "bf16x6/taps"): 2, ("fwd", "bf16x6/window"): 3, ("fwd", "winograd/x6"): 16}, log
    assert calls.count("diga_conv_window_bf16x6_f32in") == 3 and calls.count("diga_conv_taps_bf16x6_f32in_opts") == 2, calls
    assert calls.count("diga_conv_winograd_bf16x6_opts") == 16

    # the switch off = the switch absent: same launches, same bits
    feat0, rec0, log0, calls0 = _translate(enc, dec, x, **X6)
    feat1, rec1, log1, calls1 = _translate(enc, dec, x, **X6, x6_window=False)
    assert log1 == {("fwd", "bf16x6/ls"): 1, ("fwd", "bf16x6/taps"): 5, ("fwd", "winograd/x6"): 16}, log1
    assert "diga_conv_window_bf16x6_f32in" not in calls1
    if not config.DEFAULTS.x6_window:
        assert log0 == log1 and calls0 == calls1 and torch.equal(rec0, rec1) and torch.equal(feat0, feat1)
    assert_close(rec1, g.t("rec"), 1e-3, 1e-4, "translated image, x6_window off")
    assert torch.equal(feat1, feat)                               # (the encoder has no admitted layer)
    assert not torch.equal(rec1, rec)                             # (the switch does select another summation order)

    # flipped between passes of one model, in both directions: each pass is the pass of its setting
    _, rec_on, log_on, calls_on = _translate(enc, dec, x, **X6, x6_window=True)
    _, rec_off, log_off, calls_off = _translate(enc, dec, x, **X6, x6_window=False)
    assert log_on == log and calls_on == calls and torch.equal(rec_on, rec)
    assert log_off == log1 and calls_off == calls1 and torch.equal(rec_off, rec1)
    # and outside conv_math = 2 the switch selects nothing
    _, rec_f0, log_f0, calls_f0 = _translate(enc, dec, x, conv_math=0)
    _, rec_f1, log_f1, calls_f1 = _translate(enc, dec, x, conv_math=0, x6_taps=True, x6_opts=True, x6_window=True)
    assert log_f0 == log_f1 and calls_f0 == calls_f1 and torch.equal(rec_f0, rec_f1)
    print(f"translator: rec error against the capture {float((rec.cpu() - g.t('rec')).abs().max()):.2e} (x6_window on), "
          f"{float((rec1.cpu() - g.t('rec')).abs().max()):.2e} (off)")
