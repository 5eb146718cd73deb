"""Eval-mode BatchNorm (+ residual, + ReLU) folded into the bf16x6 convolutions (config.fold_eval_bn_x6 under conv_math = 2:
diga_infer_conv2d_nhwc_bf16x6 / _f32in / diga_infer_conv2d_winograd_bf16x6).

The INF instantiations of conv_fwd_x6_kernel differ from the plain ones in the drain of the staged tile only, and the Winograd form
is the plain batched bf16x6 GEMM followed by the output transform with the epilogue, so every comparison with the unfolded path -- the
plain `_bf16x6[_f32in]` / diga_conv2d_winograd_bf16x6 call followed by diga_bn_fwd(training = 0) -- is torch.equal.  Each kernel-level
case is also held to float64 with the bound formula of tests/test_gpu_infer_fold.py (_check_forms) and the convolution bounds the
project already uses: 2e-6 of scale for the bf16x6 pointwise forward (tests/test_gpu_conv_bf16x6.py), conftest.WINO_TOL for the tile.

Inputs come from local torch.Generators; torch's global RNG state is not touched.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import WINO_TOL
from test_gpu_infer_fold import (EPS, _bn_entries, _bn_eval, _bn_params, _check_forms, _coefficients, _conv_f64,
                                 _epilogue, _fill, _inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
X6_TOL = 2e-6                      # of the output scale: the bf16x6 pointwise forward against float64 (tests/test_gpu_conv_bf16x6.py)
SPLITS = ["pass", "loader"]
X6_INFER = ("diga_infer_conv2d_nhwc_bf16x6", "diga_infer_conv2d_nhwc_bf16x6_f32in", "diga_infer_conv2d_winograd_bf16x6")


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """As tests/test_gpu_infer_fold.py: the shared blocks and models go with this file, the library's scratch buffers return to the
    ones it held before, and the caching allocator gives back what became free."""
    import gc
    from diga_amd import _lib
    saved = dict(_lib._workspaces)
    yield
    _block.cache_clear()
    _tiny.cache_clear()
    _lib._workspaces.clear()
    _lib._workspaces.update(saved)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _tag():
    from diga_amd import _lib
    return _lib.PROF_TAGS.index("conv_fwd")


# ---------------------------------------------------------------------------------------------------------------- kernel level
def _image(w):
    """diga_split_bf16x6_image of [Cout,1,1,Cin] weights."""
    from diga_amd import _lib
    cout, _, _, cin = w.shape
    img = torch.empty(_lib.lib.diga_split_bf16x6_image_bytes(cout, 1, cin), dtype=torch.uint8, device=DEV)
    _lib.call("diga_split_bf16x6_image", _lib.ptr(w), _lib.ptr(img), cout, 1, cin, _lib.stream())
    return img


def _pointwise(split, x, w, bias, stride, epi=None, out=None):
    """x [N,H,W,Cin] (dense or a channel slice of a wider NHWC buffer), w [Cout,1,1,Cin] -> [N,Ho,Wo,Cout] on diga_conv2d_nhwc_bf16x6 /
    _f32in (epi None) or their `_infer` forms.  out: write there (dense or a channel slice) instead of a fresh NaN-filled tensor."""
    from diga_amd import _lib
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    if out is None:
        out = torch.full((n, ho, wo, cout), float("nan"), dtype=torch.float32, device=DEV)
    assert tuple(out.shape) == (n, ho, wo, cout) and out.stride(3) == 1 and x.stride(3) == 1
    img = _image(w)
    if split == "pass":
        trip = torch.empty(n * h * wd * cin * 6, dtype=torch.uint8, device=DEV)
        _lib.call("diga_make_triplet", _lib.ptr(x), x.stride(2), _lib.ptr(trip), n * h * wd, cin, _lib.stream())
        name, lead = "diga_conv2d_nhwc_bf16x6", [_lib.ptr(trip)]
    else:
        name, lead = "diga_conv2d_nhwc_bf16x6_f32in", [_lib.ptr(x), x.stride(2)]
    args = lead + [_lib.ptr(img), _lib.ptr(bias), _lib.ptr(out), n, h, wd, cin, ho, wo, cout, out.stride(2), 1, 1, stride, stride, 0, 0, 1, 1]
    if epi is None:
        _lib.call(name, *args, None, _tag(), _lib.stream())
    else:
        _lib.call(name.replace("diga_conv2d_", "diga_infer_conv2d_"), *args, ctypes.byref(epi), _tag(), _lib.stream())
    return out


# name, x shape (NHWC), Cout, stride -- the smallest shapes at which the drain of the 256 x (64 TN) tile can go wrong
POINTWISE = [
    ("M63_32_64", (1, 7, 9, 32), 64, 1),              # one K-step, TN = 1, the second 128-row half of the tile inactive
    ("M2046_96_256", (2, 33, 31, 96), 256, 1),        # last row tile ragged in its second half, two column tiles
    ("M260_64_320", (1, 20, 13, 64), 320, 1),         # ragged last column tile, 4 live rows in the second row tile
    ("M260_64_68", (1, 20, 13, 64), 68, 1),           # ... one column tile of which 4 columns are live past the first 64
    ("s2_128_512", (2, 17, 15, 128), 512, 2),         # the downsample form
]


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", POINTWISE, ids=[c[0] for c in POINTWISE])
def test_pointwise_infer_epilogue(case, split, with_bias):
    name, xs, cout, stride = case
    g, x, w, bias, bn = _inputs(len(name) * 11 + cout, xs, (cout, 1, 1, xs[3]))
    b = bias if with_bias else None
    y64 = _conv_f64(x, w, b, stride, 0, 1)
    res = torch.randn(tuple(y64.shape), generator=g).to(DEV)
    _check_forms(f"{name} {split}", lambda e: _pointwise(split, x, w, b, stride, e), y64, bn, res, X6_TOL)


def _reference(y64, bn, res, relu):
    gamma, beta, mean, var = (t.double() for t in bn)
    a64 = gamma / torch.sqrt(var + EPS)
    ref = y64 * a64 + (beta - mean * a64)
    if res is not None:
        ref = ref + res.double()
    return (ref.clamp_min(0.0) if relu else ref), float(a64.abs().max())


def _within_bound(got, y64, bn, res, relu, conv_tol):
    ref, amax = _reference(y64, bn, res, relu)
    err = (got.double() - ref).abs()
    bound = conv_tol * float(y64.abs().max()) * amax + 1e-6 * float(ref.abs().max()) + 1e-5 * ref.abs()
    return bool((err <= bound).all()), float(err.max())


@pytest.mark.parametrize("split", SPLITS)
def test_pointwise_residual_at_a_pitch_above_cout(split):
    """The residual as a channel slice of a wider NHWC buffer (residual_ld = 96 > Cout = 68), ragged rows and columns."""
    g, x, w, bias, bn = _inputs(41, (1, 20, 13, 64), (68, 1, 1, 64))
    wide = torch.randn((1, 20, 13, 96), generator=g).to(DEV)
    res = wide[..., 12:80]
    assert res.data_ptr() % 16 == 0 and res.stride(2) == 96
    raw = _pointwise(split, x, w, bias, 1)
    want = _bn_eval(raw, bn, res.contiguous(), True)
    ab = _coefficients(bn)                                                    # (the descriptor holds a bare pointer: keep the tensor)
    got = _pointwise(split, x, w, bias, 1, _epilogue(ab, res, True, residual_ld=96))
    assert torch.equal(got, want), int((got != want).sum())
    ok, err = _within_bound(got, _conv_f64(x, w, bias, 1, 0, 1), bn, res, True, X6_TOL)
    assert ok, err


@pytest.mark.parametrize("split", SPLITS)
def test_pointwise_input_and_output_as_channel_slices(split):
    """Input channels 32..127 of a 160-channel buffer, output into channels 8..263 of a 272-channel buffer: every other float of the
    output buffer keeps its NaN."""
    g, _, w, bias, bn = _inputs(43, (1, 1, 1, 96), (256, 1, 1, 96))
    xw = (torch.randn((2, 11, 9, 160), generator=g) + 0.25).to(DEV)
    x = xw[..., 32:128]
    res = torch.randn((2, 11, 9, 256), generator=g).to(DEV)
    raw = _pointwise(split, x, w, bias, 1)
    assert torch.equal(raw, _pointwise(split, x.contiguous(), w, bias, 1))
    want = _bn_eval(raw, bn, res, True)
    ow = torch.full((2, 11, 9, 272), float("nan"), dtype=torch.float32, device=DEV)
    ab = _coefficients(bn)
    _pointwise(split, x, w, bias, 1, _epilogue(ab, res, True), out=ow[..., 8:264])
    assert torch.equal(ow[..., 8:264], want)
    assert bool(torch.isnan(ow[..., :8]).all()) and bool(torch.isnan(ow[..., 264:]).all())
    ok, err = _within_bound(ow[..., 8:264], _conv_f64(x.contiguous(), w, bias, 1, 0, 1), bn, res, True, X6_TOL)
    assert ok, err


def _winograd_x6(x, w, bias, d, tile, epi=None):
    from diga_amd import _lib
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    out = torch.full((n, h, wd, cout), float("nan"), dtype=torch.float32, device=DEV)
    nbytes = _lib.lib.diga_conv2d_winograd_bf16x6_workspace_bytes(n, h, wd, cin, cout, d, tile)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    if epi is None:
        _lib.call("diga_conv2d_winograd_bf16x6", _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), None, _lib.ptr(ws), ws.numel(),
                  n, h, wd, cin, cin, cout, cout, d, tile, 0, None, None, None, _tag(), _lib.stream())
    else:
        _lib.call("diga_infer_conv2d_winograd_bf16x6", _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                  n, h, wd, cin, cin, cout, cout, d, tile, ctypes.byref(epi), None, _tag(), _lib.stream())
    return out


WINO = [(tile, xs, cout, d) for tile in (4, 6) for xs, cout, d in (((1, 13, 11, 128), 128, 1), ((2, 12, 12, 128), 256, 2))]


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", WINO, ids=[f"tile{t}_{xs[1]}x{xs[2]}_{xs[3]}_{co}_d{d}" for t, xs, co, d in WINO])
def test_winograd_x6_infer_epilogue(case, with_bias):
    tile, xs, cout, d = case
    g, x, w, bias, bn = _inputs(10 * tile + d + cout, xs, (cout, 3, 3, xs[3]))
    b = bias if with_bias else None
    y64 = _conv_f64(x, w, b, 1, d, d)
    res = torch.randn(tuple(y64.shape), generator=g).to(DEV)
    _check_forms(f"winograd/x6 tile {tile} d {d} {xs[3]}->{cout}", lambda e: _winograd_x6(x, w, b, d, tile, e), y64, bn, res, WINO_TOL[tile][0])


def test_a_refused_call_launches_nothing():
    """The descriptor is checked before anything is enqueued: the NaN-filled output of a refused call stays as it was."""
    from diga_amd import _lib
    g, x, w, bias, bn = _inputs(3, (1, 7, 9, 32), (64, 1, 1, 32))
    ab = _coefficients(bn)
    res = torch.randn((63 * 64 + 4,), generator=g).to(DEV)
    bad = _epilogue(ab, res[1:-3].view(1, 7, 9, 64), True)                    # 4 bytes off a 16-byte boundary
    for split in SPLITS:
        with pytest.raises(RuntimeError, match="code -1"):
            _pointwise(split, x, w, None, 1, bad)
        out = torch.full((1, 7, 9, 64), float("nan"), dtype=torch.float32, device=DEV)
        with pytest.raises(RuntimeError, match="code -1"):
            _pointwise(split, x, w, None, 1, _epilogue(None, None, True), out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and _lib.last_error() != ""
    xw = torch.randn((1, 12, 12, 128), generator=g).to(DEV)
    ww = torch.randn((128, 3, 3, 128), generator=g).to(DEV)
    ab128 = _coefficients(_bn_params(128, g))
    for tile, e in ((2, _epilogue(ab128, None, False)), (4, _epilogue(None, None, False))):
        with pytest.raises(RuntimeError, match="code -1"):
            _winograd_x6(xw, ww, None, 1, tile, e)


# ---------------------------------------------------------------------------------------------------------------- module level
# name: inplanes, planes, stride, dilation, input N, H, W (both with a downsample branch)
BLOCKS = {
    "s2_down": (256, 64, 2, 1, 2, 19, 17),             # conv2 64 -> 64: a direct fp32 kernel
    "d2_wino": (512, 128, 1, 2, 1, 17, 19),            # conv2 128 -> 128, dilation 2: Winograd
}


@functools.lru_cache(maxsize=None)
def _block(name):
    """(block in eval mode, input): built once per shape and shared by the tests below, which leave it unchanged."""
    from diga_amd.model import conv as dc
    from diga_amd.model import seg_model_noaux as sm
    inpl, planes, stride, dil, n, h, w = BLOCKS[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 6)
    ds = nn.Sequential(dc.DigaConv2d(inpl, planes * 4, 1, stride=stride, bias=False), sm._frozen_bn(planes * 4))
    blk = sm.Bottleneck(inpl, planes, stride, dilation=dil, downsample=ds)
    _fill(blk, g)
    blk = blk.to(DEV).eval()
    x = torch.randn((n, inpl, h, w), generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    return blk, x


def _run(blk, x, fold, fold_x6, grad=False, **cfg):
    """(output, path_log) of blk(x) in mode 2 under config.override(fold_eval_bn=fold, fold_eval_bn_x6=fold_x6, **cfg)."""
    from diga_amd import config
    from diga_amd.model import conv as dc
    dc.path_log = {}
    try:
        with config.override(conv_math=2, fold_eval_bn=fold, fold_eval_bn_x6=fold_x6, **cfg), torch.set_grad_enabled(grad):
            y = blk(x)
        return y, dc.path_log
    finally:
        dc.path_log = None


@pytest.mark.parametrize("split", SPLITS)
def test_strided_bottleneck_folded_equals_unfolded(split):
    blk, x = _block("s2_down")
    x6 = "bf16x6/ls" if split == "loader" else "bf16x6"
    off, log_off = _run(blk, x, False, True, x6_split=split)                 # (the new switch alone folds nothing)
    assert log_off == {("fwd", x6): 3, ("fwd", "f32"): 1}, log_off
    on, log_on = _run(blk, x, True, True, x6_split=split)
    assert torch.equal(on, off), int((on != off).sum())
    assert log_on == {("fwd", x6 + "+bn"): 3, ("fwd", "f32+bn"): 1}, log_on  # conv1 (stride 2), conv3 + skip, downsample; conv2
    # the new switch off: what the parent commit runs under fold_eval_bn in mode 2 -- the pointwise sites keep their BatchNorm
    old, log_old = _run(blk, x, True, False, x6_split=split)
    assert torch.equal(old, off) and log_old == {("fwd", x6): 3, ("fwd", "f32+bn"): 1}, log_old


@pytest.mark.parametrize("wino_x6", [False, True], ids=["wino_f32", "wino_x6"])
@pytest.mark.parametrize("split", SPLITS)
def test_dilated_bottleneck_folded_equals_unfolded(split, wino_x6):
    blk, x = _block("d2_wino")
    x6 = "bf16x6/ls" if split == "loader" else "bf16x6"
    cfg = dict(x6_split=split, x6_winograd=wino_x6)
    off, log_off = _run(blk, x, False, False, **cfg)
    assert log_off == {("fwd", x6): 3, ("fwd", "winograd/x6" if wino_x6 else "winograd"): 1}, log_off
    on, log_on = _run(blk, x, True, True, **cfg)
    # with x6_winograd this is the pair that differs under fold_eval_bn alone: the folded 3x3 layer then runs its products in fp32
    assert torch.equal(on, off), int((on != off).sum())
    assert log_on == {("fwd", x6 + "+bn"): 3, ("fwd", "winograd/x6+bn" if wino_x6 else "winograd+bn"): 1}, log_on
    # the new switch off: the parent's keys
    _, log_old = _run(blk, x, True, False, **cfg)
    assert log_old == {("fwd", x6): 3, ("fwd", "winograd+bn"): 1}, log_old


def test_switching_the_flag_between_calls_of_one_module():
    blk, x = _block("s2_down")
    outs, logs = zip(*[_run(blk, x, True, flag, x6_split="loader") for flag in (True, False, True, False)])
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    assert logs[0] == logs[2] == {("fwd", "bf16x6/ls+bn"): 3, ("fwd", "f32+bn"): 1}, logs[0]
    assert logs[1] == logs[3] == {("fwd", "bf16x6/ls"): 3, ("fwd", "f32+bn"): 1}, logs[1]


def test_grad_mode_with_trainable_weights_stays_unfolded():
    """Grad mode and conv weights that require grad: no site folds, and the gradients are those of the run with the switches off."""
    blk, x = _block("d2_wino")
    probe = torch.randn(x.shape[:1] + (512,) + x.shape[2:], generator=torch.Generator().manual_seed(8)).to(DEV)
    convs = (blk.conv1, blk.conv2, blk.conv3, blk.downsample[0])
    assert all(c.weight.requires_grad for c in convs)
    grads = {}
    for flags in ((True, True), (False, False)):
        for c in convs:
            c.weight.grad = None
        y, log = _run(blk, x, *flags, grad=True, x6_split="loader", x6_winograd=True)
        assert not _bn_entries(log), log
        (y * probe).sum().backward()
        torch.cuda.synchronize()
        grads[flags] = (y.detach(), [c.weight.grad.clone() for c in convs])
    for c in convs:
        c.weight.grad = None
    assert torch.equal(grads[(True, True)][0], grads[(False, False)][0])
    for a, b in zip(grads[(True, True)][1], grads[(False, False)][1]):
        assert torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _tiny():
    from diga_amd.model import seg_model_noaux as sm
    from diga_amd.model.model_noaux import SegModel
    from oracle import deeplab as od
    from oracle import detweights
    m = SegModel(arch=sm.TINY)
    m.load_state_dict(detweights.state_dict(od.TINY))
    return m.to(DEV).eval()


@pytest.mark.parametrize("split", SPLITS)
def test_tiny_model_and_two_scale_evaluation_fold_on_and_off(split):
    from diga_amd import config
    from diga_amd import evaluate as ev
    from diga_amd.model import conv as dc
    from diga_amd.util.metrics import runningScore
    m = _tiny()
    g = torch.Generator().manual_seed(7)
    images = (torch.rand((2, 3, 128, 192), generator=g) * 2 - 1).to(DEV)
    labels = torch.randint(0, 19, (2, 128, 192), generator=g).to(DEV)
    x6 = "bf16x6/ls" if split == "loader" else "bf16x6"
    with config.override(conv_math=2, x6_split=split, x6_winograd=True, fold_eval_bn_x6=True), torch.no_grad():
        off = m(images)
        dc.path_log = {}
        try:
            with config.override(fold_eval_bn=True):
                on = m(images)
            log = dc.path_log
        finally:
            dc.path_log = None
        for a, b, what in zip(on, off, ("shallow", "deep", "out", "feat")):
            assert torch.equal(a, b), (what, int((a != b).sum()))
        print(f"tiny {split}: {log}")
        assert log.get(("fwd", x6 + "+bn"), 0) >= 3 and log.get(("fwd", "f32+bn"), 0) >= 1, log       # trunk pointwise sites; the stem
        rs_on, rs_off = runningScore(19, verbose=False), runningScore(19, verbose=False)
        p_on = ev.evaluate_two_scale(m, images, labels, rs_on, want_pred=True, fold_bn=True)
        p_off = ev.evaluate_two_scale(m, images, labels, rs_off, want_pred=True, fold_bn=False)
    assert torch.equal(p_on, p_off)
    rs_on.get_scores(), rs_off.get_scores()
    assert np.array_equal(rs_on.confusion_matrix, rs_off.confusion_matrix) and rs_on.confusion_matrix.sum() > 0


# ---------------------------------------------------------------------------------------------------------------- dispatch
@pytest.mark.parametrize("split", SPLITS)
def test_tiny_eval_pass_launches_the_recorded_entry_points(split):
    """tests/test_gpu_conv_dispatch.py for the new paths: the TINY model's eval pass on the geometry of its `tiny_eval` scenarios, mode 2
    with x6_winograd and both folds on, launches the recorded sequence of entry points and counts the recorded path_log
    (tests/golden/conv_dispatch_x6.json: names only), and the two forms together reach the three `_infer` exports."""
    import json
    import os

    import conv_dispatch_scenarios as sc
    from conftest import GOLDEN
    from diga_amd import _lib
    with open(os.path.join(GOLDEN, "conv_dispatch_x6.json")) as f:
        want = json.load(f)
    m = _tiny()
    x = torch.randn((2, 3, 96, 128), generator=torch.Generator().manual_seed(12)).to(DEV).contiguous(memory_format=torch.channels_last)

    def run():
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()

    names = []                       # (sc.record keeps the diga_conv2d_* names and the helpers: the `_infer` exports are added here)
    _, paths, _ = sc.record(run, dict(conv_math=2, x6_split=split, x6_winograd=True, fold_eval_bn=True, fold_eval_bn_x6=True),
                            on_call=lambda name, args: names.append(name) if sc.is_conv_call(name) or name in X6_INFER else None)
    assert names == want[split]["names"], names
    assert paths == want[split]["path_log"], paths
    seen = {n for v in want.values() for n in v["names"]}
    assert set(X6_INFER) <= seen and all(n in _lib.SIGNATURES for n in X6_INFER)
