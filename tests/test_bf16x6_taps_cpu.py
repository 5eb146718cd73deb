"""CPU-side checks of bf16x6 for multi-tap convolutions and the stem (config.x6_taps; csrc/conv_bf16x6.h, model/conv.py): the configuration
surface, the planner's answers with the switch on and off, the C ABI surface, the argument checks of the new entry points -- which answer
before anything touches a device -- and the workspace query."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = ["diga_conv_taps_bf16x6_f32in", "diga_conv_taps_bf16x6_f32in_epi", "diga_infer_conv_taps_bf16x6_f32in"]
NEW_EXPORTS = FWD + ["diga_conv_taps_wgrad_bf16x6_f32in", "diga_conv_taps_wgrad_bf16x6_workspace_bytes"]
EINVAL, EALIGN, EWORKSPACE = -1, -2, -3
A = 1 << 20                      # a 16-byte aligned, non-null address: never dereferenced (every call below fails its checks)
BIG = 1 << 40


def test_step_config_x6_taps(monkeypatch):
    from diga_amd import _lib, config
    from diga_amd.model import conv as dc
    assert config.StepConfig().x6_taps is False                   # opt-in
    assert config.DEFAULTS.x6_taps is False or "DIGA_X6_TAPS" in os.environ
    assert config.StepConfig(x6_taps=True).validate().x6_taps is True
    assert config.StepConfig().replace(x6_taps=True).x6_taps is True
    with pytest.raises(ValueError):
        config.StepConfig(x6_taps="yes").validate()
    with pytest.raises(ValueError):
        config.StepConfig().replace(x6_taps=1)
    monkeypatch.setenv("DIGA_X6_TAPS", "1")
    assert config.StepConfig.from_env().x6_taps is True
    monkeypatch.setenv("DIGA_X6_TAPS", "0")
    assert config.StepConfig.from_env().x6_taps is False
    monkeypatch.delenv("DIGA_X6_TAPS")
    assert config.StepConfig.from_env().x6_taps is False
    # independent of x6_split; without conv_math = 2 the flag selects nothing
    for form in ("pass", "loader"):
        with config.override(x6_taps=True, x6_split=form):
            assert config.active().x6_taps is True
            assert dc._x6_taps() == (_lib.get_conv_math() == 2)
        for math in (0, 1):
            with config.override(x6_taps=True, x6_split=form, conv_math=math):
                assert not dc._x6_taps()
        with config.override(x6_taps=True, x6_split=form, conv_math=2):
            assert dc._x6_taps()
    assert config.active().x6_taps == config.DEFAULTS.x6_taps


# ---------------------------------------------------------------------------------------------------------------- planner
def _fwd(n, h, w, cin, k, r, dil, stride=1, **kw):
    """_plan's arguments for the forward of an r x r 'same' layer (padding = dilation * (r // 2))."""
    pad = dil * (r // 2)
    ho, wo = ((v + 2 * pad - dil * (r - 1) - 1) // stride + 1 for v in (h, w))
    return dict(n=n, hi=h, wi=w, cin=cin, k=k, r=r, s=r, stride=(stride, stride), off0=(-pad, -pad), doff=(dil, dil), ho=ho, wo=wo, **kw)


def _dgrad(n, h, w, cin, k, r, dil, **kw):
    """... for its backward-data (stride 1): dy [n,h,w,k] -> dx [n,h,w,cin], offsets negated."""
    from diga_amd.model import conv as dc
    pad = dil * (r // 2)
    return dict(n=n, hi=h, wi=w, cin=k, k=cin, r=r, s=r, stride=(1, 1), off0=(pad, pad), doff=(-dil, -dil), ho=h, wo=w, tag=dc._TAG_BWD_DATA, **kw)


def _wgrad(n, h, w, cin, k, r, dil, stride=1, **kw):
    pad = dil * (r // 2)
    ho, wo = ((v + 2 * pad - dil * (r - 1) - 1) // stride + 1 for v in (h, w))
    return (n, h, w, cin, k, r, r, (stride, stride), (pad, pad), (dil, dil), ho, wo), kw


L1 = (2, 193, 193, 64, 64, 3, 1)             # layer1.conv2
D2 = (1, 97, 97, 256, 256, 3, 2)             # a Winograd layer
L2W = (2, 97, 97, 128, 128, 3, 1)            # layer2.conv2: Winograd forward / backward-data, direct weight gradient (kp % 256)
D24 = (1, 33, 33, 256, 256, 3, 24)           # 1 x 1 and 2 x 2 sub-images: the Winograd share (0.94) is above winograd_ratio


def test_plan_with_the_switch_on():
    from diga_amd import config
    from diga_amd.model import conv as dc
    taps = dc._Path("x6rs", "", 2, "bf16x6/taps")
    for split in ("pass", "loader"):          # the loader form whatever x6_split says
        with config.override(conv_math=2, x6_taps=True, x6_split=split):
            # 3x3 64 -> 64: all three passes, with statistics and with the backward-data epilogue
            assert dc._plan(**_fwd(*L1)) == taps
            assert dc._plan(**_fwd(*L1, stats="chunks")) == taps
            assert dc._plan(**_dgrad(*L1)) == taps
            assert dc._plan(**_dgrad(*L1, epi=True)) == dc._Path("x6rs", "epi", 2, "bf16x6/taps")
            a, kw = _wgrad(*L1)
            assert dc._wgrad_plan(*a, **kw) == taps
            # Winograd keeps what it takes ...
            assert dc._plan(**_fwd(*D2)).family == "winograd" and dc._plan(**_dgrad(*D2)).family == "winograd"
            a, kw = _wgrad(*D2)
            assert dc._wgrad_plan(*a, **kw).family == "winograd"
            # ... layer2.conv2 splits: Winograd forward and backward-data (math 0), taps weight gradient (math 2)
            assert dc._plan(**_fwd(*L2W)).family == "winograd" and dc._plan(**_dgrad(*L2W)).math == 0
            a, kw = _wgrad(*L2W)
            assert dc._wgrad_plan(*a, **kw) == taps
            # ... and a share above winograd_ratio, a strided 3x3, a 7x7 go to the new family
            assert dc._plan(**_fwd(*D24)) == taps and dc._plan(**_dgrad(*D24)) == taps
            assert dc._plan(**_fwd(2, 33, 31, 128, 128, 3, 1, stride=2)) == taps
            assert dc._plan(**_fwd(1, 40, 40, 32, 64, 7, 1)) == taps
            a, kw = _wgrad(2, 33, 31, 128, 128, 3, 1, stride=2)
            assert dc._wgrad_plan(*a, **kw) == taps
            with config.override(winograd=False):
                assert dc._plan(**_fwd(*D2)) == taps and dc._plan(**_dgrad(*D2)) == taps
                a, kw = _wgrad(*D2)
                assert dc._wgrad_plan(*a, **kw) == taps
            # calls with folded options stay where they were; so do 9 x 9 = 81 taps (the live-tap mask has 64 bits)
            assert dc._plan(**_fwd(*L1, opts=(1, 0, 0))) == dc._Path("f32", "opts", 0, "f32")
            assert dc._plan(**_fwd(*L1, opts=(0, 1, 2))) == dc._Path("f32", "opts", 0, "f32")
            assert dc._plan(**_fwd(1, 40, 40, 32, 64, 9, 1)) == dc._Path("f32", "", 0, "f32")
            # the pointwise layers are where x6_split puts them
            pw = dc._plan(n=2, hi=33, wi=29, cin=64, k=256, r=1, s=1, stride=(1, 1), off0=(0, 0), doff=(1, 1), ho=33, wo=29)
            assert pw == (dc._Path("x6ls", "", 2, "bf16x6/ls") if split == "loader" else dc._Path("x6", "", 2, "bf16x6"))
            # the stem's im2col GEMM: the existing loader-form kernels, forward and weight gradient
            stem = dict(n=2, hi=33, wi=32, cin=160, k=64, r=1, s=1, stride=(1, 1), off0=(0, 0), doff=(1, 1), ho=33, wo=32, x6_ok=False)
            assert dc._plan(**stem) == dc._Path("x6ls", "", 2, "bf16x6/ls")
            assert dc._plan(stats="chunks", **stem) == dc._Path("x6ls", "", 2, "bf16x6/ls")
            assert dc._wgrad_plan(2, 33, 32, 160, 64, 1, 1, (1, 1), (0, 0), (1, 1), 33, 32, stem=True) == dc._Path("x6ls", "", 2, "bf16x6/ls")


def test_inference_epilogue_needs_fold_eval_bn_x6():
    from diga_amd import config
    from diga_amd.model import conv as dc
    geom = lambda n, h, w, cin, k, r, dil: (n, h, w, cin, k, r, r, (1, 1), (dil * (r // 2),) * 2, (dil, dil), h, w)
    stem = (2, 33, 32, 160, 64, 1, 1, (1, 1), (0, 0), (1, 1), 33, 32)
    with config.override(conv_math=2, x6_taps=True):
        with pytest.raises(RuntimeError):
            dc._plan(**_fwd(*L1, infer=True))
        assert dc.infer_kernel(*geom(*L1)) is None
        assert dc.infer_kernel(*stem, pointwise_ok=False) is None
        assert dc.infer_kernel(*geom(*D2)) == "winograd+bn"                       # (Winograd: as before)
    with config.override(conv_math=2, x6_taps=True, fold_eval_bn_x6=True):
        assert dc._plan(**_fwd(*L1, infer=True)) == dc._Path("x6rs", "infer", 2, "bf16x6/taps+bn")
        assert dc.infer_kernel(*geom(*L1)) == "bf16x6/taps+bn"
        assert dc.infer_kernel(*stem, pointwise_ok=False) == "bf16x6/ls+bn"
        assert dc.infer_kernel(*geom(2, 17, 17, 64, 18, 3, 1)) is None            # Cout % 4
        for bad in (dict(stats="chunks"), dict(epi=True)):
            with pytest.raises(RuntimeError):
                dc._plan(**_fwd(*L1, infer=True, **bad))
    with config.override(conv_math=2, fold_eval_bn_x6=True):                      # switch off: exact fp32, as before
        assert dc.infer_kernel(*geom(*L1)) == "f32+bn" and dc.infer_kernel(*stem, pointwise_ok=False) == "f32+bn"
    assert dc._ENTRY[("x6rs", "")] == FWD[0] and dc._ENTRY[("x6rs", "epi")] == FWD[1] and dc._ENTRY[("x6rs", "infer")] == FWD[2]
    assert dc._WGRAD["x6rs"][0] == NEW_EXPORTS[3]


def test_switch_off_gives_the_previous_answers():
    """With x6_taps off (spelled out, or by default) every call is planned as before this switch existed: the direct fp32 kernels for
    what Winograd does not take, in every arithmetic; and outside conv_math = 2 the switch changes nothing."""
    from diga_amd import config
    from diga_amd.model import conv as dc
    f32 = dc._Path("f32", "", 0, "f32")
    stem = dict(n=2, hi=33, wi=32, cin=160, k=64, r=1, s=1, stride=(1, 1), off0=(0, 0), doff=(1, 1), ho=33, wo=32, x6_ok=False)
    calls = [_fwd(*L1), _fwd(*L1, stats="chunks"), _dgrad(*L1), _dgrad(*L1, epi=True), _fwd(*D2), _dgrad(*D2), _fwd(*L2W), _fwd(*D24),
             _fwd(2, 33, 31, 128, 128, 3, 1, stride=2), _fwd(1, 40, 40, 32, 64, 7, 1), _fwd(*L1, opts=(1, 0, 0)), stem]
    wcalls = [_wgrad(*L1), _wgrad(*D2), _wgrad(*L2W), _wgrad(*D24), ((2, 33, 32, 160, 64, 1, 1, (1, 1), (0, 0), (1, 1), 33, 32), dict(stem=True))]
    for split in ("pass", "loader"):
        for xw in (False, True):
            with config.override(conv_math=2, x6_split=split, x6_winograd=xw, x6_taps=False):
                assert dc._plan(**_fwd(*L1)) == f32 and dc._plan(**_dgrad(*L1)) == f32
                assert dc._plan(**_dgrad(*L1, epi=True)) == dc._Path("f32", "epi", 0, "f32")
                assert dc._plan(**_fwd(*D24)) == f32 and dc._plan(**stem) == f32
                assert dc._plan(**_fwd(*D2)).family == "winograd"
                assert dc._wgrad_plan(*_wgrad(*L1)[0]) == f32 and dc._wgrad_plan(*_wgrad(*L2W)[0]) == f32
                assert dc._wgrad_plan(*wcalls[-1][0], stem=True) == dc._Path("f32", "", 0, "f32", flops=False)
                off = [dc._plan(**c) for c in calls] + [dc._wgrad_plan(*a, **kw) for a, kw in wcalls]
            with config.override(conv_math=2, x6_split=split, x6_winograd=xw):
                assert config.active().x6_taps is config.DEFAULTS.x6_taps
                if not config.DEFAULTS.x6_taps:
                    assert off == [dc._plan(**c) for c in calls] + [dc._wgrad_plan(*a, **kw) for a, kw in wcalls]
    for math in (0, 1):
        with config.override(conv_math=math, x6_taps=False):
            off = [dc._plan(**c) for c in calls if "opts" not in c or math == 0] + [dc._wgrad_plan(*a, **kw) for a, kw in wcalls]
        with config.override(conv_math=math, x6_taps=True):
            assert off == [dc._plan(**c) for c in calls if "opts" not in c or math == 0] + [dc._wgrad_plan(*a, **kw) for a, kw in wcalls]


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_exports_are_declared_bound_and_exported():
    from diga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    for name in NEW_EXPORTS:
        assert not name.startswith("diga_conv2d_")                # (the dispatch fixture enumerates those)
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/diga_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    fresh = ctypes.CDLL(_lib.LIB_PATH)                           # the dynamic symbol table of the library itself
    for name in NEW_EXPORTS:
        assert hasattr(fresh, name), f"{name} is not exported by {_lib.LIB_PATH}"
    assert len(_lib.PROF_TAGS) == 23                             # no new profiling tag
    # the argument lists of the pointwise siblings
    S = _lib.SIGNATURES
    assert S[FWD[0]] == S["diga_conv2d_nhwc_bf16x6_f32in"] and S[FWD[1]] == S["diga_conv2d_nhwc_bf16x6_f32in_epi"]
    assert S[FWD[2]] == S["diga_infer_conv2d_nhwc_bf16x6_f32in"] and S[NEW_EXPORTS[3]] == S["diga_conv2d_wgrad_bf16x6_f32in"]
    assert S[NEW_EXPORTS[4]] == S["diga_conv2d_wgrad_bf16x6_workspace_bytes"]


def _bwd_epi():
    from diga_amd import _lib
    e = _lib.BwdEpilogue()
    e.addend, e.addend_ld = A, 64
    return e


def _inf_epi(ab=A + 4096):
    from diga_amd import _lib
    e = _lib.InferEpilogue()
    e.ab, e.residual, e.residual_ld, e.relu = ab, None, 0, 1
    return e


def _call(name, in_=A, in_ld=64, img=A, out=A, n=1, hi=12, wi=12, cin=64, ho=12, wo=12, cout=64, out_ld=64, r=3, s=3, sy=1, sx=1, oy=-1, ox=-1,
          dy=1, dx=1, tail="default", tag=0):
    """One call of a forward export on a 1 x 12 x 12 x 64 -> 64 3x3 layer with fake addresses; the trailing pointer by `name`."""
    from diga_amd import _lib
    held = None
    if tail == "default":
        held = _bwd_epi() if name.endswith("_epi") else _inf_epi() if name.startswith("diga_infer") else None
        tail = ctypes.byref(held) if held is not None else None
    lead = [in_, in_ld, img] + ([] if name.endswith("_epi") else [None]) + [out]
    return getattr(_lib.lib, name)(*lead, n, hi, wi, cin, ho, wo, cout, out_ld, r, s, sy, sx, oy, ox, dy, dx, tail, tag, None)


@pytest.mark.parametrize("name", FWD)
def test_forward_entry_points_reject_bad_arguments(name):
    from diga_amd import _lib
    for kw in (dict(in_=0), dict(img=0), dict(out=0)):
        assert _call(name, **kw) == EINVAL, kw
    assert _call(name, in_=A + 4) == EALIGN and _call(name, img=A + 8) == EALIGN and _call(name, out=A + 2) == EALIGN
    assert _call(name, cin=48, in_ld=48) == EINVAL and _call(name, cin=0) == EINVAL                 # Cin % 32
    assert _call(name, in_ld=32) == EINVAL and _call(name, in_ld=66) == EINVAL and _call(name, in_ld=-1) == EINVAL
    assert _call(name, out_ld=32) == EINVAL
    assert _call(name, r=0) == EINVAL and _call(name, s=0) == EINVAL                                # R * S = 0
    assert _call(name, r=5, s=13) == EINVAL and _call(name, r=65, s=1) == EINVAL                    # R * S = 65
    assert _call(name, r=1 << 32, s=1 << 32) == EINVAL                                              # (a product that wraps)
    assert _call(name, sy=0) == EINVAL and _call(name, sx=-1) == EINVAL
    assert _call(name, n=1 << 12, hi=1 << 10, wi=1 << 9) == EINVAL                                  # 2^31 input pixels
    assert _call(name, n=1 << 12, ho=1 << 10, wo=1 << 9) == EINVAL                                  # 2^31 output pixels
    assert _call(name, oy=1 << 31) == EINVAL and _call(name, dx=-(1 << 31)) == EINVAL and _call(name, sy=1 << 31) == EINVAL
    assert _call(name, n=0) == EINVAL and _call(name, cout=0) == EINVAL
    assert _lib.last_error() != ""
    # the descriptors' rules
    if name.endswith("_epi"):
        assert _call(name, tail=None) == EINVAL                                                     # null descriptor
        assert _call(name, tail=ctypes.byref(_lib.BwdEpilogue())) == EINVAL                         # empty descriptor
        e = _bwd_epi()
        e.addend_ld = 32
        assert _call(name, tail=ctypes.byref(e)) == EINVAL                                          # addend_ld < Cout
    elif name.startswith("diga_infer"):
        assert _call(name, tail=None) == EINVAL
        assert _call(name, tail=ctypes.byref(_inf_epi(None))) == EINVAL                             # null ab
        assert _call(name, tail=ctypes.byref(_inf_epi(A + 4))) == EINVAL                            # misaligned ab
        assert _call(name, cout=18, out_ld=20) == EINVAL                                            # Cout % 4
        assert _call(name, out_ld=66) == EINVAL
        assert _call(name, tag=_lib.PROF_TAGS.index("conv_bwd_data")) == EINVAL                     # forward only
    # the old entry points keep refusing more than one tap
    old = {FWD[0]: "diga_conv2d_nhwc_bf16x6_f32in", FWD[1]: "diga_conv2d_nhwc_bf16x6_f32in_epi", FWD[2]: "diga_infer_conv2d_nhwc_bf16x6_f32in"}[name]
    assert _call(old) == EINVAL


def _wg(dy=A, dy_ld=64, x=A, x_ld=64, dw=A, ws=A, ws_bytes=BIG, n=1, hi=12, wi=12, cin=64, ho=12, wo=12, cout=64, r=3, s=3, sy=1, sx=1, oy=-1,
        ox=-1, ddy=1, ddx=1, name="diga_conv_taps_wgrad_bf16x6_f32in"):
    from diga_amd import _lib
    return getattr(_lib.lib, name)(dy, dy_ld, x, x_ld, dw, ws, ws_bytes, n, hi, wi, cin, ho, wo, cout, r, s, sy, sx, oy, ox, ddy, ddx, None)


def test_weight_gradient_entry_point_rejects_bad_arguments():
    for name in ("dy", "x", "dw", "ws"):
        assert _wg(**{name: 0}) == EINVAL, name
        assert _wg(**{name: A + 4}) == EALIGN, name
    assert _wg(cin=48, x_ld=48) == EINVAL and _wg(cin=0) == EINVAL                                  # Cin % 32
    assert _wg(cout=60, dy_ld=60) == EINVAL                                                         # Cout % 8
    assert _wg(dy_ld=32) == EINVAL and _wg(x_ld=32) == EINVAL and _wg(dy_ld=66) == EINVAL and _wg(x_ld=-1) == EINVAL
    assert _wg(r=0) == EINVAL and _wg(s=0) == EINVAL and _wg(r=5, s=13) == EINVAL and _wg(r=65, s=1) == EINVAL
    assert _wg(r=1 << 32, s=1 << 32) == EINVAL
    assert _wg(sy=0) == EINVAL and _wg(sx=-2) == EINVAL
    assert _wg(n=1 << 12, hi=1 << 10, wi=1 << 9) == EINVAL and _wg(n=1 << 12, ho=1 << 10, wo=1 << 9) == EINVAL
    assert _wg(oy=1 << 31) == EINVAL and _wg(ddx=-(1 << 31)) == EINVAL
    assert _wg(ws_bytes=64) == EWORKSPACE
    assert _wg(name="diga_conv2d_wgrad_bf16x6_f32in") == EINVAL                                     # the old entry point: pointwise only


def test_workspace_query():
    from diga_amd import _lib
    q, old = _lib.lib.diga_conv_taps_wgrad_bf16x6_workspace_bytes, _lib.lib.diga_conv2d_wgrad_bf16x6_workspace_bytes
    # rejected shapes: 0
    assert q(1, 12, 12, 64, 48, 3, 3) == 0 and q(1, 12, 12, 60, 64, 3, 3) == 0 and q(1, 12, 12, 64, 64, 0, 3) == 0
    assert q(1, 12, 12, 64, 64, 5, 13) == 0 and q(0, 12, 12, 64, 64, 3, 3) == 0 and q(1 << 12, 1 << 10, 1 << 9, 64, 64, 3, 3) == 0
    mpad = lambda m: (m + 31) // 32 * 32 + 64

    def parts(m, cout, cin, rs):
        # plan_wgrad_x6: 512 blocks wanted over the (Cout / 256) x (Cin / 128) x RS tiles, at least 8 K-steps of 32 pixels per block
        tiles = -(-cout // 256) * -(-cin // 128) * rs
        ksteps = -(-m // 32)
        splits = min(-(-512 // tiles), max(ksteps // 8, 1), 512)
        splits = -(-ksteps // -(-ksteps // splits))
        return (splits * cout * rs * cin * 4 if splits > 1 else 0) + rs * mpad(m) * 4 + 64, splits

    # 144 pixels: 4 K-steps, one split, no slab -- the table of all nine taps and the zeros
    assert q(1, 12, 12, 64, 64, 3, 3) == parts(144, 64, 64, 9)[0] == 9 * mpad(144) * 4 + 64
    # R = S = 1: the pointwise query
    assert q(2, 33, 29, 256, 64, 1, 1) == old(2, 33, 29, 256, 64, 1, 1)
    # the plan counts the taps: 2 x 193 x 193 pixels, 64 -> 64 has one channel tile; nine taps ask for ceil(512 / 9) = 57 splits where a
    # pointwise layer of that size takes 291 (the 8-K-step floor)
    m = 2 * 193 * 193
    want, splits = parts(m, 64, 64, 9)
    assert splits in (56, 57) and parts(m, 64, 64, 1)[1] > 250
    assert q(2, 193, 193, 64, 64, 3, 3) == want
    assert q(2, 193, 193, 64, 64, 3, 3) < old(2, 193, 193, 64, 64, 3, 3)         # (which sizes nine taps' slabs by the one-tap plan)
    # 7 x 7: 49 taps
    assert q(1, 40, 40, 64, 32, 7, 7) == parts(1600, 64, 32, 49)[0]
