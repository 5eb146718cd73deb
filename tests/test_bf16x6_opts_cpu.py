"""CPU-side checks of bf16x6 for convolutions with a folded input map / activation (config.x6_opts; csrc/conv_bf16x6.h, csrc/winograd.hip,
model/conv.py): the switch, the C ABI surface, the argument checks of the two new entry points -- which answer before anything touches a
device -- and the planner's answers with the switch on and off."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS_OPTS, WINO_OPTS = "diga_conv_taps_bf16x6_f32in_opts", "diga_conv_winograd_bf16x6_opts"
EINVAL, EALIGN, EWORKSPACE = -1, -2, -3
A = 1 << 20                      # a 16-byte aligned, non-null address: never dereferenced (every call below fails its checks)
BIG = 1 << 40


# ---------------------------------------------------------------------------------------------------------------- 1. the switch
def test_step_config_x6_opts(monkeypatch):
    from diga_amd import _lib, config
    from diga_amd.model import conv as dc
    assert config.StepConfig().x6_opts is False                   # opt-in
    assert config.DEFAULTS.x6_opts is False or "DIGA_X6_OPTS" in os.environ
    assert config.StepConfig(x6_opts=True).validate().x6_opts is True
    assert config.StepConfig().replace(x6_opts=True).x6_opts is True
    with pytest.raises(ValueError):
        config.StepConfig(x6_opts="yes").validate()
    with pytest.raises(ValueError):
        config.StepConfig().replace(x6_opts=1)
    monkeypatch.setenv("DIGA_X6_OPTS", "1")
    assert config.StepConfig.from_env().x6_opts is True
    monkeypatch.setenv("DIGA_X6_OPTS", "0")
    assert config.StepConfig.from_env().x6_opts is False
    monkeypatch.delenv("DIGA_X6_OPTS")
    assert config.StepConfig.from_env().x6_opts is False
    # without conv_math = 2 the flag selects nothing
    for math in (0, 1):
        with config.override(x6_opts=True, conv_math=math):
            assert not dc._x6_opts()
    with config.override(x6_opts=True, conv_math=2):
        assert dc._x6_opts()
    with config.override(x6_opts=True):
        assert dc._x6_opts() == (_lib.get_conv_math() == 2)
    assert config.active().x6_opts == config.DEFAULTS.x6_opts


# ---------------------------------------------------------------------------------------------------------------- 2. the exports
def test_exports_are_declared_bound_and_exported():
    from diga_amd import _lib
    from diga_amd.model import conv as dc
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    for name in (TAPS_OPTS, WINO_OPTS):
        assert not name.startswith("diga_conv2d_") and name.endswith("_opts")       # (the dispatch fixture enumerates diga_conv2d_*)
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/diga_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    fresh = ctypes.CDLL(_lib.LIB_PATH)                           # the dynamic symbol table of the library itself
    for name in (TAPS_OPTS, WINO_OPTS):
        assert hasattr(fresh, name), f"{name} is not exported by {_lib.LIB_PATH}"
    assert "No reflection" not in hdr
    assert len(_lib.PROF_TAGS) == 23                             # no new profiling tag
    S = _lib.SIGNATURES
    # the multi-tap sibling's list plus the options pointer behind the statistics slot; the fp32 Winograd `_opts` form's list
    res, args = S["diga_conv_taps_bf16x6_f32in"]
    assert S[TAPS_OPTS] == (res, args[:-2] + [_lib.P] + args[-2:]) and len(S[TAPS_OPTS][1]) == len(args) + 1
    assert S[WINO_OPTS] == S["diga_conv2d_winograd_f32_opts"]
    assert dc._ENTRY[("x6rs", "opts")] == TAPS_OPTS and dc._WINOGRAD_X6_OPTS == WINO_OPTS
    assert dc._ENTRY[("winograd_reflect", "opts")] == "diga_conv2d_winograd_f32_opts" and dc._ENTRY[("f32", "opts")] == "diga_conv2d_nhwc_f32_opts"


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def _opts(reflect=1, shift=0, act=0):
    from diga_amd import _lib
    return _lib.ConvOptions(reflect, shift, act)


def _taps(in_=A, in_ld=64, img=A, out=A, n=1, hi=12, wi=12, cin=64, ho=12, wo=12, cout=64, out_ld=64, r=3, s=3, sy=1, sx=1, oy=-1, ox=-1,
          dy=1, dx=1, stats=None, opts="default", tag=0, name=TAPS_OPTS):
    """One call of the multi-tap `_opts` export (or, by `name`, of its sibling without options) on a 1 x 12 x 12 x 64 -> 64 3x3 layer
    with fake addresses."""
    from diga_amd import _lib
    held = _opts() if opts == "default" else opts
    tail = [stats] + ([] if name != TAPS_OPTS else [ctypes.byref(held) if held is not None else None])
    return getattr(_lib.lib, name)(in_, in_ld, img, None, out, n, hi, wi, cin, ho, wo, cout, out_ld, r, s, sy, sx, oy, ox, dy, dx, *tail, tag, None)


def _wino(in_=A, wgt=A, out=A, ws=A, ws_bytes=BIG, n=1, h=12, w=12, cin=64, in_ld=64, cout=128, out_ld=128, d=1, tile=4, opts="default",
          name=WINO_OPTS):
    from diga_amd import _lib
    held = _opts() if opts == "default" else opts
    return getattr(_lib.lib, name)(in_, wgt, None, out, ws, ws_bytes, n, h, w, cin, in_ld, cout, out_ld, d, tile,
                                   ctypes.byref(held) if held is not None else None, None, 0, None)


def _refused(rc, want=EINVAL):
    from diga_amd import _lib
    assert rc == want, rc
    msg = _lib.last_error()
    assert msg != ""
    return msg


def test_taps_opts_rejects_bad_arguments():
    from diga_amd import _lib
    assert "null options" in _refused(_taps(opts=None))
    assert "bad options" in _refused(_taps(opts=_opts(shift=3)))
    for bad in (_opts(reflect=2), _opts(act=2), _opts(shift=-1)):
        assert "bad options" in _refused(_taps(opts=bad))
    assert "statistics" in _refused(_taps(stats=A))                                     # inference-only: no statistics slot
    assert "R * S <= 64" in _refused(_taps(r=5, s=13)) and _taps(r=65, s=1) == EINVAL    # R * S = 65
    assert _taps(r=0) == EINVAL and _taps(r=1 << 32, s=1 << 32) == EINVAL
    for kw in (dict(in_=0), dict(img=0), dict(out=0)):
        assert _taps(**kw) == EINVAL, kw
    assert _taps(in_=A + 4) == EALIGN and _taps(img=A + 8) == EALIGN and _taps(out=A + 2) == EALIGN
    assert _taps(cin=48, in_ld=48) == EINVAL and _taps(in_ld=32) == EINVAL and _taps(in_ld=-1) == EINVAL and _taps(out_ld=32) == EINVAL
    assert _taps(sy=0) == EINVAL and _taps(sx=-1) == EINVAL
    assert _taps(oy=1 << 31) == EINVAL and _taps(dx=-(1 << 31)) == EINVAL
    # the coordinates are the upsampled image's: 2^28 source rows are fine for the 32-bit walk, shifted by 2 they are not
    assert "upsampled" in _refused(_taps(hi=1 << 28, wi=1, ho=1 << 30, wo=1, opts=_opts(shift=2)))
    assert "upsampled" in _refused(_taps(hi=1, wi=1 << 30, ho=1, wo=1, opts=_opts(shift=0)))
    assert _lib.last_error() != ""


def test_winograd_opts_rejects_bad_arguments():
    assert "null options" in _refused(_wino(opts=None))
    assert "only reflect_pad" in _refused(_wino(opts=_opts(act=1)))
    assert "only reflect_pad" in _refused(_wino(opts=_opts(shift=1)))
    assert _refused(_wino(tile=2)) and _wino(tile=3) == EINVAL and _wino(tile=8) == EINVAL
    assert _wino(in_=0) == EINVAL and _wino(wgt=0) == EINVAL and _wino(out=0) == EINVAL and _wino(ws=0) == EINVAL
    assert _wino(cin=48, in_ld=48) == EINVAL and _wino(cout=64, out_ld=64) == EINVAL and _wino(out_ld=130) == EINVAL
    assert _wino(d=12) == EINVAL                                                          # the mirror needs pad < H, W
    assert _wino(in_=A + 4) == EALIGN
    assert _wino(ws_bytes=64) == EWORKSPACE
    # the workspace is the bf16x6 query's (the fp32 form's + the weight images): the fp32 size is refused
    from diga_amd import _lib
    f32 = _lib.lib.diga_conv2d_winograd_workspace_bytes(1, 12, 12, 64, 128, 1, 4)
    x6 = _lib.lib.diga_conv2d_winograd_bf16x6_workspace_bytes(1, 12, 12, 64, 128, 1, 4)
    assert 0 < f32 < x6 and _wino(ws_bytes=f32) == EWORKSPACE and _wino(ws_bytes=x6 - 1) == EWORKSPACE


def test_old_entry_points_refuse_as_before():
    from diga_amd import _lib
    # the sibling without options: same checks, same codes (and still no options argument)
    name = "diga_conv_taps_bf16x6_f32in"
    assert _taps(name=name, r=5, s=13) == EINVAL and _taps(name=name, in_=0) == EINVAL and _taps(name=name, img=A + 8) == EALIGN
    assert _taps(name=name, oy=1 << 31) == EINVAL and _taps(name=name, in_ld=32) == EINVAL
    # the pointwise loader form keeps refusing more than one tap
    assert _taps(name="diga_conv2d_nhwc_bf16x6_f32in") == EINVAL
    assert "pointwise" in _lib.last_error()
    # the fp32 Winograd `_opts` form: its own words
    f32 = "diga_conv2d_winograd_f32_opts"
    assert "null options" in _refused(_wino(name=f32, opts=None))
    assert "only reflect_pad" in _refused(_wino(name=f32, opts=_opts(act=1)))
    assert "reflection padding comes with the forward of 4x4 / 6x6 tiles" in _refused(_wino(name=f32, tile=2))
    assert _wino(name=f32, ws_bytes=64) == EWORKSPACE


# ---------------------------------------------------------------------------------------------------------------- 4. the planner
def _fwd(n, h, w, cin, k, r, dil=1, stride=1, up=0, **kw):
    """_plan's arguments for the forward of an r x r layer with padding dil * (r // 2) on the 2^up upsampling of an h x w map."""
    pad = dil * (r // 2)
    ho, wo = (((v << up) + 2 * pad - dil * (r - 1) - 1) // stride + 1 for v in (h, w))
    return dict(n=n, hi=h, wi=w, cin=cin, k=k, r=r, s=r, stride=(stride, stride), off0=(-pad, -pad), doff=(dil, dil), ho=ho, wo=wo, **kw)


UP5 = _fwd(2, 24, 20, 256, 128, 5, up=1, opts=(1, 1, 0))          # the decoder's 5x5 behind the folded upsampling
DOWN4 = dict(n=2, hi=48, wi=40, cin=64, k=128, r=4, s=4, stride=(2, 2), off0=(-1, -1), doff=(1, 1), ho=24, wo=20, opts=(1, 0, 0))
TANH7 = _fwd(2, 48, 40, 64, 3, 7, opts=(1, 0, 1))
RES3 = _fwd(2, 24, 20, 256, 256, 3, opts=(1, 0, 0))                 # a ResBlock conv
PW = dict(n=2, hi=24, wi=20, cin=64, k=64, r=1, s=1, stride=(1, 1), off0=(0, 0), doff=(1, 1), ho=24, wo=20, opts=(0, 0, 1))


def test_plan_with_the_switch_on():
    from diga_amd import config
    from diga_amd.model import conv as dc
    taps = dc._Path("x6rs", "opts", 2, "bf16x6/taps")
    f32 = dc._Path("f32", "opts", 0, "f32")
    for split in ("pass", "loader"):
        with config.override(conv_math=2, x6_split=split, x6_taps=True, x6_opts=True):
            assert dc._plan(**UP5) == taps and dc._plan(**DOWN4) == taps and dc._plan(**TANH7) == taps
            wr = dc._plan(**RES3)                                 # x6_winograd off: the reflect form stays exact fp32
            assert wr == dc._Path("winograd_reflect", "opts", 0, "winograd", wr.tile, wr.ratio) and wr.tile >= 4 and not wr.x6w
            assert dc._plan(**PW) == f32                          # pointwise calls with options: out of scope
            assert dc._plan(**dict(UP5, opts=None)) == dc._Path("x6rs", "", 2, "bf16x6/taps")
            with config.override(winograd=False):                 # what Winograd does not take goes to the taps kernels
                assert dc._plan(**RES3) == taps
        with config.override(conv_math=2, x6_split=split, x6_winograd=True, x6_opts=True):
            wr = dc._plan(**RES3)
            assert wr == dc._Path("winograd_reflect", "opts", 0, "winograd/x6", wr.tile, wr.ratio, True) and wr.tile >= 4
            assert dc._plan(**UP5) == f32                         # x6_taps off: the direct fp32 `_opts` kernels
            with config.override(winograd_max_tile=2):            # no reflect form on F(2x2,3x3): direct, as before
                assert dc._plan(**RES3) == f32
        with config.override(conv_math=2, x6_split=split, x6_taps=True, x6_winograd=True, x6_opts=True):
            assert dc._plan(**UP5) == taps and dc._plan(**RES3).x6w and dc._plan(**RES3).arith == "winograd/x6"
            for bad in (dict(stats="chunks"), dict(epi=True), dict(infer=True)):
                with pytest.raises(RuntimeError):
                    dc._plan(**dict(UP5, **bad))
                with pytest.raises(RuntimeError):
                    dc._plan(**dict(RES3, **bad))


def test_switch_off_gives_the_previous_answers():
    """With x6_opts off (spelled out, or by default) a call with options is planned as before the switch existed -- compared with the
    literal paths -- and outside conv_math = 2 the switch changes nothing."""
    from diga_amd import config
    from diga_amd.model import conv as dc
    f32 = dc._Path("f32", "opts", 0, "f32")
    calls = [UP5, DOWN4, TANH7, RES3, PW]
    for split in ("pass", "loader"):
        for xt in (False, True):
            for xw in (False, True):
                with config.override(conv_math=2, x6_split=split, x6_taps=xt, x6_winograd=xw, x6_opts=False):
                    assert dc._plan(**UP5) == f32 and dc._plan(**DOWN4) == f32 and dc._plan(**TANH7) == f32 and dc._plan(**PW) == f32
                    wr = dc._plan(**RES3)
                    assert wr == dc._Path("winograd_reflect", "opts", 0, "winograd", wr.tile, wr.ratio, False) and wr.tile in (4, 6)
                    off = [dc._plan(**c) for c in calls]
                with config.override(conv_math=2, x6_split=split, x6_taps=xt, x6_winograd=xw):
                    if not config.DEFAULTS.x6_opts:
                        assert off == [dc._plan(**c) for c in calls]
    with config.override(conv_math=0, x6_opts=False):
        off = [dc._plan(**c) for c in calls]
    with config.override(conv_math=0, x6_taps=True, x6_winograd=True, x6_opts=True):
        assert off == [dc._plan(**c) for c in calls]
    with config.override(conv_math=1, x6_opts=False):
        off = [dc._plan(**c) for c in calls]
        assert off[0].math == 1 and off[0].variant == "opts"
    with config.override(conv_math=1, x6_taps=True, x6_winograd=True, x6_opts=True):
        assert off == [dc._plan(**c) for c in calls]
    for on in (False, True):                                      # options with statistics or an epilogue: refused either way
        with config.override(conv_math=2, x6_taps=True, x6_winograd=True, x6_opts=on):
            for bad in (dict(stats="chunks"), dict(epi=True)):
                with pytest.raises(RuntimeError):
                    dc._plan(**dict(UP5, **bad))
