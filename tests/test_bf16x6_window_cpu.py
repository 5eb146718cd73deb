"""CPU-side checks of the window form of the multi-tap bf16x6 forward (config.x6_window; csrc/conv_bf16x6.h, model/conv.py): the switch,
the C ABI surface, the window rule (diga_conv_window_bf16x6_plan), the entry point's argument checks -- which answer before anything
touches a device, with the rule as the oracle on a grid of geometries -- and the planner's answers with the switch on and off."""
import ctypes
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN, WINDOW = "diga_conv_window_bf16x6_plan", "diga_conv_window_bf16x6_f32in"
EINVAL, EALIGN = -1, -2
A = 1 << 20                      # a 16-byte aligned, non-null address: never dereferenced (every call below fails its checks)
LDS = 160 * 1024


# ---------------------------------------------------------------------------------------------------------------- 1. the switch
def test_step_config_x6_window(monkeypatch):
    from diga_amd import config
    from diga_amd.model import conv as dc
    assert config.StepConfig().x6_window is False                 # opt-in
    assert config.DEFAULTS.x6_window is False or "DIGA_X6_WINDOW" in os.environ
    assert config.StepConfig(x6_window=True).validate().x6_window is True
    assert config.StepConfig().replace(x6_window=True).x6_window is True
    with pytest.raises(ValueError):
        config.StepConfig(x6_window="yes").validate()
    with pytest.raises(ValueError):
        config.StepConfig().replace(x6_window=1)
    monkeypatch.setenv("DIGA_X6_WINDOW", "1")
    assert config.StepConfig.from_env().x6_window is True
    monkeypatch.setenv("DIGA_X6_WINDOW", "0")
    assert config.StepConfig.from_env().x6_window is False
    monkeypatch.delenv("DIGA_X6_WINDOW")
    assert config.StepConfig.from_env().x6_window is False
    # it means something only under conv_math = 2 with x6_taps
    geo = (48, 40, 64, 3, 7, 7, (1, 1), 0)
    for math in (0, 1):
        with config.override(x6_window=True, x6_taps=True, conv_math=math):
            assert not dc._x6_window(*geo)
    with config.override(x6_window=True, x6_taps=False, conv_math=2):
        assert not dc._x6_window(*geo)
    with config.override(x6_window=False, x6_taps=True, conv_math=2):
        assert not dc._x6_window(*geo)
    with config.override(x6_window=True, x6_taps=True, conv_math=2):
        assert dc._x6_window(*geo)
        assert not dc._x6_window(48, 40, 64, 3, 7, 7, (-1, -1), 0)       # backward-data never asks; a negative step is refused anyway
    assert config.active().x6_window == config.DEFAULTS.x6_window


# ---------------------------------------------------------------------------------------------------------------- 2. the exports
def test_exports_are_declared_bound_and_exported():
    from diga_amd import _lib
    from diga_amd.model import conv as dc
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    fresh = ctypes.CDLL(_lib.LIB_PATH)                           # the dynamic symbol table of the library itself
    for name in (PLAN, WINDOW):
        assert not name.startswith("diga_conv2d_")               # (the dispatch fixture enumerates diga_conv2d_*)
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/diga_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(fresh, name), f"{name} is not exported by {_lib.LIB_PATH}"
    assert len(_lib.PROF_TAGS) == 23                             # no new profiling tag
    I64, P, INT = _lib.I64, _lib.P, _lib.INT
    assert _lib.SIGNATURES[PLAN] == (INT, [I64] * 9 + [P] * 3)
    assert _lib.SIGNATURES[WINDOW] == (INT, [P, I64, P, P, P] + [I64] * 14 + [P, INT, P])
    assert dc._ENTRY[("x6win", "")] == WINDOW and dc._ENTRY[("x6win", "opts")] == WINDOW


# ---------------------------------------------------------------------------------------------------------------- 3. the rule
def _rule(hi, wi, cin, cout, r, s, dy=1, dx=1, shift=0):
    """diga_conv_window_bf16x6_plan -> (th, tw, cols) or None."""
    from diga_amd import _lib
    th, tw, cols = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.lib.diga_conv_window_bf16x6_plan(hi, wi, cin, cout, r, s, dy, dx, shift, ctypes.byref(th), ctypes.byref(tw), ctypes.byref(cols))
    assert rc in (0, 1)
    if rc == 0:
        assert (th.value, tw.value, cols.value) == (-1, -1, -1)  # nothing written
        return None
    return th.value, tw.value, cols.value


def _lds(plan, r, s, dy, dx):
    """Dynamic LDS of the launch the rule plans: the weight ring, and the window of one 32-channel chunk or (if larger) the drain's stage."""
    th, tw, cols = plan
    window = (th + (r - 1) * dy) * (tw + (s - 1) * dx) * 3 * 64
    return 2 * 3 * cols * 64 + max(window, th * tw * (cols + 4) * 4)


def test_rule_admits_the_decoder_and_refuses_what_cannot_fit():
    # the three stride-1 multi-tap decoder layers of the translator (all three classes measured faster: DESIGN section 8, round 19)
    for geo in ((768, 768, 64, 3, 7, 7, 1, 1, 0), (192, 192, 128, 64, 5, 5, 1, 1, 1), (96, 96, 256, 128, 5, 5, 1, 1, 1)):
        plan = _rule(*geo)
        assert plan is not None, geo
        th, tw, cols = plan
        assert (th * tw) % 128 == 0 and th > 0 and tw > 0
        assert cols == (16 if geo[3] <= 16 else 64)
        assert _lds(plan, *geo[4:8]) <= LDS
    assert _rule(97, 97, 2048, 256, 3, 3, 24, 24) is None        # a dilated ASPP branch: the window does not fit
    assert _rule(48, 40, 64, 64, 1, 1) is None                   # R * S = 1
    assert _rule(48, 40, 64, 64, 5, 13) is None and _rule(48, 40, 64, 64, 65, 1) is None and _rule(48, 40, 64, 64, 9, 8) is None
    assert _rule(48, 40, 64, 64, 8, 8) is not None
    assert _rule(48, 40, 48, 64, 3, 3) is None and _rule(48, 40, 0, 64, 3, 3) is None and _rule(48, 40, 64, 0, 3, 3) is None
    assert _rule(0, 40, 64, 64, 3, 3) is None and _rule(48, 0, 64, 64, 3, 3) is None
    assert _rule(48, 40, 64, 64, 3, 3, 0, 1) is None and _rule(48, 40, 64, 64, 3, 3, 1, -1) is None
    assert _rule(48, 40, 64, 64, 3, 3, 1, 1, 3) is None and _rule(48, 40, 64, 64, 3, 3, 1, 1, -1) is None
    from diga_amd import _lib
    i = ctypes.c_int(0)
    assert _lib.lib.diga_conv_window_bf16x6_plan(48, 40, 64, 64, 3, 3, 1, 1, 0, None, ctypes.byref(i), ctypes.byref(i)) == 0
    # every answer on a grid: th * tw % 128 == 0, cols by Cout, LDS within the CU's
    for cout, r, s, dy, dx in itertools.product((1, 3, 16, 17, 64, 80, 256), (1, 2, 3, 5, 7), (1, 3, 4, 7), (1, 2, 6, 24), (1, 3, 12)):
        plan = _rule(33, 29, 64, cout, r, s, dy, dx)
        if plan is not None:
            assert 2 <= r * s <= 64 and (plan[0] * plan[1]) % 128 == 0 and plan[2] == (16 if cout <= 16 else 64)
            assert _lds(plan, r, s, dy, dx) <= LDS


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def _opts(reflect=1, shift=0, act=0):
    from diga_amd import _lib
    return _lib.ConvOptions(reflect, shift, act)


def _win(in_=A, in_ld=64, img=A, bias=None, out=A, n=1, hi=12, wi=12, cin=64, ho=12, wo=12, cout=64, out_ld=64, r=3, s=3, oy=-1, ox=-1, dy=1,
         dx=1, opts=None, tag=0):
    """One call of the window export on a 1 x 12 x 12 x 64 -> 64 3x3 layer with fake addresses."""
    from diga_amd import _lib
    return _lib.lib.diga_conv_window_bf16x6_f32in(in_, in_ld, img, bias, out, n, hi, wi, cin, ho, wo, cout, out_ld, r, s, oy, ox, dy, dx,
                                                  ctypes.byref(opts) if opts is not None else None, tag, None)


def _refused(rc, want=EINVAL):
    from diga_amd import _lib
    assert rc == want, rc
    msg = _lib.last_error()
    assert msg != ""
    return msg


def test_window_rejects_bad_arguments():
    for kw in (dict(in_=0), dict(img=0), dict(out=0)):
        assert "null pointer" in _refused(_win(**kw)), kw
    assert _win(in_=A + 4) == EALIGN and _win(img=A + 8) == EALIGN and _win(out=A + 2) == EALIGN and _win(bias=A + 1) == EALIGN
    assert "multiple of 32" in _refused(_win(cin=48, in_ld=48))
    assert "2 <= R * S <= 64" in _refused(_win(r=1, s=1, oy=0, ox=0))
    assert _win(r=5, s=13) == EINVAL and _win(r=65, s=1) == EINVAL and _win(r=0) == EINVAL and _win(r=1 << 32, s=1 << 32) == EINVAL
    assert _win(out_ld=32) == EINVAL
    assert "in_ld" in _refused(_win(in_ld=32)) and _win(in_ld=66) == EINVAL and _win(in_ld=-1) == EINVAL
    for bad in (_opts(reflect=2), _opts(act=2), _opts(shift=3), _opts(shift=-1)):
        assert "bad options" in _refused(_win(opts=bad))
    assert _win(n=0) == EINVAL and _win(ho=0) == EINVAL and _win(cout=0, out_ld=0) == EINVAL
    assert _win(oy=1 << 31) == EINVAL and _win(dy=1 << 31) == EINVAL and _win(dy=0) == EINVAL and _win(dx=-1) == EINVAL
    assert "upsampled" in _refused(_win(hi=1 << 28, wi=1, ho=1 << 30, wo=1, opts=_opts(shift=2)))
    # reflection with pad >= the logical extent (nn.ReflectionPad2d's rule), on every side; the same geometry without the mirror is only refused
    # for what the rule refuses
    assert "reflection" in _refused(_win(hi=2, wi=12, ho=2, wo=12, r=5, s=5, oy=-2, ox=-2, opts=_opts()))
    assert "reflection" in _refused(_win(hi=12, wi=2, ho=12, wo=2, r=5, s=5, oy=-2, ox=-2, opts=_opts()))
    assert "reflection" in _refused(_win(hi=3, wi=12, ho=6, wo=12, r=4, s=3, oy=0, ox=-1, opts=_opts()))      # the bottom mirror alone
    assert "reflection" not in _refused(_win(hi=3, wi=12, ho=3, wo=12, r=5, s=5, oy=-2, ox=-2, in_=0, opts=_opts()))
    assert "window form does not take" in _refused(_win(hi=97, wi=97, ho=97, wo=97, r=3, s=3, oy=-24, ox=-24, dy=24, dx=24))


def test_entry_point_refuses_what_the_rule_refuses():
    """The rule is the oracle: on a grid of geometries whose every other argument is in order, the entry point's only possible objection
    is the rule's, and it raises it exactly where the rule answers 0.  (A call the rule admits would reach a launch: with fake addresses
    it is not made -- a null input stands in, refused after the rule's own checks have run.)"""
    from diga_amd import _lib
    seen = set()
    for cin, cout, r, s, dy, dx, shift in itertools.product((32, 48, 64), (3, 64, 80), (1, 3, 7, 9), (1, 3, 8), (1, 2, 24), (1, 24), (0, 1, 3)):
        plan = _rule(12, 12, cin, cout, r, s, dy, dx, shift)
        kw = dict(cin=cin, in_ld=cin, cout=cout, out_ld=cout, r=r, s=s, oy=-(r // 2) * dy, ox=-(s // 2) * dx, dy=dy, dx=dx,
                  opts=_opts(reflect=0, shift=shift) if shift else None)
        if plan is None:
            assert _win(**kw) == EINVAL, kw
            assert "null pointer" not in _lib.last_error()
        seen.add(plan is None)
    assert seen == {True, False}


# ---------------------------------------------------------------------------------------------------------------- 5. the planner
def _fwd(n, h, w, cin, k, r, dil=1, stride=1, up=0, **kw):
    """_plan's arguments for the forward of an r x r layer with padding dil * (r // 2) on the 2^up upsampling of an h x w map."""
    pad = dil * (r // 2)
    ho, wo = (((v << up) + 2 * pad - dil * (r - 1) - 1) // stride + 1 for v in (h, w))
    return dict(n=n, hi=h, wi=w, cin=cin, k=k, r=r, s=r, stride=(stride, stride), off0=(-pad, -pad), doff=(dil, dil), ho=ho, wo=wo, **kw)


UP5A = _fwd(2, 24, 20, 256, 128, 5, up=1, opts=(1, 1, 0))         # the decoder's 5x5 layers behind the folded upsampling
UP5B = _fwd(2, 48, 40, 128, 64, 5, up=1, opts=(1, 1, 0))
TANH7 = _fwd(2, 96, 80, 64, 3, 7, opts=(1, 0, 1))                 # ... and its 7x7 with tanh
DOWN4 = dict(n=2, hi=48, wi=40, cin=64, k=128, r=4, s=4, stride=(2, 2), off0=(-1, -1), doff=(1, 1), ho=24, wo=20, opts=(1, 0, 0))
RES3 = _fwd(2, 24, 20, 256, 256, 3, opts=(1, 0, 0))               # a ResBlock conv (Winograd keeps it)
PLAIN5 = _fwd(2, 24, 20, 64, 64, 5)                                # no options
ASPP = _fwd(1, 97, 97, 2048, 256, 3, dil=24)                       # the window does not fit
BWD5 = dict(_fwd(2, 24, 20, 64, 64, 5), off0=(2, 2), doff=(-1, -1), tag=1)
CALLS = [UP5A, UP5B, TANH7, DOWN4, RES3, PLAIN5, ASPP, BWD5, dict(PLAIN5, stats="chunks"), dict(PLAIN5, epi=True, tag=1, doff=(-1, -1), off0=(2, 2))]
ON = dict(conv_math=2, x6_split="loader", x6_taps=True, x6_opts=True)


def test_plan_with_the_switch_on():
    from diga_amd import config
    from diga_amd.model import conv as dc
    win = dc._Path("x6win", "opts", 2, "bf16x6/window")
    taps = dc._Path("x6rs", "opts", 2, "bf16x6/taps")
    with config.override(**ON, winograd=False, x6_window=True):
        assert dc._plan(**UP5A) == win and dc._plan(**UP5B) == win and dc._plan(**TANH7) == win and dc._plan(**RES3) == win
        assert dc._plan(**PLAIN5) == dc._Path("x6win", "", 2, "bf16x6/window")
        assert dc._plan(**DOWN4) == taps                          # strided: unchanged
        assert dc._plan(**ASPP) == dc._Path("x6rs", "", 2, "bf16x6/taps")
        assert dc._plan(**BWD5) == dc._Path("x6rs", "", 2, "bf16x6/taps")          # backward-data never asks
        assert dc._plan(**dict(PLAIN5, stats="chunks")) == dc._Path("x6rs", "", 2, "bf16x6/taps")
        assert dc._plan(**CALLS[-1]) == dc._Path("x6rs", "epi", 2, "bf16x6/taps")
    with config.override(**ON, x6_window=True, fold_eval_bn=True, fold_eval_bn_x6=True, winograd=False):
        assert dc._plan(**dict(PLAIN5, infer=True)) == dc._Path("x6rs", "infer", 2, "bf16x6/taps+bn")
    with config.override(**ON, x6_window=True):                   # Winograd keeps what it takes
        assert dc._plan(**RES3).family == "winograd_reflect" and dc._plan(**TANH7) == win
    with config.override(conv_math=2, x6_split="loader", x6_taps=True, x6_opts=False, x6_window=True, winograd=False):
        assert dc._plan(**TANH7) == dc._Path("f32", "opts", 0, "f32")               # options need x6_opts (_taps_ok)
        assert dc._plan(**PLAIN5) == dc._Path("x6win", "", 2, "bf16x6/window")
    # the weight gradient never asks
    wg = dict(n=2, hi=24, wi=20, cp=64, kp=64, r=5, s=5, stride=(1, 1), padding=(2, 2), dilation=(1, 1), ho=24, wo=20)
    with config.override(**ON, winograd=False, x6_window=False):
        off = dc._wgrad_plan(**wg)
    with config.override(**ON, winograd=False, x6_window=True):
        assert dc._wgrad_plan(**wg) == off == dc._Path("x6rs", "", 2, "bf16x6/taps")


def test_switch_off_gives_the_previous_answers():
    from diga_amd import config
    from diga_amd.model import conv as dc
    lit = {id(UP5A): dc._Path("x6rs", "opts", 2, "bf16x6/taps"), id(TANH7): dc._Path("x6rs", "opts", 2, "bf16x6/taps"),
           id(PLAIN5): dc._Path("x6rs", "", 2, "bf16x6/taps"), id(DOWN4): dc._Path("x6rs", "opts", 2, "bf16x6/taps")}
    for wino in (False, True):
        with config.override(**ON, winograd=wino, x6_window=False):
            off = [dc._plan(**c) for c in CALLS]
            for c in (UP5A, TANH7, PLAIN5, DOWN4):
                assert dc._plan(**c) == lit[id(c)]
            assert all(p.family != "x6win" for p in off)
        with config.override(**ON, winograd=wino):
            if not config.DEFAULTS.x6_window:
                assert off == [dc._plan(**c) for c in CALLS]
    # outside conv_math = 2, and without x6_taps, the switch changes nothing
    for base in (dict(conv_math=0), dict(conv_math=1), dict(conv_math=2, x6_taps=False, x6_opts=True), dict(conv_math=0, x6_taps=True, x6_opts=True)):
        with config.override(**base, x6_window=False):
            off = [dc._plan(**c) for c in CALLS]
        with config.override(**base, x6_window=True):
            assert off == [dc._plan(**c) for c in CALLS]
