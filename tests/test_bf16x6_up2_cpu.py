"""CPU-side checks of the bf16x6 upsample + conv on phase-collapsed weights (config.x6_up2; csrc/conv_bf16x6.h, model/conv.py): the switch,
the collapse itself in float64 against interpolate + pad + conv2d (and why the border needs the ring), the rule
(diga_conv_up2_bf16x6_plan) against its host restatement (tools/bf16x6_emulation.py) on a grid, the entry point's refusals -- which answer
before anything touches a device --, the planner's answers and the C ABI surface."""
import ctypes
import importlib.util
import itertools
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN, COLLAPSE, UP2 = "diga_conv_up2_bf16x6_plan", "diga_collapse_up2_weights", "diga_conv_up2_bf16x6_f32in"
EINVAL, EALIGN = -1, -2
A = 1 << 20                      # a 16-byte aligned, non-null address: never dereferenced (every call below fails its checks)
TH, TW = 8, 16                   # the window kernel's output tile


def _emulation():
    spec = importlib.util.spec_from_file_location("bf16x6_emulation", os.path.join(ROOT, "tools", "bf16x6_emulation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------------------- 1. the switch
def test_step_config_x6_up2(monkeypatch):
    from diga_amd import config
    from diga_amd.model import conv as dc
    assert config.StepConfig().x6_up2 is False                    # opt-in
    assert config.DEFAULTS.x6_up2 is False or "DIGA_X6_UP2" in os.environ
    assert config.StepConfig(x6_up2=True).validate().x6_up2 is True
    assert config.StepConfig().replace(x6_up2=True).x6_up2 is True
    with pytest.raises(ValueError):
        config.StepConfig(x6_up2="yes").validate()
    with pytest.raises(ValueError):
        config.StepConfig().replace(x6_up2=1)
    monkeypatch.setenv("DIGA_X6_UP2", "1")
    assert config.StepConfig.from_env().x6_up2 is True
    monkeypatch.setenv("DIGA_X6_UP2", "0")
    assert config.StepConfig.from_env().x6_up2 is False
    monkeypatch.delenv("DIGA_X6_UP2")
    assert config.StepConfig.from_env().x6_up2 is False
    # it means something only under conv_math = 2 with x6_opts (the planner asks only where x6_taps and x6_window hold already)
    geo = (96, 96, 256, 128, 192, 192, 5, 5, (-2, -2), (1, 1), (1, 1, 0))
    for math in (0, 1):
        with config.override(x6_up2=True, x6_taps=True, x6_opts=True, x6_window=True, conv_math=math):
            assert not dc._x6_up2(*geo)
    with config.override(x6_up2=True, x6_taps=True, x6_opts=False, x6_window=True, conv_math=2):
        assert not dc._x6_up2(*geo)
    with config.override(x6_up2=False, x6_taps=True, x6_opts=True, x6_window=True, conv_math=2):
        assert not dc._x6_up2(*geo)
    with config.override(x6_up2=True, x6_taps=True, x6_opts=True, x6_window=True, conv_math=2):
        assert dc._x6_up2(*geo)
    assert config.active().x6_up2 == config.DEFAULTS.x6_up2


# ---------------------------------------------------------------------------------------------------------------- 2. the collapse, float64
def _collapsed_forward(x, wc, first, ho, wo):
    """The four stride-1 convolutions of the SOURCE image x [N,C,H,W] with the collapsed weights wc [2,2,K,R',S',C], interleaved into
    the [N,K,ho,wo] output.  Source pixels outside the image are clamped (what the kernel's window does); output pixels whose
    source rows would leave even the clamped margin stay NaN."""
    P = 4
    xp = F.pad(x, (P, P, P, P), mode="replicate")
    out = torch.full((x.shape[0], wc.shape[2], ho, wo), float("nan"), dtype=x.dtype)
    for fy in (0, 1):
        for fx in (0, 1):
            o = F.conv2d(xp, wc[fy, fx].permute(0, 3, 1, 2))      # o[y'] reads xp rows y' .. y' + R' - 1 = source rows y' - P ..
            ys, xs = torch.arange(fy, ho, 2), torch.arange(fx, wo, 2)
            yy, xx = ys // 2 + first[fy][fx][0] + P, xs // 2 + first[fy][fx][1] + P
            oky, okx = (yy >= 0) & (yy < o.shape[2]), (xx >= 0) & (xx < o.shape[3])
            out[:, :, ys[oky][:, None], xs[okx][None, :]] = o[:, :, yy[oky]][:, :, :, xx[okx]]
    return out


COLLAPSE_CASES = [(5, 5, 2, 2), (3, 3, 1, 1), (7, 7, 3, 3), (4, 4, 1, 1), (5, 3, 2, 1)]           # R, S, pad_y, pad_x
WANT_TAPS = {(5, 2): 3, (3, 1): 2, (7, 3): 4, (4, 1): 3}                                         # (R, pad) -> R'


@pytest.mark.parametrize("r,s,py,px", COLLAPSE_CASES)
@pytest.mark.parametrize("reflect", (True, False))
@pytest.mark.parametrize("h,w", ((12, 24), (13, 21)))
def test_collapse_reproduces_the_interior_in_float64(r, s, py, px, reflect, h, w):
    em = _emulation()
    g = torch.Generator().manual_seed(2000 + 100 * r + 10 * s + h)
    x = torch.randn((2, 4, h, w), generator=g, dtype=torch.float64)
    wt = torch.randn((3, r, s, 4), generator=g, dtype=torch.float64)
    ref = F.conv2d(F.pad(F.interpolate(x, scale_factor=2.0, mode="nearest"), (px, px, py, py), mode="reflect" if reflect else "constant"),
                   wt.permute(0, 3, 1, 2))
    ho, wo = ref.shape[2:]
    assert (ho, wo) == (2 * h + 2 * py - r + 1, 2 * w + 2 * px - s + 1)
    wc, first = em.collapse_up2(wt, -py, -px)
    assert wc.dtype == torch.float64 and tuple(wc.shape) == (2, 2, 3, em.up2_taps(r, -py), em.up2_taps(s, -px), 4)
    assert em.up2_taps(r, -py) == WANT_TAPS[(r, py)] and em.up2_taps(s, -px) == WANT_TAPS[(s, px)]
    got = _collapsed_forward(x, wc, first, ho, wo)
    # every output pixel whose taps all stay inside the logical image [0, 2h) x [0, 2w) is reproduced ...
    exact = (slice(None), slice(None), slice(py, 2 * h + py - r + 1), slice(px, 2 * w + px - s + 1))
    assert ref[exact].numel() > 0
    err = float((got[exact] - ref[exact]).abs().max() / ref.abs().max())
    assert err <= 1e-12, err
    # ... and where the rule takes the geometry (all but 7 x 7 on 13 rows, whose last interior row reads the padding) the interior tiles
    # of the 8 x 16 grid lie inside that region
    admitted = em.up2_rule(h, w, 32, 64, ho, wo, r, s, -py, -px)
    assert (admitted is None) == ((r, h) == (7, 13)) and admitted in (None, (wc.shape[3], wc.shape[4]))
    if admitted:
        ty, tx = -(-ho // TH), -(-wo // TW)
        inter = (slice(None), slice(None), slice(TH, (ty - 1) * TH), slice(TW, (tx - 1) * TW))
        assert ref[inter].numel() > 0
        assert py <= TH and (ty - 1) * TH <= 2 * h + py - r + 1 and px <= TW and (tx - 1) * TW <= 2 * w + px - s + 1
        err = float((got[inter] - ref[inter]).abs().max() / ref.abs().max())
        assert err <= 1e-12, err
    # every weight lands in exactly one group: each phase's collapsed taps sum to the layer's
    for fy, fx in itertools.product((0, 1), (0, 1)):
        assert float((wc[fy, fx].sum((1, 2)) - wt.sum((1, 2))).abs().max()) < 1e-12


def test_collapse_groups_of_the_5x5_layer_and_the_border():
    em = _emulation()
    # 5 x 5 at pad 2: phase 0 collapses rows {0, 1 | 2, 3 | 4} onto source rows y - 1, y, y + 1; phase 1 {0 | 1, 2 | 3, 4}
    assert em.up2_rows(5, -2, 0) == [-1, -1, 0, 0, 1] and em.up2_rows(5, -2, 1) == [-1, 0, 0, 1, 1]
    assert em.up2_rows(4, -1, 0) == [-1, 0, 0, 1] and em.up2_rows(4, -1, 1) == [0, 0, 1, 1]       # 4 x 4 at pad 1: 3 and 2 taps
    g = torch.Generator().manual_seed(2099)
    x = torch.randn((1, 4, 12, 24), generator=g, dtype=torch.float64)
    wt = torch.randn((3, 5, 5, 4), generator=g, dtype=torch.float64)
    ref = F.conv2d(F.pad(F.interpolate(x, scale_factor=2.0, mode="nearest"), (2, 2, 2, 2), mode="reflect"), wt.permute(0, 3, 1, 2))
    wc, first = em.collapse_up2(wt, -2, -2)
    got = _collapsed_forward(x, wc, first, 24, 48)
    # a pixel whose taps reach the mirror: logical -1 is source 0, logical -2 source 1 -- no "source row -1" serves both.  That is why
    # the ring of border tiles stays on the 25-tap walk.
    assert float((got[:, :, 0, 0] - ref[:, :, 0, 0]).abs().max() / ref.abs().max()) > 1e-3
    assert float((got[:, :, 23, 47] - ref[:, :, 23, 47]).abs().max() / ref.abs().max()) > 1e-3
    # fp32 weights: summed in double, rounded once
    w32 = wt.float()
    wc32, _ = em.collapse_up2(w32, -2, -2)
    assert wc32.dtype == torch.float32
    assert torch.equal(wc32[0, 0, :, 0, 0, :], (w32[:, 0, 0].double() + w32[:, 0, 1].double() + w32[:, 1, 0].double()
                                                + w32[:, 1, 1].double()).float())


# ---------------------------------------------------------------------------------------------------------------- 3. the rule
def _rule(hi, wi, cin, cout, ho, wo, r, s, oy, ox, dy=1, dx=1, shift=1, reflect=1):
    """diga_conv_up2_bf16x6_plan -> (R', S') or None."""
    from diga_amd import _lib
    rc, sc = ctypes.c_int(-1), ctypes.c_int(-1)
    ok = _lib.lib.diga_conv_up2_bf16x6_plan(hi, wi, cin, cout, ho, wo, r, s, oy, ox, dy, dx, shift, reflect, ctypes.byref(rc), ctypes.byref(sc))
    assert ok in (0, 1)
    if ok == 0:
        assert (rc.value, sc.value) == (-1, -1)                   # nothing written
        return None
    return rc.value, sc.value


def test_rule_equals_its_host_restatement_on_a_grid():
    em = _emulation()
    from diga_amd import _lib
    # the two decoder layers of the translator at the bench's size
    assert _rule(96, 96, 256, 128, 192, 192, 5, 5, -2, -2) == (3, 3)
    assert _rule(192, 192, 128, 64, 384, 384, 5, 5, -2, -2) == (3, 3)
    base = dict(hi=12, wi=24, cin=32, cout=64, ho=24, wo=48, r=5, s=5, oy=-2, ox=-2)
    assert _rule(**base) == (3, 3)
    refused = [dict(shift=0), dict(shift=2), dict(dy=2), dict(dx=2), dict(cout=16), dict(cout=3), dict(cin=48), dict(r=8, oy=-3), dict(s=8, ox=-3),
               dict(ho=16), dict(wo=32), dict(oy=1), dict(ox=1), dict(r=1, oy=0), dict(reflect=2), dict(hi=0), dict(cin=0),
               dict(hi=8), dict(wi=16),                           # a tap of the last interior row / column leaves the logical image
               dict(oy=-9), dict(ox=-17)]                         # ... of the first one
    for kw in refused:
        assert _rule(**dict(base, **kw)) is None, kw
        assert em.up2_rule(*(dict(base, **kw)[k] for k in ("hi", "wi", "cin", "cout", "ho", "wo", "r", "s", "oy", "ox")),
                           **{{"dy": "dil_y", "dx": "dil_x"}.get(k, k): v for k, v in kw.items() if k in ("dy", "dx", "shift", "reflect")}) is None, kw
    i = ctypes.c_int(0)
    assert _lib.lib.diga_conv_up2_bf16x6_plan(12, 24, 32, 64, 24, 48, 5, 5, -2, -2, 1, 1, 1, 1, None, ctypes.byref(i)) == 0
    seen = set()
    for (hi, wi), cin, cout, r, s, pad_d, shift, dil in itertools.product(((12, 24), (13, 21), (8, 24), (12, 16), (20, 40)), (32, 48, 128),
                                                                         (16, 17, 80), (2, 3, 4, 5, 7, 8), (3, 5), (0, 1), (0, 1, 2), (1, 2)):
        py, px = r // 2 - pad_d, s // 2
        ho, wo = 2 * hi + 2 * py - r + 1, 2 * wi + 2 * px - s + 1
        got = _rule(hi, wi, cin, cout, ho, wo, r, s, -py, -px, dil, dil, shift, 1)
        assert got == em.up2_rule(hi, wi, cin, cout, ho, wo, r, s, -py, -px, dil, dil, shift, 1), (hi, wi, cin, cout, r, s, py, shift, dil)
        seen.add(got)
    assert None in seen and (3, 3) in seen and (2, 2) in seen and (4, 3) in seen


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def _opts(reflect=1, shift=1, act=0):
    from diga_amd import _lib
    return _lib.ConvOptions(reflect, shift, act)


_DEFAULT = object()


def _up2(in_=A, in_ld=32, img=A, phases=A, bias=None, out=A, n=1, hi=12, wi=24, cin=32, ho=24, wo=48, cout=64, out_ld=64, r=5, s=5, oy=-2,
         ox=-2, opts=_DEFAULT, tag=0):
    """One call of the new export on a 1 x 12 x 24 x 32 -> 64 5x5 layer behind a 2x upsampling, with fake addresses."""
    from diga_amd import _lib
    if opts is _DEFAULT:
        opts = _opts()
    return _lib.lib.diga_conv_up2_bf16x6_f32in(in_, in_ld, img, phases, bias, out, n, hi, wi, cin, ho, wo, cout, out_ld, r, s, oy, ox,
                                               ctypes.byref(opts) if opts is not None else None, tag, None)


def _refused(rc, want=EINVAL):
    from diga_amd import _lib
    assert rc == want, rc
    msg = _lib.last_error()
    assert msg != ""
    return msg


def test_entry_point_rejects_bad_arguments():
    for kw in (dict(in_=0), dict(img=0), dict(phases=0), dict(out=0), dict(opts=None)):
        assert "null pointer" in _refused(_up2(**kw)), kw
    assert _up2(in_=A + 4) == EALIGN and _up2(img=A + 8) == EALIGN and _up2(phases=A + 8) == EALIGN and _up2(out=A + 2) == EALIGN
    assert _up2(bias=A + 1) == EALIGN
    assert "multiple of 32" in _refused(_up2(cin=48, in_ld=48))
    assert _up2(out_ld=32) == EINVAL
    assert "in_ld" in _refused(_up2(in_ld=16)) and _up2(in_ld=34) == EINVAL and _up2(in_ld=-1) == EINVAL
    for bad in (_opts(reflect=2), _opts(act=2), _opts(shift=3), _opts(shift=-1)):
        assert "bad options" in _refused(_up2(opts=bad))
    assert _up2(n=0) == EINVAL and _up2(ho=0) == EINVAL and _up2(cout=0, out_ld=0) == EINVAL
    assert _up2(oy=-(1 << 31)) == EINVAL
    for kw in (dict(opts=_opts(shift=0)), dict(opts=_opts(shift=2)), dict(cout=16, out_ld=16), dict(r=8, oy=-3), dict(ho=16), dict(oy=1)):
        assert "diga_conv_up2_bf16x6_plan" in _refused(_up2(**kw)), kw
    # reflection padding not smaller than the logical extent: the window entry point's check (no admitted geometry reaches it through the
    # interior condition with offsets <= 0, so it is the rule that answers)
    assert _up2(hi=2, ho=4, r=5, oy=-4) == EINVAL
    # the collapse export
    from diga_amd import _lib

    def col(w=A, wc=A, k=64, r=5, s=5, c=32, oy=-2, ox=-2):
        return _lib.lib.diga_collapse_up2_weights(w, wc, k, r, s, c, oy, ox, None)

    for kw in (dict(w=0), dict(wc=0), dict(k=0), dict(c=0), dict(r=8), dict(s=1), dict(oy=1), dict(ox=1)):
        assert col(**kw) == EINVAL, kw
    assert col(w=A + 4) == EALIGN and col(wc=A + 8) == EALIGN


def test_entry_point_refuses_what_the_rule_refuses():
    """The rule is the oracle: on a grid of geometries whose every other argument is in order, the entry point's only possible objection
    is the rule's, and it raises it exactly where the rule answers 0.  (A call the rule admits would reach a launch: with fake addresses
    it is not made.)"""
    from diga_amd import _lib
    seen = set()
    for (hi, wi), cin, cout, r, s, shift in itertools.product(((12, 24), (8, 24), (12, 16), (13, 21)), (32, 48), (16, 64, 80), (1, 3, 5, 8), (3, 4),
                                                             (0, 1, 2)):
        py, px = r // 2, s // 2
        ho, wo = (hi << shift) + 2 * py - r + 1, (wi << shift) + 2 * px - s + 1
        plan = _rule(hi, wi, cin, cout, ho, wo, r, s, -py, -px, 1, 1, shift, 0)
        if plan is None:
            kw = dict(hi=hi, wi=wi, cin=cin, in_ld=cin, cout=cout, out_ld=cout, ho=ho, wo=wo, r=r, s=s, oy=-py, ox=-px, opts=_opts(0, shift))
            assert _up2(**kw) == EINVAL, kw
            assert "null pointer" not in _lib.last_error()
        seen.add(plan is None)
    assert seen == {True, False}


# ---------------------------------------------------------------------------------------------------------------- 5. the planner
def _fwd(n, h, w, cin, k, r, dil=1, stride=1, up=0, **kw):
    """_plan's arguments for the forward of an r x r layer with padding dil * (r // 2) on the 2^up upsampling of an h x w map."""
    pad = dil * (r // 2)
    ho, wo = (((v << up) + 2 * pad - dil * (r - 1) - 1) // stride + 1 for v in (h, w))
    return dict(n=n, hi=h, wi=w, cin=cin, k=k, r=r, s=r, stride=(stride, stride), off0=(-pad, -pad), doff=(dil, dil), ho=ho, wo=wo, **kw)


DEC_A = _fwd(8, 96, 96, 256, 128, 5, up=1, opts=(1, 1, 0))          # the translator's two upsampled decoder layers, 8 crops of 768 x 768
DEC_B = _fwd(8, 192, 192, 128, 64, 5, up=1, opts=(1, 1, 0))
TANH7 = _fwd(8, 768, 768, 64, 3, 7, opts=(1, 0, 1))                 # 7 x 7 64 -> 3 with tanh: no upsampling, Cout <= 16
DOWN4 = dict(n=8, hi=768, wi=768, cin=64, k=128, r=4, s=4, stride=(2, 2), off0=(-1, -1), doff=(1, 1), ho=384, wo=384, opts=(1, 0, 0))
DOWN4B = dict(n=8, hi=384, wi=384, cin=128, k=256, r=4, s=4, stride=(2, 2), off0=(-1, -1), doff=(1, 1), ho=192, wo=192, opts=(1, 0, 0))
SMALL = _fwd(1, 4, 8, 64, 64, 5, up=1, opts=(1, 1, 0))               # one tile row: no interior
PLAIN5 = _fwd(2, 24, 20, 64, 64, 5)                                  # no options
CALLS = [DEC_A, DEC_B, TANH7, DOWN4, DOWN4B, SMALL, PLAIN5]
ON = dict(conv_math=2, x6_split="loader", x6_taps=True, x6_opts=True, x6_window=True, winograd=False)


def test_plan_with_the_switch_on_and_off():
    from diga_amd import config
    from diga_amd.model import conv as dc
    up2 = dc._Path("x6up2", "opts", 2, "bf16x6/up2")
    win = dc._Path("x6win", "opts", 2, "bf16x6/window")
    taps = dc._Path("x6rs", "opts", 2, "bf16x6/taps")
    with config.override(**ON, x6_up2=True):
        assert dc._plan(**DEC_A) == up2 and dc._plan(**DEC_B) == up2
        assert dc._plan(**TANH7) == win and dc._plan(**SMALL) == win
        assert dc._plan(**DOWN4) == taps and dc._plan(**DOWN4B) == taps
        assert dc._plan(**PLAIN5) == dc._Path("x6win", "", 2, "bf16x6/window")
    # off or absent: the parent's answers
    with config.override(**ON, x6_up2=False):
        off = [dc._plan(**c) for c in CALLS]
        assert off == [win, win, win, taps, taps, win, dc._Path("x6win", "", 2, "bf16x6/window")]
    with config.override(**ON):
        if not config.DEFAULTS.x6_up2:
            assert off == [dc._plan(**c) for c in CALLS]
    # outside conv_math = 2, or without x6_window / x6_opts / x6_taps, the switch is inert
    for base in (dict(ON, conv_math=0), dict(ON, conv_math=1), dict(ON, x6_window=False), dict(ON, x6_opts=False), dict(ON, x6_taps=False)):
        with config.override(**base, x6_up2=False):
            ref = [dc._plan(**c) for c in CALLS]
        with config.override(**base, x6_up2=True):
            assert ref == [dc._plan(**c) for c in CALLS], base
        assert all(p.family != "x6up2" for p in ref)
    # the weight gradient never asks
    wg = dict(n=2, hi=24, wi=20, cp=64, kp=64, r=5, s=5, stride=(1, 1), padding=(2, 2), dilation=(1, 1), ho=24, wo=20)
    with config.override(**ON, x6_up2=False):
        ref = dc._wgrad_plan(**wg)
    with config.override(**ON, x6_up2=True):
        assert dc._wgrad_plan(**wg) == ref
    assert dc._ENTRY[("x6up2", "opts")] == UP2 and ("x6up2", "") not in dc._ENTRY


# ---------------------------------------------------------------------------------------------------------------- 6. the C ABI
def _header_signature(hdr, name):
    """The ctypes form of the prototype of `name` in include/diga_hip.h."""
    from diga_amd import _lib
    m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/diga_hip.h"
    args = []
    for a in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(","):
        a = " ".join(a.split())
        args.append(_lib.P if "*" in a else _lib.I64 if a.startswith("int64_t ") else _lib.INT if a.startswith("int ") else None)
    return (_lib.INT if m.group(1) == "int" else _lib.SZ), args


def test_exports_header_and_signatures_agree():
    from diga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    fresh = ctypes.CDLL(_lib.LIB_PATH)                           # the dynamic symbol table of the library itself
    for name in (PLAN, COLLAPSE, UP2):
        assert not name.startswith("diga_conv2d_")               # (the dispatch fixture enumerates diga_conv2d_*)
        assert hasattr(fresh, name), f"{name} is not exported by {_lib.LIB_PATH}"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert _lib.SIGNATURES[name] == _header_signature(hdr, name), name
    I64, P, INT = _lib.I64, _lib.P, _lib.INT
    assert _lib.SIGNATURES[PLAN] == (INT, [I64] * 14 + [P] * 2)
    assert _lib.SIGNATURES[COLLAPSE] == (INT, [P, P] + [I64] * 6 + [P])
    # the window entry point's list with the phases' images behind the layer's, without the dilation
    res, args = _lib.SIGNATURES["diga_conv_window_bf16x6_f32in"]
    assert _lib.SIGNATURES[UP2] == (res, args[:3] + [P] + args[3:-5] + args[-3:])
    assert len(_lib.PROF_TAGS) == 23                             # no new profiling tag
