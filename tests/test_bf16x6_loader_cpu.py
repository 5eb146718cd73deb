"""CPU-side checks of the loader-split form of bf16x6 (config.x6_split = "loader", the `_f32in` entry points of csrc/conv_bf16x6.h):
the configuration surface, the C ABI surface and the argument checks of the three new entry points, which answer before anything
touches a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["diga_conv2d_nhwc_bf16x6_f32in", "diga_conv2d_nhwc_bf16x6_f32in_epi", "diga_conv2d_wgrad_bf16x6_f32in"]
EINVAL, EALIGN = -1, -2
A = 1 << 20                      # a 16-byte aligned, non-null address: never dereferenced (every call below fails its checks)


def test_step_config_x6_split(monkeypatch):
    from diga_amd import config
    assert config.StepConfig().x6_split == "pass"                 # the default stays the pass form
    assert config.StepConfig(x6_split="loader").validate().x6_split == "loader"
    assert config.StepConfig().replace(x6_split="loader").x6_split == "loader"
    with pytest.raises(ValueError):
        config.StepConfig(x6_split="x").validate()
    with pytest.raises(ValueError):
        config.StepConfig().replace(x6_split="x")
    monkeypatch.setenv("DIGA_X6_SPLIT", "loader")
    assert config.StepConfig.from_env().x6_split == "loader"
    monkeypatch.setenv("DIGA_X6_SPLIT", "pass")
    assert config.StepConfig.from_env().x6_split == "pass"
    monkeypatch.setenv("DIGA_X6_SPLIT", "x")
    with pytest.raises(ValueError):
        config.StepConfig.from_env()
    monkeypatch.delenv("DIGA_X6_SPLIT")
    assert config.StepConfig.from_env().x6_split == "pass"
    with config.override(x6_split="loader"):
        assert config.active().x6_split == "loader"
        from diga_amd.model import conv as dc
        assert dc._x6_loader()
    assert config.active().x6_split == config.DEFAULTS.x6_split


def test_entry_points_are_declared_bound_and_exported():
    from diga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/diga_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    fresh = ctypes.CDLL(_lib.LIB_PATH)                           # the dynamic symbol table of the library itself
    for name in NEW_ENTRY_POINTS:
        assert hasattr(fresh, name), f"{name} is not exported by {_lib.LIB_PATH}"
    assert len(_lib.PROF_TAGS) == 23                             # no new profiling tag


def _fwd(in_=A, in_ld=64, img=A, bias=0, out=A, cin=64, cout=64, r=1, s=1):
    from diga_amd import _lib
    return _lib.lib.diga_conv2d_nhwc_bf16x6_f32in(in_, in_ld, img, bias, out, 1, 4, 4, cin, 4, 4, cout, cout, r, s, 1, 1, 0, 0, 1, 1, 0,
                                                  _lib.PROF_TAGS.index("conv_fwd"), 0)


def _epi(in_=A, in_ld=64, img=A, out=A, cin=64, cout=64, r=1, s=1, epi=True):
    from diga_amd import _lib
    e = _lib.BwdEpilogue()
    return _lib.lib.diga_conv2d_nhwc_bf16x6_f32in_epi(in_, in_ld, img, out, 1, 4, 4, cin, 4, 4, cout, cout, r, s, 1, 1, 0, 0, 1, 1,
                                                      ctypes.byref(e) if epi else None, _lib.PROF_TAGS.index("conv_bwd_data"), 0)


def _wgrad(dy=A, dy_ld=64, x=A, x_ld=64, dw=A, ws=A, ws_bytes=1 << 30, cin=64, cout=64, r=1, s=1):
    from diga_amd import _lib
    return _lib.lib.diga_conv2d_wgrad_bf16x6_f32in(dy, dy_ld, x, x_ld, dw, ws, ws_bytes, 1, 4, 4, cin, 4, 4, cout, r, s, 1, 1, 0, 0, 1, 1, 0)


@pytest.mark.parametrize("call", [_fwd, _epi], ids=["f32in", "f32in_epi"])
def test_forward_entry_points_reject_bad_arguments(call):
    assert call(in_ld=32) == EINVAL                              # in_ld < Cin
    assert call(in_ld=66) == EINVAL                              # in_ld % 4 != 0
    assert call(in_ld=-4) == EINVAL
    assert call(cin=48, in_ld=48) == EINVAL                      # Cin % 32 != 0
    assert call(r=3, s=3) == EINVAL                              # pointwise only
    assert call(in_=0) == EINVAL and call(img=0) == EINVAL and call(out=0) == EINVAL
    assert call(in_=A + 4) == EALIGN                             # a misaligned fp32 operand
    assert call(in_=A + 8, in_ld=72) == EALIGN
    assert call(img=A + 4) == EALIGN


def test_epilogue_entry_point_needs_its_descriptor():
    assert _epi(epi=False) == EINVAL


def test_weight_gradient_entry_point_rejects_bad_arguments():
    assert _wgrad(dy_ld=32) == EINVAL                            # dy_ld < Cout
    assert _wgrad(x_ld=32) == EINVAL                             # x_ld < Cin
    assert _wgrad(dy_ld=66) == EINVAL and _wgrad(x_ld=70) == EINVAL      # ld % 4 != 0
    assert _wgrad(dy_ld=-1) == EINVAL and _wgrad(x_ld=-1) == EINVAL
    assert _wgrad(cin=12, x_ld=12) == EINVAL and _wgrad(cout=12, dy_ld=12) == EINVAL     # channel counts % 8
    assert _wgrad(r=3, s=3) == EINVAL
    for name in ("dy", "x", "dw", "ws"):
        assert _wgrad(**{name: 0}) == EINVAL, name
    assert _wgrad(dy=A + 4) == EALIGN and _wgrad(x=A + 4) == EALIGN and _wgrad(dw=A + 4) == EALIGN
    assert _wgrad(ws_bytes=16) == -3                             # DIGA_EWORKSPACE: the triplet form's workspace rule
