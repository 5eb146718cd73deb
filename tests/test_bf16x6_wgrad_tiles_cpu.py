"""CPU-side checks of the narrow tiles of the bf16x6 weight gradient (config.x6_wgrad_tile = "fit"; csrc/conv_bf16x6.h, model/conv.py): the
configuration field, the planner's answers with the switch off and on, the tile rule, the C ABI surface, the argument checks of the new
entry point -- which answer before anything touches a device -- and the workspace query against a restatement of the new split-K plan."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["diga_wgrad_bf16x6_tile", "diga_wgrad_bf16x6_tiled_workspace_bytes", "diga_wgrad_bf16x6_tiled_f32in"]
EINVAL, EALIGN, EWORKSPACE = -1, -2, -3
A = 1 << 20                      # a 16-byte aligned, non-null address: never dereferenced (every call below fails its checks)
BIG = 1 << 40


# ---------------------------------------------------------------------------------------------------------------- restatements
def tile_rule(cout, cin):
    """The three-line rule of the issue: BM by Cout, BN by Cin, the uninstantiated (128, 64) answers (128, 128)."""
    bm = 64 if cout <= 64 else 128 if cout <= 128 else 256
    bn = 64 if cin <= 64 else 128
    return (128, 128) if (bm, bn) == (128, 64) else (bm, bn)


BLOCKS_PER_CU = {(64, 64): 3, (64, 128): 2, (128, 128): 1, (256, 64): 1}       # 160 KB of LDS / (2 x 3 x 32 x (BM + BN) x 2 B)


def wide_splits(m, cout, cin, rs=1):
    """plan_wgrad_x6: 512 blocks over the 256 x 128 tiles, at least 8 K-steps of 32 pixels per block -> (splits, steps per split)."""
    tiles = -(-cout // 256) * -(-cin // 128) * rs
    ksteps = -(-m // 32)
    splits = min(-(-512 // tiles), max(ksteps // 8, 1), 512)
    steps = -(-ksteps // splits)
    return -(-ksteps // steps), steps


def fit_splits(m, cout, cin, rs=1):
    """plan_wgrad_x6 on the tile of the tile rule: two rounds of resident blocks (256 CUs x blocks per CU) over the BM x BN tiles, the same 8-K-step floor and
    the same cap of 512 ranges; a (256, 128) shape keeps the wide plan."""
    bm, bn = tile_rule(cout, cin)
    if (bm, bn) == (256, 128):
        return wide_splits(m, cout, cin, rs)
    tiles = -(-cout // bm) * -(-cin // bn) * rs
    ksteps = -(-m // 32)
    splits = min(-(-2 * 256 * BLOCKS_PER_CU[(bm, bn)] // tiles), max(ksteps // 8, 1), 512)
    steps = -(-ksteps // splits)
    return -(-ksteps // steps), steps


def mpad(m):
    return (m + 31) // 32 * 32 + 64


def _tile(cout, cin):
    from diga_amd import _lib
    bm, bn = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = _lib.lib.diga_wgrad_bf16x6_tile(cout, cin, ctypes.byref(bm), ctypes.byref(bn))
    return rc, (bm.value, bn.value)


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_step_config_x6_wgrad_tile(monkeypatch):
    from diga_amd import config
    from diga_amd.model import conv as dc
    assert config.StepConfig().x6_wgrad_tile == "wide"             # opt-in
    assert config.DEFAULTS.x6_wgrad_tile == "wide" or "DIGA_X6_WGRAD_TILE" in os.environ
    assert config.StepConfig(x6_wgrad_tile="fit").validate().x6_wgrad_tile == "fit"
    assert config.StepConfig().replace(x6_wgrad_tile="fit").x6_wgrad_tile == "fit"
    for bad in ("narrow", "", True, 1, None):
        with pytest.raises(ValueError):
            config.StepConfig(x6_wgrad_tile=bad).validate()
    with pytest.raises(ValueError):
        config.StepConfig().replace(x6_wgrad_tile="Fit")
    monkeypatch.setenv("DIGA_X6_WGRAD_TILE", "fit")
    assert config.StepConfig.from_env().x6_wgrad_tile == "fit"
    monkeypatch.setenv("DIGA_X6_WGRAD_TILE", "wide")
    assert config.StepConfig.from_env().x6_wgrad_tile == "wide"
    monkeypatch.setenv("DIGA_X6_WGRAD_TILE", "tall")
    with pytest.raises(ValueError):
        config.StepConfig.from_env()
    monkeypatch.delenv("DIGA_X6_WGRAD_TILE")
    assert config.StepConfig.from_env().x6_wgrad_tile == "wide"
    # without conv_math = 2 the switch selects nothing; with it, only the layers the tile rule moves
    for math in (0, 1):
        with config.override(x6_wgrad_tile="fit", conv_math=math):
            assert not dc._x6_fit(64, 64)
    with config.override(x6_wgrad_tile="fit", conv_math=2):
        assert dc._x6_fit(64, 64) and dc._x6_fit(64, 256) and dc._x6_fit(128, 512) and not dc._x6_fit(512, 256)
    with config.override(x6_wgrad_tile="wide", conv_math=2):
        assert not dc._x6_fit(64, 64)
    assert config.active().x6_wgrad_tile == config.DEFAULTS.x6_wgrad_tile


# ---------------------------------------------------------------------------------------------------------------- planner
def _pw(n, h, w, cin, k):
    return (n, h, w, cin, k, 1, 1, (1, 1), (0, 0), (1, 1), h, w), {}


def _c3(n, h, w, cin, k):
    return (n, h, w, cin, k, 3, 3, (1, 1), (1, 1), (1, 1), h, w), {}


# (call, whether the tile rule moves it) -- layer1's and layer2's narrow layers, the stem, and a layer on the wide tile
WCALLS = [(_pw(2, 97, 97, 64, 64), True), (_pw(2, 97, 97, 256, 64), True), (_pw(2, 97, 97, 64, 256), True), (_pw(2, 49, 49, 512, 128), True),
          (_c3(2, 97, 97, 64, 64), True), (_c3(2, 49, 49, 128, 128), True),
          (((2, 97, 97, 160, 64, 1, 1, (1, 1), (0, 0), (1, 1), 97, 97), dict(stem=True)), True),
          (_pw(2, 49, 49, 256, 512), False)]


def _answers():
    from diga_amd.model import conv as dc
    return [dc._wgrad_plan(*a, **kw) for (a, kw), _ in WCALLS]


def test_plan_with_the_switch_off_and_on():
    from diga_amd import config
    from diga_amd.model import conv as dc
    ls, taps = dc._Path("x6ls", "", 2, "bf16x6/ls"), dc._Path("x6rs", "", 2, "bf16x6/taps")
    ls_fit = dc._Path("x6ls", "", 2, "bf16x6/ls/fit", fit=True)
    taps_fit = dc._Path("x6rs", "", 2, "bf16x6/taps/fit", fit=True)
    for split in ("pass", "loader"):
        for x6_taps in (False, True):
            with config.override(conv_math=2, x6_split=split, x6_taps=x6_taps, x6_wgrad_tile="wide"):
                off = _answers()
                assert not any(p.fit or p.arith.endswith("/fit") for p in off)
            with config.override(conv_math=2, x6_split=split, x6_taps=x6_taps):          # the default is the switch off
                if config.DEFAULTS.x6_wgrad_tile == "wide":
                    assert _answers() == off
            with config.override(conv_math=2, x6_split=split, x6_taps=x6_taps, x6_wgrad_tile="fit"):
                on = _answers()
            for (_, moves), a, b in zip(WCALLS, off, on):
                if a.family in ("x6ls", "x6rs") and moves:
                    assert b == (ls_fit if a == ls else taps_fit) and a in (ls, taps)
                else:                                      # the pass form, Winograd, the fp32 kernels and the wide layer stay put
                    assert b == a
            # what the switch is expected to reach in each configuration
            moved = [b.fit for b in on]
            if split == "loader":
                assert moved[:4] == [True] * 4
            else:
                assert moved[:4] == [False] * 4 and all(p == dc._Path("x6", "", 2, "bf16x6") for p in on[:4])
            assert moved[4:7] == [x6_taps] * 3 and moved[7] is False
            if x6_taps:
                assert on[4] == taps_fit and on[5] == taps_fit and on[6] == ls_fit
    # outside conv_math = 2 the switch changes nothing
    for math in (0, 1):
        for x6_taps in (False, True):
            with config.override(conv_math=math, x6_split="loader", x6_taps=x6_taps, x6_wgrad_tile="wide"):
                off = _answers()
            with config.override(conv_math=math, x6_split="loader", x6_taps=x6_taps, x6_wgrad_tile="fit"):
                assert _answers() == off
    # forward and backward-data never read it
    call = dict(n=2, hi=33, wi=29, cin=64, k=64, r=1, s=1, stride=(1, 1), off0=(0, 0), doff=(1, 1), ho=33, wo=29)
    with config.override(conv_math=2, x6_split="loader", x6_taps=True, x6_wgrad_tile="fit"):
        assert dc._plan(**call) == ls and dc._plan(tag=dc._TAG_BWD_DATA, **call) == ls
    assert dc._WGRAD_FIT[0] == NEW_EXPORTS[2]
    assert dc._WGRAD["x6ls"][0] == "diga_conv2d_wgrad_bf16x6_f32in" and dc._WGRAD["x6rs"][0] == "diga_conv_taps_wgrad_bf16x6_f32in"


# ---------------------------------------------------------------------------------------------------------------- tile rule
def test_tile_rule():
    counts = [8, 24, 32, 56, 64, 72, 96, 128, 136, 160, 256, 264, 320, 512, 2048]
    for cout in counts:
        for cin in counts:
            assert _tile(cout, cin) == (0, tile_rule(cout, cin)), (cout, cin)
    assert _tile(64, 64)[1] == (64, 64) and _tile(64, 256)[1] == (64, 128) and _tile(128, 512)[1] == (128, 128)
    assert _tile(256, 64)[1] == (256, 64) and _tile(128, 64)[1] == (128, 128) and _tile(320, 72)[1] == (256, 128)
    for bad in ((0, 64), (64, 0), (12, 64), (64, 12), (-8, 64), (64, -64)):
        assert _tile(*bad) == (EINVAL, (-7, -7)), bad
    from diga_amd import _lib
    b = ctypes.c_int(0)
    assert _lib.lib.diga_wgrad_bf16x6_tile(64, 64, None, ctypes.byref(b)) == EINVAL
    assert _lib.lib.diga_wgrad_bf16x6_tile(64, 64, ctypes.byref(b), None) == EINVAL


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_exports_are_declared_bound_and_exported():
    from diga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_EXPORTS:
        # (the recorded fixture of the entry-check test enumerates these prefixes)
        assert not name.startswith(("diga_conv2d_", "diga_conv_taps_", "diga_infer_conv", "diga_split_bf16")) and "batched_bf16x6" not in name
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/diga_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert name in doc, f"{name} is not documented in INTEGRATION.md"
    fresh = ctypes.CDLL(_lib.LIB_PATH)                           # the dynamic symbol table of the library itself
    for name in NEW_EXPORTS:
        assert hasattr(fresh, name), f"{name} is not exported by {_lib.LIB_PATH}"
    assert len(_lib.PROF_TAGS) == 23                             # no new profiling tag
    S = _lib.SIGNATURES
    assert S[NEW_EXPORTS[2]] == S["diga_conv_taps_wgrad_bf16x6_f32in"]
    assert S[NEW_EXPORTS[1]] == S["diga_conv_taps_wgrad_bf16x6_workspace_bytes"]


def _wg(dy=A, dy_ld=None, x=A, x_ld=None, dw=A, ws=A, ws_bytes=BIG, n=1, hi=12, wi=12, cin=64, ho=12, wo=12, cout=64, r=3, s=3, sy=1, sx=1,
        oy=-1, ox=-1, ddy=1, ddx=1, name="diga_wgrad_bf16x6_tiled_f32in"):
    from diga_amd import _lib
    dy_ld = cout if dy_ld is None else dy_ld
    x_ld = cin if x_ld is None else x_ld
    return getattr(_lib.lib, name)(dy, dy_ld, x, x_ld, dw, ws, ws_bytes, n, hi, wi, cin, ho, wo, cout, r, s, sy, sx, oy, ox, ddy, ddx, None)


# one shape per tile, the wide one (which runs the existing entry points' checks) included; 3x3 and 1x1
SHAPES = [dict(cout=64, cin=64), dict(cout=64, cin=256), dict(cout=128, cin=128), dict(cout=256, cin=64), dict(cout=512, cin=256),
          dict(cout=64, cin=64, r=1, s=1, oy=0, ox=0), dict(cout=24, cin=160, r=1, s=1, oy=0, ox=0), dict(cout=512, cin=256, r=1, s=1, oy=0, ox=0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s.values()))
def test_entry_point_rejects_bad_arguments(shape):
    from diga_amd import _lib
    cout, cin, rs = shape["cout"], shape["cin"], shape.get("r", 3) * shape.get("s", 3)
    for name in ("dy", "x", "dw", "ws"):
        assert _wg(**{name: 0}, **shape) == EINVAL, name           # null
        assert _wg(**{name: A + 4}, **shape) == EALIGN, name       # misaligned
    base = {k: v for k, v in shape.items() if k not in ("r", "s")}
    assert _wg(**base, r=65, s=1) == EINVAL and _wg(**base, r=5, s=13) == EINVAL                     # R * S = 65
    assert _wg(**base, r=0, s=3) == EINVAL and _wg(**base, r=3, s=0) == EINVAL and _wg(**base, r=1 << 32, s=1 << 32) == EINVAL
    assert _wg(**dict(shape, cin=48, r=3, s=3)) == EINVAL                                            # Cin % 32 with more than one tap
    assert _wg(**dict(shape, cin=44)) == EINVAL and _wg(**dict(shape, cin=0)) == EINVAL              # Cin % 8 in any case
    assert _wg(**dict(shape, cout=60)) == EINVAL and _wg(**dict(shape, cout=0)) == EINVAL            # Cout % 8
    assert _wg(dy_ld=cout - 8, **shape) == EINVAL and _wg(x_ld=cin - 8, **shape) == EINVAL           # pitches below the channel count
    assert _wg(dy_ld=cout + 2, **shape) == EINVAL and _wg(x_ld=cin + 2, **shape) == EINVAL and _wg(x_ld=-1, **shape) == EINVAL
    assert _wg(sy=0, **shape) == EINVAL and _wg(sx=-2, **shape) == EINVAL
    assert _wg(n=0, **shape) == EINVAL and _wg(hi=0, **shape) == EINVAL
    assert _wg(n=1 << 12, hi=1 << 10, wi=1 << 9, **shape) == EINVAL and _wg(n=1 << 12, ho=1 << 10, wo=1 << 9, **shape) == EINVAL
    if rs > 1:
        assert _wg(**dict(shape, oy=1 << 31)) == EINVAL and _wg(ddx=-(1 << 31), **shape) == EINVAL
    need = _lib.lib.diga_wgrad_bf16x6_tiled_workspace_bytes(1, 12, 12, cout, cin, shape.get("r", 3), shape.get("s", 3))
    assert need > 0
    assert _wg(ws_bytes=need - 1, **shape) == EWORKSPACE and _wg(ws_bytes=64, **shape) == EWORKSPACE   # a short workspace
    assert _lib.last_error() != ""


def test_pointwise_shapes_take_cin_multiples_of_8_only_without_taps():
    """Cin = 72 (% 8, not % 32) passes the shape rule at R = S = 1 -- the call then fails on its short workspace, the last check before
    the launch -- and is refused with more than one tap."""
    kw = dict(cout=40, cin=72, ws_bytes=64)
    assert _wg(r=1, s=1, oy=0, ox=0, **kw) == EWORKSPACE
    assert _wg(r=3, s=3, **kw) == EINVAL
    assert _wg(r=1, s=2, oy=0, **kw) == EINVAL


def test_workspace_query():
    from diga_amd import _lib
    q = _lib.lib.diga_wgrad_bf16x6_tiled_workspace_bytes
    taps, pw = _lib.lib.diga_conv_taps_wgrad_bf16x6_workspace_bytes, _lib.lib.diga_conv2d_wgrad_bf16x6_workspace_bytes
    # refused shapes: 0
    assert q(1, 12, 12, 64, 48, 3, 3) == 0 and q(1, 12, 12, 60, 64, 3, 3) == 0 and q(1, 12, 12, 64, 64, 0, 3) == 0
    assert q(1, 12, 12, 64, 64, 5, 13) == 0 and q(0, 12, 12, 64, 64, 3, 3) == 0 and q(1 << 12, 1 << 10, 1 << 9, 64, 64, 3, 3) == 0
    assert q(1, 12, 12, 64, 44, 1, 1) == 0 and q(1, 12, 12, 64, 72, 1, 2) == 0 and q(1, 12, 12, 0, 64, 1, 1) == 0
    assert q(1, 12, 12, 64, 72, 1, 1) > 0                        # Cin % 8 is enough for one tap

    def want(n, h, w, cout, cin, r, s):
        m, rs = n * h * w, r * s
        splits, _ = fit_splits(m, cout, cin, rs)
        return (splits * cout * rs * cin * 4 if splits > 1 else 0) + rs * mpad(m) * 4 + 64

    cases = [(1, 12, 12, 64, 64, 3, 3), (2, 17, 19, 64, 64, 1, 1), (1, 5, 5, 64, 64, 1, 1), (2, 33, 29, 64, 256, 1, 1), (2, 17, 19, 256, 64, 1, 1),
             (2, 17, 19, 320, 64, 1, 1), (2, 17, 19, 128, 512, 1, 1), (2, 17, 19, 24, 160, 1, 1), (2, 17, 19, 40, 72, 1, 1),
             (4, 97, 97, 64, 64, 3, 3), (16, 193, 193, 64, 64, 3, 3), (16, 193, 193, 64, 64, 1, 1), (16, 193, 193, 64, 256, 1, 1),
             (16, 97, 97, 128, 512, 1, 1), (16, 97, 97, 128, 128, 3, 3), (16, 385, 385, 64, 160, 1, 1), (1, 40, 40, 64, 32, 7, 7)]
    for c in cases:
        assert q(*c) == want(*c), c
    # 144 pixels: 4 K-steps, one split, no slab -- the table of all nine taps and the zeros
    assert q(1, 12, 12, 64, 64, 3, 3) == 9 * mpad(144) * 4 + 64
    # the new plan asks for more, shorter ranges than the wide one where the floor of 8 K-steps leaves room: 64 -> 64 3x3 on 4 x 97 x 97
    m = 4 * 97 * 97
    assert fit_splits(m, 64, 64, 9)[0] > wide_splits(m, 64, 64, 9)[0] and fit_splits(m, 64, 64, 9)[1] >= 8
    # ... the cap of 512 ranges binds where one tile covers the layer (64 -> 64 1x1 on 16 x 193 x 193: 1536 wanted, the floor allows 2328)
    assert fit_splits(16 * 193 * 193, 64, 64)[0] == wide_splits(16 * 193 * 193, 64, 64)[0] == 504
    assert fit_splits(16 * 193 * 193, 64, 256)[0] == 504 and wide_splits(16 * 193 * 193, 64, 256)[0] == 256
    # ... and the same ranges where the floor decides in both
    assert fit_splits(646, 64, 64) == wide_splits(646, 64, 64) == (2, 11)
    # a (256, 128) shape: the existing queries
    for c in [(2, 33, 29, 512, 256, 3, 3), (2, 193, 193, 256, 128, 3, 3), (2, 33, 29, 320, 96, 3, 3)]:
        assert tile_rule(c[3], c[4]) == (256, 128) and q(*c) == taps(*c) == want(*c) and q(*c) > 0
    for c in [(2, 33, 29, 512, 256, 1, 1), (16, 97, 97, 2048, 512, 1, 1), (2, 33, 29, 264, 72, 1, 1)]:
        assert q(*c) == pw(*c) == want(*c) and q(*c) > 0
