"""CPU-side checks of bf16x6 for the Winograd-domain GEMMs (config.x6_winograd; csrc/conv_bf16x6.h, csrc/winograd.hip): the configuration
surface, the C ABI surface, the argument checks of the new entry points -- which answer before anything touches a device -- and the
workspace queries."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["diga_gemm_batched_bf16x6_f32in", "diga_wgrad_batched_bf16x6_f32in", "diga_wgrad_batched_bf16x6_workspace_bytes",
               "diga_conv2d_winograd_bf16x6", "diga_conv2d_winograd_bf16x6_workspace_bytes", "diga_conv2d_wgrad_winograd_bf16x6",
               "diga_conv2d_wgrad_winograd_bf16x6_workspace_bytes"]
EINVAL, EALIGN, EWORKSPACE = -1, -2, -3
A = 1 << 20                      # a 16-byte aligned, non-null address: never dereferenced (every call below fails its checks)
BIG = 1 << 40


def test_step_config_x6_winograd(monkeypatch):
    from diga_amd import _lib, config
    from diga_amd.model import conv as dc
    assert config.StepConfig().x6_winograd is False               # opt-in
    assert config.DEFAULTS.x6_winograd is False or "DIGA_X6_WINOGRAD" in os.environ
    assert config.StepConfig(x6_winograd=True).validate().x6_winograd is True
    assert config.StepConfig().replace(x6_winograd=True).x6_winograd is True
    with pytest.raises(ValueError):
        config.StepConfig(x6_winograd="yes").validate()
    with pytest.raises(ValueError):
        config.StepConfig().replace(x6_winograd=1)
    monkeypatch.setenv("DIGA_X6_WINOGRAD", "1")
    assert config.StepConfig.from_env().x6_winograd is True
    monkeypatch.setenv("DIGA_X6_WINOGRAD", "0")
    assert config.StepConfig.from_env().x6_winograd is False
    monkeypatch.delenv("DIGA_X6_WINOGRAD")
    assert config.StepConfig.from_env().x6_winograd is False
    # independent of x6_split; without conv_math = 2 the flag selects nothing
    for form in ("pass", "loader"):
        with config.override(x6_winograd=True, x6_split=form):
            assert config.active().x6_winograd is True
            assert dc._wino_x6() == (_lib.get_conv_math() == 2)
    assert config.active().x6_winograd == config.DEFAULTS.x6_winograd
    assert not dc._wino_x6() or config.DEFAULTS.x6_winograd


def test_exports_are_declared_bound_and_exported():
    from diga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/diga_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    fresh = ctypes.CDLL(_lib.LIB_PATH)                           # the dynamic symbol table of the library itself
    for name in NEW_EXPORTS:
        assert hasattr(fresh, name), f"{name} is not exported by {_lib.LIB_PATH}"
    assert len(_lib.PROF_TAGS) == 23                             # no new profiling tag


def _gemm(a=A, rows=256, batches=3, k=64, imgs=A, cout=128, out=A):
    from diga_amd import _lib
    return _lib.lib.diga_gemm_batched_bf16x6_f32in(a, rows, batches, k, imgs, cout, out, 0)


def test_batched_gemm_rejects_bad_arguments():
    assert _gemm(rows=128) == EINVAL and _gemm(rows=384) == EINVAL and _gemm(rows=0) == EINVAL      # rows_per_batch % 256
    assert _gemm(k=48) == EINVAL and _gemm(k=0) == EINVAL                                           # K % 32
    assert _gemm(cout=64) == EINVAL and _gemm(cout=130) == EINVAL                                   # Cout > 64, Cout % 4
    assert _gemm(batches=0) == EINVAL and _gemm(batches=1 << 16) == EINVAL
    assert _gemm(rows=1 << 24, batches=128) == EINVAL                                               # 2^31 rows: 32-bit row indices
    assert _gemm(a=0) == EINVAL and _gemm(imgs=0) == EINVAL and _gemm(out=0) == EINVAL
    assert _gemm(a=A + 4) == EALIGN and _gemm(imgs=A + 8) == EALIGN and _gemm(out=A + 4) == EALIGN


def _wgrad(z=A, v=A, du=A, ws=A, ws_bytes=BIG, rows=256, batches=3, cout=256, cin=128):
    from diga_amd import _lib
    return _lib.lib.diga_wgrad_batched_bf16x6_f32in(z, v, du, ws, ws_bytes, rows, batches, cout, cin, 0)


def test_batched_weight_gradient_rejects_bad_arguments():
    from diga_amd import _lib
    q = _lib.lib.diga_wgrad_batched_bf16x6_workspace_bytes
    assert _wgrad(rows=100) == EINVAL and _wgrad(rows=0) == EINVAL and _wgrad(rows=1 << 31) == EINVAL       # rows % 32, 32-bit rows
    assert _wgrad(cout=128) == EINVAL and _wgrad(cin=64) == EINVAL and _wgrad(cin=0) == EINVAL              # Cout % 256, Cin % 128
    assert _wgrad(batches=0) == EINVAL and _wgrad(batches=1 << 16) == EINVAL
    for name in ("z", "v", "du", "ws"):
        assert _wgrad(**{name: 0}) == EINVAL, name
        assert _wgrad(**{name: A + 4}) == EALIGN, name
    assert _wgrad(rows=1312, batches=16, ws_bytes=16) == EWORKSPACE
    assert q(1312, 16, 256, 128) >= 64 and q(1312, 16, 256, 128) % 4 == 0
    # rejected shapes: 0
    assert q(100, 3, 256, 128) == 0 and q(256, 3, 128, 128) == 0 and q(256, 3, 256, 64) == 0 and q(256, 0, 256, 128) == 0
    # the split-K plan is the bf16x6 family's with `batches` in place of R*S: at least 8 K-steps per block -> a 256-row product has
    # one split and needs no slab; 1312 rows (41 K-steps) allow 5
    assert q(256, 3, 256, 128) == 64
    assert q(1312, 3, 256, 128) == 5 * 256 * 3 * 128 * 4 + 64


def _layer(in_=A, wgt=A, bias=0, out=A, v_keep=0, ws=A, ws_bytes=BIG, n=1, h=12, w=12, cin=128, in_ld=128, cout=128, out_ld=128, d=1, tile=4,
           flip=0, stats=0, epi=None, tab=0):
    from diga_amd import _lib
    return _lib.lib.diga_conv2d_winograd_bf16x6(in_, wgt, bias, out, v_keep, ws, ws_bytes, n, h, w, cin, in_ld, cout, out_ld, d, tile, flip,
                                                stats, ctypes.byref(epi) if epi is not None else None, tab,
                                                _lib.PROF_TAGS.index("conv_fwd"), 0)


def test_layer_entry_point_rejects_bad_arguments():
    from diga_amd import _lib
    for name in ("in_", "wgt", "out", "ws"):
        assert _layer(**{name: 0}) == EINVAL, name
        assert _layer(**{name: A + 4}) == EALIGN, name
    assert _layer(bias=A + 4) == EALIGN and _layer(v_keep=A + 4) == EALIGN and _layer(tab=A + 8) == EALIGN
    assert _layer(cin=48, in_ld=48) == EINVAL                    # Cin % 32
    assert _layer(cout=64, out_ld=64) == EINVAL and _layer(cout=130, out_ld=132) == EINVAL      # Cout > 64, Cout % 4
    assert _layer(in_ld=64) == EINVAL and _layer(in_ld=130) == EINVAL and _layer(out_ld=64) == EINVAL and _layer(out_ld=130) == EINVAL
    assert _layer(tile=3) == EINVAL and _layer(tile=8) == EINVAL
    assert _layer(d=0) == EINVAL and _layer(n=0) == EINVAL
    assert _layer(n=1 << 20, h=64, w=64) == EINVAL               # 2^32 pixels
    assert _layer(ws_bytes=1024) == EWORKSPACE
    assert _layer(stats=A, tile=2) == EINVAL                     # statistics: tiles 4 / 6
    assert _layer(stats=A + 4) == EINVAL
    assert _layer(v_keep=A, flip=1) == EINVAL                    # keeping V: the forward
    e = _lib.BwdEpilogue()
    assert _layer(epi=e) == EINVAL                               # empty descriptor
    e.addend, e.addend_ld = A, 64
    assert _layer(epi=e) == EINVAL                               # addend_ld < Cout
    e.addend_ld = 128
    assert _layer(epi=e, bias=A) == EINVAL and _layer(epi=e, stats=A) == EINVAL and _layer(epi=e, v_keep=A) == EINVAL


def _layer_wgrad(dy=A, x=A, v=0, dw=A, ws=A, ws_bytes=BIG, n=1, h=12, w=12, cin=128, x_ld=128, cout=256, dy_ld=256, d=1, tile=4, tab=0):
    from diga_amd import _lib
    return _lib.lib.diga_conv2d_wgrad_winograd_bf16x6(dy, x, v, dw, ws, ws_bytes, n, h, w, cin, x_ld, cout, dy_ld, d, tile, tab, 0)


def test_layer_weight_gradient_entry_point_rejects_bad_arguments():
    for name in ("dy", "dw", "ws"):
        assert _layer_wgrad(**{name: 0}) == EINVAL, name
        assert _layer_wgrad(**{name: A + 4}) == EALIGN, name
    assert _layer_wgrad(x=0) == EINVAL                           # neither x nor a kept V
    assert _layer_wgrad(x=A + 4) == EALIGN and _layer_wgrad(v=A + 4) == EALIGN and _layer_wgrad(tab=A + 8) == EALIGN
    assert _layer_wgrad(cout=128, dy_ld=128) == EINVAL and _layer_wgrad(cin=64, x_ld=64) == EINVAL
    assert _layer_wgrad(x_ld=64) == EINVAL and _layer_wgrad(dy_ld=258) == EINVAL
    assert _layer_wgrad(tile=5) == EINVAL and _layer_wgrad(d=0) == EINVAL
    assert _layer_wgrad(ws_bytes=1024) == EWORKSPACE


def test_workspace_queries():
    from diga_amd import _lib
    L = _lib.lib
    fq, wq = L.diga_conv2d_winograd_bf16x6_workspace_bytes, L.diga_conv2d_wgrad_winograd_bf16x6_workspace_bytes
    # rejected shapes: 0
    assert fq(1, 12, 12, 48, 128, 1, 4) == 0 and fq(1, 12, 12, 128, 64, 1, 4) == 0 and fq(1, 12, 12, 128, 130, 1, 4) == 0
    assert fq(1, 12, 12, 128, 128, 1, 3) == 0 and fq(0, 12, 12, 128, 128, 1, 4) == 0 and fq(1, 12, 12, 128, 128, 0, 4) == 0
    assert wq(1, 12, 12, 128, 128, 1, 4, 0) == 0 and wq(1, 12, 12, 64, 256, 1, 4, 0) == 0 and wq(1, 12, 12, 128, 256, 1, 5, 0) == 0
    # one shape: the fp32 layout's tile table, V and M (and U, which the split reads) + the weight images
    n, h, w, cin, cout, d = 2, 25, 25, 256, 160, 2
    for tile in (2, 4, 6):
        prod = (tile + 2) ** 2
        tp = L.diga_conv2d_winograd_tile_table_bytes(n, h, w, d, tile) // 16
        assert tp % 256 == 0 and tp > 0
        v_bytes = L.diga_conv2d_winograd_v_floats(n, h, w, cin, d, tile) * 4
        assert v_bytes == prod * tp * cin * 4
        images = prod * L.diga_split_bf16x6_image_bytes(cout, 1, cin)
        parts = tp * 16 + v_bytes + prod * tp * cout * 4 + images
        assert fq(n, h, w, cin, cout, d, tile) >= parts
        assert fq(n, h, w, cin, cout, d, tile) == L.diga_conv2d_winograd_workspace_bytes(n, h, w, cin, cout, d, tile) + images
        # weight gradient: tile table + Z + dU (+ V when it is recomputed) + the bf16x6 plan's slabs
        for kept in (0, 1):
            got = wq(n, h, w, 128, 256, d, tile, kept)
            base = tp * 16 + prod * tp * 256 * 4 + prod * 256 * 128 * 4 + (0 if kept else prod * tp * 128 * 4)
            slab = L.diga_wgrad_batched_bf16x6_workspace_bytes(tp, prod, 256, 128) - 64
            assert got == base + slab + 64
