"""Host side of the eval-mode BatchNorm fold for the bf16x6 convolutions (config.fold_eval_bn_x6) that needs no GPU: the
configuration field and its environment default, the three `_infer` exports (library, header, binding), their argument checks --
all of which precede any launch -- and the planner's answers on the geometries of conv_dispatch_scenarios."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import conv_dispatch_scenarios as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("diga_infer_conv2d_nhwc_bf16x6", "diga_infer_conv2d_nhwc_bf16x6_f32in", "diga_infer_conv2d_winograd_bf16x6")
EINVAL, EALIGN = -1, -2


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_field_defaults_off_and_is_validated_as_a_bool():
    from diga_amd import config
    assert config.StepConfig().fold_eval_bn_x6 is False
    before = config.active()
    with config.override(fold_eval_bn_x6=True) as cfg:
        assert cfg.fold_eval_bn_x6 is True and config.active() is cfg
        assert cfg.fold_eval_bn is before.fold_eval_bn            # a switch of its own: the fp32 fold's field is not touched
    assert config.active() is before
    with pytest.raises(ValueError, match="fold_eval_bn_x6"):
        config.StepConfig(fold_eval_bn_x6="yes").validate()
    with pytest.raises(ValueError, match="fold_eval_bn_x6"):
        config.active().replace(fold_eval_bn_x6=1)
    assert config.StepConfig(fold_eval_bn_x6=True).validate().fold_eval_bn_x6 is True


@pytest.mark.parametrize("value,want", [(None, False), ("1", True), ("0", False), ("true", True), ("", False)])
def test_environment_gives_the_default(value, want):
    """DIGA_FOLD_EVAL_BN_X6 is read once, at import: checked in a fresh interpreter (config.py imports nothing heavy)."""
    env = {k: v for k, v in os.environ.items() if k not in ("DIGA_FOLD_EVAL_BN_X6", "DIGA_FOLD_EVAL_BN")}
    if value is not None:
        env["DIGA_FOLD_EVAL_BN_X6"] = value
    code = ("import importlib.util, sys; s = importlib.util.spec_from_file_location('cfg', sys.argv[1]); m = importlib.util.module_from_spec(s); "
            "sys.modules['cfg'] = m; s.loader.exec_module(m); print(m.DEFAULTS.fold_eval_bn_x6, m.DEFAULTS.fold_eval_bn)")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "diga_amd", "config.py")], env=env, capture_output=True, text=True,
                         check=True).stdout.strip()
    assert out == f"{want} False"


# ---------------------------------------------------------------------------------------------------------------- ABI
def _header_arity(name):
    """Number of parameters of `name`'s declaration in include/diga_hip.h."""
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/diga_hip.h"
    return len([p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()])


@pytest.mark.parametrize("name", EXPORTS)
def test_export_exists_in_library_header_and_binding(name):
    from diga_amd import _lib
    assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES[name]
    fn = getattr(_lib.lib, name)
    assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert restype is _lib.INT and len(argtypes) == _header_arity(name)
    # the sibling without the epilogue has the statistics pointer where this one has the descriptor: same arity
    sibling = {"diga_infer_conv2d_nhwc_bf16x6": "diga_conv2d_nhwc_bf16x6", "diga_infer_conv2d_nhwc_bf16x6_f32in": "diga_conv2d_nhwc_bf16x6_f32in",
               "diga_infer_conv2d_winograd_bf16x6": "diga_conv2d_winograd_f32_infer"}[name]
    assert argtypes == _lib.SIGNATURES[sibling][1]


def test_header_no_longer_says_exact_fp32_only():
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    assert "Exact-fp32 kernels only" not in hdr
    from diga_amd.model import conv as dc
    assert dc._WINOGRAD_X6 == "diga_conv2d_winograd_bf16x6" and dc._WINOGRAD_X6_INFER == "diga_infer_conv2d_winograd_bf16x6"
    assert dc._ENTRY[("x6", "infer")] == EXPORTS[0] and dc._ENTRY[("x6ls", "infer")] == EXPORTS[1]


class _Host:
    """Host buffers with chosen alignment: the checks under test read pointer VALUES only and return before any launch."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(4096 + 64)
        self.base = (ctypes.addressof(self.buf) + 63) // 64 * 64

    def at(self, off):
        return ctypes.c_void_p(self.base + off)


def _epi(ab, residual=None, residual_ld=0, relu=1):
    from diga_amd import _lib
    e = _lib.InferEpilogue()
    e.ab, e.residual, e.residual_ld, e.relu = ab, residual, residual_ld, relu
    return e


def _pointwise(name, h, infer, cout=64, out_ld=None, null=False):
    """One call of a pointwise `_infer` export on a 1 x 4 x 4 x 32 -> cout layer with host pointers."""
    from diga_amd import _lib
    ptrs = [None] * 3 if null else [h.at(0), h.at(256), h.at(512)]              # input, weight image, output
    lead = [ptrs[0]] + ([32] if "f32in" in name else []) + [ptrs[1], None, ptrs[2]]
    rc = getattr(_lib.lib, name)(*lead, 1, 4, 4, 32, 4, 4, cout, cout if out_ld is None else out_ld, 1, 1, 1, 1, 0, 0, 1, 1,
                                 None if infer is None else ctypes.byref(infer), 0, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("name", EXPORTS[:2])
def test_pointwise_argument_errors_return_a_code_without_a_device(name):
    h = _Host()
    ab, res = h.at(1024), h.at(2048)
    for what, rc_want, kw in (
            ("null pointers", EINVAL, dict(infer=_epi(ab), null=True)),
            ("null infer", EINVAL, dict(infer=None)),
            ("null ab", EINVAL, dict(infer=_epi(None))),
            ("Cout % 4", EINVAL, dict(infer=_epi(ab), cout=18)),
            ("out_ld % 4", EINVAL, dict(infer=_epi(ab), out_ld=66)),
            ("odd residual_ld", EINVAL, dict(infer=_epi(ab, res, 65))),
            ("residual_ld < Cout", EINVAL, dict(infer=_epi(ab, res, 60))),
            ("misaligned residual", EINVAL, dict(infer=_epi(ab, h.at(2052), 64))),
            ("misaligned ab", EINVAL, dict(infer=_epi(h.at(1028))))):
        rc, msg = _pointwise(name, h, **kw)
        assert rc in (EINVAL, EALIGN) and rc == rc_want and msg != "", (name, what, rc, msg)


def _winograd(h, infer, tile=4, cout=128, null=False):
    from diga_amd import _lib
    ptrs = [None] * 4 if null else [h.at(0), h.at(256), h.at(512), h.at(768)]     # input, weights, output, workspace
    rc = _lib.lib.diga_infer_conv2d_winograd_bf16x6(ptrs[0], ptrs[1], None, ptrs[2], ptrs[3], 1 << 40, 1, 8, 8, 128, 128, cout, cout, 1, tile,
                                                    None if infer is None else ctypes.byref(infer), None, 0, None)
    return rc, _lib.last_error()


def test_winograd_argument_errors_return_a_code_without_a_device():
    h = _Host()
    ab, res = h.at(1024), h.at(2048)
    for what, kw in (("null pointers", dict(infer=_epi(ab), null=True)), ("null infer", dict(infer=None)), ("null ab", dict(infer=_epi(None))),
                     ("tile 2", dict(infer=_epi(ab), tile=2)), ("Cout % 4", dict(infer=_epi(ab), cout=130)),
                     ("odd residual_ld", dict(infer=_epi(ab, res, 129))), ("misaligned ab", dict(infer=_epi(h.at(1028))))):
        rc, msg = _winograd(h, **kw)
        assert rc == EINVAL and msg != "", (what, rc, msg)


# ---------------------------------------------------------------------------------------------------------------- planner
def _geometry(name):
    """(n, h, w, padded Cin, Cout, r, s, stride, padding, dilation, ho, wo) of a layer of conv_dispatch_scenarios, as DigaConv2d sees it."""
    from diga_amd.model import conv as dc
    _, cin, cout, k, stride, pad, dil, _, _ = next(x for x in sc.LAYERS if x[0] == name)
    h, w = sc.HW
    ho, wo = ((v + 2 * pad - dil * (k - 1) - 1) // stride + 1 for v in (h, w))
    return sc.N, h, w, dc._pad_to(cin), cout, k, k, (stride, stride), (pad, pad), (dil, dil), ho, wo


def test_infer_kernel_answers_with_the_flag_on():
    from diga_amd import config
    from diga_amd.model import conv as dc
    pw, c3, head = _geometry("pw_64_256"), _geometry("c3_128_128_winograd"), _geometry("pw_256_19_bias")
    for split, want in (("pass", "bf16x6+bn"), ("loader", "bf16x6/ls+bn")):
        with config.override(conv_math=2, x6_split=split, fold_eval_bn_x6=True):
            assert dc.infer_kernel(*pw) == want
            assert dc.infer_kernel(*_geometry("pw_256_128_stride2")) == want
            assert dc.infer_kernel(*c3) == "winograd+bn"
            assert dc.infer_kernel(*head) is None                                     # Cout % 4
            assert dc.infer_kernel(*pw, pointwise_ok=False) == "f32+bn"               # (the stem's form: exact fp32 as ever)
        with config.override(conv_math=2, x6_split=split, x6_winograd=True, fold_eval_bn_x6=True):
            assert dc.infer_kernel(*pw) == want
            assert dc.infer_kernel(*c3) == "winograd/x6+bn"
            assert dc.infer_kernel(*_geometry("c3_128_256_d12_bias_direct")) == "f32+bn"
        with config.override(conv_math=2, x6_split=split, x6_winograd=True, fold_eval_bn_x6=True, winograd_max_tile=2):
            assert dc.infer_kernel(*c3) is None
    # the flag means nothing outside mode 2
    with config.override(conv_math=0, fold_eval_bn_x6=True):
        assert dc.infer_kernel(*pw) == "f32+bn" and dc.infer_kernel(*c3) == "winograd+bn"
    with config.override(conv_math=1, fold_eval_bn_x6=True):
        assert dc.infer_kernel(*pw) is None and dc.infer_kernel(*c3) is None


def test_the_plan_names_the_new_paths_and_entry_points():
    from diga_amd import config
    from diga_amd.model import conv as dc
    n, h, w, cp, cout, r, s, stride, pad, dil, ho, wo = _geometry("pw_64_256")
    call = dict(n=n, hi=h, wi=w, cin=cp, k=cout, r=r, s=s, stride=stride, off0=(0, 0), doff=dil, ho=ho, wo=wo)
    with config.override(conv_math=2, x6_split="loader", fold_eval_bn_x6=True):
        assert dc._plan(infer=True, **call) == dc._Path("x6ls", "infer", 2, "bf16x6/ls+bn")
        assert dc._plan(**call) == dc._Path("x6ls", "", 2, "bf16x6/ls")               # the plain forward is untouched
    with config.override(conv_math=2, x6_split="pass", fold_eval_bn_x6=True):
        assert dc._plan(infer=True, **call) == dc._Path("x6", "infer", 2, "bf16x6+bn")
        for bad in (dict(stats="chunks"), dict(epi=True), dict(tag=dc._TAG_BWD_DATA), dict(opts=(1, 0, 0))):
            with pytest.raises(RuntimeError):
                dc._plan(infer=True, **call, **bad)
    n, h, w, cp, cout, r, s, stride, pad, dil, ho, wo = _geometry("c3_128_128_winograd")
    call = dict(n=n, hi=h, wi=w, cin=cp, k=cout, r=r, s=s, stride=stride, off0=(-pad[0], -pad[1]), doff=dil, ho=ho, wo=wo)
    with config.override(conv_math=2, x6_winograd=True, fold_eval_bn_x6=True):
        path = dc._plan(infer=True, **call)
        assert (path.family, path.variant, path.math, path.arith, path.x6w) == ("winograd", "infer", 0, "winograd/x6+bn", True)
        assert path.tile in (4, 6)
        for bad in (dict(stats="records"), dict(epi=True)):
            with pytest.raises(RuntimeError):
                dc._plan(infer=True, **call, **bad)
    with config.override(conv_math=2, x6_winograd=True):                             # flag off: the folded layer stays exact fp32, as before
        path = dc._plan(infer=True, **call)
        assert (path.arith, path.x6w) == ("winograd+bn", False)
        assert dc._plan(**call).arith == "winograd/x6"


def test_flag_off_gives_every_answer_the_existing_test_pins():
    """tests/test_conv_plan_cpu.py::test_infer_kernel_known_answers, restated with the new field spelled out at its default."""
    from diga_amd import config
    from diga_amd.model import conv as dc
    g = {name: _geometry(name) for name in ("pw_64_256", "c3_128_128_winograd", "c3_128_256_d12_bias_direct", "pw_256_19_bias")}
    assert config.active().fold_eval_bn_x6 is False
    with config.override(conv_math=0, fold_eval_bn_x6=False):
        assert dc.infer_kernel(*g["pw_64_256"]) == "f32+bn"
        assert dc.infer_kernel(*g["c3_128_128_winograd"]) == "winograd+bn"
        assert dc.infer_kernel(*g["c3_128_256_d12_bias_direct"]) == "f32+bn"
        assert dc.infer_kernel(*g["pw_256_19_bias"]) is None
    with config.override(conv_math=0, winograd_max_tile=2, fold_eval_bn_x6=False):
        assert dc.infer_kernel(*g["c3_128_128_winograd"]) is None
    for math in (1, 2):
        for wino in (False, True):
            with config.override(conv_math=math, x6_winograd=wino, fold_eval_bn_x6=False):
                assert dc.infer_kernel(*g["pw_64_256"]) is None
                assert dc.infer_kernel(*g["c3_128_128_winograd"]) == (None if math == 1 else "winograd+bn")
