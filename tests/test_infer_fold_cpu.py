"""Host side of the eval-mode BatchNorm fold that needs no GPU: the configuration field, its environment default, validation,
and the binding's new entries."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_field_defaults_off_and_override_restores():
    from diga_amd import config
    assert config.StepConfig().fold_eval_bn is False
    before = config.active()
    with config.override(fold_eval_bn=True) as cfg:
        assert cfg.fold_eval_bn is True and config.active() is cfg
        with config.override(fold_eval_bn=False):
            assert config.active().fold_eval_bn is False
        assert config.active().fold_eval_bn is True
    assert config.active() is before and before.fold_eval_bn is config.DEFAULTS.fold_eval_bn
    with pytest.raises(RuntimeError):
        with config.override(fold_eval_bn=True):
            raise RuntimeError("body failed")
    assert config.active() is before


def test_validate_rejects_a_non_bool():
    from diga_amd import config
    with pytest.raises(ValueError, match="fold_eval_bn"):
        config.StepConfig(fold_eval_bn="yes").validate()
    with pytest.raises(ValueError, match="fold_eval_bn"):
        config.active().replace(fold_eval_bn=1)
    assert config.StepConfig(fold_eval_bn=True).validate().fold_eval_bn is True


@pytest.mark.parametrize("value,want", [(None, False), ("1", True), ("0", False), ("true", True), ("", False)])
def test_environment_gives_the_default(value, want):
    """DIGA_FOLD_EVAL_BN is read once, at import: checked in a fresh interpreter (config.py imports nothing heavy)."""
    env = {k: v for k, v in os.environ.items() if k != "DIGA_FOLD_EVAL_BN"}
    if value is not None:
        env["DIGA_FOLD_EVAL_BN"] = value
    code = ("import importlib.util, sys; s = importlib.util.spec_from_file_location('cfg', sys.argv[1]); m = importlib.util.module_from_spec(s); "
            "sys.modules['cfg'] = m; s.loader.exec_module(m); print(m.DEFAULTS.fold_eval_bn)")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "diga_amd", "config.py")], env=env, capture_output=True, text=True,
                         check=True).stdout.strip()
    assert out == str(want)


def test_binding_has_the_inference_entry_points():
    from diga_amd import _lib
    for name in ("diga_conv2d_nhwc_f32_infer", "diga_conv2d_winograd_f32_infer", "diga_bn_eval_coefficients"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    e = _lib.InferEpilogue()
    assert [f[0] for f in e._fields_] == ["ab", "residual", "residual_ld", "relu"]
    # the C struct: two pointers, an int64 and an int (padded to 8)
    assert ctypes.sizeof(e) == 32
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    assert "diga_infer_epilogue_t" in hdr
    # a null descriptor is an argument error, not a launch (host-side check: no GPU involved)
    rc = _lib.lib.diga_conv2d_nhwc_f32_infer(None, None, None, None, *([1] * 17), None, 0, None)
    assert rc == -1 and "null" in _lib.last_error()
