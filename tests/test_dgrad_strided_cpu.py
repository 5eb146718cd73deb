"""Backward-data of stride-2 multi-tap convolutions (csrc/dgrad_strided.hip, diga_dgrad_strided_f32), the part that needs no device:
the phase decomposition itself, the export, its argument rules, the host routing of DigaConv2d and the capture behind the HRNet
exchange-unit test."""
import os
import types

import pytest
import torch
import torch.nn.functional as F

import conv_entry_check_cases as cc
import dgrad_strided_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "diga_dgrad_strided_f32"
EINVAL = -1


# ---- (i) the arithmetic
@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_phase_decomposition_equals_conv2d_input(name):
    """Both sum the same float64 products in different orders: 1e-12 of the tensor's scale."""
    n, c, hi, wi, k, r, s, pad = dc.CASES[name]
    dy, w, ref = dc.operands(name)
    got = dc.dgrad_by_phases(dy.double(), w.double(), hi, wi, pad)
    assert got.shape == ref.shape
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= 1e-12 * scale, (name, err / scale)


def test_table_reaches_its_corners():
    """The properties the rows are named for."""
    assert dc.phase_rows(3, 23, 21) == [396, 360, 363, 330]
    assert len(set(dc.phase_rows(2, 17, 13))) == 4
    # uncovered: the last row and column of dx receive nothing
    n, c, hi, wi, k, r, s, pad = dc.CASES["uncovered"]
    _, _, ref = dc.operands("uncovered")
    assert float(ref[:, :, hi - 1, :].abs().max()) == 0.0 and float(ref[:, :, :, wi - 1].abs().max()) == 0.0
    assert float(ref[:, :, hi - 2, :wi - 1].abs().min()) > 0.0
    # k1: three phases without taps
    _, _, ref1 = dc.operands("k1")
    assert float(ref1[:, :, 1::2, :].abs().max()) == 0.0 and float(ref1[:, :, :, 1::2].abs().max()) == 0.0


# ---- (ii) the export
def test_export_is_declared_bound_and_outside_the_recorded_families():
    from diga_amd import _lib
    with open(os.path.join(ROOT, "include", "diga_hip.h")) as fh:
        assert f"int {NAME}(" in fh.read()
    res, args = _lib.SIGNATURES[NAME]
    assert res is _lib.INT and len(args) == 19
    assert hasattr(_lib.lib, NAME)
    assert not cc.in_scope(NAME, True) and not cc.is_query(NAME)


# ---- (iii) the rules
ORDER = ["dy", "dy_ld", "wt", "dx", "dx_ld", "N", "Hi", "Wi", "Cin", "Ho", "Wo", "Cout", "R", "S", "sy", "sx", "py", "px", "stream"]
# (fake, 16-byte aligned addresses: every call below is rejected before anything could use them)
VALID = dict(dy=0x10000, dy_ld=64, wt=0x20000, dx=0x30000, dx_ld=64, N=2, Hi=17, Wi=13, Cin=64, Ho=9, Wo=7, Cout=64, R=3, S=3, sy=2, sx=2,
             py=1, px=1, stream=0)
REJECTED = [
    ("null_dy", dict(dy=0), "null pointer"),
    ("null_wt", dict(wt=0), "null pointer"),
    ("null_dx", dict(dx=0), "null pointer"),
    ("align_dy", dict(dy=0x10004), "16-byte aligned"),
    ("align_wt", dict(wt=0x20008), "16-byte aligned"),
    ("align_dx", dict(dx=0x3000c), "16-byte aligned"),
    ("dy_ld_small", dict(dy_ld=60), "bad dy_ld"),
    ("dy_ld_mod4", dict(dy_ld=66), "bad dy_ld"),
    ("dx_ld_small", dict(dx_ld=60), "bad dx_ld"),
    ("dx_ld_mod4", dict(dx_ld=66), "bad dx_ld"),
    ("cout_mod32", dict(Cout=48), "Cout=48 must be a multiple of 32"),
    ("cin_mod4", dict(Cin=62), "Cin=62 must be a multiple of 4"),
    ("stride_1", dict(sy=1, sx=1), "only stride 2 x 2"),
    ("stride_y", dict(sy=3), "only stride 2 x 2"),
    ("stride_x", dict(sx=1), "only stride 2 x 2"),
    ("r_zero", dict(R=0), "outside 1 .. 7"),
    ("r_eight", dict(R=8), "outside 1 .. 7"),
    ("s_eight", dict(S=8), "outside 1 .. 7"),
    ("pad_negative", dict(py=-1), "padding must be"),
    ("pad_y_is_r", dict(py=3), "padding must be"),
    ("pad_x_is_s", dict(px=3), "padding must be"),
    ("ho_wrong", dict(Ho=8), "not the stride-2 output extent"),
    ("wo_wrong", dict(Wo=8), "not the stride-2 output extent"),
    ("ho_zero", dict(Hi=1, py=0, Ho=0), "not the stride-2 output extent"),
    ("negative_n", dict(N=-1), "bad shape"),
    ("n_2p30", dict(N=1 << 30), "beyond 2^30"),
    ("hi_2p30", dict(Hi=1 << 30, Ho=1 << 29), "beyond 2^30"),
    ("phase_rows_2p32", dict(N=1 << 20, Hi=128, Wi=128, Ho=64, Wo=64), "beyond 2^30"),
]


def _call(_lib, **over):
    vals = dict(VALID, **over)
    rc = getattr(_lib.lib, NAME)(*[vals[k] for k in ORDER])
    return rc, _lib.last_error()


needs_no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="host checks only: run where no device is visible")


@needs_no_device
@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_rule_rejects_with_its_message(case):
    from diga_amd import _lib
    _, over, message = case
    rc, said = _call(_lib, **over)
    assert rc == EINVAL and said.startswith("dgrad_strided: ") and message in said, (rc, said)


@needs_no_device
def test_empty_batch_is_ok_without_a_launch():
    """N == 0 passes every rule and returns before the launch (no device is visible here: a launch would report an error)."""
    from diga_amd import _lib
    rc, _ = _call(_lib, N=0)
    assert rc == 0


# ---- (iv) host routing
def test_predicate_selects_the_new_path_as_specified():
    from diga_amd.model.conv import _strided_dgrad_ok
    for name, (n, c, hi, wi, k, r, s, pad) in dc.CASES.items():
        assert _strided_dgrad_ok(r, s, (2, 2), pad, (1, 1)) == (name != "k1"), name
    assert not _strided_dgrad_ok(3, 3, (1, 1), (1, 1), (1, 1))
    assert not _strided_dgrad_ok(3, 3, (2, 1), (1, 1), (1, 1))
    assert not _strided_dgrad_ok(3, 3, (4, 4), (1, 1), (1, 1))
    assert not _strided_dgrad_ok(5, 5, (2, 2), (4, 4), (2, 2))
    assert not _strided_dgrad_ok(3, 3, (2, 2), (3, 1), (1, 1))
    assert not _strided_dgrad_ok(3, 3, (2, 2), (1, 3), (1, 1))
    assert _strided_dgrad_ok(7, 7, (2, 2), (3, 3), (1, 1))


def test_strided_dilated_5x5_still_raises(monkeypatch):
    """_Conv2dFn.backward on a hand-made context (CPU tensors, a 19-channel output so that the weight transpose is made with torch ops):
    the geometry is refused before any kernel is asked for."""
    from diga_amd import _lib
    from diga_amd.model import conv as dconv
    monkeypatch.setattr(_lib, "stream", lambda: None)
    n, c, hi, wi, k, r = 1, 32, 13, 11, 19, 5
    stride, padding, dilation = (2, 2), (4, 4), (2, 2)
    ho, wo = (hi + 8 - 8 - 1) // 2 + 1, (wi + 8 - 8 - 1) // 2 + 1
    ctx = types.SimpleNamespace(
        saved_tensors=(torch.zeros((n, hi, wi, c)), torch.zeros((k, r, r, c))),
        geom=(stride, padding, dilation, c, False, (c * r * r, 1, r * c, c)),
        x_trip=None, x_twin=None, x_is_twin=False, dy_is_twin=False, bn_box=None, chain=None, math=_lib.get_conv_math(),
        needs_input_grad=(True, False, False))
    with pytest.raises(NotImplementedError, match=r"stride \(2, 2\), dilation \(1, 1\)"):
        dconv._Conv2dFn.backward(ctx, torch.zeros((n, k, ho, wo)))


# ---- the capture behind the HRNet exchange-unit test
def test_hrnet_fuse_down_fixture_reproduces_from_functional_ops(golden):
    """Pins the capture, not the kernel: the fixture's float64 tensors are conv 3x3/2 -> train-mode BN -> ReLU -> conv 3x3/2 -> train-mode
    BN of its inputs, and their gradients under its dy."""
    z = golden("hrnet_fuse_down")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "hrnet_fuse_down.npz")) < (1 << 20)
    p = {k: z.t("w_" + k.replace(".", "_")).double() for k in [str(s) for s in z["keys"]] if not k.endswith("num_batches_tracked")}
    x = z.t("x").double().requires_grad_()
    leaves = {k: p[k].clone().requires_grad_() for k in ("0.0.weight", "0.1.weight", "0.1.bias", "1.0.weight", "1.1.weight", "1.1.bias")}
    stats = {k: p[k].clone() for k in ("0.1.running_mean", "0.1.running_var", "1.1.running_mean", "1.1.running_var")}
    h = F.conv2d(x, leaves["0.0.weight"], None, 2, 1)
    h = F.relu(F.batch_norm(h, stats["0.1.running_mean"], stats["0.1.running_var"], leaves["0.1.weight"], leaves["0.1.bias"], True, 0.1, 1e-5))
    h = F.conv2d(h, leaves["1.0.weight"], None, 2, 1)
    y = F.batch_norm(h, stats["1.1.running_mean"], stats["1.1.running_var"], leaves["1.1.weight"], leaves["1.1.bias"], True, 0.1, 1e-5)
    y.backward(z.t("dy").double())
    got = {"y": y.detach(), "dx": x.grad}
    got.update({"g_" + k.replace(".", "_"): v.grad for k, v in leaves.items()})
    got.update({"b_" + k.replace(".", "_"): v for k, v in stats.items()})
    assert tuple(z["x"].shape) == (2, 32, 19, 17) and tuple(z["y"].shape) == (2, 128, 5, 5)
    for k, v in got.items():
        want = z.t(k)
        assert want.dtype == torch.float64 and want.shape == v.shape, k
        scale = float(z["scale_" + k])
        assert scale == float(want.abs().max()) and float(z["err32_" + k]) >= 0.0, k
        assert float((v - want).abs().max()) <= 1e-12 * scale, k
    assert sorted(k for k in z if k.startswith("err32_")) == sorted("err32_" + k for k in got)
