"""Backward-data of stride-2 multi-tap convolutions on the GPU (csrc/dgrad_strided.hip): the entry point against float64
torch.nn.grad.conv2d_input on the shape table of tests/dgrad_strided_cases.py, its determinism, DigaConv2d(3x3, stride 2) forward and
backward under the three conv arithmetics, and the downward path of HRNet's exchange unit against the capture of the reference.

Bounds.  Entry point: the project's bound for direct fp32 kernels, conftest.WINO_TOL[0] (1e-5 of the tensor's scale), every element;
dx is pre-filled with NaN, so an element the kernel does not write fails.  Module: test_gpu_conv.py's bounds for the same arithmetic
(fp32 direct kernels: rtol 1e-5 and 2e-6 / 3e-6 / 3e-6 of scale for y / dx / dw; bf16x3: 3e-5 of scale); the input gradient is exact
fp32 under every conv_math and is held to the fp32 bound in all three.  Exchange unit: 4 x the reference's own fp32-against-float64
error on each tensor, as stored in the fixture (the OCR head's rule); seed 2400, the first tried, keeps the reference's fp32 run inside
that bound on every element, so no share of elements is excepted.

Measured on an MI355X (max error / scale against float64; the printed lines of a run with -s):
  entry point       2.2e-7 (k1, k2) .. 5.6e-7 (odd, pitched)
  module            y 5.8e-7 .. 8.1e-7 (fp32, bf16x6 mode), 4.6e-6 .. 5.4e-6 (bf16x3); x.grad 4.6e-7 .. 5.9e-7 in all three modes;
                    weight.grad 1.8e-7 .. 3.8e-7 (fp32, bf16x6 mode), 4.9e-6 .. 6.2e-6 (bf16x3)
  exchange unit     y 4.5e-7 (reference fp32 3.1e-7), dx 5.7e-7 (4.0e-7), weight gradients 3.7e-7 / 8.2e-7 (2.6e-7 / 4.7e-7), BatchNorm
                    gradients 0 .. 6.2e-7 (0 .. 6.1e-7; the last bias gradient is a sum of float16-grid values, exact in any order),
                    running statistics 7.5e-8 .. 1.1e-7 (6.5e-8 .. 8.6e-8)"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dgrad_strided_cases as dc
from conftest import WINO_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0
ROWS = sorted(dc.CASES) + ["pitched"]


def run_entry(name):
    """One call of diga_dgrad_strided_f32 on a row of the table: (dx [N, C, Hi, Wi] on the CPU, the float64 reference)."""
    from diga_amd import _lib
    pitched = name == "pitched"
    n, c, hi, wi, k, r, s, pad = dc.CASES["odd" if pitched else name]
    dy, w, ref = dc.operands("odd" if pitched else name)
    ho, wo = dc.out_extent(hi, wi, r, s, pad)
    # pitched: dy is channels 16 .. 80 of a 96-wide buffer, dx channels 32 .. 96 of a 128-wide one
    dy_ld, dy_off, dx_ld, dx_off = (96, 16, 128, 32) if pitched else (k, 0, c, 0)
    dyb = torch.full((n, ho, wo, dy_ld), SENTINEL, dtype=torch.float32, device=DEV)
    dyb[..., dy_off:dy_off + k] = dy.permute(0, 2, 3, 1).to(DEV)
    wt = w.permute(1, 2, 3, 0).contiguous().to(DEV)            # [C][R][S][K]
    dxb = torch.full((n, hi, wi, dx_ld), SENTINEL, dtype=torch.float32, device=DEV)
    dxb[..., dx_off:dx_off + c] = float("nan")
    dyv, dxv = dyb[..., dy_off:], dxb[..., dx_off:]
    _lib.call("diga_dgrad_strided_f32", C.c_void_p(dyv.data_ptr()), dy_ld, C.c_void_p(wt.data_ptr()), C.c_void_p(dxv.data_ptr()), dx_ld,
              n, hi, wi, c, ho, wo, k, r, s, 2, 2, pad[0], pad[1], _lib.stream())
    torch.cuda.synchronize()
    out = dxb.cpu()
    outside = torch.cat([out[..., :dx_off], out[..., dx_off + c:]], dim=-1)
    assert bool((outside == SENTINEL).all()), f"{name}: bytes outside the channel slice of dx were written"
    return out[..., dx_off:dx_off + c].permute(0, 3, 1, 2), ref


@pytest.mark.parametrize("name", ROWS)
def test_entry_point_vs_float64(name):
    got, ref = run_entry(name)
    assert got.shape == ref.shape
    assert not bool(torch.isnan(got).any()), f"{name}: {int(torch.isnan(got).sum())} elements of dx were not written"
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max()) / scale
    print(f"dgrad_strided {name}: max error {err:.2e} of scale")
    assert err <= WINO_TOL[0][0], (name, err)


@pytest.mark.parametrize("name", ROWS)
def test_entry_point_is_deterministic(name):
    """Fixed summation order: two calls on the same inputs give the same bits."""
    a, _ = run_entry(name)
    b, _ = run_entry(name)
    assert torch.equal(a, b)


# ---- DigaConv2d(C, K, 3, stride=2, padding=1)
MODULE_CASES = {"odd": (2, 64, 17, 13, 64), "even": (2, 32, 16, 12, 96), "pad48": (1, 48, 9, 11, 96)}      # N, C, Hi, Wi, K


@functools.lru_cache(maxsize=None)
def module_reference(name):
    n, c, hi, wi, k = MODULE_CASES[name]
    g = torch.Generator().manual_seed(2450 + sorted(MODULE_CASES).index(name))
    x = torch.randn((n, c, hi, wi), generator=g)
    w = torch.randn((k, c, 3, 3), generator=g) * (2.0 / (c * 9)) ** 0.5
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    yr = F.conv2d(xr, wr, None, 2, 1)
    probe = torch.randn(yr.shape, generator=g)
    (yr * probe.double()).sum().backward()
    return x, w, probe, yr.detach(), xr.grad, wr.grad


def held(got, want, rtol, atol_of_scale, what):
    got, want = got.detach().cpu().double(), want.double()
    scale = float(want.abs().max())
    err = (got - want).abs()
    print(f"{what}: max error {float(err.max()) / scale:.2e} of scale")
    assert bool((err <= atol_of_scale * scale + rtol * want.abs()).all()), (what, float(err.max()) / scale)


@pytest.mark.parametrize("math", [0, 1, 2], ids=["f32", "bf16x3", "bf16x6"])
@pytest.mark.parametrize("name", sorted(MODULE_CASES))
def test_module_forward_backward(name, math):
    from diga_amd import _lib
    from diga_amd.model import conv as dconv
    from diga_amd.model.conv import DigaConv2d
    n, c, hi, wi, k = MODULE_CASES[name]
    x, w, probe, yr, dxr, dwr = module_reference(name)
    m = DigaConv2d(c, k, 3, stride=2, padding=1, bias=False)
    with torch.no_grad():
        m.weight.copy_(w)
    m = m.to(DEV)
    prev = _lib.get_conv_math()
    _lib.set_conv_math(math)
    dconv.path_log = log = {}
    try:
        xd = x.to(DEV).requires_grad_()
        y = m(xd)
        (y * probe.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        dconv.path_log = None
        _lib.set_conv_math(prev)
    assert log.get(("dgrad", "f32/s2")) == 1, log
    # (y / dw: the direct fp32 kernels in modes 0 and 2 -- multi-tap layers leave fp32 in mode 2 only under config.x6_taps -- and
    # split-bf16 in mode 1; dx: exact fp32 in all three)
    rtol, a_y, a_dw = (0.0, 3e-5, 3e-5) if math == 1 else (1e-5, 2e-6, 3e-6)
    held(y, yr, rtol, a_y, f"{name} math {math} y")
    held(xd.grad, dxr, 1e-5, 3e-6, f"{name} math {math} x.grad")
    held(m.weight.grad, dwr, rtol, a_dw, f"{name} math {math} weight.grad")


# ---- the downward path of HRNet's exchange unit
def test_hrnet_fuse_down_vs_reference_capture(golden):
    """conv 3x3/2 32->32, BN, ReLU, conv 3x3/2 32->128, BN in train mode, built from DigaConv2d / DigaTrainableBatchNorm2d and loaded by
    the reference's state-dict keys; every tensor within 4 x the reference's own fp32 error against float64, every element."""
    from diga_amd.model.conv import DigaConv2d
    from diga_amd.model.norm import DigaTrainableBatchNorm2d
    z = golden("hrnet_fuse_down")
    chain = nn.Sequential(nn.Sequential(DigaConv2d(32, 32, 3, stride=2, padding=1, bias=False), DigaTrainableBatchNorm2d(32)),
                          nn.Sequential(DigaConv2d(32, 128, 3, stride=2, padding=1, bias=False), DigaTrainableBatchNorm2d(128)))
    sd = {k: z.t("w_" + k.replace(".", "_")) for k in [str(s) for s in z["keys"]]}
    sd = {k: v if k.endswith("num_batches_tracked") else v.float() for k, v in sd.items()}
    chain.load_state_dict(sd)
    chain = chain.to(DEV).train()
    x = z.t("x").float().to(DEV).requires_grad_()
    h = chain[0][1](chain[0][0](x), relu=True)
    y = chain[1][1](chain[1][0](h))
    y.backward(z.t("dy").float().to(DEV))
    torch.cuda.synchronize()
    got = {"y": y, "dx": x.grad}
    got.update({"g_" + k.replace(".", "_"): p.grad for k, p in chain.named_parameters()})
    got.update({"b_" + k.replace(".", "_"): b for k, b in chain.named_buffers() if not k.endswith("num_batches_tracked")})
    assert {"err32_" + k for k in got} == {k for k in z if k.startswith("err32_")}
    failed = []
    for k, v in got.items():
        want, scale, err32 = z.t(k), float(z["scale_" + k]), float(z["err32_" + k])
        err = float((v.detach().cpu().double() - want).abs().max()) / scale
        print(f"hrnet fuse-down {k:22s} error {err:.2e} of scale, reference fp32 {err32:.2e}")
        if not err <= 4.0 * err32:
            failed.append((k, err, err32))
    assert not failed, failed
    assert all(int(b) == 4 for k, b in chain.named_buffers() if k.endswith("num_batches_tracked"))
