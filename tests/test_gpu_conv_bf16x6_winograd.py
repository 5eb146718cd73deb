"""GPU tests of bf16x6 for the Winograd-domain GEMMs of the stride-1 3x3 layers (config.x6_winograd under conv_math = 2;
csrc/conv_bf16x6.h, csrc/winograd.hip): the transforms stay fp32, the (tile + 2)^2 products per layer run on the loader-split bf16x6
kernels in one batched launch.

  1. the batched forward GEMM, bit for bit against the pointwise `_f32in` entry point run on every batch alone;
  2. the batched weight-gradient GEMM against float64, against the pointwise `_f32in` weight gradient per batch, and for determinism;
  3. WINO_CASES x tile {2, 4, 6} as layers against float64 and against the fp32 Winograd path on the same inputs;
  4. flag off is today's mode 2, and modes 0 / 1 do not see the flag;
  5. BatchNorm statistics from the output transform and the backward-data epilogue on a dilated bottleneck;
  6. the flag switched between forward and backward;  7. the whole small model against the float64 oracle.
`conv.path_log` proves which path ran: every case must select the new one -- nothing here skips."""
import dataclasses
import zlib

import pytest
import torch
import torch.nn.functional as F

from diga_amd import config

from conftest import WINO_TOL, assert_close
from oracle import deeplab as od
from oracle import detweights, synth
from test_gpu_conv import CASES, WINO_CASES
from test_gpu_conv_bf16x6 import FWD_TOL_F32, _Mode, _block_state, _inputs, _make_block, _run_layer

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEW_EXPORTS = ("diga_gemm_batched_bf16x6_f32in", "diga_wgrad_batched_bf16x6_f32in", "diga_conv2d_winograd_bf16x6",
               "diga_conv2d_wgrad_winograd_bf16x6")


@pytest.fixture(autouse=True)
def _leave_global_rng_and_arithmetic_untouched():
    """As tests/test_gpu_conv_bf16x6.py: layer constructors draw from torch's global generators and later tests are sensitive to the
    draw, so every test hands the generators -- and the process-wide conv arithmetic -- back as it found them."""
    from diga_amd import _lib
    cpu, gpu = torch.get_rng_state(), (torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    math = _lib.get_conv_math()
    yield
    _lib.set_conv_math(math)
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _spy(monkeypatch):
    """Record (name, args) of every library call."""
    from diga_amd import _lib
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


def _names(calls):
    return [c[0] for c in calls]


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max()) / float(ref.detach().abs().max())


# ------------------------------------------------------------------------------------------------ 1. batched forward GEMM
@pytest.mark.parametrize("rows", [256, 512], ids=["1tile", "2tiles"])
@pytest.mark.parametrize("batches", [3, 16])
def test_batched_forward_gemm_equals_pointwise_entry_point_per_batch(batches, rows):
    """Every batch's block of the batched GEMM is torch.equal to diga_conv2d_nhwc_bf16x6_f32in on that batch alone (its rows as an
    N = 1 pointwise layer, its weights as diga_split_bf16x6_image): K = 32 / 64 / 96 = prologue only / one ring turn / wrap-around of the
    two stages, Cout = 128 / 160 / 320 = one full column tile / ragged tiles of both widths.  One and two row tiles per batch, every
    batch with its own weights and one batch all zero: a wrong batch index or a leak from a neighbour shows as a non-zero."""
    from diga_amd import _lib
    tag = _lib.PROF_TAGS.index("conv_fwd")
    zero_b = 1
    for k in (32, 64, 96):
        for cout in (128, 160, 320):
            g = synth.gen(7000 + 97 * batches + rows + 3 * k + cout)
            a = torch.randn((batches * rows, k), generator=g) * torch.exp2(torch.randint(-6, 7, (batches * rows, 1), generator=g).float())
            w = torch.randn((batches, cout, k), generator=g) * (2.0 / k) ** 0.5
            w[zero_b] = 0.0
            ad, wd = a.to(DEV), w.to(DEV)
            ib = _lib.lib.diga_split_bf16x6_image_bytes(cout, 1, k)
            imgs = torch.zeros(batches * ib, dtype=torch.uint8, device=DEV)
            for b in range(batches):
                _lib.call("diga_split_bf16x6_image", _lib.ptr(wd[b]), _lib.ptr(imgs[b * ib:]), cout, 1, k, _lib.stream())
            guard = 512
            buf = torch.full((batches * rows * cout + guard,), 7.0, dtype=torch.float32, device=DEV)
            _lib.call("diga_gemm_batched_bf16x6_f32in", _lib.ptr(ad), rows, batches, k, _lib.ptr(imgs), cout, _lib.ptr(buf), _lib.stream())
            torch.cuda.synchronize()
            assert bool((buf[batches * rows * cout:] == 7.0).all()), "written past the output"
            out = buf[:batches * rows * cout].view(batches, rows, cout)
            for b in range(batches):
                ref = torch.full((rows, cout), 7.0, dtype=torch.float32, device=DEV)
                _lib.call("diga_conv2d_nhwc_bf16x6_f32in", _lib.ptr(ad[b * rows:]), k, _lib.ptr(imgs[b * ib:]), None, _lib.ptr(ref), 1, 1, rows, k,
                          1, rows, cout, cout, 1, 1, 1, 1, 0, 0, 1, 1, None, tag, _lib.stream())
                assert torch.equal(out[b], ref), (k, cout, b)
            assert not bool(out[zero_b].any()), (k, cout, "the zero-weight batch")
            assert bool(out[0].any()) and bool(out[2].any())
            # ... and the products are the right ones (the pointwise kernel's own bound against float64)
            want = torch.einsum("brk,bck->brc", ad.double().view(batches, rows, k), wd.double())
            assert _rel(out, want) < 2e-6, (k, cout)


# ------------------------------------------------------------------------------------------------ 2. batched weight-gradient GEMM
@pytest.mark.parametrize("cout,cin", [(256, 128), (512, 256)])
@pytest.mark.parametrize("rows", [256, 1312])
@pytest.mark.parametrize("batches", [3, 16])
def test_batched_weight_gradient_gemm(batches, rows, cout, cin):
    """dU_b = Z_b^T V_b against float64, e = max |t - t64| / max |t64| per batch: e <= 1.5 x the same statistic of
    diga_conv2d_wgrad_bf16x6_f32in on the batch alone (another split-K tree: a bound, not an equality; 1.5 = the margin
    test_per_layer_error_against_float64_and_exact_fp32 gives a max statistic) and e < 3e-6 (what that test holds weight gradients
    to); two calls agree bit for bit (fixed-order reduce); an all-zero batch of Z gives an exactly zero slice of dU.  rows = 1312 is
    no multiple of 256 (a block's last K-steps run past its range) and splits five ways."""
    from diga_amd import _lib
    g = synth.gen(8000 + 31 * batches + rows + cout + cin)
    z = torch.randn((batches, rows, cout), generator=g)
    v = torch.randn((batches, rows, cin), generator=g) + 0.25
    zero_b = batches - 2
    z[zero_b] = 0.0
    zd, vd = z.to(DEV), v.to(DEV)
    nb = _lib.lib.diga_wgrad_batched_bf16x6_workspace_bytes(rows, batches, cout, cin)
    assert nb >= 64
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        buf = torch.full((cout * batches * cin + 256,), 7.0, dtype=torch.float32, device=DEV)
        _lib.call("diga_wgrad_batched_bf16x6_f32in", _lib.ptr(zd), _lib.ptr(vd), _lib.ptr(buf), _lib.ptr(ws), ws.numel(), rows, batches, cout,
                  cin, _lib.stream())
        torch.cuda.synchronize()
        assert bool((buf[cout * batches * cin:] == 7.0).all()), "written past dU"
        outs.append(buf[:cout * batches * cin].view(cout, batches, cin))
    assert torch.equal(outs[0], outs[1])
    du = outs[0]
    assert not bool(du[:, zero_b].any())
    nb1 = _lib.lib.diga_conv2d_wgrad_bf16x6_workspace_bytes(1, 1, rows, cout, cin, 1, 1)
    ws1 = torch.empty(nb1, dtype=torch.uint8, device=DEV)
    for b in range(batches):
        if b == zero_b:
            continue
        t64 = zd[b].double().t() @ vd[b].double()
        one = torch.empty((cout, cin), dtype=torch.float32, device=DEV)
        _lib.call("diga_conv2d_wgrad_bf16x6_f32in", _lib.ptr(zd[b]), cout, _lib.ptr(vd[b]), cin, _lib.ptr(one), _lib.ptr(ws1), ws1.numel(),
                  1, 1, rows, cin, 1, rows, cout, 1, 1, 1, 1, 0, 0, 1, 1, _lib.stream())
        e, e1 = _rel(du[:, b], t64), _rel(one, t64)
        if b in (0, batches - 1):
            print(f"\n[x6 winograd wgrad gemm] batches {batches} rows {rows} {cout}x{cin} batch {b}: batched {e:.2e}, alone {e1:.2e}, ratio {e / e1:.2f}")
        assert e <= 1.5 * e1, (b, e, e1)
        assert e < 3e-6, (b, e)


# ------------------------------------------------------------------------------------------------ 3. layers
_REF = {}


def _wino_inputs(case):
    """Seeded inputs and the float64 reference of test_gpu_conv.py::test_winograd_f32_vs_float64 for one row of WINO_CASES, computed
    once and shared by the tile sizes and by test 6 (never modified)."""
    name, n, cin, h, w, cout, d = case
    if name not in _REF:
        g = synth.gen(zlib.crc32(name.encode()) % 10000 + 31)
        x = torch.randn((n, cin, h, w), generator=g) + 0.5
        wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
        b = torch.randn(cout, generator=g)
        xr, wr, br = x.double().requires_grad_(), wt.double().requires_grad_(), b.double().requires_grad_()
        yr = F.conv2d(xr, wr, br, 1, d, d)
        probe = torch.randn(yr.shape, generator=g)
        (yr * probe.double()).sum().backward()
        _REF[name] = (x, wt, b, probe, yr.detach(), xr.grad, wr.grad)
    return _REF[name]


def _wino_layer(case, wt, b):
    from diga_amd.model.conv import DigaConv2d
    name, n, cin, h, w, cout, d = case
    m = DigaConv2d(cin, cout, 3, stride=1, padding=d, dilation=d, bias=True)
    with torch.no_grad():
        m.weight.copy_(wt)
        m.bias.copy_(b)
    return m.to(DEV)


def _fwd_bwd(m, x, probe, math, x6w, bwd_x6w=None):
    """One forward + backward of layer m under conv arithmetic `math`, the forward with config.x6_winograd = x6w and the backward
    with bwd_x6w (default: the same): (y, dx, dw, path log)."""
    m.weight.grad = None
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    with _Mode(math) as log:
        with config.override(x6_winograd=x6w):
            y = m(xd)
        with config.override(x6_winograd=x6w if bwd_x6w is None else bwd_x6w):
            (y * probe.to(DEV)).sum().backward()
            torch.cuda.synchronize()
        log = dict(log)
    return y.detach(), xd.grad, m.weight.grad.clone(), log


@pytest.mark.parametrize("tile", [2, 4, 6], ids=["F2x2", "F4x4", "F6x6"])
@pytest.mark.parametrize("case", WINO_CASES, ids=[c[0] for c in WINO_CASES])
def test_layers_against_float64_and_fp32_winograd(case, tile, monkeypatch):
    """Forward, backward-data and backward-weight of every row of WINO_CASES with the tile forced and the ratio gate opened (as
    test_winograd_f32_vs_float64), in mode 0 and in mode 2 with x6_winograd, on the same inputs:
      * path_log: forward and backward-data on "winograd/x6", the weight gradient too exactly when Cout % 256 == 0 and Cin % 128 == 0
        (else the unchanged fp32 weight gradient);
      * every tensor within WINO_TOL[tile] of float64 and no further from it than 1.5 x the fp32 Winograd path (the layer's error
        is the fp32 transforms': DESIGN section 11);
      * wide layers: the weight gradient on a recomputed V is torch.equal to the one on the kept V."""
    from diga_amd.model import conv as dc
    name, n, cin, h, w, cout, d = case
    monkeypatch.setattr(config.active(), "winograd", True)
    monkeypatch.setattr(config.active(), "winograd_ratio", 10.0)
    monkeypatch.setattr(dc, "_wino_plan", lambda hi, wi, dd: (tile, 0.5))
    calls = _spy(monkeypatch)
    x, wt, b, probe, yr, dxr, dwr = _wino_inputs(case)
    m = _wino_layer(case, wt, b)
    wide = cout % 256 == 0 and cin % 128 == 0
    y0, dx0, dw0, log0 = _fwd_bwd(m, x, probe, 0, False)
    assert log0 == {("fwd", "winograd"): 1, ("dgrad", "winograd"): 1, ("wgrad", "winograd" if wide else "f32"): 1}, log0
    assert not any(nm in NEW_EXPORTS for nm in _names(calls)), _names(calls)
    calls.clear()
    y2, dx2, dw2, log2 = _fwd_bwd(m, x, probe, 2, True)
    assert log2 == {("fwd", "winograd/x6"): 1, ("dgrad", "winograd/x6"): 1, ("wgrad", "winograd/x6" if wide else "f32"): 1}, log2
    nm2 = _names(calls)
    assert nm2.count("diga_conv2d_winograd_bf16x6") == 2 and (nm2.count("diga_conv2d_wgrad_winograd_bf16x6") == 1) == wide, nm2
    assert not any("winograd_f32" in c for c in nm2), nm2
    fwd_call = next(a for c, a in calls if c == "diga_conv2d_winograd_bf16x6")
    assert (fwd_call[4].value is not None) == wide               # wide layers keep their V for the weight gradient
    row = []
    for got0, got2, want, what in ((y0, y2, yr, "y"), (dx0, dx2, dxr, "dx"), (dw0, dw2, dwr, "dw")):
        e0, e2 = _rel(got0, want), _rel(got2, want)
        row.append(f"{what} f32 {e0:.2e} x6 {e2:.2e} ratio {e2 / e0:.2f}")
    print(f"\n[x6 winograd table] tile {tile} {name:10s} K={cin:4d} | " + " | ".join(row))
    for got0, got2, want, what in ((y0, y2, yr, "y"), (dx0, dx2, dxr, "dx"), (dw0, dw2, dwr, "dw")):
        e0, e2 = _rel(got0, want), _rel(got2, want)
        assert e2 < WINO_TOL[tile][1 if what == "dw" else 0], (what, e2)
        assert e2 <= 1.5 * e0, f"{name} tile {tile} {what}: x6 {e2:.2e} vs fp32 Winograd {e0:.2e} of scale"
    if wide:
        calls.clear()
        with config.override(winograd_keep_v=False):
            _, _, dw_re, log_re = _fwd_bwd(m, x, probe, 2, True)
        assert log_re[("wgrad", "winograd/x6")] == 1
        assert all(a[4].value is None for c, a in calls if c == "diga_conv2d_winograd_bf16x6")
        assert next(a for c, a in calls if c == "diga_conv2d_wgrad_winograd_bf16x6")[2].value is None       # no kept V handed over
        assert torch.equal(dw_re, dw2)


# ------------------------------------------------------------------------------------------------ 4. flag off / other modes
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("3x3_dil2", "3x3_dil4")], ids=lambda c: c[0])
def test_flag_off_is_todays_mode_2_and_other_modes_do_not_see_it(case, monkeypatch):
    calls = _spy(monkeypatch)
    x, wt, b, probe = _inputs(case)[:4]
    res = {}
    for math, flag in ((0, False), (2, False), (0, True), (1, False), (1, True)):
        with config.override(x6_winograd=flag):
            res[(math, flag)] = _run_layer(case, math, x, wt, b, probe)
    assert not any(nm in NEW_EXPORTS for nm in _names(calls)), _names(calls)
    assert any("winograd" in a for _, a in res[(0, False)][4]), res[(0, False)][4]       # (the rows do take the Winograd path)

    def same(p, q):
        assert p[4] == q[4], (p[4], q[4])
        for i in range(4):
            assert (p[i] is None and q[i] is None) or torch.equal(p[i], q[i]), i
    same(res[(2, False)], res[(0, False)])
    same(res[(0, True)], res[(0, False)])
    same(res[(1, True)], res[(1, False)])
    # ... and with the flag on, mode 2 does take the new path on these rows
    with config.override(x6_winograd=True):
        on = _run_layer(case, 2, x, wt, b, probe)
    assert on[4][("fwd", "winograd/x6")] == 1 and on[4][("dgrad", "winograd/x6")] == 1 and on[4][("wgrad", "winograd/x6")] == 1, on[4]
    assert _names(calls).count("diga_conv2d_winograd_bf16x6") == 2 and _names(calls).count("diga_conv2d_wgrad_winograd_bf16x6") == 1


# ------------------------------------------------------------------------------------------------ 5. statistics and epilogue
@pytest.mark.parametrize("tile", [4, 6], ids=["F4x4", "F6x6"])
def test_output_transform_bn_statistics(tile, monkeypatch):
    """test_winograd_output_transform_bn_statistics on the new path, at its bounds: the "d1_ragged" row (33 x 29, dilation 1: the plan
    takes 6 x 6 tiles, 4 x 4 under a cap of 4) with train-mode BatchNorm behind the conv.  y with statistics is torch.equal to y without;
    BatchNorm fed by the records against float64 and against BatchNorm that re-reads y; running statistics."""
    from diga_amd.model.conv import DigaConv2d
    from diga_amd.model.norm import DigaBatchNorm2d
    case = next(c for c in WINO_CASES if c[0] == "d1_ragged")
    name, n, cin, h, w, cout, dil = case
    monkeypatch.setattr(config.active(), "winograd_max_tile", tile)
    monkeypatch.setattr(config.active(), "winograd_ratio", 10.0)
    calls = _spy(monkeypatch)
    g = synth.gen(zlib.crc32(name.encode()) % 10000 + 11 + tile)
    x = torch.randn((n, cin, h, w), generator=g) + 2.0
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
    conv = DigaConv2d(cin, cout, 3, stride=1, padding=dil, dilation=dil, bias=False)
    bn_a, bn_b = DigaBatchNorm2d(cout), DigaBatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(wt)
        for bn in (bn_a, bn_b):
            bn.weight.copy_(torch.linspace(0.5, 1.5, cout))
            bn.bias.copy_(torch.linspace(-0.2, 0.2, cout))
            for p in bn.parameters():
                p.requires_grad = False
    conv, bn_a, bn_b = conv.to(DEV).train(), bn_a.to(DEV).train(), bn_b.to(DEV).train()
    conv.emit_bn_stats = True
    xd = x.to(DEV)
    with config.override(x6_winograd=True), _Mode(2) as log:
        y = conv(xd)
        part = getattr(y, "_diga_bn_partials", None)
        assert part is not None and part[1][0] == "records" and part[1][1] > 0
        fused = bn_a(y, relu=True)
        with config.override(winograd_stats=False):
            y2 = conv(xd)
            assert not hasattr(y2, "_diga_bn_partials") and torch.equal(y2, y)
            plain = bn_b(y2, relu=True)
        torch.cuda.synchronize()
        log = dict(log)
    assert log == {("fwd", "winograd/x6"): 2}, log
    layer_calls = [a for c, a in calls if c == "diga_conv2d_winograd_bf16x6"]
    assert len(layer_calls) == 2 and layer_calls[0][15] == tile and layer_calls[1][15] == tile
    assert layer_calls[0][17].value is not None and layer_calls[1][17].value is None       # statistics buffer: first call only
    yd = y.detach().double().cpu()
    mean, var = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
    ref = torch.relu((yd - mean[None, :, None, None]) / torch.sqrt(var + bn_a.eps)[None, :, None, None]
                     * bn_a.weight.double().cpu()[None, :, None, None] + bn_a.bias.double().cpu()[None, :, None, None])
    assert_close(fused.cpu(), ref, rtol=2e-5, atol=2e-5, what=f"{name} BN on records")
    assert_close(fused.cpu(), plain.cpu(), rtol=1e-5, atol=1e-5, what=f"{name} records vs statistics pass")
    cnt = yd.numel() // cout
    assert_close(bn_a.running_mean.cpu(), 0.1 * mean, rtol=1e-5, atol=1e-6, what="running_mean")
    assert_close(bn_a.running_var.cpu(), 0.9 + 0.1 * var * cnt / (cnt - 1), rtol=1e-5, atol=1e-6, what="running_var")
    recs = int(part[1][1])
    counts = part[0][recs * 3 * cout: recs * 3 * cout + recs]
    assert float(counts.sum()) == n * h * w


def test_dilated_bottleneck_with_backward_epilogue(monkeypatch):
    """One bottleneck of layer3's widths (1024 -> 256 -> 1024, dilation 2, identity residual, train-mode BatchNorm) on the map
    test_residual_junction_fused_backward_vs_float64 uses for them (2 x 33 x 33), in mode 2 with x6_winograd: conv2 runs forward,
    backward-data WITH the epilogue that finishes bn1's gradient, and its weight gradient on "winograd/x6".  y, dx and the three weight
    gradients against the float64 oracle with the device's ReLU patterns pinned, at the 2e-5 of scale of
    test_residual_junction_epilogues_and_forward_statistics; fuse_bwd on and off agree within the same bound."""
    from diga_amd.model import norm as dn
    planes, inpl, dil, n, h, w = 256, 1024, 2, 2, 33, 33
    nm = f"x6wino{planes}.b0"
    sd = _block_state(nm, inpl, planes)
    blk = _make_block(sd, nm, inpl, planes, dil)
    g = synth.gen(planes + 6)
    x = torch.randn((n, inpl, h, w), generator=g).relu_() + 0.1 * torch.randn((n, inpl, h, w), generator=g)
    probe = torch.randn((n, inpl, h, w), generator=g)
    calls = _spy(monkeypatch)

    def run(fuse):
        for p in blk.parameters():
            p.grad = None
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
        seen, hooks = {}, []
        hooks.append(blk.bn1.register_forward_hook(lambda m, a, o: seen.__setitem__(1, (o.detach() > 0).cpu().double())))
        hooks.append(blk.bn2.register_forward_hook(lambda m, a, o: seen.__setitem__(2, (o.detach() > 0).cpu().double())))
        hooks.append(blk.register_forward_hook(lambda m, a, o: seen.__setitem__(3, (o.detach() > 0).cpu().double())))
        calls.clear()
        with config.override(x6_winograd=True, x6_split="loader", fuse_bwd=fuse), _Mode(2) as log:
            assert dn.fuse_backward_enabled() == fuse
            y = blk(xd)
            (y * probe.to(DEV)).sum().backward()
            torch.cuda.synchronize()
            log = dict(log)
        for hk in hooks:
            hk.remove()
        grads = {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None}
        return y.detach().clone(), xd.grad.clone(), grads, seen, log, list(calls)

    y1, dx1, gr1, masks, log1, calls1 = run(True)
    y0, dx0, gr0, masks0, log0, calls0 = run(False)
    for log in (log1, log0):
        assert log[("fwd", "winograd/x6")] == 1 and log[("dgrad", "winograd/x6")] == 1 and log[("wgrad", "winograd/x6")] == 1, log
        assert not any(a in ("winograd", "f32") for _, a in log), log
    epi1 = [a[18] for c, a in calls1 if c == "diga_conv2d_winograd_bf16x6"]
    epi0 = [a[18] for c, a in calls0 if c == "diga_conv2d_winograd_bf16x6"]
    assert len(epi1) == 2 and epi1[0] is None and epi1[1] is not None, "fuse_bwd: backward-data of conv2 carries the epilogue"
    assert epi0 == [None, None]
    assert torch.equal(y1, y0) and all(torch.equal(masks[k], masks0[k]) for k in masks)

    sd64 = {k: v.double().requires_grad_(v.dim() == 4) for k, v in sd.items()}
    xr = x.double().requires_grad_()
    yr = od.bottleneck_fixed_masks(sd64, nm, xr, 1, dil, False, (masks[1], masks[2], masks[3]))
    (yr * probe.double()).sum().backward()
    errs = {"y": _rel(y1, yr), "dx fused": _rel(dx1, xr.grad), "dx plain": _rel(dx0, xr.grad)}
    assert len(gr1) == 3 and gr1.keys() == gr0.keys()
    for k in gr1:
        errs["fused " + k] = _rel(gr1[k], sd64[f"{nm}.{k}"].grad)
        errs["plain " + k] = _rel(gr0[k], sd64[f"{nm}.{k}"].grad)
    print(f"\n[x6 winograd bottleneck] worst error / scale vs float64: {max(errs.values()):.1e} ({max(errs, key=errs.get)})")
    for k, v in errs.items():
        assert v < 2e-5, f"{k}: {v:.2e} of scale"
    assert _rel(dx1, dx0) < 2e-5
    for k in gr1:
        assert _rel(gr1[k], gr0[k]) < 2e-5, k


# ------------------------------------------------------------------------------------------------ 6. flag switched inside a graph
@pytest.mark.parametrize("fwd_on,bwd_on", [(True, False), (False, True)], ids=["on_off", "off_on"])
def test_flag_switched_between_forward_and_backward(fwd_on, bwd_on, monkeypatch):
    """The flag is read per call and a kept V is fp32 either way: the "d1_wide" row (384 -> 512: wide, its forward keeps V) with the
    forward under one setting and the backward under the other runs, on the path each call selected, within WINO_TOL of float64."""
    from diga_amd.model import conv as dc
    tile = 4
    case = next(c for c in WINO_CASES if c[0] == "d1_wide")
    monkeypatch.setattr(config.active(), "winograd_ratio", 10.0)
    monkeypatch.setattr(dc, "_wino_plan", lambda hi, wi, dd: (tile, 0.5))
    calls = _spy(monkeypatch)
    x, wt, b, probe, yr, dxr, dwr = _wino_inputs(case)
    m = _wino_layer(case, wt, b)
    y, dx, dw, log = _fwd_bwd(m, x, probe, 2, fwd_on, bwd_on)
    tag_f, tag_b = ("winograd/x6" if on else "winograd" for on in (fwd_on, bwd_on))
    assert log == ({("fwd", tag_f): 1, ("dgrad", tag_b): 1, ("wgrad", tag_b): 1}), log
    fwd_name = "diga_conv2d_winograd_bf16x6" if fwd_on else "diga_conv2d_winograd_f32_keep"
    wg_name = "diga_conv2d_wgrad_winograd_bf16x6" if bwd_on else "diga_conv2d_wgrad_winograd_f32"
    kept = next(a for c, a in calls if c == fwd_name)[4].value
    assert kept is not None and next(a for c, a in calls if c == wg_name)[2].value == kept       # the forward's V feeds the weight gradient
    for got, want, what in ((y, yr, "y"), (dx, dxr, "dx"), (dw, dwr, "dw")):
        e = _rel(got, want)
        assert e < WINO_TOL[tile][1 if what == "dw" else 0], (what, e)


# ------------------------------------------------------------------------------------------------ 7. whole model
def test_whole_small_model_gradients_vs_float64_with_pinned_switches():
    """The construction of test_gpu_conv_bf16x6.py::test_whole_model_gradients_vs_float64_with_pinned_switches for the small backbone at
    96 x 128, in mode 2 with x6_split = "loader" and x6_winograd, at that test's mode-2 bounds: logits within 8e-5 of scale, every
    parameter gradient within 5e-5.  At this size layer4's conv2 (128 -> 128, dilation 4, 13 x 17 map) and the ASPP's 3x3 layers of
    small dilation take the Winograd path: path_log must show forward and backward-data on "winograd/x6"."""
    from diga_amd.model import seg_model_noaux as sm
    from diga_amd.model.model_noaux import SegModel
    from diga_amd.model.norm import DigaBatchNorm2d, DigaGroupNorm
    arch_d, arch_o, hw = sm.TINY, od.TINY, (96, 128)
    sd32 = detweights.state_dict(arch_o)
    m = SegModel(arch=arch_d)
    m.load_state_dict(sd32)
    m = m.to(DEV).train()
    m.final.head[0].p = 0.0
    g = synth.gen(4242)
    x = torch.rand((2, 3) + hw, generator=g) * 2 - 1
    xd = x.to(DEV)
    with config.override(x6_split="loader", x6_winograd=True), _Mode(2) as log:
        seen, hooks = {}, []
        names = {mod: n for n, mod in m.named_modules()}
        for mod in m.modules():
            if isinstance(mod, DigaBatchNorm2d) or (isinstance(mod, DigaGroupNorm) and ".conv2d_list." in names[mod]):
                hooks.append(mod.register_forward_hook(lambda mo, i, o, n=names[mod]: seen.__setitem__(n, (o.detach() > 0).cpu().double())))
        hooks.append(m.layer0[3].register_forward_hook(lambda mo, i, o: seen.__setitem__("pool_in", i[0].detach().cpu().double())))
        hooks.append(m.final.bottleneck[0].se[1].register_forward_hook(lambda mo, i, o: seen.__setitem__("se", (o.detach() > 0).cpu().double())))
        try:
            with torch.no_grad():
                out_plain = m(xd)[2]
        finally:
            for h in hooks:
                h.remove()
        masks = {"layer0": seen["layer0.1"], "se": seen["se"],
                 "pool_idx": F.max_pool2d(seen["pool_in"], 3, 2, 1, ceil_mode=True, return_indices=True)[1]}
        for li in range(4):
            for bi in range(arch_o.layers[li]):
                for k in (1, 2, 3):
                    masks[f"layer{li + 1}.{bi}.{k}"] = seen[f"layer{li + 1}.{bi}.bn{k}"]
        for b in range(5):
            masks[f"aspp.{b}"] = seen[f"final.conv2d_list.{b}.1"]
        trainable = [k for k, (_, kind) in od.state_shapes(arch_o).items() if kind in ("conv", "bias", "gn_w", "gn_b", "lin", "head")]
        sd64 = {k: (v.double().requires_grad_() if k in trainable else v.double()) for k, v in sd32.items()}
        _, _, out_r, feat_r = od.forward_fixed_masks(sd64, x.double(), dataclasses.replace(arch_o, droprate=0.0), masks,
                                                     keep_mask=torch.ones(2, arch_o.aspp_width))
        probe = torch.randn(out_r.shape, generator=g)
        probe_f = 0.1 * torch.randn(feat_r.shape, generator=g)
        ((out_r * probe.double()).sum() + (feat_r * probe_f.double()).sum()).backward()
        log.clear()
        _, _, out, feat = m(xd)
        assert torch.equal(out.detach(), out_plain)
        e_fwd = _rel(out, out_r)
        print(f"\n[x6 winograd model] TINY: logits within {e_fwd:.1e} of scale of the float64 oracle")
        assert e_fwd < FWD_TOL_F32
        ((out * probe.to(DEV)).sum() + (feat * probe_f.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        log = dict(log)
    assert log.get(("fwd", "winograd/x6"), 0) > 0 and log.get(("dgrad", "winograd/x6"), 0) > 0, log
    assert not any(a == "winograd" for _, a in log), log
    assert all(log.get((p, "bf16x6/ls"), 0) > 0 for p in ("fwd", "dgrad", "wgrad")), log
    named = dict(m.named_parameters())
    worst, worst_k = 0.0, None
    for k in trainable:
        ref = sd64[k].grad
        e = float((named[k].grad.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        if e > worst:
            worst, worst_k = e, k
        assert e < 5e-5, (k, e)
    print(f"[x6 winograd model] TINY: all {len(trainable)} parameter gradients within {worst:.1e} of scale (worst: {worst_k}); paths {log}")
