"""GPU tests of the narrow tiles of the bf16x6 weight gradient (config.x6_wgrad_tile = "fit" under conv_math = 2; csrc/conv_bf16x6.h:
conv_wgrad_x6_kernel<64, 64> / <64, 128> / <128, 128> / <256, 64>, diga_wgrad_bf16x6_tiled_f32in; model/conv.py: _Path.fit).

  (a) dw bit for bit against the wide tile's entry points where both split-K plans cut the pixels into the same ranges;
  (b) a shape whose ranges differ: against float64 and against the wide tile's error;
  (c) through DigaConv2d: path_log, equality with the "wide" run, the switch flipped between forward and backward;
  (d) the whole small model with all four x6 switches.
The split-K plans are restated in tests/test_bf16x6_wgrad_tiles_cpu.py (which checks them against the library's workspace query)."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from diga_amd import config

from conftest import assert_close
from oracle import deeplab as od
from oracle import detweights, synth
from test_bf16x6_wgrad_tiles_cpu import fit_splits, tile_rule, wide_splits
from test_gpu_conv_bf16x6 import FWD_TOL_F32, _inputs, _Mode

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _leave_global_rng_and_arithmetic_untouched():
    """As tests/test_gpu_conv_bf16x6.py: every test hands torch's generators and the process-wide conv arithmetic back as it found them."""
    from diga_amd import _lib
    cpu, gpu = torch.get_rng_state(), (torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    math = _lib.get_conv_math()
    yield
    _lib.join_side()
    _lib.set_conv_math(math)
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max()) / float(ref.detach().abs().max())


def _wgrad(entry, query, dy, x, cout, cin, k, stride, pad, dil):
    """One call of a loader-form weight-gradient entry point: dy [N,Ho,Wo,>=Cout] and x [N,H,W,>=Cin] fp32 (channel slices of wider
    tensors read in place), dw [Cout,k,k,Cin] pre-filled with NaN."""
    from diga_amd import _lib
    n, h, w, _ = x.shape
    _, ho, wo, _ = dy.shape
    nbytes = getattr(_lib.lib, query)(n, ho, wo, cout, cin, k, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dw = torch.full((cout, k, k, cin), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call(entry, _lib.ptr(dy), dy.stride(2), _lib.ptr(x), x.stride(2), _lib.ptr(dw), _lib.ptr(ws), ws.numel(), n, h, w, cin, ho, wo, cout,
              k, k, stride, stride, -pad, -pad, dil, dil, _lib.stream())
    torch.cuda.synchronize()
    return dw


def _wide(dy, x, cout, cin, k, stride, pad, dil):
    if k == 1:
        return _wgrad("diga_conv2d_wgrad_bf16x6_f32in", "diga_conv2d_wgrad_bf16x6_workspace_bytes", dy, x, cout, cin, k, stride, pad, dil)
    return _wgrad("diga_conv_taps_wgrad_bf16x6_f32in", "diga_conv_taps_wgrad_bf16x6_workspace_bytes", dy, x, cout, cin, k, stride, pad, dil)


def _fit(dy, x, cout, cin, k, stride, pad, dil):
    return _wgrad("diga_wgrad_bf16x6_tiled_f32in", "diga_wgrad_bf16x6_tiled_workspace_bytes", dy, x, cout, cin, k, stride, pad, dil)


# name, N, Cin, H, W, Cout, k, stride, pad, dilation, bias (the tuple of test_gpu_conv.CASES), tile, pixel ranges, pitched operands
CASES = [
    (("t01_64x64_two_ranges", 2, 64, 17, 19, 64, 1, 1, 0, 1, False), (64, 64), 2, False),          # M = 646, not a multiple of 32
    (("t02_64x64_partial_kstep", 1, 64, 5, 5, 64, 1, 1, 0, 1, False), (64, 64), 1, False),          # one partial K-step
    (("t03_64x256_seven_ranges", 2, 256, 33, 29, 64, 1, 1, 0, 1, False), (64, 128), 7, False),      # two Cin tiles
    (("t04_256x64", 2, 64, 17, 19, 256, 1, 1, 0, 1, False), (256, 64), 2, False),
    (("t05_320x64_ragged_cout_tile", 2, 64, 17, 19, 320, 1, 1, 0, 1, False), (256, 64), 2, False),
    (("t06_128x512", 2, 512, 17, 19, 128, 1, 1, 0, 1, False), (128, 128), 2, False),
    (("t07_24x160_head_and_stem", 2, 160, 17, 19, 24, 1, 1, 0, 1, False), (64, 128), 2, False),     # ragged in both directions
    (("t08_40x72_clamped_chunks", 2, 72, 17, 19, 40, 1, 1, 0, 1, False), (64, 128), 2, True),
    (("t09_64x64_3x3", 2, 64, 17, 19, 64, 3, 1, 1, 1, False), (64, 64), 2, True),
    (("t10_64x64_3x3_stride2", 2, 64, 17, 19, 64, 3, 2, 1, 1, False), (64, 64), 1, False),
    (("t11_128x128_3x3_dil2", 2, 128, 33, 29, 128, 3, 1, 2, 2, False), (128, 128), 7, False),
    (("t12_64x32_3x3_minimal_cin", 2, 32, 17, 19, 64, 3, 1, 1, 1, False), (64, 64), 2, False),
]


def _pitched(t, extra, lead):
    """t [N,H,W,C] as a channel slice (offset `lead`, a multiple of 4 floats: 16-byte aligned) of a wider NaN-filled tensor."""
    n, h, w, c = t.shape
    wide = torch.full((n, h, w, c + extra), float("nan"), dtype=torch.float32, device=t.device)
    wide[..., lead:lead + c] = t
    return wide[..., lead:lead + c]


@pytest.mark.parametrize("case,tile,ranges,pitched", CASES, ids=[c[0][0] for c in CASES])
def test_narrow_tile_equals_wide_tile(case, tile, ranges, pitched):
    """(a) dw of diga_wgrad_bf16x6_tiled_f32in against dw of the existing entry point on the same tensors, torch.equal, dw pre-filled
    with NaN.  Both plans cut the pixels into the same ranges -- asserted from the two restatements: at these sizes the floor of 8
    K-steps per block decides in both -- so a 16 x 16 sub-tile of dw sees the same fragments in the same MFMA sequence, range by range,
    and the slabs are added in the same fixed order.  Every dw is also held to F.conv2d's float64 weight gradient at
    test_conv_fwd_bwd's 3e-6 of scale.  Pitched cases read dy and x as channel slices of wider tensors (dy_ld > Cout, x_ld > Cin)."""
    name, n, cin, h, w, cout, k, stride, pad, dil, _ = case
    x, _, _, probe, _, _, dwr, _ = _inputs(case)
    xd, dy = x.permute(0, 2, 3, 1).contiguous().to(DEV), probe.permute(0, 2, 3, 1).contiguous().to(DEV)
    if pitched:
        xd, dy = _pitched(xd, 8, 4), _pitched(dy, 24, 8)
        assert xd.stride(2) > cin and dy.stride(2) > cout
    m, rs = n * dy.shape[1] * dy.shape[2], k * k
    assert tile_rule(cout, cin) == tile != (256, 128)
    plan_w, plan_f = wide_splits(m, cout, cin, rs), fit_splits(m, cout, cin, rs)
    assert plan_f == plan_w and plan_f[0] == ranges == max(-(-m // 32) // 8, 1), (plan_w, plan_f)      # the floor decides in both
    got = _fit(dy, xd, cout, cin, k, stride, pad, dil)
    want = _wide(dy, xd, cout, cin, k, stride, pad, dil)
    assert not torch.isnan(got).any() and not torch.isnan(want).any()
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} elements differ, worst {float((got - want).abs().max()):.3e}"
    ref = dwr.permute(0, 2, 3, 1)
    print(f"\n[bf16x6 wgrad tiles] {name:30s} tile {tile} ranges {ranges}: {_rel(got, ref):.2e} of scale vs float64")
    assert_close(got, ref, 1e-5, 3e-6 * float(ref.abs().max()), f"{name} grad weight vs float64")


def test_wide_shape_runs_the_existing_entry_point():
    """A (256, 128) shape through the new entry point is the existing entry point: bit for bit, pointwise and multi-tap."""
    for case in (("t13_264x136", 2, 136, 17, 19, 264, 1, 1, 0, 1, False), ("t14_264x160_3x3", 1, 160, 9, 11, 264, 3, 1, 1, 1, False)):
        name, n, cin, h, w, cout, k, stride, pad, dil, _ = case
        assert tile_rule(cout, cin) == (256, 128)
        x, _, _, probe, _, _, dwr, _ = _inputs(case)
        xd, dy = x.permute(0, 2, 3, 1).contiguous().to(DEV), probe.permute(0, 2, 3, 1).contiguous().to(DEV)
        got, want = _fit(dy, xd, cout, cin, k, stride, pad, dil), _wide(dy, xd, cout, cin, k, stride, pad, dil)
        assert torch.equal(got, want), name
        ref = dwr.permute(0, 2, 3, 1)
        assert_close(got, ref, 1e-5, 3e-6 * float(ref.abs().max()), f"{name} grad weight vs float64")


def test_other_pixel_ranges_than_the_wide_plan():
    """(b) 64 -> 64 3x3 on 4 x 97 x 97 (layer1.conv2's shape at a quarter of the batch): nine taps on one 64 x 64 tile ask for
    ceil(2 * 256 * 3 / 9) = 171 ranges where the wide plan asks for ceil(512 / 9) = 57, and the floor allows 147 -- another split-K tree.
    dw within 3e-6 of scale of float64, and no further from it than 1.5 x the existing entry point on the same inputs."""
    n, c, hw, k = 4, 64, 97, 3
    m = n * hw * hw
    sf, sw = fit_splits(m, c, c, k * k), wide_splits(m, c, c, k * k)
    assert sf[0] != sw[0] and sf[0] > sw[0] and sf[1] >= 8, (sf, sw)
    g = synth.gen(1697)
    x = torch.randn((n, c, hw, hw), generator=g)
    dy = torch.randn((n, c, hw, hw), generator=g)
    wr = torch.zeros((c, c, k, k), dtype=torch.float64, requires_grad=True)
    (F.conv2d(x.double(), wr, None, 1, 1, 1) * dy.double()).sum().backward()
    ref = wr.grad.permute(0, 2, 3, 1)
    xd, dyd = x.permute(0, 2, 3, 1).contiguous().to(DEV), dy.permute(0, 2, 3, 1).contiguous().to(DEV)
    got, wide = _fit(dyd, xd, c, c, k, 1, 1, 1), _wide(dyd, xd, c, c, k, 1, 1, 1)
    e_fit, e_wide = _rel(got, ref), _rel(wide, ref)
    print(f"\n[bf16x6 wgrad tiles] 64x64 3x3 4x97x97: fit {sf[0]} ranges {e_fit:.2e}, wide {sw[0]} ranges {e_wide:.2e} of scale vs float64")
    assert not torch.isnan(got).any()
    assert_close(got, ref, 1e-5, 3e-6 * float(ref.abs().max()), "grad weight vs float64")
    assert e_fit <= 1.5 * e_wide, (e_fit, e_wide)


# ------------------------------------------------------------------------------------------------ (c) through the layer
LAYERS = [("3x3_64_64", 64, 64, 3, 1, "bf16x6/taps"), ("1x1_256_64", 256, 64, 1, 0, "bf16x6/ls")]


@pytest.mark.parametrize("name,cin,cout,k,pad,arith", LAYERS, ids=[c[0] for c in LAYERS])
def test_through_the_layer(name, cin, cout, k, pad, arith):
    """DigaConv2d forward and backward under conv_math = 2, x6_split = "loader", x6_taps, on 2 x 17 x 19 -- where the two plans cut the
    pixels alike (asserted), so the "fit" weight gradient is torch.equal to the "wide" one.  path_log shows the /fit key under "fit" and the
    previous keys under "wide"; output and input gradient never move; the switch is read per call, so flipping it between forward and
    backward gives the backward's kernel."""
    from diga_amd.model.conv import DigaConv2d
    case = (name, 2, cin, 17, 19, cout, k, 1, pad, 1, False)
    n, h, w = 2, 17, 19
    assert fit_splits(n * h * w, cout, cin, k * k) == wide_splits(n * h * w, cout, cin, k * k) and tile_rule(cout, cin) != (256, 128)
    x, wt, _, probe, yr, dxr, dwr, _ = _inputs(case)
    m = DigaConv2d(cin, cout, k, padding=pad, bias=False)
    with torch.no_grad():
        m.weight.copy_(wt)
    m = m.to(DEV)

    def run(fwd_tile, bwd_tile):
        m.weight.grad = None
        xd = x.to(DEV).requires_grad_()
        with config.override(x6_split="loader", x6_taps=True), _Mode(2) as log:
            with config.override(x6_wgrad_tile=fwd_tile):
                y = m(xd)
            with config.override(x6_wgrad_tile=bwd_tile):
                (y * probe.to(DEV)).sum().backward()
                torch.cuda.synchronize()
            log = dict(log)
        return y.detach(), xd.grad, m.weight.grad.clone(), log

    keys = lambda tile: {("fwd", arith): 1, ("dgrad", arith): 1, ("wgrad", arith + ("/fit" if tile == "fit" else "")): 1}
    y_w, dx_w, dw_w, log_w = run("wide", "wide")
    y_f, dx_f, dw_f, log_f = run("fit", "fit")
    assert log_w == keys("wide"), log_w                   # the previous keys
    assert log_f == keys("fit"), log_f
    assert torch.equal(y_f, y_w) and torch.equal(dx_f, dx_w)
    assert torch.equal(dw_f, dw_w), int((dw_f != dw_w).sum())
    assert_close(dw_f, dwr, 1e-5, 3e-6 * float(dwr.abs().max()), f"{name} grad weight vs float64")
    assert_close(y_f, yr, 1e-5, 2e-6 * float(yr.abs().max()), f"{name} forward vs float64")
    for fwd_tile, bwd_tile in (("wide", "fit"), ("fit", "wide")):
        y, dx, dw, log = run(fwd_tile, bwd_tile)
        assert log == keys(bwd_tile), (fwd_tile, bwd_tile, log)
        assert torch.equal(y, y_w) and torch.equal(dx, dx_w) and torch.equal(dw, dw_w)
    # outside conv_math = 2 the switch is not read
    with config.override(x6_wgrad_tile="fit"), _Mode(0) as log0:
        m.weight.grad = None
        (m(x.to(DEV)) * probe.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert not any("bf16x6" in a for _, a in log0), dict(log0)


# ------------------------------------------------------------------------------------------------ (d) the small model
def test_whole_small_model_with_all_four_x6_switches():
    """The construction of test_gpu_conv_bf16x6_taps.py::test_whole_small_model_leaves_nothing_on_the_fp32_pipe... -- the small backbone
    at 96 x 128 against the float64 oracle with the device's ReLU patterns and max-pool choices pinned -- in mode 2 with
    x6_split = "loader", x6_winograd, x6_taps AND x6_wgrad_tile = "fit", at that test's bounds: logits within 8e-5 of scale, every
    parameter gradient within 5e-5.  path_log: narrow-tile weight gradients of both kinds ran, nothing is on the fp32 kernels."""
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
    named = dict(m.named_parameters())
    with config.override(x6_split="loader", x6_winograd=True, x6_taps=True, x6_wgrad_tile="fit"), _Mode(2) as log:
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
        print(f"\n[bf16x6 wgrad tiles model] TINY: logits within {e_fwd:.1e} of scale of the float64 oracle")
        assert e_fwd < FWD_TOL_F32
        ((out * probe.to(DEV)).sum() + (feat * probe_f.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        log = dict(log)
    assert {a for _, a in log} <= {"bf16x6/ls", "winograd/x6", "bf16x6/taps", "bf16x6/ls/fit", "bf16x6/taps/fit"}, log
    assert log.get(("wgrad", "bf16x6/ls/fit"), 0) > 0 and log.get(("wgrad", "bf16x6/taps/fit"), 0) > 0, log
    assert not any(a.endswith("/fit") for p, a in log if p != "wgrad"), log
    worst, worst_k = 0.0, None
    for k in trainable:
        ref = sd64[k].grad
        e = float((named[k].grad.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        if e > worst:
            worst, worst_k = e, k
        assert e < 5e-5, (k, e)
    print(f"[bf16x6 wgrad tiles model] TINY: all {len(trainable)} parameter gradients within {worst:.1e} of scale (worst: {worst_k}); paths {log}")
