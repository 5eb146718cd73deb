"""GPU tests of the bf16x6 arithmetic (conv_math = 2, csrc/conv_bf16x6.h): fp32 operands carried exactly as three bf16 planes, six
bf16 MFMAs per product, on the pointwise layers; every other layer exactly as in conv_math = 0.

  * the split passes bit for bit against the torch restatement (tools/bf16x6_emulation.py);
  * a per-layer error table against float64, mode 2 next to the exact-fp32 kernels measured on the same inputs;
  * bit-identity of every non-pointwise layer with mode 0;
  * the backward-data epilogues and the forward BatchNorm statistics on a residual junction;
  * the whole model against the float64 oracle and the reference's capture at the exact-fp32 bounds;
  * the forward -> backward arithmetic guard.
`conv.path_log` proves which kernels ran: a layer that silently fell back to fp32 fails its test."""
import dataclasses
import importlib.util
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

from diga_amd import config

from conftest import assert_close
from oracle import deeplab as od
from oracle import detweights, synth
from test_gpu_conv import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _leave_global_rng_untouched():
    """Layer constructors here draw their initial weights from torch's global generators.  Tests that run later in the same process do
    the same and some are sensitive to the draw, so every test of this file hands the generators back in the state it found them."""
    cpu, gpu = torch.get_rng_state(), (torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _emulation():
    spec = importlib.util.spec_from_file_location("bf16x6_emulation", os.path.join(ROOT, "tools", "bf16x6_emulation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Mode:
    """`with _Mode(2) as log:` -- run the body under a conv arithmetic with conv.path_log collecting; both restored on exit."""

    def __init__(self, math):
        self.math = math

    def __enter__(self):
        from diga_amd import _lib
        from diga_amd.model import conv as dc
        self.prev, self.prev_log = _lib.get_conv_math(), dc.path_log
        _lib.set_conv_math(self.math)
        dc.path_log = {}
        return dc.path_log

    def __exit__(self, *exc):
        from diga_amd import _lib
        from diga_amd.model import conv as dc
        _lib.join_side()
        _lib.set_conv_math(self.prev)
        dc.path_log = self.prev_log
        return False


def _bits(t):
    return t.to(torch.bfloat16).view(torch.int16)


def _lds_swz(r):
    return ((0x78 >> (((r >> 2) & 3) * 2)) & 3) ^ (((r >> 1) & 1) << 1)


# ------------------------------------------------------------------------------------------------ 4. split passes
@pytest.mark.parametrize("c", [32, 96, 256])
@pytest.mark.parametrize("m", [1, 77, 2046])
def test_activation_split_is_bit_exact(m, c):
    from diga_amd import _lib
    em = _emulation()
    g = synth.gen(1000 + m + c)
    ld = c + 8                                                    # a channel slice of a wider tensor
    x = torch.randn((m, ld), generator=g) * torch.exp2(torch.randint(-20, 21, (m, ld), generator=g).float())
    xd = x.to(DEV)
    trip = torch.zeros(m * c * 6 + 64, dtype=torch.uint8, device=DEV)
    _lib.call("diga_make_triplet", _lib.ptr(xd), ld, _lib.ptr(trip), m, c, _lib.stream())
    torch.cuda.synchronize()
    assert int(trip[m * c * 6:].sum()) == 0                      # nothing written past the image
    got = trip[:m * c * 6].cpu().view(torch.int16).reshape(m, c // 8, 3, 8)
    planes = em.split3(x[:, :c])
    assert planes[3] == 0.0
    for p in range(3):
        assert torch.equal(got[:, :, p, :].reshape(m, c), _bits(planes[p])), f"plane {p}"


@pytest.mark.parametrize("c", [32, 96, 256])
@pytest.mark.parametrize("k", [19, 64, 320])
def test_weight_split_image_is_bit_exact(k, c):
    from diga_amd import _lib
    em = _emulation()
    g = synth.gen(2000 + k + c)
    w = torch.randn((k, c), generator=g) * (2.0 / c) ** 0.5
    nbytes = _lib.lib.diga_split_bf16x6_image_bytes(k, 1, c)
    bn = 128 if k > 64 else 64
    tiles, ksteps = (k + bn - 1) // bn, c // 32
    assert nbytes == tiles * ksteps * 3 * bn * 64
    img = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
    wd = w.to(DEV)
    _lib.call("diga_split_bf16x6_image", _lib.ptr(wd), _lib.ptr(img), k, 1, c, _lib.stream())
    torch.cuda.synchronize()
    assert int(img[nbytes:].sum()) == 0
    raw = img[:nbytes].cpu().view(torch.int16).reshape(tiles, ksteps, 3, bn, 4, 8)
    pos = torch.tensor([[s ^ _lds_swz(r) for s in range(4)] for r in range(bn)])             # logical slot s of row r sits at pos[r][s]
    logical = torch.gather(raw, 4, pos.view(1, 1, 1, bn, 4, 1).expand(tiles, ksteps, 3, bn, 4, 8)).reshape(tiles, ksteps, 3, bn, 32)
    planes = em.split3(w)
    rows = torch.arange(tiles * bn).clamp_max(k - 1)                                         # rows past Cout repeat the last channel
    for p in range(3):
        want = _bits(planes[p])[rows].reshape(tiles, bn, ksteps, 32).permute(0, 2, 1, 3)
        assert torch.equal(logical[:, :, p], want), f"plane {p}"


# ------------------------------------------------------------------------------------------------ 5. per-layer error table
POINTWISE_CASES = [c for c in CASES if c[6] == 1]                # the nine 1x1 rows of test_gpu_conv.CASES (head_19 is eligible too)
assert [c[0] for c in POINTWISE_CASES] == ["1x1_64_256", "1x1_256_64", "1x1_stride2", "head_19", "big_m", "wide_stride2", "wide_many_splits",
                                           "1x1_ragged_320", "1x1_1024_bias"]
# the pointwise layers of tools/bench_conv.py::SHAPES (name, Cin, Cout, stride) on a small map: 2 images of 33 x 31
BENCH_PAIRS = [("l1.conv1.first", 64, 64, 1), ("l1.conv1", 256, 64, 1), ("l1.conv3", 64, 256, 1), ("l2.conv1.first", 256, 128, 2),
               ("l2.conv1", 512, 128, 1), ("l2.conv3", 128, 512, 1), ("l2.down", 256, 512, 2), ("l3.conv1.first", 512, 256, 1),
               ("l3.conv1", 1024, 256, 1), ("l3.conv3", 256, 1024, 1), ("l3.down", 512, 1024, 1), ("l4.conv1.first", 1024, 512, 1),
               ("l4.conv1", 2048, 512, 1), ("l4.conv3", 512, 2048, 1), ("l4.down", 1024, 2048, 1), ("aspp.1x1", 2048, 256, 1),
               ("head", 256, 19, 1)]
TABLE_ROWS = [(c, True) for c in POINTWISE_CASES] + [(("bench." + nm, 2, cin, 33, 31, cout, 1, s, 0, 1, False), False)
                                                     for nm, cin, cout, s in BENCH_PAIRS]


def _run_layer(case, math, x, wt, b, probe):
    from diga_amd.model.conv import DigaConv2d
    name, n, cin, h, w, cout, k, stride, pad, dil, bias = case
    m = DigaConv2d(cin, cout, k, stride=stride, padding=pad, dilation=dil, bias=bias)
    with torch.no_grad():
        m.weight.copy_(wt)
        if bias:
            m.bias.copy_(b)
    m = m.to(DEV)
    need_dx = stride == 1 or k == 1
    xd = x.to(DEV).requires_grad_(need_dx)
    with _Mode(math) as log:
        y = m(xd)
        (y * probe.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        log = dict(log)
    return y.detach(), (xd.grad if need_dx else None), m.weight.grad, (m.bias.grad if bias else None), log


def _inputs(case):
    """Same seeded inputs and float64 reference as tests/test_gpu_conv.py::test_conv_fwd_bwd."""
    name, n, cin, h, w, cout, k, stride, pad, dil, bias = case
    g = synth.gen(zlib.crc32(name.encode()) % 10000)
    x = torch.randn((n, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g) if bias else None
    xr, wr = x.double().requires_grad_(), wt.double().requires_grad_()
    br = b.double().requires_grad_() if bias else None
    yr = F.conv2d(xr, wr, br, stride, pad, dil)
    probe = torch.randn(yr.shape, generator=g)
    (yr * probe.double()).sum().backward()
    return x, wt, b, probe, yr.detach(), xr.grad, wr.grad, (br.grad if bias else None)


@pytest.mark.parametrize("case,bounded", TABLE_ROWS, ids=[c[0] for c, _ in TABLE_ROWS])
def test_per_layer_error_against_float64_and_exact_fp32(case, bounded):
    """The acceptance criterion of the arithmetic.  y, dx, dw of one pointwise layer in mode 0 and in mode 2 on the device, each against
    F.conv2d in float64 (error = max |t - t64| / max |t64|), one table row per shape:
      (a) the rows of test_gpu_conv.CASES: mode 2 meets the bounds that test holds the direct fp32 kernels to, unchanged
          (assert_close(.., 1e-5, a * scale), a = 2e-6 / 3e-6 / 3e-6); the bench rows reach K = 2048 and get the ratio only;
      (b) every row and tensor: err2 <= 1.5 * err0, err0 being the exact-fp32 kernels on the same inputs (1.5 = the noise of a max
          statistic, not room for a worse arithmetic);
      (c) forward, backward-data and backward-weight all ran on bf16x6 in mode 2 (path_log) -- no fallback -- and on none in mode 0."""
    name = case[0]
    x, wt, b, probe, yr, dxr, dwr, dbr = _inputs(case)
    y0, dx0, dw0, _, log0 = _run_layer(case, 0, x, wt, b, probe)
    y2, dx2, dw2, db2, log2 = _run_layer(case, 2, x, wt, b, probe)

    def err(t, ref):
        return float((t.cpu().double() - ref).abs().max()) / float(ref.abs().max())

    e0 = (err(y0, yr), err(dx0, dxr), err(dw0, dwr))
    e2 = (err(y2, yr), err(dx2, dxr), err(dw2, dwr))
    print(f"\n[bf16x6 table] {name:22s} K={case[2]:4d} | y f32 {e0[0]:.2e} x6 {e2[0]:.2e} ratio {e2[0] / e0[0]:.2f} | "
          f"dx f32 {e0[1]:.2e} x6 {e2[1]:.2e} ratio {e2[1] / e0[1]:.2f} | dw f32 {e0[2]:.2e} x6 {e2[2]:.2e} ratio {e2[2] / e0[2]:.2f}")
    assert log2 == {("fwd", "bf16x6"): 1, ("dgrad", "bf16x6"): 1, ("wgrad", "bf16x6"): 1}, log2
    assert log0 == {("fwd", "f32"): 1, ("dgrad", "f32"): 1, ("wgrad", "f32"): 1}, log0
    if bounded:
        assert_close(y2, yr, 1e-5, 2e-6 * float(yr.abs().max()), f"{name} forward")
        assert_close(dx2, dxr, 1e-5, 3e-6 * float(dxr.abs().max()), f"{name} grad input")
        assert_close(dw2, dwr, 1e-5, 3e-6 * float(dwr.abs().max()), f"{name} grad weight")
        if dbr is not None:
            assert_close(db2, dbr, 1e-5, 1e-5 * float(dbr.abs().max()), f"{name} grad bias")
    for what, a0, a2 in zip(("y", "dx", "dw"), e0, e2):
        assert a2 <= 1.5 * a0, f"{name} {what}: bf16x6 {a2:.2e} vs exact fp32 {a0:.2e} of scale"


# ------------------------------------------------------------------------------------------------ 6. everything else is mode 0
@pytest.mark.parametrize("case", [c for c in CASES if c[6] != 1], ids=lambda c: c[0])
def test_other_layers_are_bit_identical_to_exact_fp32(case):
    x, wt, b, probe = _inputs(case)[:4]
    y0, dx0, dw0, db0, log0 = _run_layer(case, 0, x, wt, b, probe)
    y2, dx2, dw2, db2, log2 = _run_layer(case, 2, x, wt, b, probe)
    assert log2 == log0 and not any(a == "bf16x6" for _, a in log2), (log0, log2)
    assert torch.equal(y0, y2)
    assert (dx0 is None and dx2 is None) or torch.equal(dx0, dx2)
    assert torch.equal(dw0, dw2)
    assert (db0 is None and db2 is None) or torch.equal(db0, db2)


# ------------------------------------------------------------------------------------------------ 7. epilogues
def _block_state(pfx, inplanes, planes):
    shapes = {f"{pfx}.conv1.weight": ((planes, inplanes, 1, 1), "conv"), f"{pfx}.conv2.weight": ((planes, planes, 3, 3), "conv"),
              f"{pfx}.conv3.weight": ((planes * 4, planes, 1, 1), "conv")}
    for bn, c in (("bn1", planes), ("bn2", planes), ("bn3", planes * 4)):
        shapes.update({f"{pfx}.{bn}.weight": ((c,), "bn_w"), f"{pfx}.{bn}.bias": ((c,), "bn_b"),
                       f"{pfx}.{bn}.running_mean": ((c,), "bn_rm"), f"{pfx}.{bn}.running_var": ((c,), "bn_rv")})
    return {k: detweights.fill(k, shp, kind) for k, (shp, kind) in shapes.items()}


def _make_block(sd, pfx, inplanes, planes, dilation):
    from diga_amd.model import seg_model_noaux as sm
    blk = sm.Bottleneck(inplanes, planes, 1, dilation=dilation, downsample=None)
    own = blk.state_dict()
    for k in own:
        if not k.endswith("num_batches_tracked"):
            own[k] = sd[f"{pfx}.{k}"]
    blk.load_state_dict(own)
    return blk.to(DEV).train()


def test_residual_junction_epilogues_and_forward_statistics(monkeypatch):
    """Three bottlenecks in a row (identity residuals, train-mode BatchNorm, fuse_bwd on: the construction of
    test_gpu_bf16x3_parity.py::test_residual_junction_fused_backward_vs_float64, layer1 widths), in mode 2:
      * y, dx and every weight gradient against the float64 oracle with the device's ReLU patterns pinned, at that test's MODE-0 bound
        2e-5 of scale -- conv1 / conv3 run on bf16x6 with the backward-data epilogue (residual add, mask bits, BatchNorm-backward sums);
      * the forward statistics the bf16x6 epilogue hands bn1 / bn3 of the first block (momentum 1: the running statistics ARE the
        batch statistics the layer finalised) against a float64 two-pass mean / variance of the same conv's own output: no further
        from it than 2 x what mode 0 shows on the same inputs."""
    from diga_amd import _lib
    from diga_amd.model import norm as dn
    planes, inpl, dil, n, h, w = 64, 256, 1, 2, 31, 29
    names = [f"junction{planes}.b{i}" for i in range(3)]
    sds = [_block_state(nm, inpl, planes) for nm in names]
    blocks = [_make_block(sd, nm, inpl, planes, dil) for sd, nm in zip(sds, names)]
    g = synth.gen(planes + 5)
    x = torch.randn((n, inpl, h, w), generator=g).relu_() + 0.1 * torch.randn((n, inpl, h, w), generator=g)
    probe = torch.randn((n, inpl, h, w), generator=g)
    blocks[0].bn1.momentum = blocks[0].bn3.momentum = 1.0
    assert config.active().fuse_bwd and dn.fuse_backward_enabled()
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])

    def run(math):
        for b in blocks:
            for p in b.parameters():
                p.grad = None
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
        seen, hooks = {}, []
        for i, b in enumerate(blocks):
            hooks.append(b.bn1.register_forward_hook(lambda m, a, o, i=i: seen.__setitem__((i, 1), (o.detach() > 0).cpu().double())))
            hooks.append(b.bn2.register_forward_hook(lambda m, a, o, i=i: seen.__setitem__((i, 2), (o.detach() > 0).cpu().double())))
            hooks.append(b.register_forward_hook(lambda m, a, o, i=i: seen.__setitem__((i, 3), (o.detach() > 0).cpu().double())))
        hooks.append(blocks[0].conv1.register_forward_hook(lambda m, a, o: seen.__setitem__("c1", o.detach().cpu().double())))
        hooks.append(blocks[0].conv3.register_forward_hook(lambda m, a, o: seen.__setitem__("c3", o.detach().cpu().double())))
        calls.clear()
        with _Mode(math) as log:
            y = xd
            for b in blocks:
                y = b(y)
            (y * probe.to(DEV)).sum().backward()
            torch.cuda.synchronize()
            log = dict(log)
        for hk in hooks:
            hk.remove()
        stats = {}
        for key, bn in (("c1", blocks[0].bn1), ("c3", blocks[0].bn3)):
            yd = seen[key]
            cnt = yd.numel() // yd.shape[1]
            mean, var = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
            got_mean, got_var = bn.running_mean.double().cpu(), bn.running_var.double().cpu() * (cnt - 1) / cnt
            stats[key] = (float((got_mean - mean).abs().max() / mean.abs().max()), float((got_var - var).abs().max() / var.max()))
        grads = {f"{i}.{k}": p.grad.clone() for i, b in enumerate(blocks) for k, p in b.named_parameters() if p.grad is not None}
        return y.detach().clone(), xd.grad.clone(), grads, seen, stats, log, list(calls)

    _, _, _, _, stats0, log0, _ = run(0)
    y2, dx2, gr2, masks, stats2, log2, calls2 = run(2)
    assert not any(a == "bf16x6" for _, a in log0)
    # conv1 and conv3 of three blocks on bf16x6 in all three passes; conv2 on the exact-fp32 paths
    assert log2[("fwd", "bf16x6")] == 6 and log2[("dgrad", "bf16x6")] == 6 and log2[("wgrad", "bf16x6")] == 6, log2
    assert sum(a != "bf16x6" for (_, a), cnt in log2.items() for _ in range(cnt)) == 9, log2
    # conv3 of every block (3 epilogues) + conv1 of blocks 1 and 2 (junctions) finish a BatchNorm's gradient on the bf16x6 kernel
    assert calls2.count("diga_conv2d_nhwc_bf16x6_epi") == 5, calls2

    sd64 = {}
    for sd in sds:
        sd64.update({k: v.double().requires_grad_(v.dim() == 4) for k, v in sd.items()})
    xr = x.double().requires_grad_()
    yr = xr
    for i, nm in enumerate(names):
        yr = od.bottleneck_fixed_masks(sd64, nm, yr, 1, dil, False, (masks[(i, 1)], masks[(i, 2)], masks[(i, 3)]))
    (yr * probe.double()).sum().backward()

    def rel(a, b):
        return float((a.detach().cpu().double() - b.detach()).abs().max()) / float(b.detach().abs().max())

    errs = {"y": rel(y2, yr), "dx": rel(dx2, xr.grad)}
    for k in gr2:
        i, nm = k.split(".", 1)
        errs[k] = rel(gr2[k], sd64[f"{names[int(i)]}.{nm}"].grad)
    print(f"\n[bf16x6 junction] worst error / scale vs float64: {max(errs.values()):.1e} ({max(errs, key=errs.get)})")
    for k, v in errs.items():
        assert v < 2e-5, f"{k}: {v:.2e} of scale"
    for key in ("c1", "c3"):
        print(f"[bf16x6 statistics] {key}: mean f32 {stats0[key][0]:.2e} x6 {stats2[key][0]:.2e} | var f32 {stats0[key][1]:.2e} x6 {stats2[key][1]:.2e}")
    for key in ("c1", "c3"):
        assert stats2[key][0] <= 2 * stats0[key][0], (key, "mean", stats2[key], stats0[key])
        assert stats2[key][1] <= 2 * stats0[key][1], (key, "var", stats2[key], stats0[key])


# ------------------------------------------------------------------------------------------------ 8. whole model
FWD_TOL_F32 = 8e-5


def _all_three_passes(log):
    return all(log.get((p, "bf16x6"), 0) > 0 for p in ("fwd", "dgrad", "wgrad"))


@pytest.mark.parametrize("arch_name,hw", [("TINY", (96, 128)), ("RESNET101", (64, 96))])
def test_whole_model_gradients_vs_float64_with_pinned_switches(arch_name, hw):
    """The construction of test_gpu_bf16x3_parity.py::test_whole_model_gradients_vs_float64_with_pinned_switches in mode 2, at its MODE-0
    bounds: logits within 8e-5 of scale, every parameter gradient elementwise within 5e-5 (small backbone) / 1e-4 (ResNet-101)."""
    from diga_amd.model import seg_model_noaux as sm
    from diga_amd.model.model_noaux import SegModel
    from diga_amd.model.norm import DigaBatchNorm2d, DigaGroupNorm
    arch_d, arch_o = getattr(sm, arch_name), getattr(od, arch_name)
    sd32 = detweights.state_dict(arch_o)
    m = SegModel(arch=arch_d)
    m.load_state_dict(sd32)
    m = m.to(DEV).train()
    m.final.head[0].p = 0.0
    g = synth.gen(4242)
    x = torch.rand((2, 3) + hw, generator=g) * 2 - 1
    xd = x.to(DEV)
    with _Mode(2) as log:
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
        e_fwd = float((out.detach().cpu().double() - out_r.detach()).abs().max() / out_r.detach().abs().max())
        print(f"\n[bf16x6 model] {arch_name}: logits within {e_fwd:.1e} of scale of the float64 oracle")
        assert e_fwd < FWD_TOL_F32
        ((out * probe.to(DEV)).sum() + (feat * probe_f.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        log = dict(log)
    assert _all_three_passes(log), log
    named = dict(m.named_parameters())
    tol = 1e-4 if arch_name == "RESNET101" else 5e-5
    worst, worst_k = 0.0, None
    for k in trainable:
        ref = sd64[k].grad
        e = float((named[k].grad.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        if e > worst:
            worst, worst_k = e, k
        assert e < tol, (k, e)
    print(f"[bf16x6 model] {arch_name}: all {len(trainable)} parameter gradients within {worst:.1e} of scale (worst: {worst_k}); paths {log}")


def test_forward_backward_train_golden(golden):
    """The construction of test_gpu_model.py::test_forward_backward_train_golden (the reference's capture, weight gradients in line) in
    mode 2 with the bounds of its conv_math == 0 branch."""
    from diga_amd.model import seg_model_noaux as sm
    from diga_amd.model.model_noaux import SegModel
    g = golden("model")
    m = SegModel(arch=sm.RESNET101)
    m.load_state_dict(detweights.state_dict(od.RESNET101))
    m = m.to(DEV).train()
    m.final.head[0].p = 0.0
    with _Mode(2) as log:
        _, _, out, feat = m(g.t("x").to(DEV))
        scale = float(g.t("out_train").abs().max())
        assert float((out.detach().cpu() - g.t("out_train")).abs().max()) < 1e-3 * scale
        assert_close(out, g.t("out_train"), 1e-3, 2e-4, "train logits")
        (out * g.t("probe").to(DEV)).sum().backward()
        torch.cuda.synchronize()
        log = dict(log)
    assert _all_three_passes(log), log
    named = dict(m.named_parameters())
    ref = g.t("g_head")
    assert_close(named["final.head.1.weight"].grad, ref, 5e-3, 1e-3 * float(ref.abs().max()), "head grad")
    for n in ["layer0.0.weight", "layer1.0.conv1.weight", "layer2.3.conv2.weight", "layer3.22.conv3.weight",
              "layer4.0.downsample.0.weight", "final.conv2d_list.3.0.weight", "final.conv2d_list.0.1.weight",
              "final.bottleneck.0.se.0.weight", "final.bottleneck.1.bias"]:
        l1 = g["g_" + n.replace(".", "_")].tolist()[1]
        assert float(named[n].grad.abs().sum()) == pytest.approx(l1, rel=2e-2), n
    sd = m.state_dict()
    assert_close(sd["layer1.0.bn1.running_mean"], g.t("rm_after"), 1e-4, 1e-6, "running mean")
    assert_close(sd["layer4.2.bn3.running_var"], g.t("rv_after"), 1e-3, 1e-6, "running var")


# ------------------------------------------------------------------------------------------------ 9. mode switch hygiene
def test_arithmetic_change_between_forward_and_backward():
    """A bf16x6 forward of a layer whose weight gradient is wanted saves the triplet of its input; its bytes are only readable by
    the bf16x6 weight-gradient kernel, so changing the arithmetic before backward() raises the existing error.  A layer that saved
    nothing mode-specific (no weight gradient wanted) just runs its backward in the new arithmetic, correctly."""
    from diga_amd import _lib
    from diga_amd.model.conv import DigaConv2d
    g = synth.gen(77)
    m = DigaConv2d(64, 128, 1, bias=False).to(DEV)
    x = torch.randn((2, 64, 9, 11), generator=g).to(DEV).requires_grad_()
    prev = _lib.get_conv_math()
    try:
        _lib.set_conv_math(2)
        y = m(x)
        _lib.set_conv_math(0)
        with pytest.raises(RuntimeError, match="arithmetic .* changed between forward and backward"):
            y.sum().backward()
        m.weight.requires_grad_(False)
        _lib.set_conv_math(2)
        y = m(x)
        _lib.set_conv_math(0)
        x.grad = None
        y.sum().backward()
        want = m.weight.detach().double().sum(0).reshape(1, 64, 1, 1).expand(2, 64, 9, 11)
        assert_close(x.grad, want, 1e-5, 3e-6 * float(want.abs().max()), "grad input after the mode change")
    finally:
        _lib.set_conv_math(prev)
        _lib.join_side()
