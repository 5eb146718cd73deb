"""OCR head on the GPU: the four kernels of csrc/ocr.hip against float64, their determinism, and the module
(diga_amd/model/networks/ocrnet_module.py) against the capture of the reference class and against the float64 restatement.

Kernel-level bounds (tests 1-3): the yardstick is the restatement (tests/ocr_cases.py) run in fp32 on the CPU, measured against float64
in the test itself; a kernel's max error / scale may be 3 x the yardstick's on the same inputs (different summation trees over
thousands of pixels), with a floor of 2^-20 of scale.  Every operand is a slice of a NaN-filled allocation with guard rows in front
and behind; outputs are checked for NaNs inside and for writes outside.

Head-level bounds (test 5): fp32 convolutions: 4 x the capture's err32_* (the reference class in fp32 on the CPU against itself in
float64).  bf16x3 convolutions: the yardstick is the same head with the two fused operations replaced by torch compositions on the
GPU; with the kernels in, the error against the capture may be 1.5 x that (gradients: assert_mostly_close, 1e-4 of the elements).

Measured on an MI355X (max error / scale against float64; the printed lines of a run with -s):
  kernels, region gather   region 0.8e-7 .. 1.2e-7 (float64 accumulation), dx 1.0e-7 .. 2.1e-7, ds 0.6e-7 .. 1.3e-7 (logits +-90: 4.1e-7);
                           fp32 restatement on the same inputs 1.1e-7 .. 9.7e-7; one pixel: region = x exactly, ds 6e-8 of max |g|
  kernels, attention       out 2.5e-7 .. 4.7e-7, attn 2.2e-7 .. 4.0e-7, dq 1.4e-7 .. 3.2e-7, d_key 1.8e-7 .. 2.6e-7, d_val 1.8e-7 .. 2.1e-7
                           (logits of magnitude 90: 1.4e-6 / 1.2e-6 / 8.7e-7 / 1.2e-6 / 4.6e-7); restatement 2.5e-7 .. 8.6e-7 (3.7e-6)
  head vs capture, f32     outputs 1.9e-7 (soft) .. 4.0e-6 (seg), gradients 1.4e-8 .. 6.6e-6, running statistics 5e-8 .. 2.3e-7, eval pass
                           2.0e-7 .. 4.9e-7, against bounds of 4 x the capture's own fp32 error
  head vs capture, bf16x3  outputs 4.8e-6 .. 6.6e-5, gradients up to 2.2e-4; 0.7 .. 1.2 x the head on torch compositions for every tensor.
                           g_soft_object_regions_3_bias (both heads at fp32 rounding level): L2 1.6e-7, composed 3.2e-7.  With an fp32
                           region sum this tensor was at 8.0e-7: see the note on float64 in csrc/ocr.hip
  widest instantiations    K = 32 with 1024 channels: region 0.4e-7, dx 1.8e-7, ds 1.6e-7; out 4.0e-7, attn 2.5e-7, dq 4.1e-7, d_key 3.8e-7
  real widths as shipped   default Winograd tiles: max error 0.77 .. 1.18 x the head on torch compositions (bound 1.5 x), but for the auxiliary
                           classifier's bias gradient, 1.86 x in one class of 19 -- gradients are held elementwise up to 8 elements and in L2:
                           8.6e-7 against 7.8e-7 (1.34e-6 while the region sum was scaled by the fp32 1 / sum)
  real widths (F(2x2))     0.9 .. 2.2 x the fp32 restatement's error (bound 4 x), worst g_augmented_rep_0_weight 1.5e-5
"""
import ctypes as C

import pytest
import torch

import ocr_cases as oc
from conftest import WINO_TOL, assert_mostly_close, winograd_tile

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8                 # guard rows in front of and behind every operand
FLOOR = 2.0 ** -20


def _lib():
    from diga_amd import _lib
    return _lib


def put(t, ld=0):
    """CPU [N, P, C] -> the same values as a [N, P, C] view of pitch `ld` inside a NaN-filled, guarded GPU allocation."""
    n, p, c = t.shape
    ld = ld or c
    buf = torch.full(((n * p + 2 * GUARD) * ld,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[GUARD * ld:(GUARD + n * p) * ld].view(n, p, ld)[..., :c]
    view.copy_(t)
    view._guard, view._ld = buf, ld
    return view


def fresh(n, p, c, ld=0):
    return put(torch.full((n, p, c), float("nan")), ld)


def take(view, what):
    """The payload of an output view on the CPU, after checking that it holds no NaN and that nothing around it was written."""
    n, p, c = view.shape
    buf, ld = view._guard, view._ld
    assert bool(torch.isnan(buf[:GUARD * ld]).all()) and bool(torch.isnan(buf[(GUARD + n * p) * ld:]).all()), f"{what}: guard rows written"
    rows = buf[GUARD * ld:(GUARD + n * p) * ld].view(n * p, ld)
    assert bool(torch.isnan(rows[:, c:]).all()), f"{what}: written past the row"
    assert not bool(torch.isnan(rows[:, :c]).any()), f"{what}: NaN in the result (a read outside the operands, or an element never written)"
    return rows[:, :c].reshape(n, p, c).cpu()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def workspace(n, p, k, c):
    lib = _lib()
    nbytes = lib.lib.diga_ocr_workspace_bytes(n, p, k, c)
    assert nbytes > 0
    return torch.full((nbytes // 4 + 4 * GUARD,), float("nan"), dtype=torch.float32, device=DEV), nbytes


def run_region(x, s, d_region, ld_x=0, ld_s=0):
    """diga_ocr_region_fwd + _bwd on guarded operands: (region, stat, dx, ds) on the CPU."""
    lib = _lib()
    n, p, c = x.shape
    k = s.shape[2]
    xg, sg, dg = put(x, ld_x), put(s, ld_s), put(d_region)
    region, stat = fresh(n, k, c), fresh(1, 1, n * k * (c + 2))      # stat: [N][K][C] low-order part of region, then [N][K][2]
    ws, nbytes = workspace(n, p, k, c)
    st = lib.stream()
    lib.call("diga_ocr_region_fwd", ptr(xg), ld_x or c, ptr(sg), ld_s or k, ptr(region), ptr(stat), n, p, k, c, ptr(ws), nbytes, st)
    dx, ds = fresh(n, p, c, ld_x), fresh(n, p, k, ld_s)
    lib.call("diga_ocr_region_bwd", ptr(xg), ld_x or c, ptr(sg), ld_s or k, ptr(stat), ptr(region), ptr(dg), ptr(dx), ld_x or c, ptr(ds),
             ld_s or k, n, p, k, c, st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nbytes // 4:]).all()), "region_fwd wrote past its workspace"
    stat = take(stat, "stat").reshape(-1)
    lo, stat = stat[:n * k * c].reshape(n, k, c), stat[n * k * c:].reshape(n, k, 2)
    # region + lo is the float64 sum to ~2^-48: the pair the backward's dot is made of
    assert float(lo.abs().max()) <= 2.0 ** -24 * float(take(region, "region").abs().max())
    return take(region, "region"), stat, take(dx, "dx"), take(ds, "ds")


def run_attend(q, key, val, d_out, scale, ld_q=0, ld_out=0, keep_attn=True):
    """diga_ocr_attend_fwd + _bwd on guarded operands: (out, attn, dq, d_key, d_val) on the CPU."""
    lib = _lib()
    n, p, d = q.shape
    k, dv = key.shape[1], val.shape[2]
    qg, kg, vg, dog = put(q, ld_q), put(key), put(val), put(d_out, ld_out)
    out = fresh(n, p, dv, ld_out)
    attn = fresh(n, p, k) if keep_attn else None
    st = lib.stream()
    lib.call("diga_ocr_attend_fwd", ptr(qg), ld_q or d, ptr(kg), ptr(vg), ptr(out), ld_out or dv, ptr(attn), n, p, k, d, dv, float(scale), st)
    if not keep_attn:
        torch.cuda.synchronize()
        return take(out, "out"), None, None, None, None
    dq, d_key, d_val = fresh(n, p, d, ld_q), fresh(n, k, d), fresh(n, k, dv)
    ws, nbytes = workspace(n, p, k, max(d, dv))
    lib.call("diga_ocr_attend_bwd", ptr(qg), ld_q or d, ptr(kg), ptr(vg), ptr(attn), ptr(dog), ld_out or dv, ptr(dq), ld_q or d, ptr(d_key),
             ptr(d_val), n, p, k, d, dv, float(scale), ptr(ws), nbytes, st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nbytes // 4:]).all()), "attend_bwd wrote past its workspace"
    return take(out, "out"), take(attn, "attn"), take(dq, "dq"), take(d_key, "d_key"), take(d_val, "d_val")


def held(got, ref64, ref32, what, natural=None):
    """max error / scale of `got` against float64, held to 3 x the fp32 restatement's on the same inputs (floor 2^-20).  `natural`:
    the scale of the terms a tensor is a difference of, for one that vanishes identically (ds of a single pixel: w (g - dot) = 0)."""
    scale = float(ref64.abs().max())
    if natural is not None and scale <= 1e-9 * natural:
        scale = natural
    err = float((got.double() - ref64).abs().max()) / scale
    yard = float((ref32.double() - ref64).abs().max()) / scale
    print(f"  {what:28s} kernel {err:.2e}  fp32 restatement {yard:.2e}  of scale {scale:.3g}")
    assert bool(torch.isfinite(got).all()), what
    assert err <= max(3.0 * yard, FLOOR), f"{what}: {err:.3e} of scale, fp32 restatement {yard:.3e}"


_REF = {}


def region_refs(name, magnitude=1.0):
    """(inputs, float64 reference, fp32 yardstick) of a region case: computed once, shared, never written."""
    key = ("region", name, magnitude)
    if key not in _REF:
        inp = oc.region_inputs(name, magnitude=magnitude)
        _REF[key] = (inp, oc.region_reference(*inp, torch.float64), oc.region_reference(*inp, torch.float32))
    return _REF[key]


def attend_refs(name):
    key = ("attend", name)
    if key not in _REF:
        inp = oc.attend_inputs(name)
        _REF[key] = (inp, oc.attend_reference(*inp, torch.float64), oc.attend_reference(*inp, torch.float32))
    return _REF[key]


# ------------------------------------------------------------------------------------------------ 1, 2: region gather
@pytest.mark.parametrize("name", list(oc.REGION_CASES))
def test_region_gather_against_float64(name):
    n, p, k, c, ld_x, ld_s = oc.REGION_CASES[name]
    (x, s, dr), r64, r32 = region_refs(name)
    region, stat, dx, ds = run_region(x, s, dr, ld_x, ld_s)
    g_scale = float(torch.matmul(dr.double(), x.double().transpose(1, 2)).abs().max())         # max |<d_region[k], x[p]>|
    for got, a, b, what in zip((region, dx, ds), r64, r32, ("region", "dx", "ds")):
        held(got, a, b, f"{name} {what}", natural=g_scale if what == "ds" else None)
    m64 = s.double().max(dim=1).values
    assert torch.equal(stat[..., 0].double(), m64), "stat[..., 0] is the maximum of the class map"
    z64 = torch.exp(s.double() - m64[:, None, :]).sum(dim=1)
    assert float(((stat[..., 1].double() * z64) - 1).abs().max()) <= 3 * max(p, 16) * 2.0 ** -24
    if p == 1:
        assert torch.equal(region, x.expand(n, k, c)), "one pixel: every region is that pixel"


def test_region_gather_with_logits_of_magnitude_90():
    (x, s, dr), r64, r32 = region_refs("small", magnitude=90.0)
    assert float(s.abs().max()) == 90.0 and float(s.max() - s.min()) > 170          # exp(s) overflows fp32 without the maximum subtraction
    region, stat, dx, ds = run_region(x, s, dr)
    for got, a, b, what in zip((region, dx, ds), r64, r32, ("region", "dx", "ds")):
        held(got, a, b, f"logits +-90 {what}")


# ------------------------------------------------------------------------------------------------ 3: object attention
@pytest.mark.parametrize("name", list(oc.ATTEND_CASES))
def test_object_attention_against_float64(name):
    n, p, k, d, dv, ld_q, ld_out, mag = oc.ATTEND_CASES[name]
    (q, key, val, do, scale), r64, r32 = attend_refs(name)
    if mag:
        assert abs(float((scale * q.double() @ key.double().transpose(1, 2)).abs().max()) - mag) < 1e-9
    got = run_attend(q, key, val, do, scale, ld_q, ld_out)
    for g, a, b, what in zip(got, r64, r32, ("out", "attn", "dq", "d_key", "d_val")):
        held(g, a, b, f"{name} {what}")
    rowsum = got[1].double().sum(dim=2)
    assert float((rowsum - 1).abs().max()) <= 4 * 2.0 ** -23, "attn rows sum to 1 within 4 ulp"
    out_only = run_attend(q, key, val, do, scale, ld_q, ld_out, keep_attn=False)[0]
    assert torch.equal(out_only, got[0]), "attn = NULL changes the bits of out"


# ------------------------------------------------------------------------------------------------ 4: determinism
@pytest.mark.parametrize("name", ["prime_p", "wide"])
def test_kernels_are_deterministic(name):
    (x, s, dr), _, _ = region_refs(name)
    a, b = run_region(x, s, dr), run_region(x, s, dr)
    for u, v, what in zip(a, b, ("region", "stat", "dx", "ds")):
        assert torch.equal(u, v), f"region {what} differs between two runs"
    (q, key, val, do, scale), _, _ = attend_refs(name)
    a, b = run_attend(q, key, val, do, scale), run_attend(q, key, val, do, scale)
    for u, v, what in zip(a, b, ("out", "attn", "dq", "d_key", "d_val")):
        assert torch.equal(u, v), f"attention {what} differs between two runs"


def test_autograd_functions_match_the_entry_points():
    """ocr_region_gather / ocr_object_attention (the module-level callables) give the bits of the direct calls, on a pitched x."""
    from diga_amd.model.networks import ocrnet_module as om
    (x, s, dr), _, _ = region_refs("pitched")
    xg = put(x, 96).detach().requires_grad_()                   # a leaf over the pitched rows
    sg = s.to(DEV).requires_grad_()
    r = om.ocr_region_gather(xg, sg)
    r.backward(dr.to(DEV))
    want = run_region(x, s, dr, 96, 24)
    assert torch.equal(r.detach().cpu(), want[0]) and torch.equal(xg.grad.cpu(), want[2]) and torch.equal(sg.grad.cpu(), want[3])
    (q, key, val, do, scale), _, _ = attend_refs("small")
    qg, kg, vg = (t.to(DEV).requires_grad_() for t in (q, key, val))
    o = om.ocr_object_attention(qg, kg, vg, scale)
    o.backward(do.to(DEV))
    want = run_attend(q, key, val, do, scale)
    for g, w in zip((o.detach(), qg.grad, kg.grad, vg.grad), (want[0], want[2], want[3], want[4])):
        assert torch.equal(g.cpu(), w)


# ------------------------------------------------------------------------------------------------ 5: the head against the capture
def _head(sd, cfg=oc.SMALL_CFG):
    from diga_amd.model.networks.ocrnet_module import OCRNet
    head = OCRNet(cfg)
    head.load_state_dict(sd)
    head.augmented_rep[3].p = 0.0                    # Dropout2d off, as in the capture
    return head.to(DEV)


def _head_step(head, x, probes):
    """One train-mode step of the module: the tensors of the capture by name."""
    head.train()
    head.zero_grad(set_to_none=True)
    xin = x.to(DEV).requires_grad_()
    soft, seg, aug = head(xin)
    ((soft * probes[0].to(DEV)).sum() + (seg * probes[1].to(DEV)).sum()).backward()
    res = {"soft": soft, "seg": seg, "aug": aug, "dx": xin.grad}
    for k, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        res["g_" + k.replace(".", "_")] = p.grad
    nbt = set()
    for k, b in head.named_buffers():
        if k.endswith("num_batches_tracked"):
            nbt.add(int(b))
        else:
            res["b_" + k.replace(".", "_")] = b
    return {k: v.detach().double().cpu() for k, v in res.items()}, nbt


def _head_eval(head, x):
    head.eval()
    with torch.no_grad():
        soft, seg, aug = head(x.to(DEV))
    return {"soft_eval": soft.double().cpu(), "seg_eval": seg.double().cpu(), "aug_eval": aug.double().cpu()}


def _compose(monkeypatch):
    from diga_amd.model.networks import ocrnet_module as om
    monkeypatch.setattr(om, "ocr_region_gather", oc.region_gather)
    monkeypatch.setattr(om, "ocr_object_attention", oc.object_attention)


def _capture_run(z, composed=False):
    sd = oc.fixture_state(z)
    with pytest.MonkeyPatch.context() as mp:
        if composed:
            _compose(mp)
        head = _head(sd)
        got, nbt = _head_step(head, z.t("x").float(), [z.t("probe_soft").float(), z.t("probe_seg").float()])
        got.update(_head_eval(head, z.t("x_eval").float()))
    return got, nbt


def test_head_against_the_capture_of_the_reference_class(golden, conv_math):
    z = golden("ocr_head")
    got, nbt = _capture_run(z)
    assert nbt == {int(z["nbt"])}
    names = [k for k in z if k.startswith(("g_", "b_")) or k in ("soft", "seg", "aug", "dx", "soft_eval", "seg_eval", "aug_eval")]
    assert len(names) == 58
    composed = _capture_run(z, composed=True)[0] if conv_math == 1 else None
    failures = []
    for k in names:
        want, scale = z.t(k), float(z["scale_" + k])
        assert got[k].shape == want.shape, k
        err = float((got[k] - want).abs().max()) / scale
        e32 = float(z["err32_" + k])
        if conv_math == 0:
            bound = 4.0 * e32
            print(f"  f32    {k:52s} {err:.2e}  (capture's fp32 {e32:.2e}, bound {bound:.2e})")
            if not err <= bound:
                failures.append(f"{k}: {err:.3e} of scale > {bound:.3e}")
            continue
        yard = float((composed[k] - want).abs().max()) / scale
        l2 = float((got[k] - want).norm() / want.norm().clamp_min(1e-300))
        l2_yard = float((composed[k] - want).norm() / want.norm().clamp_min(1e-300))
        print(f"  bf16x3 {k:52s} {err:.2e}  (composed head {yard:.2e})  L2 {l2:.2e} (composed {l2_yard:.2e})")
        try:
            if k.startswith("g_") or k == "dx":
                assert_mostly_close(got[k], want, 0.0, 1.5 * yard * scale, 1e-4, max(1.5 * l2_yard, 1e-300), what=k)
            else:
                assert err <= 1.5 * yard, f"{k}: {err:.3e} of scale, composed head {yard:.3e}"
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 6: the real widths
def test_head_at_the_real_widths_against_float64():
    """720 / 512 / 256 channels, 19 classes, N = 1, 9 x 7: the 720-channel 3x3 convolution and D = 256 in the attention kernels.
    Runs with the Winograd tiles capped at F(2x2,3x3) (set_conv_math(0, exact=True): the direct kernels' error level).  With the
    default 4x4 tiles the 3x3 layer's forward error (4e-5 of scale) flips ReLUs behind it and the gradients of a
    net this small move by 1e-3 .. 1e-1 of scale against float64; the head as shipped, default tiles, is held to the same head on
    torch compositions by the next test.  Bound per tensor: 4 x the fp32 restatement's own error against float64
    (as for the capture), not below the bound the F(2x2) layer is held to everywhere else in the suite (conftest.WINO_TOL[2]);
    gradients may have 1e-4 of their elements (8 for small tensors) beyond it, as in assert_mostly_close."""
    from diga_amd import config
    lib = _lib()
    prev, prev_tile = lib.get_conv_math(), config.active().winograd_max_tile
    lib.set_conv_math(0, exact=True)
    try:
        _real_widths()
    finally:
        lib.set_conv_math(prev)
        config.active().winograd_max_tile = prev_tile         # whatever cap the session ran with


def _real_case():
    """Seeded state, input, probes and the float64 step of the head at the real widths: computed once, shared, never written."""
    if "real" not in _REF:
        sd = oc.random_state(oc.REAL_CFG, 77)
        g = torch.Generator().manual_seed(78)
        x = torch.randn((1, 720, 9, 7), generator=g)
        probes = [torch.randn((1, 19, 9, 7), generator=g) for _ in range(2)]
        _REF["real"] = (sd, x, probes, oc.head_step(sd, x, probes, 256, torch.float64))
    return _REF["real"]


def test_head_at_the_real_widths_as_shipped_adds_nothing_to_the_composed_head(monkeypatch):
    """The same head and step in the configuration a user gets: fp32 convolutions with the default Winograd tiles (the 720-channel 3x3
    layer on 4x4 tiles here).  Its error against float64 is the convolutions' (ReLU flips behind a 4e-5 forward error), so the
    yardstick is the issue's for coarser convolutions: the same head with the two fused operations replaced by torch compositions
    on the GPU.  With the kernels in, the error may be 1.5 x that; gradients through assert_mostly_close (1e-4 of the elements, 8
    for small tensors; L2 1.5 x the composed head's)."""
    sd, x, probes, r64 = _real_case()
    assert winograd_tile(1, 720, 9, 7, 512, 3, 1, 1, 1) > 2
    got, _ = _head_step(_head(sd, oc.REAL_CFG), x, probes)
    _compose(monkeypatch)
    comp, _ = _head_step(_head(sd, oc.REAL_CFG), x, probes)
    failures = []
    for k, want in r64.items():
        scale = float(want.abs().max())
        err, yard = float((got[k] - want).abs().max()) / scale, float((comp[k] - want).abs().max()) / scale
        l2 = float((got[k] - want).norm() / want.norm().clamp_min(1e-300))
        l2_yard = float((comp[k] - want).norm() / want.norm().clamp_min(1e-300))
        print(f"  default tiles {k:52s} {err:.2e}  (composed head {yard:.2e})  L2 {l2:.2e} (composed {l2_yard:.2e})")
        try:
            if k.startswith("g_") or k == "dx":
                assert_mostly_close(got[k], want, 0.0, 1.5 * yard * scale, 1e-4, max(1.5 * l2_yard, 1e-300), what=k)
            else:
                assert err <= 1.5 * yard, f"{k}: {err:.3e} of scale, composed head {yard:.3e}"
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def _real_widths():
    cfg = oc.REAL_CFG
    sd, x, probes, r64 = _real_case()
    r32 = oc.head_step(sd, x, probes, 256, torch.float32)
    got, _ = _head_step(_head(sd, cfg), x, probes)
    tile = winograd_tile(1, 720, 9, 7, 512, 3, 1, 1, 1)
    failures = []
    for k, want in r64.items():
        scale = float(want.abs().max())
        if k in ("g_pixel_representations_0_bias", "g_soft_object_regions_0_bias"):
            scale = float(r64[k.replace("_0_bias", "_1_bias")].abs().max())         # a vanishing gradient: see the capture
        err = float((got[k] - want).abs().max()) / scale
        yard = float((r32[k].double() - want).abs().max()) / scale
        bound = max(4.0 * yard, WINO_TOL[tile][1 if k.startswith("g_") else 0])
        print(f"  {k:52s} {err:.2e}  (fp32 restatement {yard:.2e}, bound {bound:.2e}, tile {tile})")
        if k.startswith("g_") or k == "dx":
            bad = float(((got[k] - want).abs() > bound * scale).double().mean())
            if bad > max(1e-4, 8.0 / want.numel()):
                failures.append(f"{k}: {bad:.2e} of the elements beyond {bound:.2e} of scale (worst {err:.2e})")
        elif not err <= bound:
            failures.append(f"{k}: {err:.3e} of scale > {bound:.3e}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 7: wiring
def test_wiring_into_the_two_headed_loss(golden, monkeypatch):
    from diga_amd.util.loss import upsample_ce_distill_aux
    lib = _lib()
    z = golden("ocr_head")
    sd = oc.fixture_state(z)
    student, teacher = _head(sd).train(), _head(sd).train()
    x = z.t("x").float().to(DEV)                                  # 2 B maps: B labelled + B unlabelled
    labels = torch.randint(0, 19, (1, 26, 22), generator=torch.Generator().manual_seed(5)).to(DEV)
    labels[0, :3] = 255
    attn_args = []
    real_call = lib.call

    def spy(name, *args):
        if name == "diga_ocr_attend_fwd":
            attn_args.append(args[6].value)
        return real_call(name, *args)

    monkeypatch.setattr(lib, "call", spy)
    torch.cuda.synchronize()
    from diga_amd.model.networks import ocrnet_module as om
    assert om.FUSED_ATTENTION_NO_GRAD is False               # the documented rule: the no_grad attention is the torch composition
    with torch.no_grad():
        t_aux, t_main, t_feat = teacher(x)
        assert attn_args == [], "the no_grad pass ran the attention kernel"
        monkeypatch.setattr(om, "FUSED_ATTENTION_NO_GRAD", True)
        k_main = teacher(x)[1]
        monkeypatch.setattr(om, "FUSED_ATTENTION_NO_GRAD", False)
    assert attn_args == [None], "the no_grad pass on the kernel asked for the attention map"
    assert t_main.grad_fn is None and t_feat.grad_fn is None and k_main.grad_fn is None       # nothing saved
    assert float((k_main - t_main).abs().max()) <= 1e-4 * float(t_main.abs().max())             # the two forms of the rule agree
    s_aux, s_main, _ = student(x)
    assert len(attn_args) == 2 and attn_args[1] is not None
    total, ce, distil = upsample_ce_distill_aux(s_main, s_aux, t_main, t_aux, labels)
    total.backward()
    assert bool(torch.isfinite(total)) and float(ce) > 0
    for k, p in student.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if not k.endswith(".0.bias") or k.startswith("segmentation_classes"):
            assert float(p.grad.abs().max()) > 0, k
    assert all(p.grad is None for p in teacher.parameters())
    # the relation on its own, as the reference's module returns it: [N, P, K], rows summing to one; from the kernel when nothing is
    # differentiated, a differentiable composition otherwise
    with torch.no_grad():
        pix = student.pixel_representations[1](student.pixel_representations[0](x), relu=True)
        obj = student.obj_region_representations(pix, s_aux)
        rel = student.pixel_region_relations(pix, obj)
    assert len(attn_args) == 3 and attn_args[2] is not None
    assert tuple(rel.shape) == (2, 13 * 11, 19) and float((rel.double().sum(2) - 1).abs().max()) <= 4 * 2.0 ** -23
    student.zero_grad(set_to_none=True)
    rel_g = student.pixel_region_relations(pix, obj)
    assert len(attn_args) == 3 and rel_g.requires_grad
    assert float((rel_g - rel).abs().max()) <= 1e-5
    (rel_g * torch.randn(rel_g.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))).sum().backward()
    for k, p in student.pixel_region_relations.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
