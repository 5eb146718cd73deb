"""DAFormer decode head on the GPU: the depthwise 3x3 entry points (csrc/dwconv.hip) and the resize-into-a-slice kernels
(csrc/pyramid.hip) against float64, the module (diga_amd/model/networks/daformer_head.py) against the capture of the reference class,
and the MiT student with head="daformer".

Bounds.  Depthwise passes: 1e-5 of the tensor's scale on every element, the project's bound for its direct fp32 kernels.  Resize: the
tolerances tests/test_gpu_segformer_head.py applies to the pyramid kernels.  Head against the capture, fp32 convolutions: 4 x the
fixture's err32_* for every stored quantity (the bottleneck of the capture's widths runs on the direct kernel, winograd_tile == 0, so
no tile cap is involved); bf16x3 convolutions: 1.5 x the same head on torch compositions (F.conv2d(groups=C), F.interpolate + cat).
Student (1024 -> 256 bottleneck: Winograd F(4x4) by default): against the float64 restatement with the tiles capped at F(2x2), every
element within 4 x the fp32 restatement's own error and not below conftest.WINO_TOL[2], the float64 reference taking the ReLU decisions
of the run it is compared with (test_student_step_against_the_restatement); as shipped: 1.5 x the student on torch compositions.

Measured on an MI355X (max error / scale against float64; the printed lines of a run with -s):
  depthwise entry points   y 0 .. 1.3e-7, dx 0 .. 1.2e-7, dw9 0.4e-7 .. 1.6e-7 on the six shapes (centre tap only: y and dx exact)
  head vs capture, f32     3.9e-11 .. 1.9e-6 on the 110 stored quantities against bounds of 1.5e-7 .. 4.2e-6; nearest to its bound:
                           g_embed_layers_0_proj_bias_sample, 1.87e-6 of 2.97e-6
  head vs capture, bf16x3  logits 7.9e-6, gradients up to 1.6e-2 (ReLU flips); 0.84 .. 1.27 x the head on torch compositions
  feat_raw (return_raw)    1.9e-7 of the float64 restatement
  student, F(2x2) tiles    logits 1.35e-6 (fp32 restatement 1.51e-6); against the plain float64 run one depthwise channel with a ReLU
                           site decided the other way: the 9 taps of its depthwise weight, its BatchNorm pair and one row of
                           embed_layers.2's matrix at 1.4e-2 of scale -- hence the shared decisions; under them every tensor at 1.1e-7 ..
                           1.6e-6 (fp32 restatement 2.0e-7 .. 1.6e-6); 3 student sites and 1 restatement site of 8.4 M differ from
                           float64, the largest pre-activation among them 7.8e-8 of scale
  student as shipped       0.79 .. 1.40 x the student on torch compositions (g_conv_seg_weight nearest to the 1.5 x bound)
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import daformer_cases as dc
from conftest import WINO_TOL, assert_close, assert_mostly_close, winograd_tile

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0e37
_REF = {}


@pytest.fixture(autouse=True)
def _leave_the_global_generators_alone():
    """Module constructors and torch.manual_seed draw from / reset torch's global generators, and tests elsewhere in the suite
    initialise layers from them (test_conv_fullsize_linearity_and_adjoint's adjoint identity is a cancelling sum whose relative error
    depends on those weights): every test of this file hands the CPU and device generator states back as it found them."""
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        yield


def _lib():
    from diga_amd import _lib
    return _lib


def ptr(t):
    return C.c_void_p(t.data_ptr())


def put(t, ld=0, off=0):
    """CPU NCHW tensor -> ([rows, ld] GPU buffer, its [rows, C] operand window at column `off`); everything around the window is NaN."""
    n, c, h, w = t.shape
    buf = torch.full((n * h * w, ld or c), float("nan"), dtype=torch.float32, device=DEV)
    win = buf[:, off:off + c]
    win.copy_(t.permute(0, 2, 3, 1).reshape(-1, c))
    return buf, win


def fresh(rows, c, ld=0, off=0):
    """Output window pre-filled with NaN inside a buffer whose other columns hold a sentinel."""
    buf = torch.full((rows, ld or c), SENTINEL, dtype=torch.float32, device=DEV)
    buf[:, off:off + c] = float("nan")
    return buf, buf[:, off:off + c]


def take(buf, win, off, what):
    """The window on the CPU after checking: no NaN inside, the sentinel's bits everywhere else."""
    c = win.shape[1]
    bits = buf.view(torch.int32)
    want = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    assert bool((bits[:, :off] == want).all()) and bool((bits[:, off + c:] == want).all()), f"{what}: pad columns written"
    assert not bool(torch.isnan(win).any()), f"{what}: NaN in the result (a read outside the operand, or an element never written)"
    return win.cpu()


def nchw(rows, n, h, w):
    return rows.reshape(n, h, w, -1).permute(0, 3, 1, 2)


def dw_refs(name):
    """(operands, float64 y / dx / dw9 of torch): computed once, shared, never written."""
    if name not in _REF:
        n, h, w_, c, d = dc.DW_CASES[name][:5]
        x, w, dy = dc.dw_operands(name)
        xd, wd, dyd = x.double(), w.double(), dy.double()
        _REF[name] = ((x, w, dy), F.conv2d(xd, wd, None, 1, d, d, c), torch.nn.grad.conv2d_input(xd.shape, wd, dyd, 1, d, d, c),
                      dc.tap_major(torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, 1, d, d, c)))
    return _REF[name]


def held(got, ref, what, bound=1e-5):
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max()) / scale
    print(f"  {what:36s} {err:.2e} of scale {scale:.3g}")
    assert got.shape == ref.shape and err <= bound, f"{what}: {err:.3e} of scale"
    return err


# ------------------------------------------------------------------------------------------------ 1: depthwise entry points
@pytest.mark.parametrize("name", list(dc.DW_CASES))
def test_depthwise_entry_points_against_float64(name):
    lib = _lib()
    n, h, w_, c, d, ld_in, ld_out, off = dc.DW_CASES[name]
    (x, w, dy), y64, dx64, dw64 = dw_refs(name)
    rows = n * h * w_
    w9 = dc.tap_major(w).to(DEV)
    st = lib.stream()
    _, xg = put(x, ld_in, off)
    ybuf, yg = fresh(rows, c, ld_out, off)
    lib.call("diga_dwconv3x3_f32", ptr(xg), ld_in or c, ptr(w9), ptr(yg), ld_out or c, n, h, w_, c, d, 0, st)
    y = nchw(take(ybuf, yg, off, "y"), n, h, w_)
    held(y, y64, f"{name} y")
    # backward-data: the same kernel on dy with the taps reversed
    _, gg = put(dy, ld_in, off)
    dxbuf, dxg = fresh(rows, c, ld_out, off)
    lib.call("diga_dwconv3x3_f32", ptr(gg), ld_in or c, ptr(w9), ptr(dxg), ld_out or c, n, h, w_, c, d, 1, st)
    held(nchw(take(dxbuf, dxg, off, "dx"), n, h, w_), dx64, f"{name} dx")
    # weight gradient, twice: bit-equal
    nbytes = lib.lib.diga_dwconv3x3_wgrad_workspace_bytes(n, h, w_, c)
    assert nbytes == n * ((h + 3) // 4) * 9 * c * 4
    _, gp = put(dy, ld_out, off)              # (dy on the other pitch)
    outs = []
    for _ in range(2):
        ws = torch.full((nbytes // 4 + 64,), float("nan"), dtype=torch.float32, device=DEV)
        dw9 = torch.full((9, c), float("nan"), dtype=torch.float32, device=DEV)
        lib.call("diga_dwconv3x3_f32_wgrad", ptr(gp), ld_out or c, ptr(xg), ld_in or c, ptr(dw9), ptr(ws), nbytes, n, h, w_, c, d, st)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws[nbytes // 4:]).all()), "the weight gradient wrote past its workspace"
        assert not bool(torch.isnan(dw9).any())
        outs.append(dw9.cpu())
    assert torch.equal(outs[0], outs[1]), "the weight gradient differs between two runs"
    held(outs[0], dw64, f"{name} dw9")
    if name == "centre_only":
        assert torch.equal(y, w[:, 0, 1, 1][None, :, None, None] * x), "only the centre tap is in range: y = w_centre * x in fp32 bits"


def test_depthwise_autograd_function_matches_the_entry_points():
    """depthwise_conv3x3 on a channel slice of a wider NHWC buffer (the way the head calls it): the bits of the direct calls, and the
    arithmetic is logged as exact fp32 under every conv_math."""
    from diga_amd.model import conv as dconv
    from diga_amd.model.networks import daformer_head as dh
    lib = _lib()
    n, h, w_, c, d = dc.DW_CASES["pitched"][:5]
    (x, w, dy), _, _, _ = dw_refs("pitched")
    _, xg = put(x, 48, 0)
    xin = xg.view(n, h, w_, c).permute(0, 3, 1, 2).detach().requires_grad_()
    wg = w.to(DEV).requires_grad_()
    prev, dconv.path_log = dconv.path_log, {}
    prev_math = lib.get_conv_math()
    try:
        lib.set_conv_math(1)
        y = dh.depthwise_conv3x3(xin, wg, d)
        y.backward(dy.to(DEV))
        log = dict(dconv.path_log)
    finally:
        dconv.path_log = prev
        lib.set_conv_math(prev_math)
    assert log == {("fwd", "f32/dw"): 1, ("dgrad", "f32/dw"): 1, ("wgrad", "f32/dw"): 1}
    w9 = dc.tap_major(w).to(DEV)
    st = lib.stream()
    y0, dx0 = torch.empty((n, h, w_, c), device=DEV), torch.empty((n, h, w_, c), device=DEV)
    g = dy.to(DEV).permute(0, 2, 3, 1).contiguous()
    lib.call("diga_dwconv3x3_f32", ptr(xg), 48, ptr(w9), ptr(y0), c, n, h, w_, c, d, 0, st)
    lib.call("diga_dwconv3x3_f32", ptr(g), c, ptr(w9), ptr(dx0), c, n, h, w_, c, d, 1, st)
    nbytes = lib.lib.diga_dwconv3x3_wgrad_workspace_bytes(n, h, w_, c)
    ws, dw9 = torch.empty(nbytes, dtype=torch.uint8, device=DEV), torch.empty((9, c), device=DEV)
    lib.call("diga_dwconv3x3_f32_wgrad", ptr(g), c, ptr(xg), 48, ptr(dw9), ptr(ws), nbytes, n, h, w_, c, d, st)
    assert torch.equal(y.detach().permute(0, 2, 3, 1), y0) and torch.equal(xin.grad.permute(0, 2, 3, 1), dx0)
    assert torch.equal(wg.grad, dw9.t().reshape(c, 1, 3, 3))


# ------------------------------------------------------------------------------------------------ 2: resize into a slice
RESIZE_E, RESIZE_N = 24, 2


@pytest.mark.parametrize("grids", [dc.GRIDS, dc.GRIDS_EVAL], ids=["capture", "odd"])
def test_resize_into_a_slice_against_float64(grids):
    """Each stage grid resized to the first one, written into its slice of a sentinel-filled 4E-wide buffer: against F.interpolate in
    float64 and its autograd (test_pyramid_sum_kernels_vs_torch's tolerances), the other slices bit-unchanged, ratio 1 a bit copy."""
    lib = _lib()
    (H, W), e, n = grids[0], RESIZE_E, RESIZE_N
    st = lib.stream()
    want_bits = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    for k, (h, w) in enumerate(grids):
        g = torch.Generator().manual_seed(100 * h + w)
        src = torch.randn((n, e, h, w), generator=g)
        if (h, w) == (H, W):                  # equal grids are a plain copy: values a weighted sum would not carry over
            src[0, 0, 0, :4] = torch.tensor([-0.0, float("inf"), float("-inf"), float("nan")])
        prb = torch.randn((n, e, H, W), generator=g)
        s64 = src.double().requires_grad_()
        ref = s64 if (h, w) == (H, W) else F.interpolate(s64, size=(H, W), mode="bilinear", align_corners=False)
        (ref * prb.double()).sum().backward()
        buf = torch.full((n * H * W, 4 * e), SENTINEL, dtype=torch.float32, device=DEV)
        win = buf[:, k * e:(k + 1) * e]
        win.fill_(float("nan"))
        sg = src.to(DEV).permute(0, 2, 3, 1).contiguous()
        lib.call("diga_pyramid_resize_fwd", ptr(sg), h, w, ptr(win), 4 * e, H, W, n, e, st)
        bits = buf.view(torch.int32)
        assert bool((bits[:, :k * e] == want_bits).all()) and bool((bits[:, (k + 1) * e:] == want_bits).all()), "another slice was written"
        out = nchw(win.cpu(), n, H, W)
        if (h, w) == (H, W):
            assert torch.equal(out.contiguous().view(torch.int32), src.view(torch.int32)), "equal grids copy the bits"
        else:
            assert_close(out, ref, 2e-6, 1e-5, f"resize {h}x{w}")
        # the adjoint on the pitched slice of a gradient buffer
        gbuf = torch.full((n * H * W, 4 * e), float("nan"), dtype=torch.float32, device=DEV)
        gwin = gbuf[:, k * e:(k + 1) * e]
        gwin.copy_(prb.permute(0, 2, 3, 1).reshape(-1, e))
        ds = torch.full((n, h, w, e), float("nan"), dtype=torch.float32, device=DEV)
        lib.call("diga_pyramid_resize_bwd", ptr(gwin), 4 * e, H, W, ptr(ds), h, w, n, e, st)
        assert_close(ds.permute(0, 3, 1, 2), s64.grad, 1e-5, 1e-5 * float(s64.grad.abs().max()), f"adjoint {h}x{w}")
        # <R x, g> == <x, R^T g>, as test_pyramid_sum_bwd_is_the_exact_adjoint (equal grids: on the finite part of the source)
        if (h, w) == (H, W):
            out, src = out.clone(), src.clone()
            out[0, 0, 0, :4] = src[0, 0, 0, :4] = 0.0
        a, b =float((out.double() * prb.double()).sum()), float((src.double() * ds.permute(0, 3, 1, 2).double().cpu()).sum())
        assert abs(a - b) < 1e-5 * max(abs(a), 1.0), ((h, w), a, b)


def test_resize_refuses_to_downsample():
    lib = _lib()
    a, b = torch.empty((1, 8, 8, 4), device=DEV), torch.empty((1, 4, 4, 4), device=DEV)
    assert lib.lib.diga_pyramid_resize_fwd(ptr(a), 8, 8, ptr(b), 4, 4, 4, 1, 4, lib.stream()) == -1 and "upsampling only" in lib.last_error()
    assert lib.lib.diga_pyramid_resize_bwd(ptr(b), 4, 4, 4, ptr(a), 8, 8, 1, 4, lib.stream()) == -1


# ------------------------------------------------------------------------------------------------ 3: the head against the capture
def _new_head(sd, **over):
    from diga_amd.model.networks.daformer_head import DAFormerHead
    in_channels = [sd[f"embed_layers.{i}.proj.weight"].shape[1] for i in range(4)]
    kw = dict(in_channels=in_channels, channels=sd["conv_seg.weight"].shape[1], feature_strides=[4, 8, 16, 32],
              num_classes=sd["conv_seg.weight"].shape[0], in_index=[0, 1, 2, 3], act_cfg=dict(type="ReLU"), dropout_ratio=0,
              norm_cfg=dict(type="BN", requires_grad=True), align_corners=False)
    kw.update(over)
    head = DAFormerHead(**kw)
    head.load_state_dict(sd)
    return head.to(DEV)


def _compose(mp):
    from diga_amd.model.networks import daformer_head as dh
    mp.setattr(dh, "USE_TORCH_DEPTHWISE", True)
    mp.setattr(dh.DAFormerHead, "raw_features", dc.composed_raw_features)


def _head_step(head, feats, prb, feats_eval=None):
    """One train-mode step (and an eval-mode forward) of the module: dc.head_step's tensors, whole, by name."""
    head.train()
    head.zero_grad(set_to_none=True)
    xs = [f.to(DEV).requires_grad_() for f in feats]
    raw = {}
    hook = head.fuse_layer.register_forward_hook(lambda m, i, o: raw.__setitem__("feat_raw", i[0]))      # (the ASPP's input)
    try:
        logits, feat = head(xs)
    finally:
        hook.remove()
    res = {"logits": logits, "feat": feat, "feat_raw": raw["feat_raw"]}
    (logits * prb.to(DEV)).sum().backward()
    for i, x in enumerate(xs):
        res[f"dc{i + 1}"] = x.grad
    for k, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        res["g_" + k.replace(".", "_")] = p.grad
    nbt = set()
    for k, b in head.named_buffers():
        if k.endswith("num_batches_tracked"):
            nbt.add(int(b))
        else:
            res["b_" + k.replace(".", "_")] = b.clone()
    if feats_eval is not None:
        head.eval()
        with torch.no_grad():
            lo, ft = head([f.to(DEV) for f in feats_eval])
        res["logits_eval"] = lo
        head.train()
    return {k: v.detach().double().cpu() for k, v in res.items()}, nbt


def _capture_run(composed=False):
    feats, feats_eval = dc.inputs(), dc.inputs(dc.GRIDS_EVAL, n=1, tag="eval")
    prb = dc.probe((dc.BATCH, dc.CLASSES) + dc.GRIDS[0])
    with pytest.MonkeyPatch.context() as mp:
        if composed:
            _compose(mp)
        head = _new_head(dc.state())
        got, nbt = _head_step(head, feats, prb, feats_eval)
    return dc.stored(got), nbt, got


def _capture_float64():
    """The float64 restatement's whole tensors on the capture's inputs (it reproduces the capture to 1e-12, tests/test_daformer_head_cpu.py):
    what an L2 distance is taken against where the fixture keeps a sample and a norm.  Computed once, shared, never written."""
    if "capture64" not in _REF:
        _REF["capture64"] = dc.head_step(dc.state(), dc.inputs(), dc.probe((dc.BATCH, dc.CLASSES) + dc.GRIDS[0]),
                                         dc.inputs(dc.GRIDS_EVAL, n=1, tag="eval"), torch.float64)
    return _REF["capture64"]


def test_head_against_the_capture_of_the_reference_class(golden, conv_math):
    z = golden("daformer_head")
    assert winograd_tile(dc.BATCH, 4 * dc.CHANNELS, *dc.GRIDS[0], dc.CHANNELS, 3, 1, 1, 1) == 0      # the bottleneck: a direct kernel
    got, nbt, whole = _capture_run()
    assert nbt == {int(z["nbt"])}
    names = [k for k in z if not k.startswith(("scale_", "err32_")) and k not in ("keys", "shapes", "nbt", "state_sum", "inputs_sum")]
    assert len(names) == 110 and sorted(names) == sorted(got)
    composed, _, composed_whole = _capture_run(composed=True) if conv_math == 1 else (None, None, None)
    failures = []
    for k in names:
        want, scale, e32 = z.t(k), float(z["scale_" + k]), float(z["err32_" + k])
        assert got[k].shape == want.shape, k
        err = float((got[k] - want).abs().max()) / scale
        if conv_math == 0:
            bound = 4.0 * e32
            print(f"  f32    {k:64s} {err:.2e}  (capture's fp32 {e32:.2e}, bound {bound:.2e})")
            if not err <= bound:
                failures.append(f"{k}: {err:.3e} of scale > {bound:.3e}")
            continue
        yard = float((composed[k] - want).abs().max()) / scale
        if k.endswith("_norm"):
            # as the fixture's err32 of a norm: the L2 distance of the tensor from the float64 one, in units of the norm (the
            # difference of two norms is a chance figure: 1e-7 against 5e-8 with both heads at their rounding level)
            ref = _capture_float64()[k[:-5]]
            err, yard = float((whole[k[:-5]] - ref).norm()) / scale, float((composed_whole[k[:-5]] - ref).norm()) / scale
        print(f"  bf16x3 {k:64s} {err:.2e}  (composed head {yard:.2e})")
        if not err <= 1.5 * yard:
            failures.append(f"{k}: {err:.3e} of scale, composed head {yard:.3e}")
    assert not failures, "\n".join(failures)


def test_return_raw_is_a_view_of_the_concat_buffer(monkeypatch):
    lib = _lib()
    feats = dc.inputs()
    head = _new_head(dc.state(), return_raw=True).train()
    dsts = []
    real_call = lib.call

    def spy(name, *args):
        if name == "diga_pyramid_resize_fwd":
            dsts.append(args[3].value)
        return real_call(name, *args)

    monkeypatch.setattr(lib, "call", spy)
    with torch.no_grad():
        logits, raw = head([f.to(DEV) for f in feats])
    n, (h, w) = dc.BATCH, dc.GRIDS[0]
    assert tuple(raw.shape) == (n, 4 * dc.E, h, w) and raw.permute(0, 2, 3, 1).is_contiguous()
    assert len(dsts) == 4 and dsts == [raw.data_ptr() + 4 * dc.E * k for k in range(4)], "feat_raw is not the buffer the kernels wrote"
    assert raw.data_ptr() == raw.untyped_storage().data_ptr()
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in dc.state().items()}
    ref = dc.raw_features(sd64, [f.double() for f in feats])
    held(raw.cpu(), ref, "feat_raw", bound=1e-5)
    assert tuple(logits.shape) == (n, dc.CLASSES, h, w)


# ------------------------------------------------------------------------------------------------ 4: the student
def _student():
    from diga_amd.model.segformer import SegFormerStudent
    torch.manual_seed(2602)
    m = SegFormerStudent("mit_b1", head="daformer", drop_path_rate=0.0)
    g = torch.Generator().manual_seed(2603)
    with torch.no_grad():                      # non-trivial BatchNorm affine pairs and a prediction conv of order 1
        for k, p in m.final.named_parameters():
            if ".bn." in k:
                p.copy_((1.0 if k.endswith("weight") else 0.0) + 0.2 * torch.randn(p.shape, generator=g))
        m.final.conv_seg.weight.copy_(torch.randn(m.final.conv_seg.weight.shape, generator=g) / 16.0)
    m.set_head_dropout(0.0)
    return m.to(DEV).train()


def _student_step(m, x, prb, masks=None):
    """`masks` (a dict): receives the ReLU decisions of the pass, output > 0 of every BatchNorm of the head by its state-dict prefix."""
    from diga_amd.model.norm import DigaTrainableBatchNorm2d
    sd0 = {k: v.detach().clone().cpu() for k, v in m.final.state_dict().items()}
    feats = {}
    hooks = [m.backbone.register_forward_hook(lambda mod, i, o: feats.__setitem__("f", [t.detach().float().cpu() for t in o]))]
    if masks is not None:
        for name, mod in m.final.named_modules():
            if isinstance(mod, DigaTrainableBatchNorm2d):
                hooks.append(mod.register_forward_hook(lambda mod, i, o, name=name: masks.__setitem__(name, (o.detach() > 0).cpu())))
    m.zero_grad(set_to_none=True)
    out = m(x)
    for h in hooks:
        h.remove()
    (out[2] * prb).sum().backward()
    got = {"logits": out[2]}
    for k, p in m.final.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        got["g_" + k.replace(".", "_")] = p.grad
    return out, {k: v.detach().double().cpu() for k, v in got.items()}, sd0, feats["f"]


def _student_case():
    g = torch.Generator().manual_seed(2604)
    return torch.randn((2, 3, 128, 128), generator=g).to(DEV), torch.randn((2, 19, 32, 32), generator=g).to(DEV)


def _student_refs(sd0, feats, prb):
    """float64 and fp32 restatement steps on the backbone's features: computed once per distinct feature set, shared, never written."""
    key = ("student", dc.checksum(feats))
    if key not in _REF:
        r64 = dc.head_step(sd0, feats, prb.cpu(), feats, torch.float64)
        r32 = dc.head_step(sd0, feats, prb.cpu(), feats, torch.float32)
        _REF[key] = (r64, r32)
    return _REF[key]


FLIP = 1e-5          # a ReLU site may be decided the other way only where |float64 pre-activation| <= this, in units of the tensor's scale


def test_student_step_against_the_restatement():
    """One training step of the mit_b1 student with head="daformer" at 2 x 3 x 128 x 128, Dropout2d off: logits and every head-parameter
    gradient against the same backbone features pushed through the float64 restatement, EVERY element within 4 x the fp32 restatement's
    own error and not below WINO_TOL[2].  Winograd tiles capped at F(2x2) (the 1024 -> 256 bottleneck takes F(4x4) by default, whose
    4e-5 forward error is the next test's subject).

    ReLU decisions.  The head has 8.4 M ReLU sites at this size with pre-activations of order 1; two fp32 runs differ by ~1e-6 there, so
    a few sites sit on different sides of zero in any two runs, and one such site moves the gradients in front of it by O(1e-2) of scale
    (measured: one depthwise channel -- the 9 taps of its weight, its BatchNorm pair, one row and one bias of its stage's embedding).
    No elementwise bound survives that, and an allowance for it hides real errors, so the float64 reference takes the decisions of the
    run it is compared with (daformer_cases.forward(masks=)): the student's own, read from its BatchNorm outputs, for `got`; the fp32
    restatement's for the yardstick.  The masks are held to the plain float64 run: a site may be decided differently only where the
    float64 pre-activation is within FLIP = 1e-5 of the tensor's scale (the bound of the fp32 kernels that produce it) of zero."""
    from diga_amd import config
    lib = _lib()
    prev, prev_tile = lib.get_conv_math(), config.active().winograd_max_tile
    lib.set_conv_math(0, exact=True)
    masks = {}
    try:
        m = _student()
        x, prb = _student_case()
        out, got, sd0, feats = _student_step(m, x, prb, masks)
        with torch.no_grad():
            again = m(x)[2]
    finally:
        lib.set_conv_math(prev)
        config.active().winograd_max_tile = prev_tile
    c2, c4, logits, feat = out
    dims = m.backbone.embed_dims
    assert tuple(c2.shape) == (2, dims[1], 16, 16) and tuple(c4.shape) == (2, dims[3], 4, 4)
    assert tuple(logits.shape) == (2, 19, 32, 32) and tuple(feat.shape) == (2, 256, 32, 32)
    assert torch.equal(again, logits), "a second forward under no_grad changes the bits of the logits"
    assert len(masks) == 8
    # the plain float64 run (its pre-activations judge both sets of masks), the fp32 restatement with its own decisions, and float64
    # under each run's decisions
    pre64, pre32 = {}, {}
    dc.head_step(sd0, feats, prb.cpu(), feats, torch.float64, pre=pre64)
    r32 = dc.head_step(sd0, feats, prb.cpu(), feats, torch.float32, pre=pre32)
    masks32 = {k: v > 0 for k, v in pre32.items()}
    failures = []
    for who, mk in (("student", masks), ("fp32 restatement", masks32)):
        for k, (count, worst) in dc.mask_disagreements(mk, pre64).items():
            print(f"  ReLU decisions, {who:16s} {k:48s} {count} of {pre64[k].numel()} sites differ from float64, largest |pre| {worst:.2e} of scale")
            if worst > FLIP:
                failures.append(f"{who}: a ReLU site of {k} with |float64 pre-activation| {worst:.2e} of scale is decided the other way")
    want_got = dc.head_step(sd0, feats, prb.cpu(), feats, torch.float64, masks=masks)
    want_32 = dc.head_step(sd0, feats, prb.cpu(), feats, torch.float64, masks=masks32)
    tile = 2
    for k, v in got.items():
        want = want_got[k]
        scale = float(want.abs().max())
        err = float((v - want).abs().max()) / scale
        yard = float((r32[k] - want_32[k]).abs().max()) / float(want_32[k].abs().max())
        bound = max(4.0 * yard, WINO_TOL[tile][1 if k.startswith("g_") else 0])
        print(f"  {k:64s} {err:.2e}  (fp32 restatement {yard:.2e}, bound {bound:.2e})")
        if not err <= bound:
            failures.append(f"{k}: {err:.3e} of scale > {bound:.3e}")
    assert not failures, "\n".join(failures)


def test_student_as_shipped_adds_nothing_to_the_student_on_torch_compositions(monkeypatch):
    """The same step with the default Winograd tiles: its error against float64 is the convolutions', so the yardstick is the same
    student with the depthwise convs and the resizes replaced by torch compositions on the GPU; 1.5 x that per tensor, gradients
    through assert_mostly_close (1e-4 of the elements, L2 1.5 x the composed student's)."""
    assert winograd_tile(2, 1024, 32, 32, 256, 3, 1, 1, 1) > 2
    x, prb = _student_case()
    _, got, sd0, feats = _student_step(_student(), x, prb)
    _compose(monkeypatch)
    _, comp, sd1, feats1 = _student_step(_student(), x, prb)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats1)) and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    r64, _ = _student_refs(sd0, feats, prb)
    failures = []
    for k, v in got.items():
        want = r64[k]
        scale = float(want.abs().max())
        err, yard = float((v - want).abs().max()) / scale, float((comp[k] - want).abs().max()) / scale
        l2 = float((v - want).norm() / want.norm().clamp_min(1e-300))
        l2_yard = float((comp[k] - want).norm() / want.norm().clamp_min(1e-300))
        print(f"  default tiles {k:56s} {err:.2e}  (composed {yard:.2e})  L2 {l2:.2e} (composed {l2_yard:.2e})")
        try:
            if k.startswith("g_"):
                assert_mostly_close(v, want, 0.0, 1.5 * yard * scale, 1e-4, max(1.5 * l2_yard, 1e-300), what=k)
            else:
                assert err <= 1.5 * yard, f"{k}: {err:.3e} of scale, composed student {yard:.3e}"
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
