"""GPU tests of the loader-split form of bf16x6 (config.x6_split = "loader"; the `_f32in` entry points of csrc/conv_bf16x6.h): the
GEMMs' loader waves read the fp32 tensors and write the three bf16 planes into the LDS bytes the triplet form's LDS-DMA lands them
in.  The same planes in the same LDS bytes, fed to the same MFMA code, give the same bits, so every comparison with the pass form
here is `torch.equal` -- no tolerance anywhere but in the float64 anchor of test 3.

  1. / 2. entry points against entry points (forward, weight gradient), on shapes chosen for the ring, the tile clamps, strides,
          out-of-image pixels and row pitches;
  3. every pointwise row of test_gpu_conv.CASES as a layer, with `path_log` proving that the loader form ran;
  4. the backward-data epilogue on three chained bottlenecks;  5. the whole small model;  6. the form switched inside one graph;
  7. the memory the triplets no longer take;  8. mode 0 does not see the switch."""
import pytest
import torch

from diga_amd import config

from conftest import assert_close
from oracle import deeplab as od
from oracle import detweights, synth
from test_gpu_conv import CASES
from test_gpu_conv_bf16x6 import POINTWISE_CASES, _Mode, _block_state, _inputs, _make_block, _run_layer

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def _guarded(shape, guard=256):
    """A zeroed device buffer of prod(shape) floats followed by `guard` floats that nothing may write."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.zeros(n + guard, dtype=torch.float32, device=DEV)
    return buf, buf[:n].view(shape), buf[n:]


# ------------------------------------------------------------------------------------------------ 1. forward entry points
#            name          n  hi  wi  cin cout stride off bias stats  (buffer channels, first channel)
FWD_CASES = [("a_one_kstep", 1, 7, 9, 32, 64, 1, 0, False, False, None),
             ("b_three_ksteps_ragged", 2, 17, 17, 96, 320, 1, 0, True, False, None),
             ("c_stride2_stats", 2, 33, 31, 64, 128, 2, 0, False, True, None),
             ("d_stride2_outside", 2, 33, 31, 64, 128, 2, -1, False, True, None),
             ("e_channel_slice", 2, 9, 11, 64, 64, 1, 0, False, False, (160, 32)),
             ("f_head_19", 2, 17, 17, 256, 19, 1, 0, False, False, None)]


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c[0])
def test_forward_entry_point_equals_triplet_form(case):
    from diga_amd import _lib
    name, n, hi, wi, cin, cout, stride, off, bias, stats, sl = case
    ho, wo = (hi - 1) // stride + 1, (wi - 1) // stride + 1
    g = synth.gen(3100 + cin + cout + hi)
    wide, c0 = sl if sl is not None else (cin, 0)
    buf = (torch.randn((n, hi, wi, wide), generator=g) * torch.exp2(torch.randint(-6, 7, (n, hi, wi, wide), generator=g).float())).to(DEV)
    x = buf[..., c0:c0 + cin]                                     # the fp32 operand: in place, pitch `wide`
    assert x.stride(2) == wide and x.data_ptr() % 16 == 0
    w = (torch.randn((cout, cin), generator=g) * (2.0 / cin) ** 0.5).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV) if bias else None
    st, tag = _lib.stream(), _lib.PROF_TAGS.index("conv_fwd")
    img = torch.empty(_lib.lib.diga_split_bf16x6_image_bytes(cout, 1, cin), dtype=torch.uint8, device=DEV)
    _lib.call("diga_split_bf16x6_image", _lib.ptr(w), _lib.ptr(img), cout, 1, cin, st)
    nstats = _lib.lib.diga_conv2d_stats_floats(n, ho, wo, cout) if stats else 0
    geom = (n, hi, wi, cin, ho, wo, cout, cout, 1, 1, stride, stride, off, off, 1, 1)

    # pass form: triplet of the contiguous copy, then the triplet kernel
    xc = x.contiguous()
    trip = torch.empty(n * hi * wi * cin * 6, dtype=torch.uint8, device=DEV)
    _lib.call("diga_make_triplet", _lib.ptr(xc), cin, _lib.ptr(trip), n * hi * wi, cin, st)
    _, out_p, guard_p = _guarded((n, ho, wo, cout))
    stats_p = torch.zeros(nstats, dtype=torch.float32, device=DEV) if stats else None
    _lib.call("diga_conv2d_nhwc_bf16x6", _lib.ptr(trip), _lib.ptr(img), _lib.ptr(b), _lib.ptr(out_p), *geom, _lib.ptr(stats_p), tag, st)
    # loader form: the fp32 tensor itself
    _, out_l, guard_l = _guarded((n, ho, wo, cout))
    stats_l = torch.zeros(nstats, dtype=torch.float32, device=DEV) if stats else None
    _lib.call("diga_conv2d_nhwc_bf16x6_f32in", _lib.ptr(x), wide, _lib.ptr(img), _lib.ptr(b), _lib.ptr(out_l), *geom, _lib.ptr(stats_l),
              tag, st)
    torch.cuda.synchronize()
    assert float(out_p.abs().max()) > 0 and bool(torch.isfinite(out_p).all())
    assert torch.equal(out_l, out_p), f"{name}: {int((out_l != out_p).sum())} of {out_p.numel()} outputs differ"
    assert int((guard_l != 0).sum()) == 0 and int((guard_p != 0).sum()) == 0
    if stats:
        assert float(stats_p.abs().max()) > 0
        assert torch.equal(stats_l, stats_p), f"{name}: statistics partials differ"
    if off < 0:                                                   # the first output row and column read outside the image: bias-free zeros
        assert float(out_l[:, 0].abs().max()) == 0.0 and float(out_l[:, :, 0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. weight-gradient entry points
#              name              n  hi  wi  cin cout stride (dy_ld, x_ld)
WGRAD_CASES = [("a_one_split", 1, 7, 9, 32, 64, 1, None),
               ("b_many_splits", 3, 97, 97, 64, 256, 1, None),
               ("c_stride2", 2, 33, 31, 128, 512, 2, None),
               ("d_partial_tiles", 2, 19, 23, 96, 320, 1, None),
               ("e_row_pitch", 1, 7, 9, 32, 64, 1, (80, 40))]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: c[0])
def test_weight_gradient_entry_point_equals_triplet_form(case):
    from diga_amd import _lib
    name, n, hi, wi, cin, cout, stride, lds = case
    ho, wo = (hi - 1) // stride + 1, (wi - 1) // stride + 1
    g = synth.gen(3200 + cin + cout + hi)
    dy_ld, x_ld = lds if lds is not None else (cout, cin)
    dyb = torch.randn((n, ho, wo, dy_ld), generator=g).to(DEV)
    xb = torch.randn((n, hi, wi, x_ld), generator=g).to(DEV)
    dy, x = dyb[..., dy_ld - cout:], xb[..., x_ld - cin:]           # (the last channels of the wider buffers: offsets 16 and 8 floats)
    assert dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    st = _lib.stream()
    nbytes = _lib.lib.diga_conv2d_wgrad_bf16x6_workspace_bytes(n, ho, wo, cout, cin, 1, 1)
    geom = (n, hi, wi, cin, ho, wo, cout, 1, 1, stride, stride, 0, 0, 1, 1)

    dyc, xc = dy.contiguous(), x.contiguous()
    dy_trip = torch.empty(n * ho * wo * cout * 6, dtype=torch.uint8, device=DEV)
    x_trip = torch.empty(n * hi * wi * cin * 6, dtype=torch.uint8, device=DEV)
    _lib.call("diga_make_triplet", _lib.ptr(dyc), cout, _lib.ptr(dy_trip), n * ho * wo, cout, st)
    _lib.call("diga_make_triplet", _lib.ptr(xc), cin, _lib.ptr(x_trip), n * hi * wi, cin, st)
    _, dw_p, guard_p = _guarded((cout, cin))
    ws_p = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    _lib.call("diga_conv2d_wgrad_bf16x6", _lib.ptr(dy_trip), _lib.ptr(x_trip), _lib.ptr(dw_p), _lib.ptr(ws_p), nbytes, *geom, st)
    _, dw_l, guard_l = _guarded((cout, cin))
    ws_l = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    _lib.call("diga_conv2d_wgrad_bf16x6_f32in", _lib.ptr(dy), dy_ld, _lib.ptr(x), x_ld, _lib.ptr(dw_l), _lib.ptr(ws_l), nbytes, *geom, st)
    torch.cuda.synchronize()
    assert float(dw_p.abs().max()) > 0 and bool(torch.isfinite(dw_p).all())
    assert torch.equal(dw_l, dw_p), f"{name}: {int((dw_l != dw_p).sum())} of {dw_p.numel()} weight gradients differ"
    assert int((guard_l != 0).sum()) == 0 and int((guard_p != 0).sum()) == 0


# ------------------------------------------------------------------------------------------------ 3. layers
ANCHORED = ("1x1_stride2", "1x1_ragged_320")                     # additionally held to float64 at the bounds of the pass form's table


def _run_layer_form(case, form, x, wt, b, probe):
    with config.override(x6_split=form):
        return _run_layer(case, 2, x, wt, b, probe)


@pytest.mark.parametrize("case", POINTWISE_CASES, ids=lambda c: c[0])
def test_layers_equal_pass_form(case):
    name = case[0]
    x, wt, b, probe, yr, dxr, dwr, dbr = _inputs(case)
    y_p, dx_p, dw_p, db_p, log_p = _run_layer_form(case, "pass", x, wt, b, probe)
    y_l, dx_l, dw_l, db_l, log_l = _run_layer_form(case, "loader", x, wt, b, probe)
    assert log_p == {("fwd", "bf16x6"): 1, ("dgrad", "bf16x6"): 1, ("wgrad", "bf16x6"): 1}, log_p
    assert log_l == {("fwd", "bf16x6/ls"): 1, ("dgrad", "bf16x6/ls"): 1, ("wgrad", "bf16x6/ls"): 1}, log_l
    assert torch.equal(y_l, y_p), f"{name} y"
    assert torch.equal(dx_l, dx_p), f"{name} dx"
    assert torch.equal(dw_l, dw_p), f"{name} dw"
    assert (db_l is None and db_p is None) or torch.equal(db_l, db_p), f"{name} db"
    if name in ANCHORED:
        assert_close(y_l, yr, 1e-5, 2e-6 * float(yr.abs().max()), f"{name} forward")
        assert_close(dx_l, dxr, 1e-5, 3e-6 * float(dxr.abs().max()), f"{name} grad input")
        assert_close(dw_l, dwr, 1e-5, 3e-6 * float(dwr.abs().max()), f"{name} grad weight")


def test_layer_reads_a_channel_slice_in_place(monkeypatch):
    """A layer whose input is channels 32..95 of a 160-channel NHWC buffer: the loader form hands the kernels the view itself
    (in_ld = x_ld = 160, no copy, no triplet); results equal the pass form's, which runs on a contiguous copy."""
    from diga_amd import _lib
    from diga_amd.model.conv import DigaConv2d
    g = synth.gen(3300)
    m = DigaConv2d(64, 96, 1, bias=False).to(DEV)
    buf = torch.randn((2, 9, 11, 160), generator=g).to(DEV)
    probe = torch.randn((2, 96, 9, 11), generator=g).to(DEV)
    calls, orig = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a)), orig(name, *a))[1])
    res = {}
    for form in ("pass", "loader"):
        m.weight.grad = None
        x = buf[..., 32:96].permute(0, 3, 1, 2).requires_grad_()
        calls.clear()
        with config.override(x6_split=form), _Mode(2):
            y = m(x)
            (y * probe).sum().backward()
            torch.cuda.synchronize()
        res[form] = (y.detach().clone(), x.grad.clone(), m.weight.grad.clone(), [(nm, a) for nm, a in calls])
    for i, what in enumerate(("y", "dx", "dw")):
        assert torch.equal(res["loader"][i], res["pass"][i]), what
    names = [nm for nm, _ in res["loader"][3]]
    assert "diga_make_triplet" not in names
    fwd = [a for nm, a in res["loader"][3] if nm == "diga_conv2d_nhwc_bf16x6_f32in"]
    wg = [a for nm, a in res["loader"][3] if nm == "diga_conv2d_wgrad_bf16x6_f32in"]
    assert len(fwd) == 2 and len(wg) == 1                         # forward + backward-data, one weight gradient
    assert fwd[0][0].value == buf.data_ptr() + 32 * 4 and fwd[0][1] == 160        # the view itself at the buffer's pitch
    assert wg[0][2].value == buf.data_ptr() + 32 * 4 and wg[0][3] == 160


# ------------------------------------------------------------------------------------------------ 4. / 7. chained bottlenecks
_JUNCTION = {}


def _junction(form):
    """Three chained bottlenecks with the residual junctions fused (the construction of
    test_gpu_conv_bf16x6.py::test_residual_junction_epilogues_and_forward_statistics), forward + backward in mode 2 under one operand
    form: run once (results, launches; also warms the workspaces up), then once more behind empty_cache() + reset_peak_memory_stats()
    for the peak.  Computed once per form and shared by tests 4 and 7."""
    if form in _JUNCTION:
        return _JUNCTION[form]
    from diga_amd import _lib
    from diga_amd.model import norm as dn
    planes, inpl, dil, n, h, w = 64, 256, 1, 2, 31, 29
    names = [f"junction{planes}.b{i}" for i in range(3)]
    blocks = [_make_block(_block_state(nm, inpl, planes), nm, inpl, planes, dil) for nm in names]
    g = synth.gen(planes + 5)
    x = torch.randn((n, inpl, h, w), generator=g).relu_() + 0.1 * torch.randn((n, inpl, h, w), generator=g)
    probe = torch.randn((n, inpl, h, w), generator=g).to(DEV)
    assert config.active().fuse_bwd and dn.fuse_backward_enabled()
    calls, orig = [], _lib.call
    out = None
    for measured in (False, True):
        for b in blocks:
            for p in b.parameters():
                p.grad = None
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
        if measured:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
        else:
            _lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        try:
            with config.override(x6_split=form), _Mode(2) as log:
                y = xd
                for b in blocks:
                    y = b(y)
                (y * probe).sum().backward()
                torch.cuda.synchronize()
                log = dict(log)
        finally:
            _lib.call = orig
        if measured:
            peak = torch.cuda.max_memory_allocated()
        else:
            # (kept on the host: nothing of one form's results may sit in device memory while the other form's peak is taken)
            grads = {f"{i}.{k}": p.grad.cpu() for i, b in enumerate(blocks) for k, p in b.named_parameters() if p.grad is not None}
            out = (y.detach().cpu(), xd.grad.cpu(), grads, log, list(calls))
        del y, xd
    _JUNCTION[form] = out + (peak,)
    return _JUNCTION[form]


def test_backward_data_epilogue_equals_pass_form():
    y_p, dx_p, gr_p, log_p, calls_p, _ = _junction("pass")
    y_l, dx_l, gr_l, log_l, calls_l, _ = _junction("loader")
    assert calls_p.count("diga_conv2d_nhwc_bf16x6_epi") == 5 and calls_p.count("diga_conv2d_nhwc_bf16x6_f32in_epi") == 0, calls_p
    assert calls_l.count("diga_conv2d_nhwc_bf16x6_f32in_epi") == 5 and calls_l.count("diga_conv2d_nhwc_bf16x6_epi") == 0, calls_l
    assert "diga_make_triplet" not in calls_l and "diga_make_triplet" in calls_p
    assert log_l[("fwd", "bf16x6/ls")] == 6 and log_l[("dgrad", "bf16x6/ls")] == 6 and log_l[("wgrad", "bf16x6/ls")] == 6, log_l
    assert not any(a == "bf16x6" for _, a in log_l), log_l
    assert torch.equal(y_l, y_p) and torch.equal(dx_l, dx_p)
    assert gr_l.keys() == gr_p.keys() and len(gr_l) == 9           # 3 blocks x 3 conv weights (the BatchNorm affines are frozen)
    for k in gr_p:
        assert torch.equal(gr_l[k], gr_p[k]), k


def test_loader_form_takes_less_memory():
    """The pass form keeps the triplet of every eligible layer's input (1.5 x the input) for its weight gradient and builds one of
    every incoming gradient; the loader form builds none, so its peak on the same graph is strictly lower."""
    peak_p, peak_l = _junction("pass")[5], _junction("loader")[5]
    print(f"\n[bf16x6 loader] peak allocated on three chained bottlenecks: pass {peak_p / 2 ** 20:.1f} MiB, loader {peak_l / 2 ** 20:.1f} MiB")
    assert peak_l < peak_p, (peak_l, peak_p)


# ------------------------------------------------------------------------------------------------ 5. / 6. whole model
_MODEL = {}


def _model_run(fwd_form, bwd_form):
    """One forward + backward of the small backbone model at 96 x 128 in mode 2, the forward under one operand form and the backward
    under another: (logits, loss, parameter gradients, path log).  The loss is a fixed linear probe of logits and features (torch's
    sum is deterministic), dropout off.  Cached per (forward form, backward form)."""
    key = (fwd_form, bwd_form)
    if key in _MODEL:
        return _MODEL[key]
    from diga_amd.model import seg_model_noaux as sm
    from diga_amd.model.model_noaux import SegModel
    m = SegModel(arch=sm.TINY)
    m.load_state_dict(detweights.state_dict(od.TINY))
    m = m.to(DEV).train()
    m.final.head[0].p = 0.0
    g = synth.gen(4242)
    x = (torch.rand((2, 3, 96, 128), generator=g) * 2 - 1).to(DEV)
    with _Mode(2) as log:
        with config.override(x6_split=fwd_form):
            _, _, out, feat = m(x)
        probe = torch.randn(out.shape, generator=g).to(DEV)
        probe_f = (0.1 * torch.randn(feat.shape, generator=g)).to(DEV)
        loss = (out * probe).sum() + (feat * probe_f).sum()
        with config.override(x6_split=bwd_form):
            loss.backward()
            torch.cuda.synchronize()
        log = dict(log)
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    _MODEL[key] = (out.detach().clone(), loss.detach().clone(), grads, log)
    return _MODEL[key]


def _assert_same_model_run(got, want, what):
    assert torch.equal(got[0], want[0]), f"{what}: logits"
    assert torch.equal(got[1], want[1]), f"{what}: loss"
    assert got[2].keys() == want[2].keys() and len(want[2]) > 0
    for k in want[2]:
        assert torch.equal(got[2][k], want[2][k]), f"{what}: gradient of {k}"


def test_whole_model_equals_pass_form():
    want, got = _model_run("pass", "pass"), _model_run("loader", "loader")
    for p in ("fwd", "dgrad", "wgrad"):
        assert want[3].get((p, "bf16x6"), 0) > 0 and (p, "bf16x6/ls") not in want[3], want[3]
        assert got[3].get((p, "bf16x6/ls"), 0) == want[3][(p, "bf16x6")] and (p, "bf16x6") not in got[3], (got[3], want[3])
    _assert_same_model_run(got, want, "loader form")


@pytest.mark.parametrize("fwd_form,bwd_form", [("loader", "pass"), ("pass", "loader")])
def test_form_switched_between_forward_and_backward(fwd_form, bwd_form):
    """The form is read per call: a pass-form backward of a loader-form forward builds the triplets the forward did not save, a
    loader-form backward ignores the saved ones -- either way the all-pass bits."""
    want, got = _model_run("pass", "pass"), _model_run(fwd_form, bwd_form)
    tag_f, tag_b = ("bf16x6/ls" if f == "loader" else "bf16x6" for f in (fwd_form, bwd_form))
    assert got[3].get(("fwd", tag_f), 0) == want[3][("fwd", "bf16x6")], got[3]
    assert got[3].get(("dgrad", tag_b), 0) == want[3][("dgrad", "bf16x6")], got[3]
    assert got[3].get(("wgrad", tag_b), 0) == want[3][("wgrad", "bf16x6")], got[3]
    _assert_same_model_run(got, want, f"forward {fwd_form}, backward {bwd_form}")


# ------------------------------------------------------------------------------------------------ 8. mode 0 untouched
def test_exact_fp32_does_not_see_the_switch():
    case = next(c for c in CASES if c[0] == "1x1_64_256")
    x, wt, b, probe = _inputs(case)[:4]
    res = {}
    for form in ("pass", "loader"):
        cfg = config.active().replace()
        cfg.x6_split = form
        with config.use(cfg):
            res[form] = _run_layer(case, 0, x, wt, b, probe)
    for form in res:
        assert not any(a.startswith("bf16x6") for _, a in res[form][4]), res[form][4]
    assert res["pass"][4] == res["loader"][4]
    for i, what in enumerate(("y", "dx", "dw")):
        assert torch.equal(res["loader"][i], res["pass"][i]), what
