"""GPU parity of MiT-B0 (embed dims 32/64/160/256 over 1/2/5/8 heads: head_dim 32): the head_dim-32 instantiation of the attention
kernels against float64 on the same fp16-rounded operands, the head_dim entry points at 64 against the old entry points bit for bit,
the B0 widths through the other MiT kernels, the mit_b0 encoder against captures of the REFERENCE module (tests/golden/mit_b0.npz,
mit_b0_768.npz; tools/gen_golden.py::gen_mit_b0) and the three student wirings on it.

Bounds: those of tests/test_gpu_mit.py for the same entry point and metric (same operands, same score distribution, same
arithmetic); MIT_TOL is imported from there.  Measured on the MI355X: see DESIGN.md section 9b."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mit as om
from oracle import synth
from test_gpu_mit import MIT_TOL, _rel, h16

pytestmark = pytest.mark.gpu
DEV = "cuda"
B0 = om.MitArch(embed_dims=(32, 64, 160, 256), depths=(2, 2, 2, 2))


def _lib():
    from diga_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------- 1. attention at head_dim 32
def _attn_operands(b, heads, n, nk, d, ldq=None, ldkv=None):
    g = synth.gen(b * 1000 + heads * 100 + n + nk + d)
    c = heads * d
    ldq, ldkv = ldq or c, ldkv or 2 * c
    q = h16(torch.randn((b * n, ldq), generator=g)).to(DEV)
    kv = h16(torch.randn((b * nk, ldkv), generator=g)).to(DEV)
    d_out = h16(torch.randn((b * n, ldq), generator=g)).to(DEV)
    return q, kv, d_out


def _attn_ref(q, kv, b, heads, n, nk, d, scale):
    """float64 attention on the dense [rows][heads*d] / [rows][2*heads*d] column windows of q / kv (leaves: for .grad)."""
    c = heads * d
    qr = q[:, :c].double().cpu().requires_grad_()
    kvr = kv[:, :2 * c].double().cpu().requires_grad_()
    qh = qr.reshape(b, n, heads, d).permute(0, 2, 1, 3)
    kvh = kvr.reshape(b, nk, 2, heads, d).permute(2, 0, 3, 1, 4)
    s = (qh @ kvh[0].transpose(-2, -1)) * scale
    ref = (s.softmax(-1) @ kvh[1]).transpose(1, 2).reshape(b * n, c)
    lse_ref = torch.logsumexp(s, -1) / np.log(2.0)
    return qr, kvr, ref, lse_ref


def _fwd(q, kv, out, lse, b, heads, d, n, nk, scale):
    lib = _lib()
    P = lib.ptr
    lib.call("diga_mit_attention_hd_fwd", P(q), q.stride(0), P(kv), kv.stride(0), P(out), out.stride(0), P(lse), b, heads, d, n, nk, scale,
             lib.stream())


def _bwd(q, kv, out, d_out, lse, dq, dkv, b, heads, d, n, nk, scale):
    lib = _lib()
    P = lib.ptr
    ws = torch.empty(lib.lib.diga_mit_attention_hd_bwd_workspace_bytes(b, heads, d, n, nk), dtype=torch.uint8, device=DEV)
    lib.call("diga_mit_attention_hd_bwd", P(q), q.stride(0), P(kv), kv.stride(0), P(out), P(d_out), out.stride(0), P(lse), P(dq), P(dkv), P(ws),
             ws.numel(), b, heads, d, n, nk, scale, lib.stream())


ATTN32_CASES = [(2, 8, 12, 12), (2, 2, 300, 12), (1, 5, 70, 130), (1, 2, 257, 64), (1, 1, 513, 608), (1, 1, 2304, 576), (1, 8, 576, 576)]


@pytest.mark.parametrize("b,heads,n,nk", ATTN32_CASES)
def test_attention_head_dim_32_forward_backward(b, heads, n, nk):
    d, scale = 32, 32 ** -0.5
    q, kv, d_out = _attn_operands(b, heads, n, nk, d)
    out = torch.empty_like(q)
    lse = torch.empty((b, heads, n), device=DEV)
    _fwd(q, kv, out, lse, b, heads, d, n, nk, scale)
    qr, kvr, ref, lse_ref = _attn_ref(q, kv, b, heads, n, nk, d, scale)
    e_out = _rel(out, ref)
    e_lse = float((lse.double().cpu() - lse_ref).abs().max())
    ref.backward(d_out.double().cpu())
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    _bwd(q, kv, out, d_out, lse, dq, dkv, b, heads, d, n, nk, scale)
    e_dq, e_dkv = _rel(dq, qr.grad), _rel(dkv, kvr.grad)
    print(f"attention head_dim 32 {(b, heads, n, nk)}: out {e_out:.2e} lse {e_lse:.2e} dq {e_dq:.2e} dkv {e_dkv:.2e}")
    assert e_out < 2e-3
    assert e_lse < 1e-3
    assert e_dq < 4e-3
    assert e_dkv < 4e-3
    dkv2 = torch.empty_like(kv)
    _bwd(q, kv, out, d_out, lse, dq, dkv2, b, heads, d, n, nk, scale)
    assert torch.equal(dkv, dkv2), "dK / dV partial slabs must reduce in a fixed order"


def test_attention_head_dim_32_pitched_operands():
    b, heads, n, nk, d, scale = 1, 5, 70, 130, 32, 32 ** -0.5
    c = heads * d
    q, kv, _ = _attn_operands(b, heads, n, nk, d, ldq=c + 8, ldkv=2 * c + 8)
    out = torch.full((b * n, c + 8), 7.0, dtype=torch.float16, device=DEV)
    lse = torch.empty((b, heads, n), device=DEV)
    _fwd(q, kv, out, lse, b, heads, d, n, nk, scale)
    _, _, ref, lse_ref = _attn_ref(q, kv, b, heads, n, nk, d, scale)
    assert _rel(out[:, :c], ref) < 2e-3
    assert float((lse.double().cpu() - lse_ref).abs().max()) < 1e-3
    assert bool((out[:, c:] == 7.0).all()), "the columns behind the heads belong to the caller"


def test_attention_rejects_other_head_widths_without_a_launch():
    lib = _lib()
    P = lib.ptr
    q, kv, _ = _attn_operands(1, 2, 16, 16, 48)
    out = torch.full_like(q, 3.0)
    rc = lib.lib.diga_mit_attention_hd_fwd(P(q), 96, P(kv), 192, P(out), 96, None, 1, 2, 48, 16, 16, 0.125, lib.stream())
    assert rc != 0 and "48" in lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    with pytest.raises(Exception, match="48"):
        _fwd(q, kv, out, None, 1, 2, 48, 16, 16, 0.125)


# ---------------------------------------------------------------------------------------------- 2. head_dim 64: new == old, bit for bit
@pytest.mark.parametrize("b,heads,n,nk", [(1, 5, 70, 130), (1, 1, 513, 608)])
def test_head_dim_entry_points_at_64_equal_the_old_ones(b, heads, n, nk):
    lib = _lib()
    P = lib.ptr
    d, scale, c = 64, 0.125, heads * 64
    q, kv, d_out = _attn_operands(b, heads, n, nk, d)
    res = []
    for new in (False, True):
        out = torch.empty_like(q)
        lse = torch.empty((b, heads, n), device=DEV)
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        if new:
            _fwd(q, kv, out, lse, b, heads, d, n, nk, scale)
            _bwd(q, kv, out, d_out, lse, dq, dkv, b, heads, d, n, nk, scale)
        else:
            lib.call("diga_mit_attention_fwd", P(q), c, P(kv), 2 * c, P(out), c, P(lse), b, heads, n, nk, scale, lib.stream())
            ws = torch.empty(lib.lib.diga_mit_attention_bwd_workspace_bytes(b, heads, n, nk), dtype=torch.uint8, device=DEV)
            lib.call("diga_mit_attention_bwd", P(q), c, P(kv), 2 * c, P(out), P(d_out), c, P(lse), P(dq), P(dkv), P(ws), ws.numel(), b, heads,
                     n, nk, scale, lib.stream())
        res.append((out, lse, dq, dkv))
    for a, bb, name in zip(res[0], res[1], ("out", "lse", "dq", "dkv")):
        assert torch.equal(a, bb), name


# ---------------------------------------------------------------------------------------------- 3. B0 widths through the other ops
B0_GEMM_CASES = [(300, 32, 32), (513, 64, 32), (129, 32, 2048), (777, 128, 32), (64, 32, 128), (300, 160, 160), (129, 640, 160), (5, 160, 640)]


@pytest.mark.parametrize("m,n,k", B0_GEMM_CASES)
def test_gemm_nt_epilogues_at_b0_widths(m, n, k):
    from diga_amd.model.networks.MixTransfomer import _Ops
    g = synth.gen(m + n + k)
    a = h16(torch.randn((m, k), generator=g)).to(DEV)
    w = h16(torch.randn((n, k), generator=g) / k ** 0.5).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    res = torch.randn((m, n), generator=g).to(DEV)
    rps = (m + 2) // 3
    seg = torch.tensor([1.0, 0.0, 1.25, 2.0][: (m + rps - 1) // rps]).to(DEV)
    ops = _Ops(torch.device(DEV))
    ref = a.double() @ w.double().t()
    assert _rel(ops.gemm(a, w, None, n, out_f32=True), ref) < 1e-5
    assert _rel(ops.gemm(a, w, bias, n), ref + bias.double()) < 2e-3
    segrow = seg[torch.arange(m, device=DEV) // rps].double()[:, None]
    want = res.double() + segrow * (0.5 * ref + bias.double())
    assert _rel(ops.gemm(a, w, bias, n, out_f32=True, residual=res, seg=seg, rows_per_seg=rps, alpha=0.5), want) < 1e-5
    base = h16(torch.randn((m, n), generator=g)).to(DEV)
    out = base.clone()
    ops.gemm(a, w, None, n, out=out, accumulate=True)
    assert _rel(out, base.double() + ref) < 2e-3


@pytest.mark.parametrize("m,n,k", B0_GEMM_CASES)
def test_gemm_tn_weight_gradient_at_b0_widths(m, n, k):
    from diga_amd.model.networks.MixTransfomer import _Ops
    g = synth.gen(7 * m + n + k)
    dy = h16(torch.randn((m, n), generator=g)).to(DEV)
    x = h16(torch.randn((m, k), generator=g)).to(DEV)
    ops = _Ops(torch.device(DEV))
    dw, db = ops.wgrad(dy, x, 0.25, bias=True)
    assert tuple(dw.shape) == (n, k)
    assert _rel(dw, 0.25 * dy.double().t() @ x.double()) < 2e-5
    assert _rel(db, 0.25 * dy.double().sum(0)) < 2e-5
    assert torch.equal(dw, ops.wgrad(dy, x, 0.25)), "split-K slabs must reduce in a fixed order"
    assert _rel(ops.colsum(dy, 2.0), 2.0 * dy.double().sum(0)) < 2e-5


@pytest.mark.parametrize("c", [32, 160])
@pytest.mark.parametrize("m", [37, 1000])
def test_layernorm_forward_backward_at_b0_widths(m, c):
    from diga_amd.model.networks.MixTransfomer import _Ops
    g = synth.gen(c + m)
    x = (torch.randn((m, c), generator=g) * 2 + 0.5).to(DEV)
    gamma = (1 + 0.2 * torch.randn(c, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(c, generator=g)).to(DEV)
    ops = _Ops(torch.device(DEV))
    y16, y32, mean, rstd = ops.ln_fwd(x, gamma, beta, 1e-6, want16=True, want32=True)
    xr = x.double().cpu().requires_grad_()
    gr, br = gamma.double().cpu().requires_grad_(), beta.double().cpu().requires_grad_()
    yr = F.layer_norm(xr, (c,), gr, br, 1e-6)
    assert _rel(y32, yr) < 2e-6 and _rel(y16, yr) < 1e-3
    dy = h16(torch.randn((m, c), generator=g)).to(DEV)
    dres = torch.randn((m, c), generator=g).to(DEV)
    (yr * (3.0 * dy.double().cpu())).sum().backward()
    dx32, dx16, dg, db = ops.ln_bwd(dy, x, gamma, mean, rstd, dres, True, True, 0.5, gscale=3.0)
    assert _rel(dx32, xr.grad + dres.double().cpu()) < 1e-5
    assert _rel(dx16, xr.grad + dres.double().cpu()) < 1e-3
    assert _rel(dg, 0.5 * gr.grad) < 1e-5 and _rel(db, 0.5 * br.grad) < 1e-5


@pytest.mark.parametrize("c", [128, 640])
def test_dwconv_gelu_forward_backward_at_b0_widths(c):
    lib = _lib()
    P = lib.ptr
    b, h, w = 2, 9, 7
    g = synth.gen(b * h + w + c)
    x = h16(torch.randn((b, h, w, c), generator=g)).to(DEV)
    wt = (0.4 * torch.randn((c, 1, 3, 3), generator=g)).to(DEV)
    bias = (0.1 * torch.randn(c, generator=g)).to(DEV)
    wt9 = wt.reshape(c, 9).t().contiguous()
    u = torch.empty_like(x)
    hh = torch.empty_like(x)
    lib.call("diga_mit_dwconv_gelu_fwd", P(x), P(wt9), P(bias), P(u), P(hh), b, h, w, c, lib.stream())
    xr = x.double().cpu().permute(0, 3, 1, 2).requires_grad_()
    wr, br = wt.double().cpu().requires_grad_(), bias.double().cpu().requires_grad_()
    ur = F.conv2d(xr, wr, br, 1, 1, 1, c)
    assert _rel(u.permute(0, 3, 1, 2), ur) < 1e-3
    assert _rel(hh.permute(0, 3, 1, 2), F.gelu(u.double().cpu().permute(0, 3, 1, 2))) < 1e-3
    dh = h16(torch.randn((b, h, w, c), generator=g)).to(DEV)
    u_leaf = u.double().cpu().permute(0, 3, 1, 2).requires_grad_()
    (F.gelu(u_leaf) * dh.double().cpu().permute(0, 3, 1, 2)).sum().backward()
    du_ref = u_leaf.grad
    ur.backward(h16(du_ref).double())
    du = torch.empty_like(x)
    dx = torch.empty_like(x)
    dw = torch.empty((c, 9), device=DEV)
    dbias = torch.empty(c, device=DEV)
    ws = torch.empty(lib.lib.diga_mit_dwconv_bwd_workspace_bytes(b, h, c), dtype=torch.uint8, device=DEV)
    lib.call("diga_mit_dwconv_gelu_bwd", P(dh), P(u), P(x), P(wt9.flip(0).contiguous()), P(du), P(dx), P(dw), P(dbias), 2.0, 0, P(ws),
             ws.numel(), b, h, w, c, lib.stream())
    assert _rel(du.permute(0, 3, 1, 2), du_ref) < 1e-3
    assert _rel(dx.permute(0, 3, 1, 2), xr.grad) < 2e-3
    assert _rel(dw.reshape(c, 1, 3, 3), 2.0 * wr.grad) < 5e-4
    assert _rel(dbias, 2.0 * br.grad) < 5e-4


def test_patch_embedding_im2col_into_160_columns_at_width_32():
    """7x7 stride 4 pad 3 on the image: 147 gathered values per row, zero-padded to Kp = 160; the GEMM behind it has N = 32."""
    from diga_amd.model.networks.MixTransfomer import _conv16, _Ops
    g = synth.gen(732)
    b, h, w, cout = 2, 37, 29, 32
    x = h16(torch.randn((b, 3, h, w), generator=g)).float()
    wt = h16(torch.randn((cout, 3, 7, 7), generator=g) / 147 ** 0.5).float()
    ops = _Ops(torch.device(DEV))
    w16, _, kp = _conv16(wt.to(DEV), True)
    assert kp == 160
    cols, ho, wo = ops.im2col(x.to(DEV), 2, b, h, w, 3, 7, 4, 3, kp)
    assert tuple(cols.shape) == (b * ho * wo, 160) and bool((cols[:, 147:] == 0).all())
    y = ops.gemm(cols, w16, None, cout, out_f32=True).view(b, ho, wo, cout).permute(0, 3, 1, 2)
    yr = F.conv2d(x.double(), wt.double(), None, 4, 3)
    assert tuple(y.shape) == tuple(yr.shape) and _rel(y, yr) < 1e-5


# ---------------------------------------------------------------------------------------------- 4.-6. the encoder
def _model():
    from diga_amd.model.networks import MixTransfomer as M
    m = M.mit_b0()
    m.load_state_dict(om.state_dict(B0))
    return m.to(DEV)


def test_mit_b0_forward_backward_vs_reference_capture(golden):
    g = golden("mit_b0")
    m = _model().eval()                                            # eval(): DropPath off, as in the capture
    outs = m(g.t("x").to(DEV))
    worst = 0.0
    for i, o in enumerate(outs):
        want = g.t(f"c{i + 1}")
        assert tuple(o.shape) == tuple(want.shape)
        worst = max(worst, _rel(o, want))
    sum((o * g.t(f"probe{i + 1}").to(DEV)).sum() for i, o in enumerate(outs)).backward()
    named = dict(m.named_parameters())
    keys = g["keys"].tolist()
    ratio = np.array([float(named[k].grad.norm()) for k in keys]) / np.maximum(g["grad_norms"], 1e-12)
    gerr = {}
    for k in [n[2:] for n in g if n.startswith("g_")]:
        name = [n for n in keys if n.replace(".", "_") == k][0]
        gerr[name] = _rel(named[name].grad.reshape(-1)[::int(g["gstep_" + k])], g.t("g_" + k))
    print(f"mit_b0 vs reference: features max err {worst:.2e} of scale, sampled gradients {max(gerr.values()):.2e}, "
          f"gradient-norm ratios {ratio.min():.4f} .. {ratio.max():.4f}")
    assert worst < MIT_TOL["features"]
    bad = [(k, r) for k, r in zip(keys, ratio) if abs(r - 1.0) > MIT_TOL["grad_norm"]]
    assert not bad, bad[:10]
    assert max(gerr.values()) < MIT_TOL["grad_sample"], sorted(gerr.items(), key=lambda kv: -kv[1])[:5]


def test_mit_b0_benchmark_geometry_vs_reference_capture(golden):
    """768x768: stage 1 runs 36864 queries against 576 keys on ONE head of width 32."""
    g = golden("mit_b0_768")
    x = torch.rand((1, 3, 768, 768), generator=synth.gen(int(g["seed"]))) * 2 - 1
    m = _model().eval()
    with torch.no_grad():
        outs = m(x.to(DEV))
    assert [tuple(o.shape) for o in outs] == [(1, 32, 192, 192), (1, 64, 96, 96), (1, 160, 48, 48), (1, 256, 24, 24)]
    errs = []
    for o, key, step, mx in zip(outs, ("c1_sample", "c2_sample", "c3_sample", "c4_sample"), (211, 53, 7, 3), g["maxs"]):
        errs.append(float((o.float().cpu().reshape(-1)[::step] - g.t(key)).abs().max()) / float(mx))
    print("mit_b0 at 768x768 vs reference: feature samples " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < MIT_TOL["features"], errs
    sums = np.array([float(o.abs().sum()) for o in outs])
    assert np.allclose(sums, g["sums"], rtol=2e-3)


def test_mit_b0_ragged_input_size_vs_oracle():
    hw = (100, 76)
    m = _model().eval()
    x = torch.rand((2, 3) + hw, generator=synth.gen(hw[0])) * 2 - 1
    sd = {k: v.clone().requires_grad_() for k, v in om.state_dict(B0).items()}
    want = om.forward(sd, x, B0)
    sum((o * o).sum() for o in want).backward()
    got = m(x.to(DEV))
    assert [tuple(o.shape) for o in got] == [tuple(o.shape) for o in want]
    for a, b in zip(got, want):
        assert _rel(a, b) < 1e-2
    sum((o * o).sum() for o in got).backward()
    named = dict(m.named_parameters())
    ratios = [float(named[k].grad.norm()) / max(float(sd[k].grad.norm()), 1e-12) for k in sd]
    assert 0.95 < min(ratios) and max(ratios) < 1.05, (min(ratios), max(ratios))


# ---------------------------------------------------------------------------------------------- 7. the student on mit_b0
@pytest.mark.parametrize("head", ["segformer", "aspp", "daformer"])
def test_student_on_mit_b0_trains_a_step(head):
    from diga_amd.model.segformer import SegFormerStudent
    from diga_amd.util import utils as U
    torch.manual_seed(11)
    m = SegFormerStudent("mit_b0", head=head, drop_path_rate=0.0)
    m.backbone.load_state_dict(om.state_dict(B0))
    m.set_head_dropout(0.0)
    m = m.to(DEV).train()
    x = (torch.rand((2, 3, 128, 128), generator=synth.gen(128)) * 2 - 1).to(DEV)
    c2, c4, logits, feat = m(x)
    at = 4 if head == "aspp" else 32                               # logits at 1/32 (ASPP on the last stage) or 1/4 scale
    fch = {"segformer": 768, "aspp": 256, "daformer": 256}[head]
    assert tuple(c2.shape) == (2, 64, 16, 16) and tuple(c4.shape) == (2, 256, 4, 4)
    assert tuple(logits.shape) == (2, 19, at, at) and tuple(feat.shape) == (2, fch, at, at)
    assert all(bool(torch.isfinite(t).all()) for t in (c2, c4, logits, feat))
    gp = synth.gen(7)
    p_log, p_feat = torch.randn(logits.shape, generator=gp).to(DEV), torch.randn(feat.shape, generator=gp).to(DEV)

    def loss_of(lg, ft):
        return (lg * p_log).sum() + 0.1 * (ft * p_feat).sum()

    loss_of(logits, feat).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    full = {k: p.grad.clone() for k, p in m.backbone.named_parameters()}
    # the wiring: the same backbone gradients from the backbone alone under the head's input-gradients as probes
    m.zero_grad(set_to_none=True)
    outs = m.backbone(x)
    leaves = [o.detach().requires_grad_() for o in outs]
    if head == "aspp":
        res = m.final(leaves[3])
        lg, ft = res["out"], res["feat"]
    else:
        lg, ft = m.final(leaves)
    loss_of(lg, ft).backward()
    probes = [torch.zeros_like(o) if lf.grad is None else lf.grad for o, lf in zip(outs, leaves)]
    sum((o * p).sum() for o, p in zip(outs, probes)).backward()
    # (equal bit for bit: the head and the backbone's backward are deterministic, and autograd adds the same two fp32 terms into c1..c3)
    differ = [k for k, p in m.backbone.named_parameters() if not torch.equal(p.grad, full[k])]
    assert not differ, differ[:5]
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = U.DigaSGD([{"params": list(m.parameters())}], lr=1e-2, momentum=0.9, weight_decay=0.0)
    opt.step(found_inf=m.grad_overflow)
    assert m.grad_overflow.cpu().tolist()[0] == 0
    changed = [k for k, p in m.named_parameters() if not torch.equal(p.detach(), before[k])]
    assert len(changed) > 0.9 * len(before), (len(changed), len(before))
