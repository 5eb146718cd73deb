"""The MiT attention kernels (diga_mit_attention_hd_fwd / _bwd at head_dim 32 and 64) on score distributions other than the
unit-Gaussian logits of ATTN_CASES / ATTN32_CASES: trained attention is peaked.  Families, all built from randn operands rounded to fp16:

  peaked4 / peaked16   q scaled by tau = 4 (logit std 4, moderate) or 16 (saturated: nearly one-hot rows)
  offset+ / offset-    the last 8 of the D dims of every q are 4, of every k +4 or -4: +-128 scale on every logit of a row.  Softmax is
                       invariant to it in exact arithmetic; the kernels see |s c| of several tens in exp2(s c - lse)
  ramp_up / ramp_down  those 8 dims of key j carry j delta and those of every q are 16, so that the logit rises / falls 0.5 per key at
                       D = 64 (delta 1/32: 8 * 16 / 32 * 64**-0.5) and 0.53 at D = 32 (delta 3/128: 3 * 32**-0.5; that scale is irrational,
                       no fp16 values give 0.5 exactly); j delta is exact in fp16 for every j < 200.  Rising: the running maximum moves in
                       EVERY 64-key block (alpha = exp2((m - mn) c) far below 1); falling: the maximum sits in block 0, later blocks' p fall
                       through fp32's subnormal range to zero (fast_exp2 has no denormal rescue) with the masked tail keys behind them.
                       Why q = 16 and not the offset family's 4: the slope is the product q delta, and dQ = dS K sums dS, ROUNDED TO FP16
                       BY THE KERNELS' DEFINITION, against key entries that grow with delta while sum_j dS_ij = 0 cancels their common
                       part.  With q = 4 (key entries up to 25) the float64 evaluation of the definition (`_bwd_as_defined`) is by itself
                       6.4e-3 of scale from the exact dq at (1, 1, 33, 200), D = 64 -- no kernel could meet 4e-3; with q = 16 the key
                       entries stay below 6.3, the range of the Gaussian entries beside them, and the definition is within 1.6e-3 (CPU).
                       The family is there for the moving maximum, not for the operand scale (DESIGN.md section 9b notes the sensitivity)
  ties                 all keys equal, V random: out is the mean of V, lse = s c log2(e) + log2(Nk)

Forward bounds, every family: the project's (out 2e-3 of scale, lse 1e-3 absolute; tests/test_gpu_mit.py).  They come from fp16
storage of P and O and hold for any distribution: out is a convex combination of V rows with weights good to 2^-11 relative.
Backward: the project's 4e-3 of scale against float64 autograd, for every family but the saturated one.  There the exact gradient of
q and k tends to zero and what the kernels return is dominated, by design, by roundings the definition of the kernels contains:
delta = rowsum(dO * O) is taken from the fp16 O, and P and dS enter the last MFMAs in fp16.  `_bwd_as_defined` evaluates that
definition in float64 with exactly those three roundings; its distance from the exact gradient is measured on the CPU per output,
and the bound is max(4e-3, 3 x that distance) (3 = the project's margin over a measured value).  dV keeps 4e-3 everywhere.

CPU-measured distances of the definition from the exact float64 gradient, `_rel` metric (recomputed by the test; kept here for the
reader, and the test checks that they have not moved):

  SATURATED_DISTANCE[(D, (b, heads, n, nk))] = (dq, dk)             -- see the table below the imports
"""
import math

import pytest
import torch

from oracle import synth
from test_gpu_mit import _rel, h16
from test_gpu_mit_b0 import _attn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 2, 70, 130), (2, 1, 257, 65), (1, 1, 33, 200)]
FAMILIES = ["peaked4", "peaked16", "offset+", "offset-", "ramp_up", "ramp_down", "ties"]
# distance of the kernels' stated definition (fp16 O in delta, fp16 P and dS) from the exact gradient, saturated family, on the CPU
SATURATED_DISTANCE = {
    (32, (1, 2, 70, 130)): (1.070e-03, 1.110e-03),
    (32, (2, 1, 257, 65)): (9.793e-04, 9.522e-04),
    (32, (1, 1, 33, 200)): (1.079e-03, 6.421e-04),
    (64, (1, 2, 70, 130)): (9.248e-04, 7.127e-04),
    (64, (2, 1, 257, 65)): (4.711e-04, 7.702e-04),
    (64, (1, 1, 33, 200)): (1.218e-03, 1.609e-03),
}


def _lib():
    from diga_amd import _lib
    return _lib


def _poison(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0xFF)
    return t


def _ramp_delta(d):
    return 0.03125 if d == 64 else 0.0234375


def hash_seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) * 7919


def _operands(family, b, heads, n, nk, d):
    """CPU fp16 operands q [b*n][heads*d], kv [b*nk][2*heads*d] (K | V), d_out [b*n][heads*d] of one score family."""
    g = synth.gen(hash_seed(family) + b * 1000 + heads * 100 + n + nk + d)
    c = heads * d
    q = torch.randn((b * n, heads, d), generator=g)
    k = torch.randn((b * nk, heads, d), generator=g)
    v = torch.randn((b * nk, heads, d), generator=g)
    d_out = h16(torch.randn((b * n, c), generator=g))
    if family.startswith("peaked"):
        q = q * float(family[len("peaked"):])
    elif family.startswith("offset"):
        q[..., d - 8:] = 4.0
        k[..., d - 8:] = 4.0 if family.endswith("+") else -4.0
    elif family.startswith("ramp"):
        j = torch.arange(nk, dtype=torch.float32).repeat(b)                        # key index within its image
        q[..., d - 8:] = 16.0
        k[..., d - 8:] = ((1.0 if family == "ramp_up" else -1.0) * _ramp_delta(d) * j).view(-1, 1, 1)
    elif family == "ties":
        k = k.view(b, nk, heads, d)[:, :1].expand(b, nk, heads, d).reshape(b * nk, heads, d)
    else:
        raise ValueError(family)
    q, k, v = h16(q), h16(k), h16(v)
    if family.startswith("ramp"):
        want = ((1.0 if family == "ramp_up" else -1.0) * _ramp_delta(d) * j).view(-1, 1, 1).expand(-1, heads, 8)
        assert torch.equal(k[..., d - 8:].float(), want)                           # exact in fp16
    return q.reshape(b * n, c), torch.cat([k.reshape(b * nk, c), v.reshape(b * nk, c)], 1).contiguous(), d_out


def _bwd_as_defined(q, kv, d_out, b, heads, n, nk, d, scale):
    """float64 evaluation of the backward kernels' stated definition (mit_attn.hip, the comments above attn_bwd_dq_kernel and
    attn_bwd_dkv_kernel): P = exp2(S c - lse), dP = dO V^T, delta = rowsum(dO * O) from the fp16 O, dS = P (dP - delta) scale;
    dQ = dS K and dK = dS^T Q with dS rounded to fp16, dV = P^T dO with P rounded to fp16.  Everything else exact."""
    c = heads * d
    qh = q.double().reshape(b, n, heads, d).permute(0, 2, 1, 3)
    kvh = kv.double().reshape(b, nk, 2, heads, d).permute(2, 0, 3, 1, 4)
    kh, vh = kvh[0], kvh[1]
    do = d_out.double().reshape(b, n, heads, d).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-2, -1)) * scale
    p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    o16 = (p @ vh).half().double()
    delta = (do * o16).sum(-1, keepdim=True)
    ds = p * (do @ vh.transpose(-2, -1) - delta) * scale
    ds16, p16 = ds.half().double(), p.half().double()
    dq = (ds16 @ kh).permute(0, 2, 1, 3).reshape(b * n, c)
    dk = (ds16.transpose(-2, -1) @ qh).permute(0, 2, 1, 3).reshape(b * nk, c)
    dv = (p16.transpose(-2, -1) @ do).permute(0, 2, 1, 3).reshape(b * nk, c)
    return dq, dk, dv


def _run(q, kv, d_out, b, heads, n, nk, d, scale):
    """Forward and backward on the device; q / d_out (and with them out / dq) may be pitched.  Every buffer the kernels write is
    poisoned first.  Returns out, lse, dq, dkv (device tensors, full pitch)."""
    lib = _lib()
    P = lib.ptr
    qd, kvd, dod = q.to(DEV), kv.to(DEV), d_out.to(DEV)
    out = _poison(tuple(qd.shape), torch.float16)
    lse = _poison((b, heads, n), torch.float32)
    lib.call("diga_mit_attention_hd_fwd", P(qd), qd.stride(0), P(kvd), kvd.stride(0), P(out), out.stride(0), P(lse), b, heads, d, n, nk,
             scale, lib.stream())
    dq = _poison(tuple(qd.shape), torch.float16)
    dkv = _poison(tuple(kvd.shape), torch.float16)
    ws = _poison((lib.lib.diga_mit_attention_hd_bwd_workspace_bytes(b, heads, d, n, nk),), torch.uint8)
    lib.call("diga_mit_attention_hd_bwd", P(qd), qd.stride(0), P(kvd), kvd.stride(0), P(out), P(dod), out.stride(0), P(lse), P(dq), P(dkv),
             P(ws), ws.numel(), b, heads, d, n, nk, scale, lib.stream())
    return out, lse, dq, dkv


def _finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("b,heads,n,nk", SHAPES)
@pytest.mark.parametrize("d", [32, 64])
def test_attention_on_non_gaussian_scores(d, b, heads, n, nk, family):
    scale, c = d ** -0.5, heads * d
    q, kv, d_out = _operands(family, b, heads, n, nk, d)
    qr, kvr, ref, lse_ref = _attn_ref(q, kv, b, heads, n, nk, d, scale)
    ref.backward(d_out.double())
    bound_dq = bound_dk = 4e-3
    if family == "peaked16":
        m_dq, m_dk, m_dv = _bwd_as_defined(q, kv, d_out, b, heads, n, nk, d, scale)
        dist = (_rel(m_dq, qr.grad), _rel(m_dk, kvr.grad[:, :c]), _rel(m_dv, kvr.grad[:, c:]))
        print(f"saturated head_dim {d} {(b, heads, n, nk)}: the definition is {dist[0]:.3e} (dq) {dist[1]:.3e} (dk) {dist[2]:.3e} (dv) from exact")
        table = SATURATED_DISTANCE[(d, (b, heads, n, nk))]
        assert all(abs(got - want) <= 0.1 * want for got, want in zip(dist[:2], table)), (dist, table)
        bound_dq, bound_dk = max(4e-3, 3 * dist[0]), max(4e-3, 3 * dist[1])
    out, lse, dq, dkv = _run(q, kv, d_out, b, heads, n, nk, d, scale)
    e_out = _rel(out, ref)
    e_lse = float((lse.double().cpu() - lse_ref).abs().max())
    e_dq, e_dkv = _rel(dq, qr.grad), _rel(dkv, kvr.grad)
    if family == "ties":
        # dq_i = sum_j dS_ij k_j with all k_j equal and sum_j dS_ij = 0: the exact gradient is ZERO by cancellation (autograd in float64
        # returns 1e-16) and `_rel` has no scale to refer to.  The scale of this sum is that of the terms that cancel:
        # max_i sum_j |dS_ij| max|k|, from the exact float64 dS
        qh = q.double().reshape(b, n, heads, d).permute(0, 2, 1, 3)
        kvh = kv.double().reshape(b, nk, 2, heads, d).permute(2, 0, 3, 1, 4)
        doh = d_out.double().reshape(b, n, heads, d).permute(0, 2, 1, 3)
        p = ((qh @ kvh[0].transpose(-2, -1)) * scale).softmax(-1)
        dp = doh @ kvh[1].transpose(-2, -1)
        ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
        assert float(qr.grad.abs().max()) < 1e-12
        e_dq = float(dq.double().abs().max()) / float(ds.abs().sum(-1).max() * kvh[0].abs().max())
    e_dk, e_dv = _rel(dkv[:, :c], kvr.grad[:, :c]), _rel(dkv[:, c:], kvr.grad[:, c:])
    print(f"attention [{family}] head_dim {d} {(b, heads, n, nk)}: out {e_out:.2e} lse {e_lse:.2e} dq {e_dq:.2e} dkv {e_dkv:.2e} "
          f"(dk {e_dk:.2e} dv {e_dv:.2e}); bounds dq {bound_dq:.2e} dk {bound_dk:.2e}")
    assert _finite(out, lse, dq, dkv)
    assert e_out < 2e-3
    assert e_lse < 1e-3
    if family == "peaked16":
        assert e_dq < bound_dq
        assert e_dk < bound_dk
        assert e_dv < 4e-3
    else:
        assert e_dq < 4e-3
        assert e_dkv < 4e-3
        assert e_dv < 4e-3
    if family == "ties":
        vmean = kv[:, c:].double().reshape(b, nk, c).mean(1, keepdim=True).expand(b, n, c).reshape(b * n, c)
        assert _rel(out, vmean) < 2e-3
        s = (q.double().reshape(b, n, heads, d) * kv[:, :c].double().reshape(b, nk, heads, d)[:, :1]).sum(-1) * scale   # [b][n][heads]
        want = s.permute(0, 2, 1) * math.log2(math.e) + math.log2(nk)
        assert float((lse.double().cpu() - want).abs().max()) < 1e-3


@pytest.mark.parametrize("family", ["offset+", "offset-"])
@pytest.mark.parametrize("d", [32, 64])
def test_attention_is_invariant_to_a_common_offset(d, family):
    """The same operands with and without the +-128 scale offset on every logit: out and the lse minus the offset agree within the
    forward bounds, each against the other's float64 reference."""
    b, heads, n, nk = SHAPES[0]
    scale, c = d ** -0.5, heads * d
    q, kv, d_out = _operands(family, b, heads, n, nk, d)
    q0, kv0 = q.clone().view(b * n, heads, d), kv.clone().view(b * nk, 2 * heads, d)
    q0[..., d - 8:] = 0
    kv0[:, :heads, d - 8:] = 0
    q0, kv0 = q0.view(b * n, c), kv0.view(b * nk, 2 * c)
    _, _, ref0, lse0 = _attn_ref(q0, kv0, b, heads, n, nk, d, scale)
    out, lse, _, _ = _run(q, kv, d_out, b, heads, n, nk, d, scale)
    shift = (128.0 if family.endswith("+") else -128.0) * scale * math.log2(math.e)
    assert _rel(out, ref0) < 2e-3
    assert float((lse.double().cpu() - shift - lse0).abs().max()) < 1e-3


EDGE_SHAPES = [(1, 1, 1, 1), (1, 2, 1, 130), (2, 1, 256, 64), (1, 1, 257, 65), (1, 3, 64, 63)]


@pytest.mark.parametrize("b,heads,n,nk", EDGE_SHAPES)
@pytest.mark.parametrize("d", [32, 64])
def test_attention_edge_shapes(d, b, heads, n, nk):
    """One query, one key, exact multiples of the 256-query and 64-key blocks and one more / one less, at Gaussian scores."""
    scale, c = d ** -0.5, heads * d
    g = synth.gen(b * 1000 + heads * 100 + n + nk + d + 5)
    q = h16(torch.randn((b * n, c), generator=g))
    kv = h16(torch.randn((b * nk, 2 * c), generator=g))
    d_out = h16(torch.randn((b * n, c), generator=g))
    qr, kvr, ref, lse_ref = _attn_ref(q, kv, b, heads, n, nk, d, scale)
    ref.backward(d_out.double())
    out, lse, dq, dkv = _run(q, kv, d_out, b, heads, n, nk, d, scale)
    e_out, e_lse = _rel(out, ref), float((lse.double().cpu() - lse_ref).abs().max())
    if nk > 1:
        e_dq, e_dkv = _rel(dq, qr.grad), _rel(dkv, kvr.grad)
    else:
        # one key: the softmax is 1 whatever q is; dq and dk are exactly zero (dS = P (dP - delta) scale with delta = dP) and `_rel`
        # has no scale to refer to.  They are held to the scale of the term that cancels instead: |dP| scale |k| resp. |dP| scale |q|
        assert float(qr.grad.abs().max()) == 0 and float(kvr.grad[:, :c].abs().max()) == 0
        dp = float((d_out.double().reshape(b * n, heads, d) * kv[:, c:].double().reshape(1, heads, d)).sum(-1).abs().max()) * scale
        e_dq = float(dq.double().abs().max()) / (dp * float(kv[:, :c].double().abs().max()))
        e_dkv = max(_rel(dkv[:, c:], kvr.grad[:, c:]), float(dkv[:, :c].double().abs().max()) / (dp * float(q.double().abs().max())))
    print(f"attention edge shape head_dim {d} {(b, heads, n, nk)}: out {e_out:.2e} lse {e_lse:.2e} dq {e_dq:.2e} dkv {e_dkv:.2e}")
    assert _finite(out, lse, dq, dkv)
    assert e_out < 2e-3
    assert e_lse < 1e-3
    assert e_dq < 4e-3
    assert e_dkv < 4e-3
    _, _, _, dkv2 = _run(q, kv, d_out, b, heads, n, nk, d, scale)
    assert torch.equal(dkv, dkv2), "dK / dV partial slabs must reduce in a fixed order"


@pytest.mark.parametrize("d", [32, 64])
def test_attention_backward_with_pitched_operands(d):
    """q, out, d_out and dq with a row pitch of heads * D + 8 (kv dense: dkv is written densely); the eight columns behind the heads
    hold garbage on input and must keep their poison in dq and out."""
    b, heads, n, nk = 1, 3, 70, 130
    scale, c = d ** -0.5, heads * d
    g = synth.gen(9000 + d)
    q = h16(torch.randn((b * n, c + 8), generator=g))
    kv = h16(torch.randn((b * nk, 2 * c), generator=g))
    d_out = h16(torch.randn((b * n, c + 8), generator=g))
    q[:, c:] = 1000.0                                                  # never read: would show in every result
    d_out[:, c:] = -1000.0
    qr, kvr, ref, lse_ref = _attn_ref(q, kv, b, heads, n, nk, d, scale)
    ref.backward(d_out[:, :c].double())
    out, lse, dq, dkv = _run(q, kv, d_out, b, heads, n, nk, d, scale)
    assert out.stride(0) == c + 8 and dq.stride(0) == c + 8
    e_out, e_lse = _rel(out[:, :c], ref), float((lse.double().cpu() - lse_ref).abs().max())
    e_dq, e_dkv = _rel(dq[:, :c], qr.grad), _rel(dkv, kvr.grad)
    print(f"attention pitched backward head_dim {d}: out {e_out:.2e} lse {e_lse:.2e} dq {e_dq:.2e} dkv {e_dkv:.2e}")
    assert e_out < 2e-3 and e_lse < 1e-3
    assert e_dq < 4e-3
    assert e_dkv < 4e-3
    for name, t in (("out", out), ("dq", dq)):
        assert bool((t[:, c:].contiguous().view(torch.uint8) == 0xFF).all()), f"{name}: the columns behind the heads belong to the caller"
