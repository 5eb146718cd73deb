"""MiT-B0 (embed dims 32/64/160/256, heads 1/2/5/8: head_dim 32 in every stage) without a GPU: the module tree against the capture
of the REFERENCE module (tests/golden/mit_b0.npz, tools/gen_golden.py::gen_mit_b0 -- the first image of gen_mit's input recipe,
one image so that the file stays inside the size limit), the oracle at the B0 widths against the same capture, the three student
wirings, and the ctypes signatures of the head_dim entry points."""
import numpy as np
import pytest
import torch

from oracle import mit as om

B0 = om.MitArch(embed_dims=(32, 64, 160, 256), depths=(2, 2, 2, 2))


def test_mit_b0_constructs_with_the_reference_s_state_dict_layout(golden):
    from diga_amd.model.networks import MixTransfomer as M
    g = golden("mit_b0")
    m = M.mit_b0()
    assert type(m).__name__ == "mit_b0" and m.embed_dims == [32, 64, 160, 256] and m.depths == [2, 2, 2, 2]
    sd = m.state_dict()
    assert list(sd.keys()) == g["keys"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == g["shapes"].tolist()
    want = sum(int(np.prod([int(d) for d in s.split(",")])) for s in g["shapes"].tolist())
    assert sum(p.numel() for p in m.parameters()) == want
    for s in range(4):
        for blk in getattr(m, f"block{s + 1}"):
            assert blk.attn.dim // blk.attn.num_heads == 32 and blk.attn.scale == 32 ** -0.5


def test_other_head_widths_still_raise():
    from diga_amd.model.networks.MixTransfomer import Attention
    with pytest.raises(NotImplementedError, match="48"):
        Attention(dim=96, num_heads=2)
    Attention(dim=64, num_heads=2)
    Attention(dim=128, num_heads=2)


@pytest.mark.parametrize("head", ["segformer", "aspp", "daformer"])
def test_student_constructs_on_mit_b0(head):
    from diga_amd.model.segformer import SegFormerStudent
    m = SegFormerStudent("mit_b0", head=head)
    assert m.backbone.embed_dims == [32, 64, 160, 256]
    assert sum(p.numel() for p in m.final.parameters()) > 0


def test_oracle_layout_at_the_b0_widths_matches_the_capture(golden):
    g = golden("mit_b0")
    shp = om.state_shapes(B0)
    assert list(shp.keys()) == g["keys"].tolist()
    assert [",".join(str(d) for d in s) for s, _ in shp.values()] == g["shapes"].tolist()


def test_oracle_forward_backward_at_the_b0_widths_vs_reference(golden):
    g = golden("mit_b0")
    sd = {k: v.requires_grad_() for k, v in om.state_dict(B0).items()}
    outs = om.forward(sd, g.t("x"), B0)
    for i, o in enumerate(outs):
        want = g.t(f"c{i + 1}")
        assert tuple(o.shape) == tuple(want.shape)
        assert float((o - want).abs().max()) < 2e-5 * float(want.abs().max()), i
    sum((o * g.t(f"probe{i + 1}")).sum() for i, o in enumerate(outs)).backward()
    norms = np.array([float(sd[k].grad.norm()) for k in g["keys"].tolist()])
    assert np.allclose(norms, g["grad_norms"], rtol=2e-4, atol=1e-7)
    for k in [n[2:] for n in g if n.startswith("g_")]:
        name = [n for n in sd if n.replace(".", "_") == k][0]
        want = g.t("g_" + k)
        got = sd[name].grad.reshape(-1)[::int(g["gstep_" + k])]
        assert float((got - want).abs().max()) < 1e-4 * float(want.abs().max()) + 1e-7, name


def test_drop_path_scales_layout_values_and_frequencies():
    """`_drop_path_scales` on the CPU device (plain torch: the draw needs no kernel): per stage [depth][2][B], values 0 or 1 / keep_b with
    keep_b = 1 - linspace(0, rate, 8)[b], nothing in eval() or at rate 0, block 0 never dropped, and over n = 4000 draws at B = 8 the
    keep frequency of every (block, branch) within 5 standard deviations sqrt(p (1 - p) / (n B)) of keep_b."""
    from diga_amd.model.networks import MixTransfomer as M
    rate, B, n = 0.5, 8, 4000
    m = M.mit_b0()
    dev = torch.device("cpu")
    m.eval()
    assert m._drop_path_scales(m._cfg(), B, dev) == [None] * 4
    m.train()
    m.reset_drop_path(0.0)
    assert m._drop_path_scales(m._cfg(), B, dev) == [None] * 4
    m.reset_drop_path(rate)
    cfg = m._cfg()
    keep = torch.tensor([1.0 - v.item() for v in torch.linspace(0, rate, 8)])   # fp32 roundings of the double differences
    torch.manual_seed(1234)
    kept = torch.zeros((8, 2), dtype=torch.float64)
    differ = torch.zeros(8, dtype=torch.bool)
    for it in range(n):
        sc = m._drop_path_scales(cfg, B, dev)
        if it < 3:
            assert [tuple(s.shape) for s in sc] == [(d, 2, B) for d in m.depths]
        flat = torch.cat(sc, 0)                                                # [8][2][B], encoder order
        want = (1.0 / keep).view(8, 1, 1)
        assert bool(((flat == 0) | (flat == want)).all())
        kept += (flat != 0).double().sum(-1)
        differ |= ((flat[:, 0] != 0) != (flat[:, 1] != 0)).any(-1)
    freq = kept / (n * B)
    assert bool((freq[0] == 1.0).all())                                        # block 0: rate 0
    bound = 5 * torch.sqrt(keep * (1 - keep) / (n * B)).double()
    assert bool(((freq - keep.double().view(8, 1)).abs() <= bound.view(8, 1)).all()), (freq, keep)
    assert bool(differ[1:].all()), "the attention and the Mix-FFN branch of a block must not share one draw"


def test_head_dim_entry_points_are_declared_and_bound():
    import os
    from diga_amd import _lib
    INT, SZ, P, I64, F32 = _lib.INT, _lib.SZ, _lib.P, _lib.I64, _lib.F32
    S = _lib.SIGNATURES
    # the three head_dim-64 entry points keep their signatures
    assert S["diga_mit_attention_fwd"] == (INT, [P, I64, P, I64, P, I64, P, I64, I64, I64, I64, F32, P])
    assert S["diga_mit_attention_bwd_workspace_bytes"] == (SZ, [I64, I64, I64, I64])
    assert S["diga_mit_attention_bwd"] == (INT, [P, I64, P, I64, P, P, I64, P, P, P, P, SZ, I64, I64, I64, I64, F32, P])
    # their siblings take head_dim behind `heads`
    for old, new, at in (("diga_mit_attention_fwd", "diga_mit_attention_hd_fwd", 9),
                         ("diga_mit_attention_bwd_workspace_bytes", "diga_mit_attention_hd_bwd_workspace_bytes", 2),
                         ("diga_mit_attention_bwd", "diga_mit_attention_hd_bwd", 14)):
        res, args = S[old]
        assert S[new] == (res, args[:at] + [I64] + args[at:]), new
        assert hasattr(_lib.lib, new)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "diga_mit.h")) as fh:
        header = fh.read()
    with open(os.path.join(root, "INTEGRATION.md")) as fh:
        doc = fh.read()
    for name in ("diga_mit_attention_hd_fwd", "diga_mit_attention_hd_bwd_workspace_bytes", "diga_mit_attention_hd_bwd"):
        assert name + "(" in header and name in doc, name
    # the workspace query needs no device: both widths, and nothing for a width that is not built
    q = _lib.lib.diga_mit_attention_hd_bwd_workspace_bytes
    assert q(2, 8, 64, 576, 576) == _lib.lib.diga_mit_attention_bwd_workspace_bytes(2, 8, 576, 576)
    slab64 = q(2, 8, 64, 576, 576) - 2 * 8 * 576 * 4
    assert q(2, 8, 32, 576, 576) == slab64 // 2 + 2 * 8 * 576 * 4
    assert q(2, 8, 48, 576, 576) == 0
