"""oracle/mit.py (the CPU restatement of the MiT encoder) against captures of the REFERENCE module
(G5/model/networks/MixTransfomer.py, imported by tools/gen_golden.py::gen_mit): features and parameter gradients of mit_b5
on a small non-square input, and features of mit_b1 at the benchmark geometry (768x768: 36864 queries x 576 keys in stage 1)."""
import numpy as np
import pytest
import torch

from oracle import mit as om
from oracle import synth


def test_state_dict_layout_matches_reference(golden):
    g = golden("mit")
    assert list(om.state_shapes(om.MIT_B5).keys()) == g["keys"].tolist()
    assert sum(int(np.prod(s)) for s, _ in om.state_shapes(om.MIT_B5).values()) == 81443008


@pytest.mark.timeout(600)
def test_mit_b5_forward_backward_vs_reference(golden):
    g = golden("mit")
    sd = {k: v.requires_grad_() for k, v in om.state_dict(om.MIT_B5).items()}
    outs = om.forward(sd, g.t("x"), om.MIT_B5)
    for i, o in enumerate(outs):
        want = g.t(f"c{i + 1}")
        assert float((o - want).abs().max()) < 2e-5 * float(want.abs().max()), i
    sum((o * g.t(f"probe{i + 1}")).sum() for i, o in enumerate(outs)).backward()
    norms = np.array([float(sd[k].grad.norm()) for k in g["keys"].tolist()])
    assert np.allclose(norms, g["grad_norms"], rtol=2e-4, atol=1e-7)
    for k in [n[2:] for n in g if n.startswith("g_")]:
        name = [n for n in sd if n.replace(".", "_") == k][0]
        step = int(g["gstep_" + k])
        want = g.t("g_" + k)
        got = sd[name].grad.reshape(-1)[::step]
        assert float((got - want).abs().max()) < 1e-4 * float(want.abs().max()) + 1e-7, name


B0 = om.MitArch(embed_dims=(32, 64, 160, 256), depths=(2, 2, 2, 2))


def test_drop_scales_none_is_the_former_oracle_bit_for_bit():
    """`forward(..., drop_scales=None)` (and a list of None, and all-ones scales) against the DropPath-free composition spelled out
    here from the oracle's own attention() / mlp(): same tensors, bit for bit, in the features and in every gradient."""
    import torch.nn.functional as F
    arch = om.MIT_TINY
    x = torch.rand((2, 3, 32, 48), generator=synth.gen(5)) * 2 - 1

    def plain(sd):
        outs, t = [], x
        for s in range(len(arch.embed_dims)):
            p, k = f"patch_embed{s + 1}", 7 if s == 0 else 3
            t = F.conv2d(t, sd[p + ".proj.weight"], sd[p + ".proj.bias"], stride=4 if s == 0 else 2, padding=k // 2)
            _, C, H, W = t.shape
            t = F.layer_norm(t.flatten(2).transpose(1, 2), (C,), sd[p + ".norm.weight"], sd[p + ".norm.bias"], 1e-5)
            for i in range(arch.depths[s]):
                b = f"block{s + 1}.{i}"
                t = t + om.attention(sd, b + ".attn", F.layer_norm(t, (C,), sd[b + ".norm1.weight"], sd[b + ".norm1.bias"], 1e-6), H, W,
                                     arch.num_heads[s], arch.sr_ratios[s])
                t = t + om.mlp(sd, b + ".mlp", F.layer_norm(t, (C,), sd[b + ".norm2.weight"], sd[b + ".norm2.bias"], 1e-6), H, W)
            t = F.layer_norm(t, (C,), sd[f"norm{s + 1}.weight"], sd[f"norm{s + 1}.bias"], 1e-6)
            t = t.reshape(2, H, W, -1).permute(0, 3, 1, 2).contiguous()
            outs.append(t)
        return outs

    def run(fn):
        sd = {k: v.requires_grad_() for k, v in om.state_dict(arch).items()}
        outs = fn(sd)
        sum((o * o).sum() for o in outs).backward()
        return [o.detach() for o in outs], {k: v.grad for k, v in sd.items()}

    want_o, want_g = run(plain)
    ones = [torch.ones((d, 2, 2)) for d in arch.depths]
    for ds in (None, [None] * len(arch.depths), ones):
        got_o, got_g = run(lambda sd: om.forward(sd, x, arch, drop_scales=ds))
        assert all(torch.equal(a, b) for a, b in zip(got_o, want_o))
        assert all(torch.equal(got_g[k], want_g[k]) for k in want_g)
    assert all(torch.equal(a, b) for a, b in zip(run(lambda sd: om.forward(sd, x, arch))[0], want_o))


def _droppath_run(g, scales):
    """Oracle (float32) on the capture's input with `scales` [8][2][B]: features, and the parameter gradients under the stored probes."""
    sd = {k: v.requires_grad_() for k, v in om.state_dict(B0).items()}
    outs = om.forward(sd, g.t("x"), B0, drop_scales=list(scales.split(2)))
    sum((o * g.t(f"probe{i + 1}")).sum() for i, o in enumerate(outs)).backward()
    return [o.detach() for o in outs], {k: v.grad for k, v in sd.items()}


def _droppath_samples(g):
    keys = g["keys"].tolist()
    return {[n for n in keys if n.replace(".", "_") == k[2:]][0]: (g.t(k), int(g["gstep_" + k[2:]])) for k in g if k.startswith("g_")}


def test_droppath_capture_holds_the_cases_it_is_there_for(golden):
    g = golden("mit_b0_droppath")
    s = g.t("scales")
    assert tuple(s.shape) == (8, 2, 3) and tuple(g["x"].shape) == (3, 3, 64, 64)
    keep = 1.0 - torch.linspace(0, 0.3, 8)
    for b in range(8):
        assert bool(((s[b] == 0) | (s[b] == 1.0 / keep[b])).all()), b
    drop = s == 0
    assert not bool(drop[0].any())                                           # block1.0 has rate 0
    assert bool(drop[3, 0].all())                                            # block2.1 attention: all three images
    for st in range(4):                                                      # every stage: a branch dropped for exactly one image
        assert bool((drop[2 * st:2 * st + 2].sum(-1) == 1).any()), st
    assert bool(drop[4:6, :, 2].all())                                       # image 2: the whole of stage 3
    assert bool((drop[:, 0] & ~drop[:, 1]).any()) and bool((~drop[:, 0] & drop[:, 1]).any())
    mant, _ = np.frexp(s[1:][s[1:] != 0].numpy())
    assert not bool((mant == 0.5).any())                                     # no kept scale is a power of two


def test_oracle_with_drop_scales_vs_train_mode_reference(golden):
    g = golden("mit_b0_droppath")
    outs, grads = _droppath_run(g, g.t("scales"))
    for i, o in enumerate(outs):
        want = g.t(f"c{i + 1}")
        assert tuple(o.shape) == tuple(want.shape)
        assert float((o - want).abs().max()) < 2e-5 * float(want.abs().max()), i
    keys = g["keys"].tolist()
    norms = np.array([float(grads[k].norm()) for k in keys])
    assert np.allclose(norms, g["grad_norms"], rtol=2e-4, atol=1e-7)
    zero = [k for k, n in zip(keys, g["grad_norms"]) if n == 0.0]
    assert sorted(zero) == sorted(k for k in keys if k.startswith(("block2.1.attn.", "block2.1.norm1.")))
    for name, (want, step) in _droppath_samples(g).items():
        got = grads[name].reshape(-1)[::step]
        assert float((got - want).abs().max()) < 1e-4 * float(want.abs().max()) + 1e-7, name


@pytest.mark.parametrize("wrong", ["branches_swapped", "images_0_1_swapped", "stage2_shifted_one_block"])
def test_droppath_capture_separates_wrong_masks(golden, wrong):
    """The capture must tell a mis-wired mask from the right one by a wide margin, or the GPU comparison against it (bounds MIT_TOL,
    tests/test_gpu_mit_droppath.py) could pass by accident: each wrong mask misses some stage output by >= 10 x MIT_TOL["features"]
    and some stored gradient sample by >= 10 x MIT_TOL["grad_sample"], in the metric of those tests."""
    from test_gpu_mit import MIT_TOL, _rel
    g = golden("mit_b0_droppath")
    s = g.t("scales").clone()
    if wrong == "branches_swapped":
        s = s.flip(1)
    elif wrong == "images_0_1_swapped":
        s = s[:, :, [1, 0, 2]]
    else:
        s[2:4] = s[2:4].flip(0)
    assert not torch.equal(s, g.t("scales"))
    outs, grads = _droppath_run(g, s)
    e_feat = max(_rel(o, g.t(f"c{i + 1}")) for i, o in enumerate(outs))
    e_grad = max(_rel(grads[name].reshape(-1)[::step], want) for name, (want, step) in _droppath_samples(g).items()
                 if float(want.abs().max()) > 0)
    print(f"wrong mask [{wrong}]: features miss by {e_feat:.2e}, gradient samples by {e_grad:.2e}")
    assert e_feat >= 10 * MIT_TOL["features"]
    assert e_grad >= 10 * MIT_TOL["grad_sample"]


@pytest.mark.timeout(600)
def test_mit_b1_benchmark_geometry_vs_reference(golden):
    g = golden("mit768")
    x = torch.rand((1, 3, 768, 768), generator=synth.gen(int(g["seed"]))) * 2 - 1
    with torch.no_grad():
        outs = om.forward(om.state_dict(om.MIT_B1), x, om.MIT_B1)
    assert [tuple(o.shape) for o in outs] == [(1, 64, 192, 192), (1, 128, 96, 96), (1, 320, 48, 48), (1, 512, 24, 24)]
    for o, key, step, mx in zip(outs, ("c1_sample", "c2_sample", "c3_sample", "c4_sample"), (211, 53, 7, 3), g["maxs"]):
        assert float((o.reshape(-1)[::step] - g.t(key)).abs().max()) < 2e-5 * float(mx)
    assert np.allclose([float(o.abs().sum()) for o in outs], g["sums"], rtol=1e-5)


@pytest.mark.timeout(900)
def test_mit_b5_benchmark_geometry_vs_reference(golden):
    g = golden("mit768")
    x = torch.rand((1, 3, 768, 768), generator=synth.gen(int(g["seed"]))) * 2 - 1
    with torch.no_grad():
        outs = om.forward(om.state_dict(om.MIT_B5), x, om.MIT_B5)
    for o, key, step, mx in zip(outs, ("b5_c1_sample", "b5_c2_sample", "b5_c3_sample", "b5_c4_sample"), (211, 53, 7, 3), g["b5_maxs"]):
        assert float((o.reshape(-1)[::step] - g.t(key)).abs().max()) < 3e-5 * float(mx)
    assert np.allclose([float(o.abs().sum()) for o in outs], g["b5_sums"], rtol=1e-5)
