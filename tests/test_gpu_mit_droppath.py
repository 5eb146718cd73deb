"""DropPath (stochastic depth) of the MiT encoder in train(), held to references: the capture of the REFERENCE mit_b0 in train() with
GIVEN masks (tests/golden/mit_b0_droppath.npz, tools/gen_golden.py::gen_mit_droppath) and the oracle with the same masks
(oracle/mit.py, `drop_scales`; float64).  Covers the [blocks][2][B] layout of `_drop_path_scales`, its per-stage split, the order of
the two branches, the `seg` / `rows_per_seg` arguments of both residual GEMM epilogues, `row_scale` in front of both branch backward
passes, and the gradients of branches that some or all images dropped.  tests/test_mit_oracle.py shows that the capture tells a
swapped branch, swapped images and a mask shifted by one block from the right wiring by > 200 x MIT_TOL.

Masks reach the model by replacing `_drop_path_scales` on the instance (one test records a real draw instead).  Bounds: MIT_TOL of
tests/test_gpu_mit.py, unchanged -- same operands as in eval(), the scales (<= 1.43) are applied in fp32.  Every buffer the stage
functions allocate for a kernel to write (`_Ops.empty`) and every workspace is filled with 0xFF bytes (NaN) first.
Measured on the MI355X: DESIGN.md section 9b."""
import numpy as np
import pytest
import torch

from oracle import mit as om
from oracle import synth
from test_gpu_mit import MIT_TOL, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
B0 = om.MitArch(embed_dims=(32, 64, 160, 256), depths=(2, 2, 2, 2))
ARCH = {"mit_b0": B0, "mit_b1": om.MIT_B1}


def _poison_allocations(monkeypatch):
    from diga_amd import _lib
    from diga_amd.model.networks import MixTransfomer as M
    real_ws = _lib.workspace

    def empty(self, shape, dtype=torch.float16):
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        t.view(torch.uint8).fill_(0xFF)
        return t

    def workspace(nbytes, device, tag="default"):
        buf = real_ws(nbytes, device, tag)
        buf.fill_(0xFF)
        return buf

    monkeypatch.setattr(M._Ops, "empty", empty)
    monkeypatch.setattr(_lib, "workspace", workspace)


@pytest.fixture(autouse=True)
def poisoned_buffers(monkeypatch):
    _poison_allocations(monkeypatch)


def _model(name="mit_b0"):
    from diga_amd.model.networks import MixTransfomer as M
    m = getattr(M, name)()
    m.load_state_dict(om.state_dict(ARCH[name]))
    return m.to(DEV)


def _inject(m, scales):
    """`scales` [8][2][B] (encoder order) -> what `_drop_path_scales` returns from now on: one [depth][2][B] tensor per stage."""
    per_stage = list(scales.to(DEV, torch.float32).split(list(m.depths)))
    object.__setattr__(m, "_drop_path_scales", lambda cfg, B, dev: per_stage)


def _scales(dropped, B):
    """Hand-chosen masks -> [8][2][B] scales, 0 or 1 / keep with keep = 1 - linspace(0, 0.3, 8)[block] (gen_mit_droppath's rule)."""
    keep = 1.0 - torch.linspace(0, 0.3, 8)
    s = (1.0 / keep).view(8, 1, 1).expand(8, 2, B).clone()
    for b, pair in enumerate(dropped):
        for r, imgs in enumerate(pair):
            for i in imgs:
                s[b, r, i] = 0.0
    return s


def _run(m, x, probes):
    m.zero_grad(set_to_none=True)
    outs = m(x.to(DEV))
    sum((o * p.to(DEV)).sum() for o, p in zip(outs, probes)).backward()
    torch.cuda.synchronize()
    return [o.detach() for o in outs], {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _oracle(arch, x, probes, scales):
    sd = {k: v.double().requires_grad_() for k, v in om.state_dict(arch).items()}
    outs = om.forward(sd, x.double(), arch, drop_scales=list(scales.double().cpu().split(list(arch.depths))))
    sum((o * p.double()).sum() for o, p in zip(outs, probes)).backward()
    return [o.detach() for o in outs], {k: v.grad for k, v in sd.items()}


def _compare_with_oracle(what, outs, grads, want_outs, want_grads):
    e_feat = max(_rel(o, w) for o, w in zip(outs, want_outs))
    e_grad, ratios, dead = {}, {}, []
    for k, w in want_grads.items():
        if float(w.abs().max()) == 0.0:                               # a branch every image dropped: exactly zero, not small
            assert bool((grads[k] == 0).all()), k
            dead.append(k)
            continue
        e_grad[k] = _rel(grads[k], w)
        ratios[k] = float(grads[k].double().norm()) / float(w.norm())
    print(f"{what}: features max err {max(e_feat, 0):.2e} of scale, full gradients {max(e_grad.values()):.2e}, gradient-norm ratios "
          f"{min(ratios.values()):.4f} .. {max(ratios.values()):.4f}; {len(dead)} parameters with an exactly zero gradient")
    assert e_feat < MIT_TOL["features"]
    assert max(e_grad.values()) < MIT_TOL["grad_sample"], sorted(e_grad.items(), key=lambda kv: -kv[1])[:5]
    bad = [(k, r) for k, r in ratios.items() if abs(r - 1.0) > MIT_TOL["grad_norm"]]
    assert not bad, bad[:10]
    return dead


# ---------------------------------------------------------------------------------------------- mit_b0 against the train-mode capture
@pytest.fixture(scope="module")
def capture_run(golden):
    """ONE forward + backward of mit_b0 in train() on the capture's input, masks and probes, shared by the tests below (read-only)."""
    g = golden("mit_b0_droppath")
    m = _model().train()
    _inject(m, g.t("scales"))
    probes = [g.t(f"probe{i + 1}") for i in range(4)]
    with pytest.MonkeyPatch.context() as mp:                       # (set up before the function-scoped poisoning of the first test)
        _poison_allocations(mp)
        outs, grads = _run(m, g.t("x"), probes)
    return g, m, probes, outs, grads


def test_mit_b0_train_mode_vs_reference_capture(capture_run):
    g, m, probes, outs, grads = capture_run
    worst = 0.0
    for i, o in enumerate(outs):
        want = g.t(f"c{i + 1}")
        assert tuple(o.shape) == tuple(want.shape)
        worst = max(worst, _rel(o, want))
    keys = g["keys"].tolist()
    ratio, dead = {}, []
    for k, want in zip(keys, g["grad_norms"]):
        if want == 0.0:
            assert float(grads[k].norm()) == 0.0, k
            dead.append(k)
        else:
            ratio[k] = float(grads[k].norm()) / float(want)
    gerr = {}
    for k in [n[2:] for n in g if n.startswith("g_")]:
        name = [n for n in keys if n.replace(".", "_") == k][0]
        want = g.t("g_" + k)
        got = grads[name].reshape(-1)[::int(g["gstep_" + k])]
        if float(want.abs().max()) == 0.0:
            assert bool((got == 0).all()), name
        else:
            gerr[name] = _rel(got, want)
    print(f"mit_b0 train() with given DropPath masks vs reference: features max err {worst:.2e} of scale, sampled gradients "
          f"{max(gerr.values()):.2e}, gradient-norm ratios {min(ratio.values()):.4f} .. {max(ratio.values()):.4f}, {len(dead)} parameters "
          f"with zero gradient")
    assert worst < MIT_TOL["features"]
    bad = [(k, r) for k, r in ratio.items() if abs(r - 1.0) > MIT_TOL["grad_norm"]]
    assert not bad, bad[:10]
    assert max(gerr.values()) < MIT_TOL["grad_sample"], sorted(gerr.items(), key=lambda kv: -kv[1])[:5]


def test_branch_dropped_for_all_images_has_exactly_zero_gradients(capture_run):
    g, m, probes, outs, grads = capture_run
    assert bool((g.t("scales")[3, 0] == 0).all())                              # block2.1, attention
    names = [k for k in grads if k.startswith(("block2.1.attn.", "block2.1.norm1."))]
    assert sorted(n[len("block2.1."):] for n in names) == sorted(
        f"{mod}.{wb}" for mod in ("attn.q", "attn.kv", "attn.proj", "attn.sr", "attn.norm", "norm1") for wb in ("weight", "bias"))
    for k in names:
        assert bool((grads[k] == 0).all()), k
    # ... and its Mix-FFN branch, dropped for image 2 only, and the neighbouring blocks are alive
    for k in ("block2.1.mlp.fc1.weight", "block2.1.mlp.fc2.bias", "block2.1.norm2.weight", "block2.0.attn.proj.weight", "block3.0.attn.q.weight"):
        assert float(grads[k].abs().max()) > 0, k


def test_image_with_a_whole_stage_dropped_equals_the_stage_dropped_for_all(capture_run):
    """Image 2 loses both branches of both blocks of stage 3: its rows of c3 (and of c4 behind it) must be, bit for bit, those of a run
    in which stage 3 is dropped for every image -- the scale 0 must erase the branch, bias included, whatever the other images do."""
    g, m, probes, outs, grads = capture_run
    s = g.t("scales").clone()
    assert bool((s[4:6, :, 2] == 0).all()) and bool((s[4:6, :, :2] != 0).any())
    s[4:6] = 0.0
    m2 = _model().train()
    _inject(m2, s)
    with torch.no_grad():
        outs2 = m2(g.t("x").to(DEV))
    for i in (2, 3):
        assert torch.equal(outs[i][2], outs2[i][2]), f"c{i + 1}"
        assert not torch.equal(outs[i][0], outs2[i][0])
    for i in (0, 1):
        assert torch.equal(outs[i], outs2[i])


def test_all_ones_scales_in_train_mode_equal_eval_bit_for_bit(golden):
    g = golden("mit_b0_droppath")
    probes = [g.t(f"probe{i + 1}") for i in range(4)]
    m = _model().eval()
    outs_e, grads_e = _run(m, g.t("x"), probes)
    m.train()
    _inject(m, torch.ones((8, 2, 3)))
    outs_t, grads_t = _run(m, g.t("x"), probes)
    for i, (a, b) in enumerate(zip(outs_t, outs_e)):
        assert torch.equal(a, b), f"c{i + 1}"
    differ = [k for k in grads_e if not torch.equal(grads_t[k], grads_e[k])]
    assert not differ, differ[:5]


def test_no_grad_train_mode_forward_equals_the_grad_enabled_one(capture_run):
    """The path the EMA teacher takes in train() under no_grad (need_grad False: nothing saved, no statistics kept)."""
    g, m, probes, outs, grads = capture_run
    with torch.no_grad():
        outs2 = m(g.t("x").to(DEV))
    for i, (a, b) in enumerate(zip(outs2, outs)):
        assert torch.equal(a, b), f"c{i + 1}"


# ---------------------------------------------------------------------------------------------- mit_b1 (head_dim 64) against the oracle
# DROPPED[block][branch] = images; contains: a branch dropped for both images (block2.1 Mix-FFN, block3.1 attention), a branch dropped
# for one image only in every stage, image 1 with the whole of stage 2 dropped, attention dropped / Mix-FFN kept for one image
# (block1.1, image 0) and the reverse (block3.0, image 1); block1.0 has rate 0
B1_DROPPED = [[(), ()], [(0,), ()], [(1,), (1,)], [(1,), (0, 1)], [(), (1,)], [(0, 1), ()], [(), (0,)], [(1,), ()]]


def test_mit_b1_train_mode_vs_oracle_with_the_same_masks():
    g = synth.gen(64096)
    x = torch.rand((2, 3, 64, 96), generator=g) * 2 - 1
    scales = _scales(B1_DROPPED, 2)
    m = _model("mit_b1").train()
    _inject(m, scales)
    with torch.no_grad():
        shapes = [tuple(o.shape) for o in m(x.to(DEV))]
    assert shapes == [(2, 64, 16, 24), (2, 128, 8, 12), (2, 320, 4, 6), (2, 512, 2, 3)]
    probes = [torch.randn(s, generator=g) for s in shapes]
    outs, grads = _run(m, x, probes)
    want_outs, want_grads = _oracle(om.MIT_B1, x, probes, scales)
    dead = _compare_with_oracle("mit_b1 train() with given DropPath masks vs float64 oracle", outs, grads, want_outs, want_grads)
    assert sorted(dead) == sorted(k for k in grads if k.startswith(("block2.1.mlp.", "block2.1.norm2.", "block3.1.attn.", "block3.1.norm1.")))


# ---------------------------------------------------------------------------------------------- a real draw
def test_drawn_masks_reach_the_kernels_as_drawn():
    """`_drop_path_scales` itself under torch.manual_seed at rate 0.5, recorded on its way to the stage functions: forward and backward
    against the oracle fed the recorded scales -- the wiring from the draw to the kernels, not only from injected masks."""
    m = _model().train()
    m.reset_drop_path(0.5)
    seen = []
    real = m._drop_path_scales

    def recording(cfg, B, dev):
        out = real(cfg, B, dev)
        seen.append([None if s is None else s.detach().clone() for s in out])
        return out

    object.__setattr__(m, "_drop_path_scales", recording)
    g = synth.gen(505)
    x = torch.rand((4, 3, 64, 64), generator=g) * 2 - 1
    shapes = [(4, 32, 16, 16), (4, 64, 8, 8), (4, 160, 4, 4), (4, 256, 2, 2)]
    probes = [torch.randn(s, generator=g) for s in shapes]
    torch.manual_seed(77)
    outs, grads = _run(m, x, probes)
    assert len(seen) == 1 and [tuple(s.shape) for s in seen[0]] == [(2, 2, 4)] * 4
    scales = torch.cat(seen[0], 0).cpu()
    keep = torch.tensor([1.0 - v.item() for v in torch.linspace(0, 0.5, 8)])
    assert bool(((scales == 0) | (scales == (1.0 / keep).view(8, 1, 1))).all())
    dropped = int((scales == 0).sum())
    assert 8 <= dropped <= 32, dropped                                  # (expected 16 of 64 at these rates; the seed is fixed)
    want_outs, want_grads = _oracle(B0, x, probes, scales)
    _compare_with_oracle(f"mit_b0 train() with a real draw at rate 0.5 ({dropped} of 64 dropped) vs float64 oracle", outs, grads, want_outs,
                         want_grads)
    assert np.isfinite([float(v.abs().max()) for v in grads.values()]).all()
