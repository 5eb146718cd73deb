"""The four MiT helper entry points that only round once and add nothing -- diga_mit_row_scale, diga_mit_cast_scale,
diga_mit_cast_transpose, diga_mit_weight_prep_multi -- held EXACTLY (torch.equal) to torch's own IEEE conversions on the CPU:
fp32 product, one round-to-nearest-even to fp16, subnormals kept, overflow to +-inf.

Every output buffer is filled with 0xFF bytes (NaN in fp16 and fp32) before the launch, so an element the kernel does not write
fails the comparison.  Shapes: the smallest that reach every path -- a short last segment, one 16-byte group per row, the 32x32
transpose tiles' ragged edges, the zero padding of K up to Kp, the first and the last tile of every tensor of a prep table, and the
two element counts that cross the 8192-block grid cap of the bandwidth kernels (their grid-stride loop takes a second turn;
MiT-B0 stage 1 at 16 crops of 768x768 is 18.9 M elements)."""
import ctypes

import pytest
import torch

from oracle import mit as om
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
B0 = om.MitArch(embed_dims=(32, 64, 160, 256), depths=(2, 2, 2, 2))
GRID_CAP_ITEMS = 8192 * 256                                        # blocks x threads of the capped grid (mit_ops.hip, grid_for)


def _lib():
    from diga_amd import _lib
    return _lib


def _poison(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0xFF)
    return t


def _is_poison(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def _same(got, want):
    """Bitwise equality of two tensors of one dtype (torch.equal calls NaN unequal and +0 == -0: compare the bytes)."""
    return got.dtype == want.dtype and got.shape == want.shape and got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


# fp16 edge values: zero, the smallest subnormal, the largest subnormal, the smallest normal, +-65504, a value whose double overflows
_F16_EDGES = [0.0, 2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 65504.0, -65504.0, 40000.0, -33000.0, 1.0]


# ---------------------------------------------------------------------------------------------- row_scale
@pytest.mark.parametrize("m,c,rps", [(37, 8, 5), (1000, 32, 1), (300, 160, 300), (65540, 256, 9363)])
def test_row_scale_is_the_fp32_product_rounded_once(m, c, rps):
    lib = _lib()
    P = lib.ptr
    x, seg, want = _row_scale_case(m, c, rps)
    xd, segd = x.to(DEV), seg.to(DEV)
    y = _poison((m, c), torch.float16)
    lib.call("diga_mit_row_scale", P(xd), P(y), P(segd), rps, m, c, lib.stream())
    assert torch.equal(y.cpu(), want)
    assert _same(y.cpu(), want), "signed zeros"


def _row_scale_case(m, c, rps):
    if m == 65540:
        assert m * c // 8 > GRID_CAP_ITEMS
    g = synth.gen(m + c + rps)
    x = torch.randn((m, c), generator=g).half()
    edges = torch.tensor(_F16_EDGES, dtype=torch.float16)
    flat = x.view(-1)
    at = torch.randperm(flat.numel(), generator=g)[: 8 * edges.numel()]
    flat[at] = edges.repeat(8)                                     # edge values in random places: under every kind of scale
    flat[-edges.numel():] = edges                                  # ... and in the last rows (the short last segment)
    nseg = (m + rps - 1) // rps
    seg = torch.tensor([1.0 / 0.7, 0.0, 2.0, 1.0, 1.0 / 0.9, 0.5])[torch.arange(nseg) % 6]
    want = (x.float() * seg[torch.arange(m) // rps, None]).half()
    assert bool(torch.isinf(want).any()) and bool(((want != 0) & (want.float().abs() < 2.0 ** -14)).any())
    return x, seg, want


def test_row_scale_refuses_rows_that_are_no_multiple_of_8():
    lib = _lib()
    P = lib.ptr
    x = torch.ones((16, 12), dtype=torch.float16, device=DEV)
    seg = torch.ones(16, device=DEV)
    y = _poison((16, 12), torch.float16)
    rc = lib.lib.diga_mit_row_scale(P(x), P(y), P(seg), 1, 16, 12, lib.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert _is_poison(y)


# ---------------------------------------------------------------------------------------------- cast_scale
@pytest.mark.parametrize("scale", [1.0, 1024.0, 1.0 / 0.7])
@pytest.mark.parametrize("n", [4, 1000, 8388612])
def test_cast_scale_is_the_fp32_product_rounded_once(n, scale):
    lib = _lib()
    P = lib.ptr
    if n == 8388612:
        assert n // 4 > GRID_CAP_ITEMS
    g = synth.gen(n)
    x = torch.randn(n, generator=g)
    # exact ties of the fp16 grid (odd multiples of half an ulp, normal and subnormal: they round to even), values that round to +-inf
    # (>= 65520) and values just below, fp16 subnormals; all divided by the scale so that the PRODUCT lands on them (exactly for the
    # powers of two, next to them otherwise)
    special = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(2.0 + 2.0 ** -10), 2.0 ** -25, 3 * 2.0 ** -25, -5 * 2.0 ** -25,
                            1023.5 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -26, 65504.0, 65519.996, 65520.0, -65520.0, 70000.0, -1e30, 1e-30,
                            0.0, -0.0]) / scale
    if n >= special.numel():
        at = torch.randperm(n, generator=g)[: special.numel()]
        x[at] = special
        x[-special.numel():] = special                             # ... and in the tail, which the second grid-stride turn writes
    else:
        x[:] = special[[0, 3, 11, 13]]
    want = (x * scale).half()
    if n >= special.numel():
        assert bool(torch.isinf(want).any()) and bool(((want != 0) & (want.float().abs() < 2.0 ** -14)).any())
    xd = x.to(DEV)
    y = _poison((n,), torch.float16)
    lib.call("diga_mit_cast_scale", P(xd), P(y), n, scale, lib.stream())
    assert _same(y.cpu(), want)


def test_cast_scale_refuses_a_length_that_is_no_multiple_of_4():
    lib = _lib()
    P = lib.ptr
    x = torch.ones(10, device=DEV)
    y = _poison((10,), torch.float16)
    rc = lib.lib.diga_mit_cast_scale(P(x), P(y), 10, 1.0, lib.stream())
    torch.cuda.synchronize()
    assert rc != 0 and "4" in lib.last_error()
    assert _is_poison(y)


# ---------------------------------------------------------------------------------------------- cast_transpose
@pytest.mark.parametrize("outputs", ["both", "w16", "wt16"])
@pytest.mark.parametrize("r,c", [(1, 1), (33, 31), (64, 160), (19, 256), (160, 147)])
def test_cast_transpose_equals_half_and_its_transpose(r, c, outputs):
    lib = _lib()
    P = lib.ptr
    g = synth.gen(1000 * r + c)
    w = torch.randn((r, c), generator=g)
    w.view(-1)[:: 7] *= 2.0 ** -16                                   # some fp16 subnormals
    w.view(-1)[-1] = 1.0 + 2.0 ** -11                                # a tie in the last element
    w.view(-1)[0] = 1e6                                              # rounds to inf
    wd = w.to(DEV)
    w16 = _poison((r, c), torch.float16) if outputs != "wt16" else None
    wt16 = _poison((c, r), torch.float16) if outputs != "w16" else None
    lib.call("diga_mit_cast_transpose", P(wd), P(w16), P(wt16), r, c, lib.stream())
    if w16 is not None:
        assert _same(w16.cpu(), w.half())
    if wt16 is not None:
        assert _same(wt16.cpu(), w.half().t().contiguous())


# ---------------------------------------------------------------------------------------------- weight_prep_multi, hand-built tables
def _prep_reference(w, kp, mode):
    """Plain indexing of the GEMM form rows[co][k], k = tap * Ci + ci, of a [Co][Ci][RS] fp32 tensor."""
    co, ci, rs = w.shape
    if mode == 1:
        a = torch.empty((rs, co))
        for tap in range(rs):
            a[tap] = w[:, 0, tap]
        return a, a.flip(0).contiguous()
    rows = torch.zeros((co, kp))
    for tap in range(rs):
        for i in range(ci):
            rows[:, tap * ci + i] = w[:, i, tap]
    return rows.half(), rows.half().t().contiguous()


PREP_SHAPES = {"conv3x3_ragged": (33, 5, 9, 64, 0), "one_row": (1, 32, 1, 32, 0), "depthwise": (40, 1, 9, 9, 1), "stem7x7": (96, 3, 49, 160, 0)}
PREP_TABLES = [["conv3x3_ragged"], ["one_row"], ["depthwise"], ["stem7x7"],
               ["one_row", "stem7x7"], ["depthwise", "one_row"],
               ["one_row", "conv3x3_ragged", "depthwise", "stem7x7", "one_row", "depthwise", "conv3x3_ragged"]]


@pytest.mark.parametrize("names", PREP_TABLES, ids=["+".join(t) for t in PREP_TABLES])
def test_weight_prep_multi_on_hand_built_tables(names):
    """n_tensors = 1, 2 and 7; the one-tile tensors put tensor boundaries on consecutive tiles, so the per-block binary search over the
    tile-prefix array is exercised on the first and on the last tile of every tensor."""
    lib = _lib()
    P = lib.ptr
    g = synth.gen(len(names) * 17 + len(names[0]))
    srcs, outs, entries, starts, total = [], [], [], [], 0
    for nm in names:
        co, ci, rs, kp, mode = PREP_SHAPES[nm]
        w = torch.randn((co, ci, rs), generator=g)
        w.view(-1)[::5] *= 2.0 ** -16
        wd = w.to(DEV)
        dt = torch.float16 if mode == 0 else torch.float32
        a = _poison((co, kp) if mode == 0 else (rs, co), dt)
        b = _poison((kp, co) if mode == 0 else (rs, co), dt)
        tiles_k = (kp + 31) // 32
        entries.append(lib.MitWeightPrep(wd.data_ptr(), a.data_ptr(), b.data_ptr(), co, ci, rs, kp, mode, tiles_k))
        starts.append(total)
        total += ((co + 31) // 32) * tiles_k
        srcs.append((w, wd))
        outs.append((a, b))
    arr = (lib.MitWeightPrep * len(entries))(*entries)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    ts = torch.tensor(starts, dtype=torch.int64).to(DEV)
    assert tab.numel() == len(names) * ctypes.sizeof(lib.MitWeightPrep)
    lib.call("diga_mit_weight_prep_multi", P(tab), P(ts), len(names), total, lib.stream())
    for i, nm in enumerate(names):
        co, ci, rs, kp, mode = PREP_SHAPES[nm]
        want_a, want_b = _prep_reference(srcs[i][0], kp, mode)
        assert _same(outs[i][0].cpu(), want_a), (i, nm, "a")
        assert _same(outs[i][1].cpu(), want_b), (i, nm, "b")


# ---------------------------------------------------------------------------------------------- weight_prep_multi on the real model
def _prep_expected(m):
    from diga_amd.model.networks.MixTransfomer import _conv16, _lin16
    want = {}
    for n, p in m.named_parameters():
        if p.dim() == 2:
            want[n] = _lin16(p.detach(), True)
        elif p.dim() == 4 and n.endswith("dwconv.dwconv.weight"):
            a = p.detach().reshape(p.shape[0], 9).t().contiguous()
            want[n] = (a, a.flip(0).contiguous())
        elif p.dim() == 4:
            want[n] = _conv16(p.detach(), True)[:2]
    return want


def _prep_check(m, got):
    want = _prep_expected(m)
    assert sorted(want) == sorted(got)
    for n, (a, b) in want.items():
        assert _same(got[n][0], a), (n, "a")
        assert _same(got[n][1], b), (n, "b")
    return want


def test_weight_prep_multi_on_mit_b0_rewrites_every_element_per_forward():
    from diga_amd.model.networks import MixTransfomer as M
    m = M.mit_b0()
    m.load_state_dict(om.state_dict(B0))
    m = m.to(DEV)
    got = m._prepare_weights()
    want = _prep_check(m, got)
    assert len(want) == 4 + 3 * 2 + 8 * 6                            # patch embeddings, sr convs, 6 weights per block
    a, b, kp = got["patch_embed1.proj.weight"]
    assert kp == 160 and tuple(a.shape) == (32, 160) and tuple(b.shape) == (160, 32)
    assert bool((a[:, 147:] == 0).all()) and bool((b[147:] == 0).all())
    assert bool((a[:, :147] != 0).any(0).all())
    # the buffers are persistent and rewritten in full by every forward's launch: padding included
    for a, b, _ in got.values():
        a.view(torch.uint8).fill_(0xFF)
        b.view(torch.uint8).fill_(0xFF)
    again = m._prepare_weights()
    assert all(again[n][0].data_ptr() == got[n][0].data_ptr() and again[n][1].data_ptr() == got[n][1].data_ptr() for n in got)
    _prep_check(m, again)
    # ... and they follow the master parameters (an optimizer step writes them in place)
    named = dict(m.named_parameters())
    moved = ("patch_embed1.proj.weight", "block2.1.mlp.dwconv.dwconv.weight", "block4.1.attn.kv.weight")
    before = {n: again[n][0].clone() for n in moved}
    for n in moved:
        named[n].data.mul_(1.5)
    third = m._prepare_weights()
    _prep_check(m, third)
    for n in moved:
        assert not torch.equal(third[n][0], before[n]), n
