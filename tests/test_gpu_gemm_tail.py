"""Row tails of gemm_f32_persistent_kernel: wave pieces that hold nothing but padding skip their MFMAs, and the drain is specialised on
<statistics, bias>.  Neither may change a bit of what the kernel writes.

1. Pointwise layers through diga_conv2d_nhwc_f32 with a last row tile of 16 / 64 / 65 / 128 / 129 / 192 valid rows, K = 32 and 64 (one
   and two K-steps per tile), with and without a statistics buffer and a bias:
     * the output equals, bit for bit, the same rows computed in pieces of fewer than 512 tiles -- those run, by the library's shape
       rule, on the per-tile kernel (conv_fwd_kernel, one block per tile), which takes K in the same order;
     * the output against the float64 product at test_gpu_conv.py's bound for 1x1 layers (rtol 1e-5, atol 2e-6 of the output's scale);
     * the statistics records {sum (y - s), sum (y - s)^2, s} per 64-row chunk and column equal, bit for bit, those formed from the
       per-tile kernel's output by the record's definition (include/diga_hip.h; the order of the 32 rows a lane half adds up is the
       accumulator layout of the 32x32 MFMA).  The per-tile kernel's own records cover 128-row chunks and cannot be compared
       directly.
2. Winograd products through diga_conv2d_winograd_f32 (forward and the flipped-tap backward-data form) whose second row tile holds
   33 valid rows: bit-identical to the same layer computed for halves of its output channels (256 tiles per launch: the per-tile
   kernel), and against float64 at the bound of the F(6x6) path (conftest.WINO_TOL)."""
import functools

import pytest
import torch

from conftest import WINO_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUT = 128
PIECE = 511 * 256          # rows of a launch that stays below pointwise_persistent_ok's 512 tiles


def _pointwise(a, w, bias, stats):
    """[M][K] rows as M images of one pixel (the kernels pack a pixel's image coordinates into 16 bits each)."""
    from diga_amd import _lib
    m, k = a.shape
    cout = w.shape[0]
    out = torch.empty((m, cout), dtype=torch.float32, device=a.device)
    _lib.call("diga_conv2d_nhwc_f32", _lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), m, 1, 1, k, k, 1, 1, cout, cout, 1, 1,
              1, 1, 0, 0, 1, 1, _lib.ptr(stats), _lib.PROF_TAGS.index("conv_fwd"), _lib.stream())
    return out


@functools.lru_cache(maxsize=2)
def _reference(m, k):
    """Inputs, the per-tile kernel's output (with and without bias) and the float64 product, once per shape."""
    from diga_amd import _lib
    assert _lib.get_conv_math() == 0
    g = torch.Generator().manual_seed(1000 * k + m % 997)
    a = (torch.randn((m, k), generator=g) + 0.25).to(DEV)
    w = (torch.randn((COUT, k), generator=g) * (2.0 / k) ** 0.5).to(DEV)
    bias = torch.randn(COUT, generator=g).to(DEV)
    per_tile = {}
    for with_bias in (False, True):
        b = bias if with_bias else None
        per_tile[with_bias] = torch.cat([_pointwise(a[r0:r0 + PIECE], w, b, None) for r0 in range(0, m, PIECE)])
    y64 = a.double() @ w.double().t()
    return a, w, bias, per_tile, y64


def _records_from(y):
    """[ceil(M / 64)][3][C] records as include/diga_hip.h defines them, from an output y [M][C]: per 64-row chunk s = its first row; each
    lane half lh adds up d = y - s and d * d over its rows 32 i + (e & 3) + 8 (e >> 2) + 4 lh (i = 0, 1; e = 0 .. 15) in that order,
    starting from 0; the two halves are added.  Rows beyond M are left out.  Plain fp32 operations, one rounding each."""
    m, c = y.shape
    nch = -(-m // 64)
    yp = torch.zeros((nch * 64, c), dtype=torch.float32, device=y.device)
    yp[:m] = y
    yp = yp.view(nch, 64, c)
    valid = (torch.arange(nch * 64, device=y.device) < m).view(nch, 64, 1)
    s = yp[:, 0, :]
    halves = []
    for lh in (0, 1):
        sd = torch.zeros((nch, c), dtype=torch.float32, device=y.device)
        sd2 = torch.zeros_like(sd)
        for i in (0, 1):
            for e in range(16):
                r = 32 * i + (e & 3) + 8 * (e >> 2) + 4 * lh
                d = yp[:, r, :] - s
                dd = d * d
                sd = torch.where(valid[:, r, :], sd + d, sd)
                sd2 = torch.where(valid[:, r, :], sd2 + dd, sd2)
        halves.append((sd, sd2))
    return torch.stack([halves[0][0] + halves[1][0], halves[0][1] + halves[1][1], s], dim=1)


# tiles per XCD = 64 + {0, 1, 16, 17, 31}: no last round, a last round of at most 16 tiles at both ends of that range, a longer one at both
# ends; the last row tile holds 16 rows.  Then one case each with 64, 65, 128, 129 and 192 rows in it.
SHAPES = [(256 * n - 240, k) for n in (512, 520, 640, 648, 760) for k in (32, 64)] + \
         [(256 * 519 + rows, 64) for rows in (64, 65, 128, 129, 192)]


@pytest.mark.parametrize("m,k", SHAPES, ids=[f"M{m}_K{k}" for m, k in SHAPES])
def test_pointwise_row_tail_bit_identical_to_per_tile_kernel(m, k):
    from diga_amd import _lib
    assert -(-m // 256) >= 512                                    # the persistent kernel's shape rule (COUT = 128: one column tile)
    assert _lib.lib.diga_conv2d_stats_chunk_rows(m, 1, 1, k, 1, 1, COUT, 1, 1, 1, 1, 0, 0, 0) == 64
    a, w, bias, per_tile, y64 = _reference(m, k)
    nch = -(-m // 64)
    for with_bias in (False, True):
        want = per_tile[with_bias]
        want64 = y64 + bias.double() if with_bias else y64
        scale = float(want64.abs().max())
        want_rec = _records_from(want)
        for with_stats in (False, True):
            stats = None
            if with_stats:
                stats = torch.full((_lib.lib.diga_conv2d_stats_floats(m, 1, 1, COUT),), float("nan"), dtype=torch.float32, device=DEV)
            got = _pointwise(a, w, bias if with_bias else None, stats)
            what = (m, k, "bias" if with_bias else "no bias", "stats" if with_stats else "no stats")
            assert torch.equal(got, want), what
            err = (got.double() - want64).abs()
            assert bool((err <= 2e-6 * scale + 1e-5 * want64.abs()).all()), (what, float(err.max()), scale)
            if with_stats:
                assert torch.equal(stats[:nch * 3 * COUT].view(nch, 3, COUT), want_rec), what


def _winograd(x, w_krsc, flip, tile, d):
    """x [N,H,W,Cin], w_krsc [Cout,3,3,Cin] -> [N,H,W,Cout] through diga_conv2d_winograd_f32."""
    from diga_amd import _lib
    n, h, wd, cin = x.shape
    cout = w_krsc.shape[0]
    out = torch.empty((n, h, wd, cout), dtype=torch.float32, device=x.device)
    ws = torch.empty(_lib.lib.diga_conv2d_winograd_workspace_bytes(n, h, wd, cin, cout, d, tile), dtype=torch.uint8, device=x.device)
    _lib.call("diga_conv2d_winograd_f32", _lib.ptr(x), _lib.ptr(w_krsc), None, _lib.ptr(out), _lib.ptr(ws), ws.numel(), n, h, wd, cin,
              cin, cout, cout, d, tile, flip, None, None, _lib.PROF_TAGS.index("conv_bwd_data" if flip else "conv_fwd"), _lib.stream())
    return out


def _conv3x3_f64(x, w_krsc, d, flip):
    """out[y, x, k] = sum_{r, s, c} in[y + (r - 1) d, x + (s - 1) d, c] * w[k][r][s][c] (taps reversed with flip), in float64."""
    n, h, wd, cin = x.shape
    xp = torch.zeros((n, h + 2 * d, wd + 2 * d, cin), dtype=torch.float64, device=x.device)
    xp[:, d:d + h, d:d + wd] = x.double()
    out = torch.zeros((n, h, wd, w_krsc.shape[0]), dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            wt = w_krsc[:, 2 - r, 2 - s] if flip else w_krsc[:, r, s]
            out += xp[:, r * d:r * d + h, s * d:s * d + wd] @ wt.double().t()
    return out


# name, H = W, Cin, Cout, dilation: one image, F(6x6): 17 x 17 = 289 tiles -> 512 rows per product, the second row tile of each of the
# 64 products holds 33 valid rows; 64 * 2 * (512 / 128) = 512 GEMM tiles = the persistent kernel, 256 for half of the channels
WINO_SHAPES = [("d1_102", 102, 32, 512, 1), ("d2_97", 97, 128, 512, 2)]


@pytest.mark.parametrize("flip", [0, 1], ids=["forward", "backward_data"])
@pytest.mark.parametrize("case", WINO_SHAPES, ids=[c[0] for c in WINO_SHAPES])
def test_winograd_row_tail_bit_identical_to_per_tile_kernel(case, flip):
    from diga_amd import _lib
    name, hw, cin, cout, d = case
    tile = 6
    tiles = sum(-(-((hw - a + d - 1) // d) // tile) for a in range(d)) ** 2
    assert tiles == 289 and (tile + 2) ** 2 * 2 * (cout // 128) == 512
    assert _lib.get_conv_math() == 0
    g = torch.Generator().manual_seed(77 + hw + flip)
    x = (torch.randn((1, hw, hw, cin), generator=g) + 0.5).to(DEV)
    w = (torch.randn((cout, 3, 3, cin), generator=g) * (2.0 / (cin * 9)) ** 0.5).to(DEV)
    got = _winograd(x, w, flip, tile, d)
    half = cout // 2
    for c0 in (0, half):
        part = _winograd(x, w[c0:c0 + half].contiguous(), flip, tile, d)
        assert torch.equal(got[..., c0:c0 + half], part), (name, flip, c0)
    want = _conv3x3_f64(x, w, d, flip)
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(f"winograd row tail {name} flip {flip}: max err / scale = {err:.2e}")
    assert err < WINO_TOL[tile][0], (name, flip, err)
