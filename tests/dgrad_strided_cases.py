"""Shared by test_dgrad_strided_cpu.py and test_gpu_dgrad_strided.py: the shape table of the stride-2 backward-data kernel
(diga_dgrad_strided_f32) and a float64 restatement of its phase decomposition.

The restatement follows the definition phase by phase (it is not conv_transpose): dx is split into (py, px) = (y & 1, x & 1); with
r0 = (py + pad_y) & 1 a phase's rows use the taps r = r0 + 2t, t in [0, Rp), Rp = (R - r0 + 1) // 2, and row y = 2j + py reads dy row
j + (py + pad_y - r0) // 2 - t; columns follow the same rule.  Rows no tap reaches and phases without taps stay zero."""
import functools

import torch

# name -> (N, C, Hi, Wi, K, R, S, (pad_y, pad_x)): C / K are the forward conv's input / output channels.  Each row is the smallest
# shape that reaches its corner.
CASES = {
    "odd": (2, 64, 17, 13, 64, 3, 3, (1, 1)),        # phases of different extent; two images in one phase's row space
    "even": (2, 32, 16, 12, 96, 3, 3, (1, 1)),       # last dy row out of range for the last dx row; three K-chunks; half-empty channel tile
    "uncovered": (2, 32, 8, 10, 32, 3, 3, (0, 0)),   # last row and column of dx reached by no tap
    "mtail": (3, 32, 23, 21, 32, 3, 3, (1, 1)),      # 396 / 360 / 363 / 330 rows per phase: several tiles per phase, each with a tail
    "k4": (1, 64, 12, 14, 32, 4, 4, (1, 1)),         # four taps in every phase
    "k2": (1, 32, 10, 6, 64, 2, 2, (0, 0)),          # one tap per phase
    "k1": (2, 32, 9, 7, 64, 1, 1, (0, 0)),           # three phases without taps (entry point only: the host does not route here)
    "k5": (1, 32, 11, 9, 32, 5, 5, (2, 2)),
    "r3s1": (1, 32, 9, 8, 32, 3, 1, (1, 0)),         # the two axes decide independently
}


def out_extent(hi, wi, r, s, pad):
    return (hi + 2 * pad[0] - r) // 2 + 1, (wi + 2 * pad[1] - s) // 2 + 1


def phase_rows(n, hi, wi):
    """Rows of the four phases p = 2 * py + px."""
    return [n * ((hi - py + 1) // 2) * ((wi - px + 1) // 2) for py in (0, 1) for px in (0, 1)]


def dgrad_by_phases(dy, w, hi, wi, pad):
    """dx [N, C, Hi, Wi] of dy [N, K, Ho, Wo] and w [K, C, R, S] (stride 2, dilation 1), in the dtype of its operands."""
    n, k, ho, wo = dy.shape
    _, c, r, s = w.shape
    wt = w.permute(1, 2, 3, 0)                      # [C][R][S][K]: the transpose the kernel reads in place
    g = dy.permute(0, 2, 3, 1)                      # [N][Ho][Wo][K]
    dx = torch.zeros((n, c, hi, wi), dtype=dy.dtype)
    for py in (0, 1):
        for px in (0, 1):
            hp, wp = (hi - py + 1) // 2, (wi - px + 1) // 2
            r0, s0 = (py + pad[0]) & 1, (px + pad[1]) & 1
            rp, sp = (r - r0 + 1) // 2, (s - s0 + 1) // 2
            oy, ox = (py + pad[0] - r0) // 2, (px + pad[1] - s0) // 2
            acc = torch.zeros((n, hp, wp, c), dtype=dy.dtype)
            for t in range(rp):
                for u in range(sp):
                    # rows j with 0 <= j + oy - t < Ho, columns likewise
                    j0, j1 = max(0, t - oy), min(hp, ho + t - oy)
                    i0, i1 = max(0, u - ox), min(wp, wo + u - ox)
                    if j0 >= j1 or i0 >= i1:
                        continue
                    blk = g[:, j0 + oy - t:j1 + oy - t, i0 + ox - u:i1 + ox - u, :]
                    acc[:, j0:j1, i0:i1, :] += blk @ wt[:, r0 + 2 * t, s0 + 2 * u, :].t()
            dx[:, :, py::2, px::2] = acc.permute(0, 3, 1, 2)
    return dx


@functools.lru_cache(maxsize=None)
def operands(name):
    """(dy [N, K, Ho, Wo] fp32, w [K, C, R, S] fp32, float64 conv2d_input of the two): seeded, computed once per session, read-only."""
    n, c, hi, wi, k, r, s, pad = CASES[name]
    ho, wo = out_extent(hi, wi, r, s, pad)
    g = torch.Generator().manual_seed(2400 + sorted(CASES).index(name))
    dy = torch.randn((n, k, ho, wo), generator=g)
    w = torch.randn((k, c, r, s), generator=g) * (2.0 / (k * r * s)) ** 0.5
    ref = torch.nn.grad.conv2d_input((n, c, hi, wi), w.double(), dy.double(), stride=2, padding=pad)
    return dy, w, ref
