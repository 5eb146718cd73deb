"""CPU emulation of the bf16x6 arithmetic (diga_amd/csrc/conv_bf16x6.h): fp32 operands as three bf16 planes, six (or eight)
partial products, fp32 accumulation in K-steps of 32, against float64.  Not a GPU measurement: a matmul of one 32-deep K-step
stands in for one bf16 MFMA, whose internal rounding is not modelled.

    python tools/bf16x6_emulation.py

`split3`, `product_fold` and `product_chain` are the host restatement the tests hold the kernels to
(tests/test_bf16x6_cpu.py, tests/test_gpu_conv_bf16x6.py)."""
import torch


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def split3(x):
    """fp32 x -> (a0, a1, a2, residual): a0 = bf16(x), a1 = bf16(x - a0), a2 = bf16(x - a0 - a1), as fp32 tensors, and the largest
    |x - a0 - a1 - a2| (0 for normal fp32 of magnitude >= 2^-110)."""
    a0 = bf(x)
    r = x - a0
    a1 = bf(r)
    r = r - a1
    a2 = bf(r)
    return a0, a1, a2, float((r - a2).abs().max())


SMALL = [(1, 1), (0, 2), (2, 0), (0, 1), (1, 0)]          # smallest terms first; (0, 0) last


def product_fold(a, b, kstep=32):
    """a [M, K] @ b [K, N] the way the kernels sum it: per K-step the five corrections chained from zero, the leading product into the
    running sum, one add of the corrections."""
    A, B = split3(a), split3(b)
    acc = torch.zeros(a.shape[0], b.shape[1])
    for k0 in range(0, a.shape[1], kstep):
        s = slice(k0, k0 + kstep)
        t = torch.zeros_like(acc)
        for i, j in SMALL:
            t = t + A[i][:, s] @ B[j][s]
        acc = (acc + A[0][:, s] @ B[0][s]) + t
    return acc


def product_chain(a, b):
    """The per-k fp32 fmaf chain (one rounding per k): what include/diga_hip.h says DIGA_CONV_MATH_F32 is."""
    chain = torch.zeros(a.shape[0], b.shape[1])
    for k in range(a.shape[1]):
        chain = (chain.double() + a[:, k:k + 1].double() * b[k:k + 1, :].double()).float()
    return chain


# ---- phase-collapsed weights of a convolution behind a 2x nearest upsampling (config.x6_up2; diga_collapse_up2_weights and
# diga_conv_up2_bf16x6_plan restated; tests/test_bf16x6_up2_cpu.py, tests/test_gpu_conv_bf16x6_up2.py)
def up2_rows(R, off0, phase):
    """a(phase, r) = floor((phase + off0 + r) / 2) for r = 0 .. R - 1: the SOURCE row, relative to y, that tap r of output row
    2 y + phase reads after nearest x2 upsampling (away from the padding)."""
    return [(phase + off0 + r) // 2 for r in range(R)]


def up2_taps(R, off0):
    """R': the collapsed tap count of the wider phase."""
    return max(a[-1] - a[0] + 1 for a in (up2_rows(R, off0, 0), up2_rows(R, off0, 1)))


def collapse_up2(w_krsc, off_y0, off_x0):
    """w [K, R, S, C] -> (wc [2, 2, K, R', S', C], first [2][2] = (a_y(fy, 0), a_x(fx, 0))): element (r', s') of phase (fy, fx) is the sum
    of the taps (r, s) with a_y(fy, r) - a_y(fy, 0) == r' and a_x(fx, s) - a_x(fx, 0) == s', taken in float64 in ascending (r, s) order
    and rounded to w's dtype once; a phase with fewer taps keeps zeros in the rest."""
    K, R, S, C = w_krsc.shape
    rc, sc = up2_taps(R, off_y0), up2_taps(S, off_x0)
    wc = torch.zeros(2, 2, K, rc, sc, C, dtype=torch.float64)
    first = [[None, None], [None, None]]
    wd = w_krsc.double()
    for fy in (0, 1):
        ay = up2_rows(R, off_y0, fy)
        for fx in (0, 1):
            ax = up2_rows(S, off_x0, fx)
            first[fy][fx] = (ay[0], ax[0])
            for r in range(R):
                for s in range(S):
                    wc[fy, fx, :, ay[r] - ay[0], ax[s] - ax[0], :] += wd[:, r, s, :]
    return wc.to(w_krsc.dtype), first


def up2_rule(Hi, Wi, Cin, Cout, Ho, Wo, R, S, off_y0, off_x0, dil_y=1, dil_x=1, shift=1, reflect=1):
    """diga_conv_up2_bf16x6_plan restated: (R', S') where the collapsed form takes the call, else None."""
    TH, TW, LDS = 8, 16, 160 * 1024
    if min(Hi, Wi, Cin, Cout, Ho, Wo) <= 0 or Cin % 32 != 0 or Cout <= 16:
        return None
    if shift != 1 or dil_y != 1 or dil_x != 1 or not (2 <= R <= 7 and 2 <= S <= 7) or off_y0 > 0 or off_x0 > 0 or reflect not in (0, 1):
        return None
    if 2 * 3 * 64 * 64 + max((TH + R - 1) * (TW + S - 1) * 192, TH * TW * 68 * 4) > LDS:     # the window rule (never binds at R, S <= 7)
        return None
    ty, tx = -(-Ho // TH), -(-Wo // TW)
    if ty < 3 or tx < 3:
        return None
    if TH + off_y0 < 0 or TH * (ty - 1) - 1 + off_y0 + R - 1 > 2 * Hi - 1:
        return None
    if TW + off_x0 < 0 or TW * (tx - 1) - 1 + off_x0 + S - 1 > 2 * Wi - 1:
        return None
    return up2_taps(R, off_y0), up2_taps(S, off_x0)


def operands(M, K, N, seed):
    torch.manual_seed(seed)
    a = torch.randn(M, K)
    b = torch.randn(K, N) * (2.0 / K) ** .5
    return a, b


def run(M, K, N, seed):
    a, b = operands(M, K, N, seed)
    ref = a.double() @ b.double()
    sc = ref.abs().max()
    A, B = split3(a), split3(b)
    assert A[3] == 0.0 and B[3] == 0.0, "the three planes must sum to the input exactly"
    err = lambda t: ((t.double() - ref).abs().max() / sc).item()          # noqa: E731
    chain = product_chain(a, b)
    z = lambda: torch.zeros(M, N)                                          # noqa: E731
    chunk, one, eight, main, corr, fold = z(), z(), z(), z(), z(), z()
    for k0 in range(0, K, 32):
        s = slice(k0, k0 + 32)
        p = lambda i, j: A[i][:, s] @ B[j][s]                              # noqa: E731
        chunk = chunk + a[:, s] @ b[s]
        for i, j in SMALL + [(0, 0)]:
            one = one + p(i, j)
        for i, j in [(1, 2), (2, 1)] + SMALL + [(0, 0)]:
            eight = eight + p(i, j)
        t = z()
        for i, j in SMALL:
            corr = corr + p(i, j)
            t = t + p(i, j)
        main = main + p(0, 0)
        fold = (fold + p(0, 0)) + t                                        # corrections chained from zero, one add per K-step
    print(f"K={K:5d} seed {seed} | fp32 per-k chain {err(chain):.2e}  fp32 per-32 {err(chunk):.2e} | x6 one acc {err(one):.2e}  "
          f"x8 one acc {err(eight):.2e}  x6 two acc {err(main + corr):.2e}  x6 fold {err(fold):.2e}")


if __name__ == "__main__":
    for K in (64, 256, 1024, 2048):
        for seed in (0, 1):
            run(512, K, 256, seed)
