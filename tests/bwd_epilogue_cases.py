"""The backward-data epilogue of diga_bwd_epilogue_t (include/diga_hip.h) as a definition: every operand combination the host rules
accept (check_bwd_epilogue, csrc/conv_call.h), its float64 reference, the float64 finaliser of diga_bn_bwd, and operand builders with
guard columns.  Shared by tests/test_bwd_epilogue_oracle_cpu.py (which checks this file against autograd) and
tests/test_gpu_bwd_epilogue.py (which checks the kernels against this file).  Nothing here touches a device at import.

    out      = where(mask, acc + addend, 0)
    mask     = mask_y > 0  |  bit (c & 7) of byte (c >> 3) of mask_bits  |  x * a + b > 0 (relu_ab = [a; b])  |  all ones
    partials = [ceil(M / 128)][2][C]: { sum out, sum out * (x - mean) * invstd } over the rows of each 128-row chunk
"""
import collections
import itertools

import numpy as np
import torch

CHUNK = 128                      # rows per record (diga_conv2d_epi_chunk_rows)
SENTINEL = 7.0                   # guard columns of `out`
U = 2.0 ** -24                   # fp32 unit roundoff
MASKS = ("none", "mask_y", "bits", "relu_ab")
XFORMS = ("none", "x", "x+partials")

Descriptor = collections.namedtuple("Descriptor", "addend mask x partials id")


def descriptors():
    """Every operand combination check_bwd_epilogue accepts: addend absent / given, one of four mask forms, x absent / given / given
    with mean, invstd and partials -- without the empty descriptor and without relu_ab lacking the x it reads."""
    out = []
    for addend, mask, xf in itertools.product((False, True), MASKS, XFORMS):
        if not addend and mask == "none" and xf == "none":
            continue                                             # "empty epilogue descriptor"
        if mask == "relu_ab" and xf == "none":
            continue                                             # "relu_ab needs x"
        parts = (["add"] if addend else []) + ([] if mask == "none" else [mask]) + ([] if xf == "none" else xf.split("+"))
        out.append(Descriptor(addend, mask, xf != "none", xf == "x+partials", "+".join(parts)))
    return out


DESCRIPTORS = descriptors()
assert len(DESCRIPTORS) == 21 and len({d.id for d in DESCRIPTORS}) == 21
BY_ID = {d.id: d for d in DESCRIPTORS}
assert {"add", "add+bits+x+partials", "relu_ab+x+partials", "add+mask_y+x+partials"} <= set(BY_ID)


def n_chunks(m, chunk=CHUNK):
    return -(-m // chunk)


def partials_floats(m, c):
    """What the host allocates (model/conv.py, include/diga_hip.h); the epilogue writes the first n_chunks(m) * 2 * c of them."""
    return -(-m // 64) * 2 * c


# ---------------------------------------------------------------------------------------------------------------- mask forms
def pack_bits(keep, ld_bytes=None):
    """[M][C] bool -> [M][ld_bytes] uint8, bit (c & 7) of byte (c >> 3) = keep[c], packed as tests/test_gpu_norm.py::
    test_batchnorm_relu_bits packs them.  Everything that is not a channel -- the high bits of a partial last byte, the spare bytes up
    to ld_bytes -- is set to ONE: a kernel that looks at them keeps what it must drop."""
    keep = np.asarray(keep, dtype=bool)
    m, c = keep.shape
    nb = -(-c // 8)
    ld_bytes = nb if ld_bytes is None else ld_bytes
    assert ld_bytes >= nb
    out = np.full((m, ld_bytes), 0xFF, dtype=np.uint8)
    out[:, :nb] = np.packbits(keep, axis=1, bitorder="little")
    if c % 8:
        out[:, nb - 1] |= (0xFF << (c % 8)) & 0xFF
    return torch.from_numpy(out)


def unpack_bits(bits, c):
    """The definition read back: channel ch of a row is kept where bit (ch & 7) of byte (ch >> 3) is set."""
    ch = torch.arange(c, device=bits.device)
    return ((bits[:, ch >> 3].to(torch.int32) >> (ch & 7)) & 1).bool()


def relu_ab_margin(x, a, b, planted=None):
    """min |x * a + b| in float64 (over the elements outside the bool mask `planted`).  x * a is exact in float64 and fmaf rounds the
    exact value once, so the float64 sign IS the sign of the fp32 fmaf, zero included; callers still assert a margin instead of
    relying on that for values next to zero."""
    v = (x.double() * a.double() + b.double()).abs()
    return float((v if planted is None else v[~planted]).min())


def separate_from_zero(x, a, b, margin=1e-4, step=2.0 ** -5):
    """x with every element whose x * a + b lies within `margin` of zero moved by `step` (keeps the dtype's values exact)."""
    x = x.clone()
    near = (x.double() * a.double() + b.double()).abs() <= margin
    x[near] += step
    return x


def keep_mask(ops, shape, device="cpu"):
    """The mask of the operands in `ops` (the descriptor's own), as bool [M][C] on the operands' device; all ones without a mask."""
    given = [k for k in ("mask_y", "mask_bits", "relu_ab") if ops.get(k) is not None]
    assert len(given) <= 1, given
    if not given:
        return torch.ones(shape, dtype=torch.bool, device=device)
    if given[0] == "mask_y":
        return ops["mask_y"] > 0
    if given[0] == "mask_bits":
        return unpack_bits(ops["mask_bits"], shape[1])
    return ops["x"].double() * ops["relu_ab"][0].double() + ops["relu_ab"][1].double() > 0


# ---------------------------------------------------------------------------------------------------------------- definitions
def chunk_sums(g, x, mean, invstd, chunk=CHUNK):
    """float64 records [ceil(M / chunk)][2][C] = { sum g, sum g * xhat } per chunk of rows, and the same sums of |term| (what a
    forward error bound of the fp32 sums is a multiple of)."""
    g, xhat = g.double(), (x.double() - mean.double()) * invstd.double()
    m, c = g.shape
    n = n_chunks(m, chunk)
    pad = n * chunk - m
    terms = torch.stack([g, g * xhat], dim=1)                                  # [M][2][C]
    terms = torch.cat([terms, torch.zeros((pad, 2, c), dtype=torch.float64, device=terms.device)]).reshape(n, chunk, 2, c)
    return terms.sum(1), terms.abs().sum(1)


def reference(acc64, ops):
    """The epilogue in float64, on the device of its arguments.  acc64 [M][C]: the convolution's result; ops: the operands the
    descriptor gives, logical [M][C] views (keys addend, mask_y, mask_bits ([M][bytes] uint8), relu_ab [2][C], x, mean, invstd; absent
    or None = not given).  -> (g, records or None); records only with mean and invstd."""
    acc64 = acc64.double()
    v = acc64 + ops["addend"].double() if ops.get("addend") is not None else acc64
    g = torch.where(keep_mask(ops, acc64.shape, acc64.device), v, torch.zeros((), dtype=torch.float64, device=acc64.device))
    rec = None
    if ops.get("mean") is not None:
        rec = chunk_sums(g, ops["x"], ops["mean"], ops["invstd"])[0]
    return g, rec


def finalise(g, x, gamma, mean, invstd):
    """diga_bn_bwd's formula in float64: dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)), means over the M rows."""
    g, x, gamma, mean, invstd = (t.double() for t in (g, x, gamma, mean, invstd))
    xhat = (x - mean) * invstd
    return gamma * invstd * (g - g.mean(0) - xhat * (g * xhat).mean(0))


def record_bound(abs_sums, terms=CHUNK):
    """Forward error bound of an fp32 sum of `terms` addends in any order ((terms - 1) u sum |t|, first order) plus the three roundings
    that form one addend (x - mean, * invstd, * g): (terms + 8) u sum |t| -- 136 u for the 128-row records."""
    return (terms + 8) * U * abs_sums


# ---------------------------------------------------------------------------------------------------------------- operand builders
def guarded(t, pad, fill):
    """[M][C] -> [M][C + pad] with the padding columns set to `fill`; the logical tensor is out[:, :C]."""
    m, c = t.shape
    out = torch.full((m, c + pad), fill, dtype=t.dtype)
    out[:, :c] = t
    return out


def build_operands(m, c, seed):
    """Every operand of the epilogue for an [M][C] gradient, on the CPU, seeded: a train-mode BatchNorm(+residual)+ReLU seen from
    behind.  [M][ld] tensors carry ld = C + 4 or C + 8 with NaN in the padding columns (a padding value that reaches a result shows);
    mask_bits has mask_bits_ld = ceil(C / 8) + 3 with ones in everything that is not a channel.  Logical views under "<name>", the
    padded tensors a kernel is given under "<name>_p"."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((m, c), generator=g) * 1.5 + 0.7
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    for _ in range(2):                                       # (the statistics move a little when x does: settle, then assert)
        mean = x.double().mean(0).float()
        invstd = (1.0 / torch.sqrt(x.double().var(0, unbiased=False) + 1e-5)).float()
        a = gamma * invstd
        b = beta - mean * a
        x = separate_from_zero(x, a, b)
    # Exact zeros of the relu_ab form, planted: x * a + b == 0 is dropped by the definition (keep where > 0) and kept by a kernel that
    # compares >= 0.  Two channels (different column quads, low and high nibble of a mask byte) get a = 0.5, b = -0.25; the first,
    # a middle and the last row get x = 0.5 there: 0.5 * 0.5 - 0.25 is exactly 0 in every precision.  Everywhere else the margin holds.
    planted = torch.zeros((m, c), dtype=torch.bool)
    for ch in (1, c - 2):
        a[ch], b[ch] = 0.5, -0.25
        x[:, ch] = separate_from_zero(x[:, ch], a[ch], b[ch])
        for row in (0, m // 2, m - 1):
            x[row, ch] = 0.5
            planted[row, ch] = True
    relu_ab = torch.stack([a, b]).contiguous()
    assert relu_ab_margin(x, a, b, planted) > 1e-6
    assert bool(((x.double() * a.double() + b.double())[planted] == 0).all()) and int(planted.sum()) == 6
    res = torch.randn((m, c), generator=g)
    mask_y = torch.relu(x * a + b + res)                     # the junction's output: exact zeros where the ReLU cut
    addend = torch.randn((m, c), generator=g)
    keep = mask_y > 0
    assert 0.2 < float(keep.float().mean()) < 0.8 and 0.2 < float((x * a + b > 0).float().mean()) < 0.8
    nb = -(-c // 8)
    o = dict(m=m, c=c, x=x, mean=mean, invstd=invstd, gamma=gamma, relu_ab=relu_ab, mask_y=mask_y, addend=addend,
             mask_bits=pack_bits(keep, nb + 3), mask_bits_ld=nb + 3, relu_ab_zeros=planted)
    o["addend_p"], o["x_p"], o["mask_y_p"] = guarded(addend, 4, float("nan")), guarded(x, 8, float("nan")), guarded(mask_y, 4, float("nan"))
    assert torch.equal(unpack_bits(o["mask_bits"], c), keep)
    return o


def select(o, d):
    """The operands descriptor d gives, as reference() reads them."""
    s = {}
    if d.addend:
        s["addend"] = o["addend"]
    if d.mask == "mask_y":
        s["mask_y"] = o["mask_y"]
    elif d.mask == "bits":
        s["mask_bits"] = o["mask_bits"]
    elif d.mask == "relu_ab":
        s["relu_ab"] = o["relu_ab"]
    if d.x:
        s["x"] = o["x"]
    if d.partials:
        s["mean"], s["invstd"] = o["mean"], o["invstd"]
    return s


def descriptor_fields(d, addr, ld):
    """Field values of diga_bwd_epilogue_t for descriptor d: addr[name] = address of addend / mask_y / mask_bits / x / relu_ab / mean /
    invstd / partials, ld[name] = leading dimension of addend / mask_y / x (floats) and mask_bits (bytes)."""
    f = {}
    if d.addend:
        f.update(addend=addr["addend"], addend_ld=ld["addend"])
    if d.mask == "mask_y":
        f.update(mask_y=addr["mask_y"], mask_ld=ld["mask_y"])
    elif d.mask == "bits":
        f.update(mask_bits=addr["mask_bits"], mask_bits_ld=ld["mask_bits"])
    elif d.mask == "relu_ab":
        f.update(relu_ab=addr["relu_ab"])
    if d.x:
        f.update(x=addr["x"], x_ld=ld["x"])
    if d.partials:
        f.update(mean=addr["mean"], invstd=addr["invstd"], partials=addr["partials"])
    return f
