"""The oracle of tests/test_gpu_bwd_epilogue.py checked on its own, so that the GPU file cannot be wrong the way the kernels are:

  1. reference() + finalise() of tests/bwd_epilogue_cases.py against float64 autograd through F.batch_norm (+ residual) + ReLU;
  2. the 21 descriptors against the library's own host check (check_bwd_epilogue, csrc/conv_call.h), and its invalid neighbours;
  3. diga_conv2d_epi_chunk_rows == 128 for every arithmetic, also where the forward statistics use 64-row chunks.

2. hands fake addresses to entry points, as tests/test_conv_entry_checks_cpu.py does: it runs only where no device is visible.  There
an accepted call goes on to a launch that fails for want of a device and returns the positive hipError_t (launch_status), which
cannot be confused with the negative DIGA_E* codes of a refusal -- so accepted descriptors are told from refused ones."""
import pytest
import torch
import torch.nn.functional as F

import bwd_epilogue_cases as bc
import conv_entry_check_cases as cc

M, C, EPS = 297, 64, 1e-5


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


# ------------------------------------------------------------------------------------------------ 1. the definition vs autograd
@pytest.mark.parametrize("mask", ["mask_y", "bits", "relu_ab"])
@pytest.mark.parametrize("addend", [False, True], ids=["single_consumer", "second_consumer"])
def test_reference_and_finalise_equal_float64_autograd(mask, addend):
    """y = relu(batch_norm(x) [+ residual]) in train mode, read by the convolution whose backward-data result is `acc` and (addend) by a
    second consumer whose gradient is `addend`: autograd's gradient of the BatchNorm's output is g, of its input dx.  The mask reaches
    the oracle as the junction's output (mask_y), as its packed sign bits, or -- without a residual -- as the forward coefficients."""
    g = torch.Generator().manual_seed(11 + len(mask) + int(addend))
    x = (torch.randn((M, C), generator=g) * 1.5 + 0.7).double()
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).double(), (0.3 * torch.randn(C, generator=g)).double()
    acc, add = torch.randn((M, C), generator=g).double(), torch.randn((M, C), generator=g).double()
    residual = None if mask == "relu_ab" else torch.randn((M, C), generator=g).double().requires_grad_()
    for _ in range(2):
        mean, invstd = x.mean(0), 1.0 / torch.sqrt(x.var(0, unbiased=False) + EPS)
        a = gamma * invstd
        b = beta - mean * a
        x = bc.separate_from_zero(x, a, b)
    mean, invstd = x.mean(0), 1.0 / torch.sqrt(x.var(0, unbiased=False) + EPS)
    a = gamma * invstd
    b = beta - mean * a
    assert bc.relu_ab_margin(x, a, b) > 1e-6
    x.requires_grad_()
    z = F.batch_norm(x, None, None, gamma, beta, True, 0.1, EPS)
    z.retain_grad()
    y = torch.relu(z if residual is None else z + residual)
    ((y * acc).sum() + ((y * add).sum() if addend else 0.0)).backward()

    ops = {"x": x.detach(), "mean": mean, "invstd": invstd}
    if addend:
        ops["addend"] = add
    if mask == "mask_y":
        ops["mask_y"] = y.detach()
    elif mask == "bits":
        ops["mask_bits"] = bc.pack_bits(y.detach() > 0, C // 8 + 3)
    else:
        ops["relu_ab"] = torch.stack([a, b])
    got_g, rec = bc.reference(acc, ops)
    assert 0.2 < float((got_g != 0).double().mean()) < 0.8
    assert _rel(got_g, z.grad) < 1e-12
    if residual is not None:
        assert _rel(got_g, residual.grad) < 1e-12
    assert _rel(bc.finalise(got_g, x.detach(), gamma, mean, invstd), x.grad) < 1e-12
    # the records are the chunked form of the two column sums the finaliser takes its means from
    xhat = (x.detach() - mean) * invstd
    assert rec.shape == (3, 2, C)
    assert _rel(rec.sum(0), torch.stack([got_g.sum(0), (got_g * xhat).sum(0)])) < 1e-12
    assert _rel(rec[2], torch.stack([got_g[256:].sum(0), (got_g[256:] * xhat[256:]).sum(0)])) < 1e-12


def test_packed_bits_and_guards_of_the_builders():
    o = bc.build_operands(41, 68, 5)                         # C % 8 == 4: a partial last byte
    bits = o["mask_bits"].numpy()
    assert bits.shape == (41, 9 + 3) and o["mask_bits_ld"] == 12
    assert (bits[:, 9:] == 0xFF).all() and ((bits[:, 8] >> 4) == 0xF).all()
    assert torch.equal(bc.unpack_bits(o["mask_bits"], 68), o["mask_y"] > 0)
    for name, ld in (("addend", 72), ("x", 76), ("mask_y", 72)):
        p = o[name + "_p"]
        assert p.shape == (41, ld) and torch.equal(p[:, :68], o[name]) and bool(torch.isnan(p[:, 68:]).all())
    assert bc.partials_floats(297, 64) == 5 * 2 * 64 and bc.n_chunks(297) == 3
    # the planted exact zeros of the relu_ab form are zeros of the fp32 fmaf too, and the definition drops them
    z = o["relu_ab_zeros"]
    assert int(z.sum()) == 6 and bool((torch.addcmul(o["relu_ab"][1], o["x"], o["relu_ab"][0])[z] == 0).all())
    assert not bool(bc.keep_mask({"relu_ab": o["relu_ab"], "x": o["x"]}, (41, 68))[z].any())
    g, _ = bc.reference(torch.ones((41, 68), dtype=torch.float64), {"relu_ab": o["relu_ab"], "x": o["x"]})
    assert bool((g[z] == 0).all()) and 0.2 < float((g != 0).double().mean()) < 0.8


# ------------------------------------------------------------------------------------------------ 2. the host check
ENTRIES = ["diga_conv2d_nhwc_f32_epi", "diga_conv2d_nhwc_bf16x3_epi", "diga_conv2d_nhwc_twin_epi", "diga_conv2d_winograd_f32_epi",
           "diga_conv2d_nhwc_bf16x6_f32in_epi", "diga_conv_taps_bf16x6_f32in_epi"]
E = cc.E
ADDR = dict(addend=E, mask_y=E + 0x10000, mask_bits=E + 0x20000, x=E + 0x30000, relu_ab=E + 0x40000, mean=E + 0x41000, invstd=E + 0x42000,
            partials=E + 0x50000)
host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="host checks only: run where no device is visible")


def _fields(d, cout):
    return bc.descriptor_fields(d, ADDR, dict(addend=cout + 4, mask_y=cout + 4, x=cout + 8, mask_bits=cout // 8 + 3))


def _call(entry, fields):
    from diga_amd import _lib
    assert _lib.PROF_TAGS.index("conv_bwd_data") == cc.BWD_DATA
    return cc.call(_lib, entry, dict(cc.base(entry), epi=fields, tag=cc.BWD_DATA))


@host_only
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_descriptor_is_accepted_by_the_host_check(entry):
    cout = cc.base(entry)["cout"]
    wrong = []
    for d in bc.DESCRIPTORS:
        rc, msg = _call(entry, _fields(d, cout))
        if rc in cc.REJECTED or rc == 0:                     # (0 is impossible without a device: it would mean nothing was launched)
            wrong.append((d.id, rc, msg))
    assert not wrong, wrong


@host_only
@pytest.mark.parametrize("entry", ENTRIES)
def test_invalid_neighbours_are_refused_before_any_launch(entry):
    cout = cc.base(entry)["cout"]
    full = _fields(bc.BY_ID["add+mask_y+x+partials"], cout)
    bits = _fields(bc.BY_ID["add+bits+x+partials"], cout)
    drop = lambda f, *ks: {k: v for k, v in f.items() if k not in ks}
    neighbours = {
        "empty": ({}, "empty epilogue descriptor"),
        "relu_ab_without_x": (dict(relu_ab=ADDR["relu_ab"]), "empty epilogue descriptor"),
        "add+relu_ab_without_x": (dict(addend=ADDR["addend"], addend_ld=cout + 4, relu_ab=ADDR["relu_ab"]), "relu_ab needs x"),
        "partials_without_mean": (drop(full, "mean"), "partials need x, mean and invstd"),
        "partials_without_invstd": (drop(full, "invstd"), "partials need x, mean and invstd"),
        "partials_without_x": (drop(full, "x", "x_ld"), "partials need x, mean and invstd"),
        "mask_y_and_bits": (dict(full, mask_bits=ADDR["mask_bits"], mask_bits_ld=cout // 8 + 3), "give one of mask_y, mask_bits, relu_ab"),
        "mask_y_and_relu_ab": (dict(full, relu_ab=ADDR["relu_ab"]), "give one of mask_y, mask_bits, relu_ab"),
        "bits_and_relu_ab": (dict(bits, relu_ab=ADDR["relu_ab"]), "give one of mask_y, mask_bits, relu_ab"),
        "addend_ld_below_cout": (dict(full, addend_ld=cout - 4), "bad addend"),
        "mask_bits_ld_below_cout_bits": (dict(bits, mask_bits_ld=cout // 8 - 1), "bad mask_bits"),
    }
    wrong = []
    for name, (fields, why) in neighbours.items():
        rc, msg = _call(entry, fields)
        if rc != -1 or why not in msg:                       # DIGA_EINVAL, answered by the rule in question
            wrong.append((name, rc, msg))
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------ 3. the chunk rule
def test_epilogue_records_are_128_rows_for_every_arithmetic():
    """Every caller of diga_bn_bwd_partials passes diga_conv2d_epi_chunk_rows(...): 128 for every shape and arithmetic, also for the
    stride-1 pointwise fp32 geometry whose FORWARD statistics come in 64-row chunks (the persistent GEMM, which a call with an epilogue
    never takes).  The second geometry is the large pointwise case of tests/test_gpu_bwd_epilogue.py."""
    from diga_amd import _lib
    lib = _lib.lib
    for n, h, w, cin, cout in ((1, 512, 256, 32, 128), (1, 1, 512 * 256 + 40, 32, 128), (2, 512, 256, 256, 256)):
        assert n * h * w >= 512 * 256
        geom = (n, h, w, cin, h, w, cout, 1, 1, 1, 1, 0, 0)
        assert lib.diga_conv2d_stats_chunk_rows(*geom, 0) == 64, geom
        for math in (0, 1, 2):
            assert lib.diga_conv2d_epi_chunk_rows(*geom, math) == 128, (geom, math)
        assert [lib.diga_conv2d_stats_chunk_rows(*geom, m) for m in (1, 2)] == [128, 128]
    for geom in ((2, 9, 7, 64, 9, 7, 64, 1, 1, 1, 1, 0, 0), (3, 11, 9, 32, 11, 9, 160, 3, 3, 1, 1, 2, 2), (1, 13, 13, 256, 13, 13, 256, 3, 3, 1, 1, 12, 12)):
        for math in (0, 1, 2):
            assert lib.diga_conv2d_epi_chunk_rows(*geom, math) == 128, (geom, math)
