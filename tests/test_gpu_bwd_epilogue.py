"""The backward-data epilogue (diga_bwd_epilogue_t, include/diga_hip.h) held to its definition, entry point by entry point: every
(family, shape) runs the plain entry point once, then each of the 21 operand combinations of tests/bwd_epilogue_cases.py on its `_epi`
twin with the same input, weights and backward-data geometry (off0 = +pad, doff = -dilation, [C][R][S][K] weights from
diga_weight_transpose, prof_tag = conv_bwd_data).  "Cout" below is the call's Cout = the layer's Cin.  Per combination:

  1. out[:, :Cout] == where(mask, plain + addend, 0) with ONE fp32 add, torch.equal: the accumulators come out of the same K loop and the
     epilogue is one add and one select (epi_rows, csrc/conv.hip: "same expressions in the same order"; the Winograd output transforms
     likewise);
  2. (once per shape) the plain result against the float64 convolution at the bound the project holds that path to -- which, with 1.,
     ties `out` to float64 without a second tolerance;
  3. guards: the padding columns of `out` keep their sentinel, no NaN from the NaN-filled padding columns of addend / x / mask_y or the
     all-ones spare bits of mask_bits reaches a result, `partials` is written in its first ceil(M / 128) * 2 * Cout floats and nowhere else;
  4. every record against its definition evaluated in float64 from the device's own out and x, at (128 + 8) * 2^-24 * sum |term| (derived
     in bwd_epilogue_cases.record_bound, not measured); the Winograd form writes one record per tile group, so only the column totals
     are defined and the bound counts the pixels behind one record;
  5. a second call gives the same bits.
Then diga_bn_bwd_partials on the device's own g and records.

Which kernel a shape takes is stated per shape and ASSERTED with a copy of the shape rule of conv2d_f32 / conv2d_bf16x3 / conv2d_twin
(csrc/conv.hip): a dispatch change makes the test say so instead of silently testing another kernel.  The 128-row bf16x3 pixel kernel
(conv_fwd_x3p_kernel) is reached only beyond 2^31 elements and stays out; so do the triplet form of bf16x6 and
diga_conv2d_winograd_bf16x6 with an epilogue.

Two shapes differ from what one would write down first, because the library's rules say so:
  * diga_conv2d_winograd_f32_epi refuses Cout <= 64 (asserted below), so the narrow Winograd case is Cout = 96;
  * a 3x3 dilation-12 layer on 1 x 13 x 13 has M = 169 < 256 rows and its corner pixels still see an off-centre tap: it runs on
    conv_fwd_kernel<2,32,true> (kept, and asserted); 2 x 12 x 12 (M = 288, every off-centre tap outside the image for every pixel)
    is the case that reaches conv_fwd_dma_kernel<true>.
Run with -s for the worst record error per family as a fraction of its bound."""
import collections
import ctypes
import zlib

import pytest
import torch

import bwd_epilogue_cases as bc
from conftest import WINO_TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"

Shape = collections.namedtuple("Shape", "family name n h w cin cout k dil kernel tile few")


def _sh(family, name, nhw, cin, cout, k, dil, kernel, tile=0, few=False):
    return Shape(family, name, *nhw, cin, cout, k, dil, kernel, tile, few)


M126, M297, M400 = (2, 9, 7), (3, 11, 9), (4, 10, 10)
D1, D2, DMA = "conv_fwd_kernel<1,32,true>", "conv_fwd_kernel<2,32,true>", "conv_fwd_dma_kernel<true>"
SHAPES = [
    # ---- diga_conv2d_nhwc_f32_epi
    _sh("f32", "1x1_m126_c64", M126, 64, 64, 1, 1, D1),                 # one ragged chunk
    _sh("f32", "3x3d2_m297_c64", M297, 32, 64, 3, 2, D1),               # three chunks, the last with 41 rows
    _sh("f32", "1x1_m297_c96", M297, 32, 96, 1, 1, D2),                 # a 128-column tile whose upper 32 columns do not exist
    _sh("f32", "1x1_m297_c160", M297, 32, 160, 1, 1, D2),               # a partial second column tile
    _sh("f32", "1x1_m297_c256", M297, 256, 256, 1, 1, DMA),             # second 256-row tile: 41 rows, its second half inactive
    _sh("f32", "1x1_m297_c320", M297, 256, 320, 1, 1, DMA),
    _sh("f32", "1x1_m400_c256", M400, 256, 256, 1, 1, DMA),             # second half of the second tile: 16 rows
    _sh("f32", "1x1_m400_c320", M400, 256, 320, 1, 1, DMA),
    _sh("f32", "3x3d12_m169_c256", (1, 13, 13), 256, 256, 3, 12, D2),   # M < 256: the direct kernel (see the module docstring)
    _sh("f32", "3x3d12_m288_c256", (2, 12, 12), 256, 256, 3, 12, DMA),  # every off-centre tap dead
    # pointwise_persistent_ok: the PLAIN call runs on the persistent GEMM, the call with an epilogue must not (128-row records)
    _sh("f32", "1x1_m131112_c128", (1, 216, 607), 32, 128, 1, 1, D2, few=True),
]
for _fam, _k1, _k2 in (("bf16x3", "conv_fwd_x3w_kernel<1,false,true>", "conv_fwd_x3w_kernel<2,false,true>"),
                       ("twin", "conv_fwd_x3t8_kernel<1,true>", "conv_fwd_x3t8_kernel<2,true>")):
    # 256-row tiles: M = 297 leaves the second tile 41 rows (its second half beyond M), M = 400 leaves that half 16 rows
    for _cout, _kern in ((64, _k1), (160, _k2)):
        for _mn, _nhw in (("m297", M297), ("m400", M400)):
            SHAPES.append(_sh(_fam, f"1x1_{_mn}_c{_cout}", _nhw, 32, _cout, 1, 1, _kern))
            SHAPES.append(_sh(_fam, f"3x3d2_{_mn}_c{_cout}", _nhw, 32, _cout, 3, 2, _kern))
for _tile, _kern in ((2, "winoM_output_epi2_kernel<2>"), (4, "winoM_output_epi2_kernel<4>"), (6, "winoM_output_epi2_kernel<6>")):
    for _cout in (96, 320):                                             # 320: a second 256-channel block with 64 valid channels
        SHAPES.append(_sh("wino", f"t{_tile}_d1_m286_c{_cout}", (2, 13, 11), 32, _cout, 3, 1, _kern, tile=_tile))
        SHAPES.append(_sh("wino", f"t{_tile}_d2_m323_c{_cout}", (1, 17, 19), 32, _cout, 3, 2, _kern, tile=_tile))   # sub-images < a tile
for _cout in (64, 160):                                                 # the two bf16x6 kernels share drain_stage
    SHAPES.append(_sh("x6", f"1x1_m297_c{_cout}", M297, 64, _cout, 1, 1, f"conv_fwd_x6_kernel<{1 if _cout <= 64 else 2}> (pointwise, loader)"))
    SHAPES.append(_sh("x6taps", f"3x3d2_m297_c{_cout}", M297, 64, _cout, 3, 2, f"conv_fwd_x6_kernel<{1 if _cout <= 64 else 2}> (taps)"))

FEW = ("add", "add+bits+x+partials", "relu_ab+x+partials")
CASES = [(s, d) for s in SHAPES for d in bc.DESCRIPTORS if not s.few or d.id in FEW]
_id = lambda s: f"{s.family}-{s.name}"
ENTRY = {"f32": "diga_conv2d_nhwc_f32", "bf16x3": "diga_conv2d_nhwc_bf16x3", "twin": "diga_conv2d_nhwc_twin", "wino": "diga_conv2d_winograd_f32",
         "x6": "diga_conv2d_nhwc_bf16x6_f32in", "x6taps": "diga_conv_taps_bf16x6_f32in"}
WORST = {}                       # family -> (worst record error / bound, where)


@pytest.fixture(scope="module", autouse=True)
def _print_worst_record_ratio_per_family():
    yield
    for fam, (ratio, where) in sorted(WORST.items()):
        print(f"\n[bwd epilogue] {fam}: worst record error = {ratio:.3f} of its bound ({where})")


def _m(s):
    return s.n * s.h * s.w


def _pad(s):
    return s.dil * (s.k - 1) // 2


# ------------------------------------------------------------------------------------------------ the shape rules, copied
def _persistent_ok(s):
    """pointwise_persistent_ok (csrc/conv.hip) for a stride-1, offset-free call."""
    return s.k == 1 and s.cin % 32 == 0 and s.cout % 128 == 0 and -(-_m(s) // 256) * (s.cout // 128) >= 512


def _kernel_with_epilogue(s):
    tn = 2 if s.cout > 64 else 1
    if s.family == "f32":                                               # conv2d_f32: the persistent GEMM takes no epilogue
        if _m(s) >= 256 and s.cout >= 256 and s.k * s.k * s.cin >= 256:
            return DMA
        return D2 if tn == 2 else D1
    if s.family == "bf16x3":                                            # conv2d_bf16x3: the wide kernel while 32-bit offsets reach
        fits32 = _m(s) * s.cin < (1 << 31) and s.cout * s.k * s.k * s.cin < (1 << 31)
        return f"conv_fwd_x3w_kernel<{tn},false,true>" if fits32 else f"conv_fwd_x3p_kernel<{tn},true>"
    if s.family == "twin":                                              # conv2d_twin
        return f"conv_fwd_x3t8_kernel<{tn},true>"
    if s.family == "wino":                                              # winograd_conv
        return f"winoM_output_epi2_kernel<{s.tile}>"
    return f"conv_fwd_x6_kernel<{tn}> ({'taps' if s.family == 'x6taps' else 'pointwise, loader'})"


@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_shape_takes_the_kernel_it_is_here_for(s):
    from diga_amd import _lib
    assert _kernel_with_epilogue(s) == s.kernel
    geom = (s.n, s.h, s.w, s.cin, s.h, s.w, s.cout, s.k, s.k, 1, 1, _pad(s), _pad(s))
    math = {"f32": 0, "wino": 0, "bf16x3": 1, "twin": 1, "x6": 2, "x6taps": 2}[s.family]
    assert _lib.lib.diga_conv2d_epi_chunk_rows(*geom, math) == bc.CHUNK
    if s.few:                                                           # the plain call IS on the persistent GEMM (64-row statistics)
        assert _persistent_ok(s) and _lib.lib.diga_conv2d_stats_chunk_rows(*geom, 0) == 64
    else:
        assert not _persistent_ok(s)
    if s.family in ("bf16x3", "twin", "x6", "x6taps") or s.kernel == DMA:            # 256-row tiles: the last one's second half
        rows = _m(s) - (-(-_m(s) // 256) - 1) * 256
        assert rows == {297: 41, 400: 144, 288: 32}[_m(s)]              # 41 / 32: inactive half; 144: a half with 16 rows


# ------------------------------------------------------------------------------------------------ calls
def _conv_f64(x, wt, pad, dil):
    """out[n, y, x, c] = sum_{r, s, k} in[n, y + pad - r dil, x + pad - s dil, k] * wt[c][r][s][k], zeros outside the image, in float64
    (the backward-data geometry; for 3x3 with pad = dil this is also what the Winograd entry point computes with flip = 1)."""
    n, h, w, cin = x.shape
    c, r_, s_, _ = wt.shape
    xp = torch.zeros((n, h + 2 * pad, w + 2 * pad, cin), dtype=torch.float64, device=x.device)
    xp[:, pad:pad + h, pad:pad + w] = x.double()
    out = torch.zeros((n, h, w, c), dtype=torch.float64, device=x.device)
    for r in range(r_):
        for s in range(s_):
            y0, x0 = 2 * pad - r * dil, 2 * pad - s * dil
            out += xp[:, y0:y0 + h, x0:x0 + w] @ wt[:, r, s].double().t()
    return out


def _prepare(s, dy, wt):
    """The operands one family's entry points take, built once per shape (held alive by the cache)."""
    from diga_amd import _lib
    st = _lib.stream()
    if s.family == "bf16x3":
        hi, lo = (torch.empty(wt.numel(), dtype=torch.int16, device=DEV) for _ in range(2))
        _lib.call("diga_split_bf16", _lib.ptr(wt), _lib.ptr(hi), _lib.ptr(lo), wt.numel(), st)
        return dict(lead=[dy, hi, lo])
    if s.family == "twin":
        twin = torch.empty(_m(s) * s.cin * 4, dtype=torch.uint8, device=DEV)
        _lib.call("diga_make_twin", _lib.ptr(dy), s.cin, _lib.ptr(twin), _m(s), s.cin, st)
        img = torch.empty(_lib.lib.diga_split_bf16_image_bytes(s.cout, s.k * s.k, s.cin), dtype=torch.uint8, device=DEV)
        _lib.call("diga_split_bf16_image", _lib.ptr(wt), _lib.ptr(img), s.cout, s.k * s.k, s.cin, st)
        return dict(lead=[twin, img])
    if s.family == "wino":
        ws = torch.empty(_lib.lib.diga_conv2d_winograd_workspace_bytes(s.n, s.h, s.w, s.cin, s.cout, s.dil, s.tile), dtype=torch.uint8, device=DEV)
        assert ws.numel() > 0
        return dict(lead=[dy, wt], ws=ws)
    if s.family in ("x6", "x6taps"):
        from test_gpu_conv_bf16x6_taps import _image
        return dict(lead=[dy, _image(wt)])
    return dict(lead=[dy, wt])


def _run(s, prep, out, out_ld, epi):
    """One call: the plain entry point (epi None) or its `_epi` twin, writing [M][out_ld] rows into `out`."""
    from diga_amd import _lib
    tag, st, pad = _lib.PROF_TAGS.index("conv_bwd_data"), _lib.stream(), _pad(s)
    name = ENTRY[s.family] + ("" if epi is None else "_epi")
    lead = [_lib.ptr(t) for t in prep["lead"]]
    if s.family in ("x6", "x6taps"):
        lead.insert(1, s.cin)                                           # in_ld
    mid = [] if epi is not None else [None]                             # bias
    tail = [None if epi is None else ctypes.byref(epi)]                 # statistics / the descriptor
    if s.family == "wino":
        _lib.call(name, *lead, *mid, _lib.ptr(out), _lib.ptr(prep["ws"]), prep["ws"].numel(), s.n, s.h, s.w, s.cin, s.cin, s.cout, out_ld,
                  s.dil, s.tile, 1, *tail, None, tag, st)
        return
    geom = [s.n, s.h, s.w, s.cin] + ([s.cin] if s.family in ("f32", "bf16x3") else []) + \
           [s.h, s.w, s.cout, out_ld, s.k, s.k, 1, 1, pad, pad, -s.dil, -s.dil]
    _lib.call(name, *lead, *mid, _lib.ptr(out), *geom, *tail, tag, st)


_DATA = {}


def _data(s):
    """Seeded output gradient, layer weights, their transpose, the plain entry point's result, the float64 convolution and every
    epilogue operand of one shape: built once, shared by all its tests, never modified."""
    from diga_amd import _lib
    key = _id(s)
    if key not in _DATA:
        seed = zlib.crc32(key.encode()) % 100000
        g = torch.Generator().manual_seed(seed)
        m = _m(s)
        dy = torch.randn((s.n, s.h, s.w, s.cin), generator=g).to(DEV)
        w_layer = (torch.randn((s.cin, s.k, s.k, s.cout), generator=g) * (2.0 / (s.cin * s.k * s.k)) ** 0.5).to(DEV)    # [K][R][S][C]
        wt = torch.empty((s.cout, s.k, s.k, s.cin), dtype=torch.float32, device=DEV)
        _lib.call("diga_weight_transpose", _lib.ptr(w_layer), _lib.ptr(wt), s.cin, s.k * s.k, s.cout, _lib.stream())
        assert torch.equal(wt, w_layer.permute(3, 1, 2, 0))
        prep = _prepare(s, dy, wt)
        plain = torch.full((m, s.cout), float("nan"), dtype=torch.float32, device=DEV)
        _run(s, prep, plain, s.cout, None)
        torch.cuda.synchronize()
        o = bc.build_operands(m, s.cout, seed + 1)
        dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in o.items()}
        for name in ("addend", "x", "mask_y"):                          # the logical tensors ARE the padded ones' first Cout columns
            dev[name] = dev[name + "_p"][:, :s.cout]
        keep = {"none": None, "mask_y": bc.keep_mask({"mask_y": dev["mask_y"]}, (m, s.cout)),
                "bits": bc.keep_mask({"mask_bits": dev["mask_bits"]}, (m, s.cout)),
                "relu_ab": bc.keep_mask({"relu_ab": dev["relu_ab"], "x": dev["x"]}, (m, s.cout))}
        assert torch.equal(keep["bits"], keep["mask_y"]) and not torch.equal(keep["relu_ab"], keep["mask_y"])
        assert not bool(keep["relu_ab"][dev["relu_ab_zeros"]].any())      # x * a + b == 0 exactly: dropped (keep where > 0)
        _DATA[key] = dict(dy=dy, wt=wt, prep=prep, plain=plain, ref64=_conv_f64(dy, wt, _pad(s), s.dil).reshape(m, s.cout), ops=dev, keep=keep)
    return _DATA[key]


def _epilogue_call(s, d, data):
    """Runs descriptor d on shape s -> (out [M][Cout + 8] prefilled with the sentinel, partials prefilled with NaN or None)."""
    from diga_amd import _lib
    m, c, ops = _m(s), s.cout, data["ops"]
    out = torch.full((m, c + 8), bc.SENTINEL, dtype=torch.float32, device=DEV)
    part = torch.full((bc.partials_floats(m, c),), float("nan"), dtype=torch.float32, device=DEV) if d.partials else None
    addr = {k: ops[k].data_ptr() for k in ("mask_bits", "relu_ab", "mean", "invstd")}
    addr.update({k: ops[k + "_p"].data_ptr() for k in ("addend", "x", "mask_y")}, partials=part.data_ptr() if d.partials else None)
    ld = dict(addend=ops["addend_p"].shape[1], x=ops["x_p"].shape[1], mask_y=ops["mask_y_p"].shape[1], mask_bits=ops["mask_bits_ld"])
    assert ld["addend"] > c and ld["x"] > c and ld["mask_y"] > c and ld["mask_bits"] * 8 >= c + 24
    e = _lib.BwdEpilogue()
    for k, v in bc.descriptor_fields(d, addr, ld).items():
        setattr(e, k, v)
    _run(s, data["prep"], out, c + 8, e)
    return out, part


# ------------------------------------------------------------------------------------------------ 2. plain vs float64
@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_plain_entry_point_against_float64(s):
    data = _data(s)
    got, ref = data["plain"], data["ref64"]
    assert not torch.isnan(got).any()
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max()) / scale
    print(f"\n[bwd epilogue] {_id(s)} ({s.kernel}): plain vs float64 {err:.2e} of scale")
    if s.family in ("f32", "x6", "x6taps"):
        assert_close(got, ref, 1e-5, 3e-6 * scale, _id(s))
    elif s.family == "wino":
        assert err < WINO_TOL[s.tile][0], (_id(s), err)
    else:
        assert err < 3e-5, (_id(s), err)


def test_winograd_epilogue_refuses_64_channels():
    """`Cout > 64` is a rule of every Winograd entry point (include/diga_hip.h): answered with DIGA_EINVAL before anything is launched."""
    from diga_amd import _lib
    s = next(x for x in SHAPES if x.family == "wino" and x.tile == 4 and x.cout == 96)
    data = _data(s)
    out = torch.full((_m(s), 64), bc.SENTINEL, dtype=torch.float32, device=DEV)
    e = _lib.BwdEpilogue()
    e.addend, e.addend_ld = data["ops"]["addend_p"].data_ptr(), data["ops"]["addend_p"].shape[1]
    rc = _lib.lib.diga_conv2d_winograd_f32_epi(_lib.ptr(data["dy"]), _lib.ptr(data["wt"]), _lib.ptr(out), _lib.ptr(data["prep"]["ws"]),
                                               data["prep"]["ws"].numel(), s.n, s.h, s.w, s.cin, s.cin, 64, 64, s.dil, s.tile, 1, ctypes.byref(e), None,
                                               _lib.PROF_TAGS.index("conv_bwd_data"), _lib.stream())
    torch.cuda.synchronize()
    assert rc == -1 and "Cout %" in _lib.last_error(), (rc, _lib.last_error())
    assert bool((out == bc.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 1., 3., 4., 5. per descriptor
def _wino_terms(s):
    """The largest number of pixels behind one Winograd record: tiles per block x tile^2 (+ 4), blocks = ceil(M / 128) (winograd_conv)."""
    def phase_tiles(length):
        return sum(-(-(-(-(length - a) // s.dil)) // s.tile) for a in range(s.dil) if length > a)
    tiles = s.n * phase_tiles(s.h) * phase_tiles(s.w)
    tpb = -(-tiles // bc.n_chunks(_m(s)))
    return tpb * s.tile * s.tile + 4


@pytest.mark.parametrize("s,d", CASES, ids=[f"{_id(s)}-{d.id}" for s, d in CASES])
def test_epilogue_equals_its_definition(s, d):
    data = _data(s)
    m, c, ops = _m(s), s.cout, data["ops"]
    out, part = _epilogue_call(s, d, data)
    out2, part2 = _epilogue_call(s, d, data)
    torch.cuda.synchronize()
    who = f"{_id(s)} ({s.kernel}) {d.id}"
    g = out[:, :c]
    # 3. guards
    assert bool((out[:, c:] == bc.SENTINEL).all()), f"{who}: padding columns of out were written"
    assert not torch.isnan(g).any(), f"{who}: NaN in out ({int(torch.isnan(g).sum())} elements): a padding column or an unwritten element"
    # 1. out against the plain call: one fp32 add, one select
    v = data["plain"] + ops["addend"] if d.addend else data["plain"]
    want = v if d.mask == "none" else torch.where(data["keep"][d.mask], v, torch.zeros((), device=DEV))
    if not torch.equal(g, want):
        bad = (g != want).nonzero()
        r, ch = (int(t) for t in bad[0])
        raise AssertionError(f"{who}: {bad.shape[0]} of {g.numel()} elements differ from where(mask, plain + addend, 0); first at row {r} "
                             f"channel {ch}: got {float(g[r, ch])!r}, want {float(want[r, ch])!r} (plain {float(data['plain'][r, ch])!r}); "
                             f"rows {int(bad[:, 0].min())}..{int(bad[:, 0].max())}, channels {int(bad[:, 1].min())}..{int(bad[:, 1].max())}")
    # 5. run to run
    assert torch.equal(out, out2), f"{who}: out differs between two calls"
    if not d.partials:
        return
    assert torch.equal(part.view(torch.int32), part2.view(torch.int32)), f"{who}: partials differ between two calls"
    # 3. guards of the records
    nch = bc.n_chunks(m)
    used = nch * 2 * c
    assert not torch.isnan(part[:used]).any(), f"{who}: {int(torch.isnan(part[:used]).sum())} record floats unwritten (or NaN)"
    assert bool(torch.isnan(part[used:]).all()), f"{who}: floats beyond the ceil(M / 128) records were written"
    # 4. the records against their definition, from the device's own out and x
    rec = part[:used].view(nch, 2, c).double()
    if s.family == "wino":
        ref, mag = bc.chunk_sums(g, ops["x"], ops["mean"], ops["invstd"], chunk=m)
        rec, bound = rec.sum(0, keepdim=True), bc.record_bound(mag, _wino_terms(s))
    else:
        ref, mag = bc.chunk_sums(g, ops["x"], ops["mean"], ops["invstd"])
        bound = bc.record_bound(mag)
    diff = (rec - ref).abs()
    ratio = float(torch.where(bound > 0, diff / bound.clamp_min(1e-300), (diff > 0).double() * 1e30).max())
    if ratio > WORST.get(s.family, (-1.0, ""))[0]:
        WORST[s.family] = (ratio, f"{s.name} {d.id}")
    print(f"\n[bwd epilogue] {who}: worst record error = {ratio:.3f} of its bound")
    if ratio > 1.0:
        i = int(torch.argmax((diff - bound).reshape(-1)))
        ck, which, ch = i // (2 * c), (i // c) % 2, i % c
        raise AssertionError(f"{who}: record {ck} {'sum g' if which == 0 else 'sum g*xhat'} channel {ch}: got {float(rec.reshape(-1)[i])!r}, "
                             f"want {float(ref.reshape(-1)[i])!r}, bound {float(bound.reshape(-1)[i]):.3e} ({ratio:.2f} x)")


# ------------------------------------------------------------------------------------------------ diga_bn_bwd_partials
BN_SHAPES = [next(s for s in SHAPES if _id(s) == i) for i in ("f32-1x1_m126_c64", "f32-1x1_m297_c160", "bf16x3-1x1_m400_c64", "twin-3x3d2_m400_c160")]
assert [(_m(s), s.cout) for s in BN_SHAPES] == [(126, 64), (297, 160), (400, 64), (400, 160)]


@pytest.mark.parametrize("did", ["add+bits+x+partials", "relu_ab+x+partials"])
@pytest.mark.parametrize("s", BN_SHAPES, ids=_id)
def test_bn_bwd_partials_finalises_the_device_records(s, did):
    """diga_bn_bwd_partials on the g and the records the epilogue left, leading dimensions larger than C: dx against finalise() in
    float64 at test_trainable_batchnorm_backward_train_and_eval_vs_float64's 5e-6 of scale, against diga_bn_bwd fed the unmasked
    plain + addend and the same mask (the junction's y behind the bits; relu_ab itself) at the junction test's fused-against-plain
    1e-5 of scale; guard columns of dx untouched; dx_twin = 1 gives the bytes of diga_make_twin of the fp32 dx."""
    from diga_amd import _lib
    d = bc.BY_ID[did]
    data = _data(s)
    m, c, ops = _m(s), s.cout, data["ops"]
    out, part = _epilogue_call(s, d, data)
    chunk = _lib.lib.diga_conv2d_epi_chunk_rows(s.n, s.h, s.w, s.cin, s.h, s.w, c, s.k, s.k, 1, 1, _pad(s), _pad(s), {"f32": 0, "bf16x3": 1, "twin": 1}[s.family])
    assert chunk == 128
    ws = torch.empty(67 * c, dtype=torch.float32, device=DEV)
    ld_g, ld_x, ld_dx = out.shape[1], ops["x_p"].shape[1], c + 4

    def partials_call(dx, ld, twin):
        _lib.call("diga_bn_bwd_partials", _lib.ptr(out), ld_g, _lib.ptr(ops["x_p"]), ld_x, _lib.ptr(ops["gamma"]), _lib.ptr(ops["mean"]),
                  _lib.ptr(ops["invstd"]), _lib.ptr(dx), ld, m, c, twin, _lib.ptr(part), chunk, _lib.ptr(ws), ws.numel() * 4, _lib.stream())

    dx = torch.full((m, ld_dx), bc.SENTINEL, dtype=torch.float32, device=DEV)
    partials_call(dx, ld_dx, 0)
    torch.cuda.synchronize()
    assert bool((dx[:, c:] == bc.SENTINEL).all()) and not torch.isnan(dx).any()
    want = bc.finalise(out[:, :c], ops["x"], ops["gamma"], ops["mean"], ops["invstd"])
    e64 = float((dx[:, :c].double() - want).abs().max() / want.abs().max())
    # the unfused pair: diga_bn_bwd masks and reduces plain + addend itself
    dy = (data["plain"] + ops["addend"]) if d.addend else data["plain"].clone()
    dx_plain = torch.full((m, ld_dx), bc.SENTINEL, dtype=torch.float32, device=DEV)
    ws2 = torch.empty(_lib.lib.diga_norm_workspace_bytes(m, 1, c), dtype=torch.uint8, device=DEV)
    y, ab = (ops["mask_y_p"], None) if d.mask == "bits" else (None, ops["relu_ab"])
    _lib.call("diga_bn_bwd", _lib.ptr(dy), c, _lib.ptr(ops["x_p"]), ld_x, _lib.ptr(y), ops["mask_y_p"].shape[1], _lib.ptr(ab), _lib.ptr(ops["gamma"]),
              _lib.ptr(ops["mean"]), _lib.ptr(ops["invstd"]), _lib.ptr(dx_plain), ld_dx, None, 0, m, c, 1, 0, _lib.ptr(ws2), ws2.numel(), _lib.stream())
    torch.cuda.synchronize()
    e_pair = float((dx[:, :c].double() - dx_plain[:, :c].double()).abs().max() / dx_plain[:, :c].abs().max())
    print(f"\n[bwd epilogue] bn_bwd_partials {_id(s)} {did}: {e64:.2e} of scale vs float64, {e_pair:.2e} vs diga_bn_bwd")
    assert e64 < 5e-6, (_id(s), did, e64)
    assert e_pair < 1e-5, (_id(s), did, e_pair)
    # the twin form of the same dx
    twin = torch.full((m * c * 4,), 0x5A, dtype=torch.uint8, device=DEV)
    partials_call(twin, c, 1)
    want_twin = torch.empty_like(twin)
    _lib.call("diga_make_twin", _lib.ptr(dx), ld_dx, _lib.ptr(want_twin), m, c, _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(twin, want_twin), f"{int((twin != want_twin).sum())} of {twin.numel()} twin bytes differ"
