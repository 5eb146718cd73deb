"""The bits of the bf16x6 forward kernels (csrc/conv_bf16x6.h: every instantiation of conv_fwd_x6_kernel and conv_win_x6_kernel, and the
three elementwise kernels that make their operands): the cases behind tests/test_gpu_conv_bf16x6_fwd_bits.py and its fixture
tests/golden/x6_fwd_bits.json.

These kernels use no float atomics, so every buffer a call writes is reproducible bit for bit; the fixture keeps the SHA-256 of each
(pre-filled with NaN: an element left unwritten, or written where it was not before, changes the hash).  Inputs come from the CPU
generator of the existing tests (oracle.synth.gen), so they are the same on every machine.  Only entry points of the C ABI are called, so
the same file records from any revision -- on an MI355X:

    DIGA_LIB=<library of the revision to record> python tests/x6_fwd_bits_cases.py --record <commit> [--out <file>]

A case is (id, entry-point family, keyword arguments); `kernels(case)` restates the launchers' selection rule (conv2d_bf16x6: form x tn x
variant, the options form by tn; conv_window_bf16x6: the columns of diga_conv_window_bf16x6_plan; conv_up2_bf16x6: interior + ring where
diga_conv_up2_bf16x6_plan admits the call) so that the device-free test can say which instantiations the cases reach.
"""
import ctypes
import hashlib
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "x6_fwd_bits.json")
DEV = "cuda"
BWD_DATA = 12                    # DIGA_PROF_CONV_BWD_DATA

# (N, Hi, Wi, Cin): M = 2 * 13 * 13 = 338 rows = one full 256-row tile + a ragged one whose second half-group is empty; 3 K-steps per tap
N, H, W, CIN = 2, 13, 13, 96
COUTS = (40, 136)                # TN = 1 (one ragged column tile) / TN = 2 (two column tiles, the second ragged)


def _conv(cid, form, variant, cout, k=1, stride=1, pad=0, dil=1, off=None, h=H, w=W, cin=CIN, in_ld=None, opts=None, tag=0):
    """A call of conv2d_bf16x6's entry points: form pass / loader / taps, variant plain (with statistics) / epi / infer / opts."""
    oy, ox = off if off is not None else (-pad, -pad)
    up = opts["upsample_shift"] if opts else 0
    ho = ((h << up) + 2 * pad - dil * (k - 1) - 1) // stride + 1 if off is None else (h + stride - 1) // stride
    wo = ((w << up) + 2 * pad - dil * (k - 1) - 1) // stride + 1 if off is None else (w + stride - 1) // stride
    return (cid, "conv", dict(form=form, variant=variant, n=N, h=h, w=w, cin=cin, ho=ho, wo=wo, cout=cout, k=k, stride=stride, oy=oy, ox=ox,
                              dil=dil, in_ld=in_ld or cin, opts=opts, tag=tag))


def _window(cid, cout, k, pad, dil=1, h=13, w=21, cin=64, opts=None):
    up = opts["upsample_shift"] if opts else 0
    ho, wo = (h << up) + 2 * pad - dil * (k - 1), (w << up) + 2 * pad - dil * (k - 1)
    return (cid, "window", dict(n=N, h=h, w=w, cin=cin, ho=ho, wo=wo, cout=cout, k=k, oy=-pad, ox=-pad, dil=dil, opts=opts))


def _up2(cid, cin, opts):
    # source 10 x 18, 5 x 5, pad 2 on its 2x upsampling: output 20 x 36 = 3 x 3 tiles of 8 x 16, one of them interior
    return (cid, "up2", dict(n=N, h=10, w=18, cin=cin, ho=20, wo=36, cout=72, k=5, oy=-2, ox=-2, dil=1, opts=opts))


REFLECT_UP_TANH = dict(reflect_pad=1, upsample_shift=1, activation=1)


def cases():
    out = []
    for form in ("pass", "loader"):
        for variant in ("plain", "epi", "infer"):
            out += [_conv(f"pw/{form}/{variant}/cout{co}", form, variant, co) for co in COUTS]
        # the backward-data geometry: stride 2 with offsets that leave the image at the left and the bottom (rows of zero planes)
        out.append(_conv(f"pw/{form}/epi/cout136/stride2_off", form, "epi", 136, stride=2, off=(1, -1), tag=BWD_DATA))
    out.append(_conv("pw/loader/plain/cout40/slice_of_104", "loader", "plain", 40, in_ld=104))
    for variant in ("plain", "epi", "infer"):
        out += [_conv(f"taps/3x3/{variant}/cout{co}", "taps", variant, co, k=3, pad=1) for co in COUTS]
    # dilation 14: eight of the nine taps lie outside the image for every row of a tile (live_taps steps over them)
    out += [_conv(f"taps/3x3_dil14/plain/cout{co}", "taps", "plain", co, k=3, pad=14, dil=14) for co in COUTS]
    out += [_conv("taps/3x3_stride2/plain/cout136", "taps", "plain", 136, k=3, stride=2, pad=1),
            _conv("taps/3x3_stride2/epi/cout40", "taps", "epi", 40, k=3, stride=2, pad=1, tag=BWD_DATA),
            _conv("taps/7x7/plain/cout40", "taps", "plain", 40, k=7, pad=3), _conv("taps/7x7/infer/cout136", "taps", "infer", 136, k=7, pad=3),
            _conv("taps/1x1/plain/cout40", "taps", "plain", 40)]
    out += [_conv(f"taps/3x3/opts_reflect_up1_tanh/cout{co}", "taps", "opts", co, k=3, pad=1, opts=REFLECT_UP_TANH) for co in COUTS]
    # the window form: output 13 x 21 = 2 x 2 tiles of 8 x 16, ragged both ways; two 32-channel chunks (the window is loaded twice)
    out += [_window("win/3x3/cout3", 3, 3, 1), _window("win/3x3/cout72", 72, 3, 1), _window("win/3x3_dil2/cout72", 72, 3, 2, dil=2),
            _window("win/3x3_dil2/cout3", 3, 3, 2, dil=2), _window("win/7x7/cout3", 3, 7, 3),
            _window("win/3x3/opts_reflect_up1_tanh/cout3", 3, 3, 1, h=7, w=11, opts=REFLECT_UP_TANH),
            _window("win/3x3/opts_reflect_up1_tanh/cout72", 72, 3, 1, h=7, w=11, opts=REFLECT_UP_TANH)]
    out += [_up2("up2/5x5/cin32/zero_pad", 32, dict(reflect_pad=0, upsample_shift=1, activation=0)),
            _up2("up2/5x5/cin64/reflect_tanh", 64, REFLECT_UP_TANH)]
    out += [("wb/16x256_k64_cout136", "wb", dict(rows=256, batches=16, k=64, cout=136)),
            ("triplet/338x96_of_104", "triplet", dict(m=338, c=96, ld=104)),
            ("image/136x9x96", "image", dict(k=136, rs=9, c=96)), ("image/40x1x96", "image", dict(k=40, rs=1, c=96)),
            ("winograd/12x12_128to256_tile4", "winograd", dict(n=1, h=12, w=12, cin=128, cout=256, tile=4))]
    return out


# ------------------------------------------------------------------------------------------------------------------ the selection rule
VARIANTS = ("plain", "epi", "infer")
ALL_KERNELS = {f"fwd<{tn},{form},{v}>" for tn in (1, 2) for form in ("pass", "loader", "taps") for v in VARIANTS} | \
    {"fwd<1,taps,opt>", "fwd<2,taps,opt>", "fwd<2,loader,WB>", "win<16>", "win<64>", "win<64,ring>", "win<64,up2>",
     "make_triplet", "split_image3", "split_image3_batched"}


def _plan(name, n_out, *args):
    from diga_amd import _lib
    outs = [ctypes.c_int(-7) for _ in range(n_out)]
    return getattr(_lib.lib, name)(*args, *[ctypes.byref(o) for o in outs]), [o.value for o in outs]


def kernels(case):
    """The kernel instantiations the case's call launches (needs the library, no device)."""
    _, family, a = case
    if family == "conv":
        tn = 2 if a["cout"] > 64 else 1
        split = {"split_image3"} | ({"make_triplet"} if a["form"] == "pass" else set())
        return split | {f"fwd<{tn},taps,opt>" if a["variant"] == "opts" else f"fwd<{tn},{a['form']},{a['variant']}>"}
    if family in ("window", "up2"):
        o = a["opts"] or {}
        ok, (_, _, cols) = _plan("diga_conv_window_bf16x6_plan", 3, a["h"], a["w"], a["cin"], a["cout"], a["k"], a["k"], a["dil"], a["dil"],
                                 o.get("upsample_shift", 0))
        assert ok == 1, case
        if family == "window":
            return {"split_image3", f"win<{cols}>"}
        ok, _ = _plan("diga_conv_up2_bf16x6_plan", 2, a["h"], a["w"], a["cin"], a["cout"], a["ho"], a["wo"], a["k"], a["k"], a["oy"], a["ox"], 1, 1,
                      o["upsample_shift"], o["reflect_pad"])
        assert ok == 1 and cols == 64, case
        return {"split_image3", "win<64,ring>", "win<64,up2>"}
    return {"wb": {"split_image3", "fwd<2,loader,WB>"}, "triplet": {"make_triplet"}, "image": {"split_image3"},
            "winograd": {"split_image3_batched", "fwd<2,loader,WB>"}}[family]


# ------------------------------------------------------------------------------------------------------------------ running a case
def _randn(cid, *shapes):
    import torch
    from oracle import synth
    g = synth.gen(zlib.crc32(cid.encode()) % 10000)
    return [torch.randn(s, generator=g) for s in shapes]


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _image(w_krsc):
    """diga_split_bf16x6_image of [K][R][S][C] weights."""
    import torch
    from diga_amd import _lib
    k, r, s, c = w_krsc.shape
    img = torch.full((_lib.lib.diga_split_bf16x6_image_bytes(k, r * s, c),), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.call("diga_split_bf16x6_image", _lib.ptr(w_krsc), _lib.ptr(img), k, r * s, c, _lib.stream())
    return img


def _triplet(x, m, c, ld):
    import torch
    from diga_amd import _lib
    trip = torch.full((m * c * 6,), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.call("diga_make_triplet", _lib.ptr(x), ld, _lib.ptr(trip), m, c, _lib.stream())
    return trip


def _options(o):
    from diga_amd import _lib
    d = _lib.ConvOptions()
    d.reflect_pad, d.upsample_shift, d.activation = o["reflect_pad"], o["upsample_shift"], o["activation"]
    return d


def _run_conv(cid, a):
    import torch
    from diga_amd import _lib
    n, h, w, cin, ho, wo, cout, k, ld = a["n"], a["h"], a["w"], a["cin"], a["ho"], a["wo"], a["cout"], a["k"], a["in_ld"]
    m = n * ho * wo
    x, wt, b, addend, xe, ab, res = _randn(cid, (n, h, w, ld), (cout, k, k, cin), (cout,), (m, cout), (m, cout), (2, cout), (m, cout))
    xd = x.to(DEV)
    src = xd[..., ld - cin:] if ld > cin else xd                    # (a channel slice of the wider tensor: 16-byte aligned)
    img = _image((wt * (2.0 / (cin * k * k)) ** 0.5).to(DEV))
    out = _nan(m, cout)
    got, held = {"out": out}, [xd, img]
    geometry = (n, h, w, cin, ho, wo, cout, cout, k, k, a["stride"], a["stride"], a["oy"], a["ox"], a["dil"], a["dil"])
    if a["form"] == "pass":
        assert ld == cin
        trip = _triplet(xd, n * h * w, cin, cin)
        first, name = (_lib.ptr(trip),), "diga_conv2d_nhwc_bf16x6"
    else:
        first, name = (_lib.ptr(src), ld), "diga_conv_taps_bf16x6_f32in" if a["form"] == "taps" else "diga_conv2d_nhwc_bf16x6_f32in"
    infer_name = {"pass": "diga_infer_conv2d_nhwc_bf16x6", "loader": "diga_infer_conv2d_nhwc_bf16x6_f32in", "taps": "diga_infer_conv_taps_bf16x6_f32in"}
    bias = b.to(DEV)
    if a["variant"] == "plain":
        stats = got["stats"] = _nan(_lib.lib.diga_conv2d_stats_floats(n, ho, wo, cout))
        _lib.call(name, *first, _lib.ptr(img), _lib.ptr(bias), _lib.ptr(out), *geometry, _lib.ptr(stats), a["tag"], _lib.stream())
    elif a["variant"] == "opts":
        o = _options(a["opts"])
        _lib.call(name + "_opts", *first, _lib.ptr(img), _lib.ptr(bias), _lib.ptr(out), *geometry, None, ctypes.byref(o), a["tag"], _lib.stream())
    elif a["variant"] == "epi":
        # the whole epilogue: + addend, ReLU mask of fma(x, a, b), the {sum, sum * xhat} records
        e = _lib.BwdEpilogue()
        held += [addend.to(DEV), xe.to(DEV), ab.to(DEV), (ab[0] * 0.5).to(DEV), (ab[1].abs() + 0.5).to(DEV)]
        part = got["partials"] = _nan(((m + 63) // 64) * 2 * cout)
        e.addend, e.addend_ld, e.x, e.x_ld, e.relu_ab = _lib.ptr(held[2]), cout, _lib.ptr(held[3]), cout, _lib.ptr(held[4])
        e.mean, e.invstd, e.partials = _lib.ptr(held[5]), _lib.ptr(held[6]), _lib.ptr(part)
        _lib.call(name + "_epi", *first, _lib.ptr(img), _lib.ptr(out), *geometry, ctypes.byref(e), a["tag"], _lib.stream())
    else:
        e = _lib.InferEpilogue()
        held += [ab.to(DEV), res.to(DEV)]
        e.ab, e.residual, e.residual_ld, e.relu = _lib.ptr(held[2]), _lib.ptr(held[3]), cout, 1
        _lib.call(infer_name[a["form"]], *first, _lib.ptr(img), _lib.ptr(bias), _lib.ptr(out), *geometry, ctypes.byref(e), a["tag"], _lib.stream())
    torch.cuda.synchronize()
    return got


def _run_window(cid, family, a):
    import torch
    from diga_amd import _lib
    n, h, w, cin, ho, wo, cout, k = a["n"], a["h"], a["w"], a["cin"], a["ho"], a["wo"], a["cout"], a["k"]
    x, wt, b = _randn(cid, (n, h, w, cin), (cout, k, k, cin), (cout,))
    xd, wd, bias = x.to(DEV), (wt * (2.0 / (cin * k * k)) ** 0.5).to(DEV), b.to(DEV)
    img, out = _image(wd), _nan(n * ho * wo, cout)
    o = _options(a["opts"]) if a["opts"] else None
    got = {"out": out}
    if family == "window":
        _lib.call("diga_conv_window_bf16x6_f32in", _lib.ptr(xd), cin, _lib.ptr(img), _lib.ptr(bias), _lib.ptr(out), n, h, w, cin, ho, wo, cout, cout,
                  k, k, a["oy"], a["ox"], a["dil"], a["dil"], ctypes.byref(o) if o else None, 0, _lib.stream())
    else:
        ok, (rc, sc) = _plan("diga_conv_up2_bf16x6_plan", 2, h, w, cin, cout, ho, wo, k, k, a["oy"], a["ox"], 1, 1, o.upsample_shift, o.reflect_pad)
        assert ok == 1
        wc = got["collapsed"] = _nan(4, cout, rc, sc, cin)
        _lib.call("diga_collapse_up2_weights", _lib.ptr(wd), _lib.ptr(wc), cout, k, k, cin, a["oy"], a["ox"], _lib.stream())
        phases = torch.cat([_image(wc[p]) for p in range(4)])
        _lib.call("diga_conv_up2_bf16x6_f32in", _lib.ptr(xd), cin, _lib.ptr(img), _lib.ptr(phases), _lib.ptr(bias), _lib.ptr(out), n, h, w, cin, ho, wo,
                  cout, cout, k, k, a["oy"], a["ox"], ctypes.byref(o), 0, _lib.stream())
    torch.cuda.synchronize()
    return got


def _run_other(cid, family, a):
    import torch
    from diga_amd import _lib
    if family == "triplet":
        (x,) = _randn(cid, (a["m"], a["ld"]))
        got = {"triplet": _triplet(x.to(DEV), a["m"], a["c"], a["ld"])}
    elif family == "image":
        (wt,) = _randn(cid, (a["k"], a["rs"], 1, a["c"]))
        got = {"image": _image(wt.to(DEV))}
    elif family == "wb":
        rows, batches, k, cout = a["rows"], a["batches"], a["k"], a["cout"]
        x, wt = _randn(cid, (batches * rows, k), (batches, cout, 1, 1, k))
        xd, imgs, out = x.to(DEV), torch.cat([_image(wb.to(DEV)) for wb in wt]), _nan(batches * rows, cout)
        _lib.call("diga_gemm_batched_bf16x6_f32in", _lib.ptr(xd), rows, batches, k, _lib.ptr(imgs), cout, _lib.ptr(out), _lib.stream())
        got = {"out": out}
    else:
        # the Winograd entry point builds the batched weight images (split_image3_batched_kernel) in its workspace: kept whole
        n, h, w, cin, cout, tile = a["n"], a["h"], a["w"], a["cin"], a["cout"], a["tile"]
        x, wt, b = _randn(cid, (n, h, w, cin), (cout, 3, 3, cin), (cout,))
        xd, wd, bias, out = x.to(DEV), (wt * (2.0 / (cin * 9)) ** 0.5).to(DEV), b.to(DEV), _nan(n * h * w, cout)
        nbytes = _lib.lib.diga_conv2d_winograd_bf16x6_workspace_bytes(n, h, w, cin, cout, 1, tile)
        assert nbytes > 0
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        _lib.call("diga_conv2d_winograd_bf16x6", _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bias), _lib.ptr(out), None, _lib.ptr(ws), nbytes, n, h, w, cin, cin,
                  cout, cout, 1, tile, 0, None, None, None, 0, _lib.stream())
        got = {"out": out, "workspace": ws}
    torch.cuda.synchronize()
    return got


def run(case):
    """{buffer name: tensor} of every buffer the case's call writes."""
    cid, family, a = case
    if family == "conv":
        return _run_conv(cid, a)
    if family in ("window", "up2"):
        return _run_window(cid, family, a)
    return _run_other(cid, family, a)


def sha256(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def load_fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


def record(commit, path):
    """Runs every case on the visible device and writes {commit, case id: {buffer: SHA-256 of its bytes}} to `path`."""
    got = {c[0]: {k: sha256(v) for k, v in run(c).items()} for c in cases()}
    with open(path, "w") as fh:
        json.dump({"recorded_from": commit, "sha256": got}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return got


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if "--record" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
        got = record(sys.argv[sys.argv.index("--record") + 1], path)
        print(f"{len(got)} cases -> {path}")
