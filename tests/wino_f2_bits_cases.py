"""The bits of the F(2x2,3x3) Winograd passes (csrc/winograd.hip at tile = 2: weight, input, output, output with the backward-data
epilogue, dy and dw transforms): the cases behind tests/test_gpu_winograd_f2_bits.py and its fixture tests/golden/wino_f2_bits.json.

No kernel on these paths uses float atomics, so every buffer a call writes is reproducible bit for bit; the fixture keeps the SHA-256 of
each (pre-filled with NaN / 0xFF bytes: an element left unwritten, or written where it was not before, changes the hash).  The workspace
is hashed region by region (wino_layout / wino_wgrad_layout restated below): that pins the tile table, U, V and M (Z, dU and the split-K
slab for the weight gradient) directly, where `out` would pin them only through the end result.  Every region was the same in two runs of
the recorded revision; none is left out.  Inputs come from the CPU generator of the existing tests (oracle.synth.gen) and from
bwd_epilogue_cases.build_operands, so they are the same on every machine.  Only entry points of the C ABI are called, with tile = 2
throughout, so the same file records from any revision -- on an MI355X:

    DIGA_LIB=<library of the revision to record> python tests/wino_f2_bits_cases.py --record <commit> [--out <file>]

A case is (id, family, keyword arguments).  `kernels_f2(case)` restates which of the six hand-written F(2x2) kernels of the recorded
revision the call launched, `kernels(case)` which kernels it launches now (winograd_conv / winograd_wgrad: weight, input, then output or
epilogue by descriptor; input unless V was kept, dy, dw) -- the M = 2 instantiations of the tile templates, and wino_input_kernel, the
one hand-written pass that stayed because its template form measured slower -- so that the device-free test can say that the cases
reach all of them.
"""
import ctypes
import hashlib
import json
import os
import sys
import zlib

import bwd_epilogue_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wino_f2_bits.json")
DEV = "cuda"
TILE = 2
BWD_DATA = 12                    # DIGA_PROF_CONV_BWD_DATA

# (N, H, W, dilation)
G1 = (2, 13, 11, 1)              # odd both ways: ragged last tile rows and columns; T = 84 -> Tp = 256 (padding tiles); 3 record groups of
#                                  28 tiles: each of the 4 tile lanes of the epilogue transform walks 7 tiles
G2 = (1, 17, 19, 2)              # four phases of unequal sub-image size
G3 = (1, 5, 7, 6)                # sub-images smaller than a tile; phase a = 5 is empty on the H axis
GEOMS = {"g1": G1, "g2": G2, "g3": G3}
FEW = ("add", "add+bits+x+partials", "relu_ab+x+partials")


def cases():
    out = []
    for gname in ("g1", "g2", "g3"):
        for flip in (0, 1):
            # Cout 96: one partly filled 256-channel block, written into rows of 104 floats; 320: a second block with 64 valid channels
            out.append((f"fwd/{gname}/flip{flip}/cout96_ld104", "fwd", dict(geom=gname, cin=32, cout=96, out_ld=104, flip=flip)))
            out.append((f"fwd/{gname}/flip{flip}/cout320", "fwd", dict(geom=gname, cin=32, cout=320, out_ld=320, flip=flip)))
    out.append(("keep/g1/cout96", "keep", dict(geom="g1", cin=32, cout=96)))
    for cout in (96, 320):
        out += [(f"epi/g1/cout{cout}/{d.id}", "epi", dict(geom="g1", cin=32, cout=cout, did=d.id)) for d in bc.DESCRIPTORS]
    out += [(f"epi/g2/cout320/{did}", "epi", dict(geom="g2", cin=32, cout=320, did=did)) for did in FEW]
    for gname in ("g1", "g2"):
        for src in ("x", "v_kept"):
            out.append((f"wgrad/{gname}/from_{src}", "wgrad", dict(geom=gname, cin=128, cout=256, src=src, x6=False)))
    out.append(("x6/fwd/g1", "x6fwd", dict(geom="g1", cin=128, cout=256)))
    out.append(("x6/wgrad/g1/from_x", "wgrad", dict(geom="g1", cin=128, cout=256, src="x", x6=True)))
    return out


# ------------------------------------------------------------------------------------------------------------------ the selection rule
F2_KERNELS = {"wino_weight_kernel", "wino_input_kernel", "wino_output_kernel", "wino_output_epi_kernel", "wino_dy_kernel", "wino_dw_kernel"}
EPI2 = {f"winoM_output_epi2_kernel<2,float4,4,{a},{m},{s}>" for a in ("false", "true") for m in range(4) for s in ("false", "true")}
ALL_KERNELS = {"winoM_weight_kernel<2>", "wino_input_kernel", "winoM_output_kernel<2,float4>", "winoM_dy_kernel<2,float4>",
               "winoM_dw_kernel<2,float4>"} | EPI2
assert len(EPI2) == 16


def _epi2_name(d):
    # launch_output_epi2_m: ADD = an addend is given; MASK by the first of mask_y, mask_bits, relu_ab given; SUMS = partials given
    mask = {"none": 0, "mask_y": 1, "bits": 2, "relu_ab": 3}[d.mask]
    return f"winoM_output_epi2_kernel<2,float4,4,{str(d.addend).lower()},{mask},{str(d.partials).lower()}>"


def kernels_f2(case):
    """The hand-written F(2x2) kernels the case's call launched in the recorded revision."""
    _, family, a = case
    if family == "wgrad":                                            # (the keep call that makes v_kept: weight, input, output)
        return {"wino_dy_kernel", "wino_dw_kernel", "wino_input_kernel"} | ({"wino_weight_kernel", "wino_output_kernel"} if a["src"] == "v_kept" else set())
    return {"wino_weight_kernel", "wino_input_kernel", "wino_output_epi_kernel" if family == "epi" else "wino_output_kernel"}


def kernels(case):
    """The kernels the case's call launches: instantiations of the tile templates, and the hand-written input transform."""
    _, family, a = case
    fwd = {"winoM_weight_kernel<2>", "wino_input_kernel"}
    if family == "wgrad":
        own = {"winoM_dy_kernel<2,float4>", "winoM_dw_kernel<2,float4>"}
        return own | (fwd | {"winoM_output_kernel<2,float4>"} if a["src"] == "v_kept" else {"wino_input_kernel"})
    return fwd | {_epi2_name(bc.BY_ID[a["did"]]) if family == "epi" else "winoM_output_kernel<2,float4>"}


# ------------------------------------------------------------------------------------------------------------------ workspace regions
def _phase_tiles(length, d):
    return sum(-(-(-(-(length - a) // d)) // TILE) for a in range(d) if length > a)


def padded_tiles(n, h, w, d):
    t = n * _phase_tiles(h, d) * _phase_tiles(w, d)
    return t, -(-t // 256) * 256


def _regions(ws, sizes):
    """{name: slice of the uint8 workspace}: the named regions in order, then whatever is left ("rest": the split-K slab of the weight
    gradient where there is one, and the 64 spare bytes)."""
    got, o = {}, 0
    for name, nbytes in sizes:
        got["ws." + name] = ws[o:o + nbytes]
        o += nbytes
    assert 64 <= ws.numel() - o, (ws.numel(), o)
    got["ws.rest"] = ws[o:]
    return got


def _fwd_regions(ws, g, cin, cout, x6=False):
    from diga_amd import _lib
    n, h, w, d = g
    tp = padded_tiles(n, h, w, d)[1]
    sizes = [("tab", tp * 16), ("U", 16 * cout * cin * 4)] + ([("img", 16 * _lib.lib.diga_split_bf16x6_image_bytes(cout, 1, cin))] if x6 else []) + \
            [("V", 16 * tp * cin * 4), ("M", 16 * tp * cout * 4)]
    r = _regions(ws, sizes)
    assert r["ws.rest"].numel() == 64                                # wino_layout restated exactly
    return r


# ------------------------------------------------------------------------------------------------------------------ running a case
def _randn(cid, *shapes):
    import torch
    from oracle import synth
    g = synth.gen(zlib.crc32(cid.encode()) % 10000)
    return [torch.randn(s, generator=g) for s in shapes]


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _bytes(n):
    import torch
    assert n > 0
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)


def _layer(cid, g, cin, cout):
    n, h, w, _ = g
    x, wt, b = _randn(cid, (n, h, w, cin), (cout, 3, 3, cin), (cout,))
    return x.to(DEV), (wt * (2.0 / (cin * 9)) ** 0.5).to(DEV), b.to(DEV)


def _run_fwd(cid, a):
    from diga_amd import _lib
    g = GEOMS[a["geom"]]
    n, h, w, d = g
    cin, cout, ld = a["cin"], a["cout"], a["out_ld"]
    x, wt, bias = _layer(cid, g, cin, cout)
    out = _nan(n * h * w, ld)
    ws = _bytes(_lib.lib.diga_conv2d_winograd_workspace_bytes(n, h, w, cin, cout, d, TILE))
    _lib.call("diga_conv2d_winograd_f32", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(ws), ws.numel(), n, h, w, cin, cin, cout, ld,
              d, TILE, a["flip"], None, None, BWD_DATA if a["flip"] else 0, _lib.stream())
    got = {"out": out[:, :cout], **_fwd_regions(ws, g, cin, cout)}
    if ld > cout:
        got["out_rows"] = out                                        # (with the NaN the call must leave between the rows)
    return got


def _keep(cid, g, cin, cout):
    """diga_conv2d_winograd_f32_keep -> (out, v_keep, workspace)"""
    from diga_amd import _lib
    n, h, w, d = g
    x, wt, bias = _layer(cid, g, cin, cout)
    out = _nan(n * h * w, cout)
    v = _nan(_lib.lib.diga_conv2d_winograd_v_floats(n, h, w, cin, d, TILE))
    ws = _bytes(_lib.lib.diga_conv2d_winograd_workspace_bytes(n, h, w, cin, cout, d, TILE))
    _lib.call("diga_conv2d_winograd_f32_keep", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(v), _lib.ptr(ws), ws.numel(), n, h, w,
              cin, cin, cout, cout, d, TILE, None, None, 0, _lib.stream())
    return out, v, ws


def _run_keep(cid, a):
    g = GEOMS[a["geom"]]
    out, v, ws = _keep(cid, g, a["cin"], a["cout"])
    return {"out": out, "v_keep": v, **_fwd_regions(ws, g, a["cin"], a["cout"])}       # (ws.V stays 0xFF: V went to v_keep)


def _run_epi(cid, a):
    from diga_amd import _lib
    g = GEOMS[a["geom"]]
    n, h, w, dil = g
    cin, cout, d = a["cin"], a["cout"], bc.BY_ID[a["did"]]
    m = n * h * w
    x, wt, _ = _layer(f"epi/{a['geom']}/cout{cout}", g, cin, cout)   # (one layer per shape: the descriptors differ in the epilogue alone)
    ops = {k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in bc.build_operands(m, cout, zlib.crc32(a["geom"].encode()) % 10000 + cout).items()}
    out = _nan(m, cout)
    part = _nan(bc.partials_floats(m, cout)) if d.partials else None
    addr = {k: ops[k].data_ptr() for k in ("mask_bits", "relu_ab", "mean", "invstd")}
    addr.update({k: ops[k + "_p"].data_ptr() for k in ("addend", "x", "mask_y")}, partials=part.data_ptr() if d.partials else None)
    ld = dict(addend=ops["addend_p"].shape[1], x=ops["x_p"].shape[1], mask_y=ops["mask_y_p"].shape[1], mask_bits=ops["mask_bits_ld"])
    e = _lib.BwdEpilogue()
    for k, v in bc.descriptor_fields(d, addr, ld).items():
        setattr(e, k, v)
    ws = _bytes(_lib.lib.diga_conv2d_winograd_workspace_bytes(n, h, w, cin, cout, dil, TILE))
    _lib.call("diga_conv2d_winograd_f32_epi", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(out), _lib.ptr(ws), ws.numel(), n, h, w, cin, cin, cout, cout, dil, TILE,
              1, ctypes.byref(e), None, BWD_DATA, _lib.stream())
    got = {"out": out}
    if d.partials:
        got["partials"] = part
    import torch
    torch.cuda.synchronize()                                         # (the operands die with this frame)
    return got


def _run_wgrad(cid, a):
    from diga_amd import _lib
    g = GEOMS[a["geom"]]
    n, h, w, d = g
    cin, cout, x6 = a["cin"], a["cout"], a["x6"]
    (dy,) = _randn(cid, (n, h, w, cout))
    dy = dy.to(DEV)
    x, _, _ = _layer(cid + "/layer", g, cin, cout)
    v = _keep(cid + "/layer", g, cin, cout)[1] if a["src"] == "v_kept" else None
    sfx = "_bf16x6" if x6 else ""
    ws = _bytes(getattr(_lib.lib, f"diga_conv2d_wgrad_winograd{sfx}_workspace_bytes")(n, h, w, cin, cout, d, TILE, 0 if v is None else 1))
    dw = _nan(cout, 3, 3, cin)
    _lib.call("diga_conv2d_wgrad_winograd" + ("_bf16x6" if x6 else "_f32"), _lib.ptr(dy), _lib.ptr(x) if v is None else None, _lib.ptr(v), _lib.ptr(dw),
              _lib.ptr(ws), ws.numel(), n, h, w, cin, cin, cout, cout, d, TILE, None, _lib.stream())
    tp = padded_tiles(n, h, w, d)[1]
    sizes = [("tab", tp * 16)] + ([("V", 16 * tp * cin * 4)] if v is None else []) + [("Z", 16 * tp * cout * 4), ("dU", 16 * cout * cin * 4)]
    import torch
    torch.cuda.synchronize()
    return {"dw": dw, **_regions(ws, sizes)}


def _run_x6fwd(cid, a):
    from diga_amd import _lib
    g = GEOMS[a["geom"]]
    n, h, w, d = g
    cin, cout = a["cin"], a["cout"]
    x, wt, bias = _layer(cid, g, cin, cout)
    out = _nan(n * h * w, cout)
    ws = _bytes(_lib.lib.diga_conv2d_winograd_bf16x6_workspace_bytes(n, h, w, cin, cout, d, TILE))
    _lib.call("diga_conv2d_winograd_bf16x6", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(out), None, _lib.ptr(ws), ws.numel(), n, h, w, cin, cin,
              cout, cout, d, TILE, 0, None, None, None, 0, _lib.stream())
    return {"out": out, **_fwd_regions(ws, g, cin, cout, x6=True)}


def run(case):
    """{buffer name: tensor} of every buffer the case's call writes."""
    import torch
    cid, family, a = case
    got = {"fwd": _run_fwd, "keep": _run_keep, "epi": _run_epi, "wgrad": _run_wgrad, "x6fwd": _run_x6fwd}[family](cid, a)
    torch.cuda.synchronize()
    return got


def sha256(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def load_fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


def record(commit, path):
    """Runs every case TWICE on the visible device, requires the same hashes both times, and writes
    {commit, case id: {buffer: SHA-256 of its bytes}} to `path`."""
    got = {c[0]: {k: sha256(v) for k, v in run(c).items()} for c in cases()}
    again = {c[0]: {k: sha256(v) for k, v in run(c).items()} for c in cases()}
    differ = sorted((cid, k) for cid in got for k in got[cid] if got[cid][k] != again[cid][k])
    assert not differ, f"not reproducible between two runs: {differ}"
    with open(path, "w") as fh:
        json.dump({"recorded_from": commit, "sha256": got}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return got


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if "--record" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
        got = record(sys.argv[sys.argv.index("--record") + 1], path)
        print(f"{len(got)} cases, {sum(len(v) for v in got.values())} buffers, the same in two runs -> {path}")
