"""The bits of the exact-fp32 LDS-DMA kernels of csrc/conv.hip -- gemm_f32_persistent_kernel (all eight instantiations),
conv_fwd_dma_kernel (plain and with the backward-data epilogue) and conv_wgrad_dma_kernel -- : the cases behind
tests/test_gpu_f32_gemm_bits.py and its fixture tests/golden/f32_gemm_bits.json.

None of these kernels uses float atomics and split-K sums are added in fixed order, so every buffer a call writes is reproducible bit
for bit; the fixture keeps the SHA-256 of each (pre-filled with NaN / 0xFF bytes: an element left unwritten, or written where it was
not before, changes the hash).  Inputs come from the CPU generator of the existing tests (oracle.synth.gen) and from
bwd_epilogue_cases.build_operands, so they are the same on every machine.  Only entry points of the C ABI are called, so the same file
records from any revision -- on an MI355X:

    DIGA_LIB=<library of the revision to record> python tests/f32_gemm_bits_cases.py --record <commit> [--out <file>]

A case is (id, family, keyword arguments).  `kernel(case)` restates the host's selection rule (conv2d_f32, gemm_batched_f32_dma,
diga_conv2d_wgrad_nhwc_f32, wgrad_batched_f32_dma) so that the device-free test can say that the cases reach every kernel and every
shape class named below.

Persistent kernel (>= 512 tiles of 256 x 128 on 256 blocks; rest = tiles mod 256 is the last round, and 0 < rest <= 128 is where a plan
could hand its tiles out as two half tiles each -- "split" below):
    M = 33 024 = 129 row tiles; Cout 512 -> 516 tiles, rest 4; Cout 640 -> 645 tiles, rest 133; K = 32 (one K-step per tile: the
    ring holds three tiles at once), 64, 96; ragged M = 33 024 - 200: the last row tile keeps 56 valid rows (one live wave piece).
"""
import ctypes
import hashlib
import json
import os
import sys
import zlib

import bwd_epilogue_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "f32_gemm_bits.json")
DEV = "cuda"
BWD_DATA = 12                    # DIGA_PROF_CONV_BWD_DATA
BLOCKS = 256                     # one per CU

# pointwise geometries (N, H, W) by M
GEOM = {33024: (1, 129, 256), 33024 - 200: (1, 88, 373), 127 * 256 - 56: (1, 8, 4057), 1056 + 17: (1, 29, 37)}
FULL, RAGGED, UNDER = 33024, 33024 - 200, 127 * 256 - 56
VARIANTS = ("plain", "bias", "stats", "stats+bias", "inf", "inf+bias", "inf+res", "inf+res+bias")
WINO = dict(n=1, h=192, w=192, d=1, tile=6)          # 32 x 32 tiles of 6 x 6 = 1024 tile rows, 64 products


def cases():
    out = []
    # every shape class on the plain instantiation
    for m in (FULL, RAGGED):
        for cout, k in ((512, 64), (640, 64), (512, 32), (512, 96)):
            out.append((f"pw/m{m}/cout{cout}/k{k}/plain", "pw", dict(m=m, cout=cout, k=k, variant="plain")))
    # every instantiation on the two shapes whose last round is the 4 tiles of the last row tile, full and ragged
    for m in (FULL, RAGGED):
        out += [(f"pw/m{m}/cout512/k64/{v}", "pw", dict(m=m, cout=512, k=64, variant=v)) for v in VARIANTS[1:]]
    out.append(("wino/fwd", "wino", dict(cin=64, cout=256, flip=0)))
    out.append(("wino/bwd_data", "wino", dict(cin=64, cout=256, flip=1)))
    out.append(("dma/under/plain", "pw", dict(m=UNDER, cout=512, k=256, variant="plain")))
    out.append(("dma/under/epi", "epi", dict(m=UNDER, cout=512, k=256, did="add+bits+x+partials")))
    out.append(("wgrad/1x1/m1073", "wgrad", dict(geom=GEOM[1056 + 17], cout=256, cin=128, r=1)))
    # 3 x 3: 9 taps x 27 pixel ranges of 17 K-steps, the last one of 8 with a ragged end (14 399 pixels)
    out.append(("wgrad/3x3/m14399", "wgrad", dict(geom=(1, 121, 119), cout=256, cin=128, r=3)))
    # (the Winograd weight gradient needs Cin % 128 == 0: the 192 x 192 image with 128 -> 256 channels)
    out.append(("wino/wgrad", "winowgrad", dict(cin=128, cout=256)))
    return out


# ------------------------------------------------------------------------------------------------------------------ the selection rule
def _ceil(a, b):
    return -(-a // b)


def plan_wgrad_wide(m, cout, cin, rs):
    """(splits, steps_per_split) of plan_wgrad_wide (csrc/conv.hip)."""
    tiles, ksteps = _ceil(cout, 256) * _ceil(cin, 128) * rs, _ceil(m, 32)
    best, best_eff = 1, 0.0
    for rounds in range(1, 5):
        sp = max(1, 256 * rounds // tiles)
        if ksteps // sp < 16:
            continue
        blocks = tiles * sp
        eff = blocks / (256.0 * _ceil(blocks, 256))
        if eff > best_eff + 0.02:
            best_eff, best = eff, sp
    steps = _ceil(ksteps, best)
    return _ceil(ksteps, steps), steps


def kernel(case):
    """(kernel, properties) the case's call launches."""
    _, family, a = case
    if family in ("pw", "epi"):
        m, cout, k = a["m"], a["cout"], a["k"]
        tiles = _ceil(m, 256) * (cout // 128)
        if family == "pw" and k % 32 == 0 and cout % 128 == 0 and tiles >= 512:
            v = a["variant"]
            inst = ("stats" in v, "bias" in v, 2 if "res" in v else 1 if "inf" in v else 0)
            rest = tiles % BLOCKS
            return "gemm_f32_persistent_kernel", dict(inst=inst, rest=rest, split=0 < rest <= BLOCKS // 2, ragged=m % 256 != 0, ksteps=k // 32)
        assert m >= 256 and cout >= 256 and k >= 256
        return "conv_fwd_dma_kernel", dict(epi=family == "epi", tiles=tiles, ragged=m % 256 != 0)
    if family == "wino":
        tp = _ceil(WINO["h"], WINO["tile"]) * _ceil(WINO["w"], WINO["tile"])
        assert tp % 256 == 0
        tiles = (WINO["tile"] + 2) ** 2 * tp // 256 * (a["cout"] // 128)
        assert tiles >= 512
        return "gemm_f32_persistent_kernel", dict(inst=(False, False, 0), rest=tiles % BLOCKS, split=0 < tiles % BLOCKS <= BLOCKS // 2,
                                                  ragged=False, ksteps=a["cin"] // 32, batched=True)
    if family == "wgrad":
        n, h, w = a["geom"]
        m = n * h * w
        assert a["cout"] % 256 == 0 and a["cin"] % 128 == 0 and m >= 1024
        splits, steps = plan_wgrad_wide(m, a["cout"], a["cin"], a["r"] ** 2)
        return "conv_wgrad_dma_kernel", dict(splits=splits, ragged=m % 32 != 0, batched=False)
    tp = _ceil(WINO["h"], WINO["tile"]) * _ceil(WINO["w"], WINO["tile"])
    splits, steps = plan_wgrad_wide(tp, a["cout"], a["cin"], (WINO["tile"] + 2) ** 2)
    return "conv_wgrad_dma_kernel", dict(splits=splits, ragged=False, batched=True)


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


def _pw_geometry(n, h, w, cin, cout, out_ld):
    return (n, h, w, cin, cin, h, w, cout, out_ld, 1, 1, 1, 1, 0, 0, 1, 1)


def _run_pw(cid, a):
    from diga_amd import _lib
    m, cout, k, v = a["m"], a["cout"], a["k"], a["variant"]
    n, h, w = GEOM[m]
    # one layer per shape: the variants differ in the epilogue alone
    x, wt, bias, ab, res = _randn(f"pw/{m}/{cout}/{k}", (m, k), (cout, k), (cout,), (2, cout), (m, cout))
    x, wt = x.to(DEV), (wt * (2.0 / k) ** 0.5).to(DEV)
    bias = bias.to(DEV) if "bias" in v else None
    out = _nan(m, cout)
    got = {"out": out}
    geom = _pw_geometry(n, h, w, k, cout, cout)
    if "inf" in v:
        ab = ab.to(DEV)
        res = res.to(DEV) if "res" in v else None
        e = _lib.InferEpilogue(ab=ab.data_ptr(), residual=res.data_ptr() if res is not None else None, residual_ld=cout, relu=1)
        _lib.call("diga_conv2d_nhwc_f32_infer", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(out), *geom, ctypes.byref(e), 0, _lib.stream())
    else:
        stats = _nan(_lib.lib.diga_conv2d_stats_floats(n, h, w, cout)) if "stats" in v else None
        _lib.call("diga_conv2d_nhwc_f32", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(out), *geom, _lib.ptr(stats), 0, _lib.stream())
        if stats is not None:
            got["stats"] = stats
    import torch
    torch.cuda.synchronize()                                         # (the operands die with this frame)
    return got


def _run_epi(cid, a):
    from diga_amd import _lib
    m, cout, k, d = a["m"], a["cout"], a["k"], bc.BY_ID[a["did"]]
    n, h, w = GEOM[m]
    x, wt = _randn(f"pw/{m}/{cout}/{k}", (m, k), (cout, k))          # (the layer of the plain case)
    x, wt = x.to(DEV), (wt * (2.0 / k) ** 0.5).to(DEV)
    ops = {key: (v.to(DEV) if hasattr(v, "to") else v) for key, v in bc.build_operands(m, cout, zlib.crc32(cid.encode()) % 10000).items()}
    out = _nan(m, cout)
    part = _nan(bc.partials_floats(m, cout)) if d.partials else None
    addr = {key: ops[key].data_ptr() for key in ("mask_bits", "relu_ab", "mean", "invstd")}
    addr.update({key: ops[key + "_p"].data_ptr() for key in ("addend", "x", "mask_y")}, partials=part.data_ptr() if d.partials else None)
    ld = dict(addend=ops["addend_p"].shape[1], x=ops["x_p"].shape[1], mask_y=ops["mask_y_p"].shape[1], mask_bits=ops["mask_bits_ld"])
    e = _lib.BwdEpilogue()
    for key, v in bc.descriptor_fields(d, addr, ld).items():
        setattr(e, key, v)
    _lib.call("diga_conv2d_nhwc_f32_epi", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(out), *_pw_geometry(n, h, w, k, cout, cout), ctypes.byref(e), BWD_DATA,
              _lib.stream())
    import torch
    torch.cuda.synchronize()
    got = {"out": out}
    if d.partials:
        got["partials"] = part
    return got


def _run_wino(cid, a):
    from diga_amd import _lib
    n, h, w, d, tile = (WINO[key] for key in ("n", "h", "w", "d", "tile"))
    cin, cout = a["cin"], a["cout"]
    x, wt, bias = _randn(cid, (n, h, w, cin), (cout, 3, 3, cin), (cout,))
    x, wt, bias = x.to(DEV), (wt * (2.0 / (cin * 9)) ** 0.5).to(DEV), bias.to(DEV)
    out = _nan(n * h * w, cout)
    ws = _bytes(_lib.lib.diga_conv2d_winograd_workspace_bytes(n, h, w, cin, cout, d, tile))
    _lib.call("diga_conv2d_winograd_f32", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(ws), ws.numel(), n, h, w, cin, cin, cout, cout,
              d, tile, a["flip"], None, None, BWD_DATA if a["flip"] else 0, _lib.stream())
    import torch
    torch.cuda.synchronize()
    return {"out": out, "ws": ws}                                    # (the workspace holds the products M the GEMM wrote)


def _run_wgrad(cid, a):
    from diga_amd import _lib
    n, h, w = a["geom"]
    cout, cin, r = a["cout"], a["cin"], a["r"]
    dy, x = _randn(cid, (n, h, w, cout), (n, h, w, cin))
    dy, x = dy.to(DEV), x.to(DEV)
    dw = _nan(cout, r, r, cin)
    ws = _bytes(_lib.lib.diga_conv2d_wgrad_workspace_bytes(n, h, w, cout, cin, r, r))
    pad = r // 2
    _lib.call("diga_conv2d_wgrad_nhwc_f32", _lib.ptr(dy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(ws), ws.numel(), n, h, w, cin, cin, h, w, cout, cout, r, r,
              1, 1, -pad, -pad, 1, 1, 0, _lib.stream())
    import torch
    torch.cuda.synchronize()
    return {"dw": dw, "ws": ws}                                      # (the workspace holds the split-K slabs)


def _run_winowgrad(cid, a):
    from diga_amd import _lib
    n, h, w, d, tile = (WINO[key] for key in ("n", "h", "w", "d", "tile"))
    cin, cout = a["cin"], a["cout"]
    dy, x = _randn(cid, (n, h, w, cout), (n, h, w, cin))
    dy, x = dy.to(DEV), x.to(DEV)
    ws = _bytes(_lib.lib.diga_conv2d_wgrad_winograd_workspace_bytes(n, h, w, cin, cout, d, tile, 0))
    dw = _nan(cout, 3, 3, cin)
    _lib.call("diga_conv2d_wgrad_winograd_f32", _lib.ptr(dy), _lib.ptr(x), None, _lib.ptr(dw), _lib.ptr(ws), ws.numel(), n, h, w, cin, cin, cout, cout, d,
              tile, None, _lib.stream())
    import torch
    torch.cuda.synchronize()
    return {"dw": dw, "ws": ws}                                      # (V, Z, dU and the split-K slab)


def run(case):
    """{buffer name: tensor} of every buffer the case's call writes."""
    import torch
    cid, family, a = case
    got = {"pw": _run_pw, "epi": _run_epi, "wino": _run_wino, "wgrad": _run_wgrad, "winowgrad": _run_winowgrad}[family](cid, a)
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
