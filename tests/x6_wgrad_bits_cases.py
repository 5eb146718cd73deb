"""The dw bits of the bf16x6 weight-gradient kernels (csrc/conv_bf16x6.h: conv_wgrad_x6_kernel, all seven instantiations): the cases
behind tests/test_gpu_conv_bf16x6_wgrad_bits.py and its fixture tests/golden/x6_wgrad_bits.json.

The kernels add their split-K slabs in fixed order and use no atomics, so a dw is reproducible bit for bit; the fixture keeps the
SHA-256 of its bytes (dw pre-filled with NaN) per case.  Inputs come from the CPU generators of the existing tests (`_inputs`,
synth.gen), so they are the same on every machine.  Only entry points of the C ABI are called, so the same file records from any
revision -- on an MI355X:

    DIGA_LIB=<library of the revision to record> python tests/x6_wgrad_bits_cases.py --record <commit> [--out <file>]
"""
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "x6_wgrad_bits.json")
DEV = "cuda"

# the two (256, 128) shapes of test_gpu_conv_bf16x6_wgrad_tiles.py::test_wide_shape_runs_the_existing_entry_point
WIDE_CASES = [("t13_264x136", 2, 136, 17, 19, 264, 1, 1, 0, 1, False), ("t14_264x160_3x3", 1, 160, 9, 11, 264, 3, 1, 1, 1, False)]
PASS_FORM = ("t01_64x64_two_ranges", "t05_320x64_ragged_cout_tile", "t13_264x136")
# (rows, batches, Cout, Cin, pixel ranges): one range under the floor of 8 K-steps; two Cout tiles and three ranges
BATCHED = [(320, 16, 256, 128, 1), (800, 16, 512, 128, 3)]


def tile_cases():
    """(case tuple, pitched operands) of the twelve narrow-tile shapes and the two wide ones."""
    from test_gpu_conv_bf16x6_wgrad_tiles import CASES
    return [(c, pitched) for c, _, _, pitched in CASES] + [(c, False) for c in WIDE_CASES]


@functools.lru_cache(maxsize=None)
def _host_operands(name):
    """The case and its dy and x, NHWC on the host: computed once, shared by the forms of the case (nothing stays on the device)."""
    from test_gpu_conv_bf16x6 import _inputs
    case, pitched = next((c, p) for c, p in tile_cases() if c[0] == name)
    x, _, _, probe, _, _, _, _ = _inputs(case)
    return case, pitched, probe.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()


def _operands(name):
    """dy and x of a tile case on the device (channel slices of wider NaN-filled tensors where the case says so)."""
    from test_gpu_conv_bf16x6_wgrad_tiles import _pitched
    case, pitched, dy, xd = _host_operands(name)
    dy, xd = dy.to(DEV), xd.to(DEV)
    if pitched:
        xd, dy = _pitched(xd, 8, 4), _pitched(dy, 24, 8)
    return case, dy, xd


def _tiled(name):
    from test_gpu_conv_bf16x6_wgrad_tiles import _fit
    (_, _, cin, _, _, cout, k, stride, pad, dil, _), dy, xd = _operands(name)
    return _fit(dy, xd, cout, cin, k, stride, pad, dil)


def _wide(name):
    from test_gpu_conv_bf16x6_wgrad_tiles import _wide as wide
    (_, _, cin, _, _, cout, k, stride, pad, dil, _), dy, xd = _operands(name)
    return wide(dy, xd, cout, cin, k, stride, pad, dil)


def _pass(name):
    """The pass form: diga_make_triplet on dy and x, then diga_conv2d_wgrad_bf16x6 on the two triplet images."""
    import torch
    from diga_amd import _lib
    (_, n, cin, h, w, cout, k, stride, pad, dil, _), dy, xd = _operands(name)
    assert k == 1 and dy.is_contiguous() and xd.is_contiguous()
    ho, wo = dy.shape[1], dy.shape[2]
    trips = []
    for t, m, c in ((dy, n * ho * wo, cout), (xd, n * h * w, cin)):
        trip = torch.zeros(m * c * 6, dtype=torch.uint8, device=DEV)
        _lib.call("diga_make_triplet", _lib.ptr(t), c, _lib.ptr(trip), m, c, _lib.stream())
        trips.append(trip)
    nbytes = _lib.lib.diga_conv2d_wgrad_bf16x6_workspace_bytes(n, ho, wo, cout, cin, 1, 1)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dw = torch.full((cout, 1, 1, cin), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("diga_conv2d_wgrad_bf16x6", _lib.ptr(trips[0]), _lib.ptr(trips[1]), _lib.ptr(dw), _lib.ptr(ws), ws.numel(), n, h, w, cin, ho, wo,
              cout, 1, 1, stride, stride, -pad, -pad, dil, dil, _lib.stream())
    torch.cuda.synchronize()
    return dw


def _batched(rows, batches, cout, cin):
    """diga_wgrad_batched_bf16x6_f32in: dU [Cout][batches][Cin] = Z_b^T V_b."""
    import torch
    from diga_amd import _lib
    from oracle import synth
    g = synth.gen(9000 + rows + cout)
    z = torch.randn((batches, rows, cout), generator=g).to(DEV)
    v = (torch.randn((batches, rows, cin), generator=g) + 0.25).to(DEV)
    nbytes = _lib.lib.diga_wgrad_batched_bf16x6_workspace_bytes(rows, batches, cout, cin)
    assert nbytes >= 64
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    du = torch.full((cout, batches, cin), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("diga_wgrad_batched_bf16x6_f32in", _lib.ptr(z), _lib.ptr(v), _lib.ptr(du), _lib.ptr(ws), ws.numel(), rows, batches, cout, cin,
              _lib.stream())
    torch.cuda.synchronize()
    return du


def cases():
    """(case id, function returning the dw of the case): every tile shape through the tiled entry point and through the wide
    loader-form entry point of its tap count, three shapes through the pass form, two batched Winograd-domain products."""
    out = []
    for (c, _) in tile_cases():
        out.append((c[0] + "/tiled", functools.partial(_tiled, c[0])))
        out.append((c[0] + "/wide", functools.partial(_wide, c[0])))
    out += [(name + "/pass", functools.partial(_pass, name)) for name in PASS_FORM]
    out += [(f"batched_{rows}x{batches}_{cout}x{cin}", functools.partial(_batched, rows, batches, cout, cin)) for rows, batches, cout, cin, _ in BATCHED]
    return out


def sha256(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def load_fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


def record(commit, path):
    """Runs every case on the visible device and writes {commit, case id: SHA-256 of the dw bytes} to `path`."""
    got = {cid: sha256(run()) for cid, run in cases()}
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
