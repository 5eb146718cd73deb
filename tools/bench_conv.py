#!/usr/bin/env python3
"""Per-shape timing of the conv kernels (forward, backward-data, backward-weight) on the layer
geometries of ResNet-101 DeepLabV2 at the C2 size (16 images of 768x768 -> 193x193 / 97x97 maps).

    python tools/bench_conv.py [--images 16] [--reps 5] [--math f32|bf16x3|bf16x6] [--x6-split pass|loader] [--pointwise-only]
                                 [--x6-winograd] [--winograd-only] [--x6-taps] [--no-winograd] [--winograd-max-tile 2|4|6] [--taps-only]
                                 [--x6-wgrad-tile wide|fit] [--narrow-only]
Prints one line per (shape, pass): ms, TFLOP/s, fraction of the 157.3 TFLOP/s fp32 MFMA peak, and the
share of a training step's conv time that shape accounts for (count x time).
--math bf16x6: the pointwise layers run on bf16x6, the rest on the exact-fp32 paths; the operand split passes are part of the
figures (forward: inside the timed call; backward: the elementwise launches -- triplet of dy, weight images -- are added to dgrad).
--x6-split loader: the bf16x6 GEMMs split their fp32 operands in the loader waves (config.x6_split): no triplet passes, the weight
images remain.
--x6-winograd (with --math bf16x6): the Winograd-domain GEMMs of the stride-1 3x3 layers on bf16x6 too (config.x6_winograd); the batched
weight-image split is inside the timed calls.  --winograd-only: time the rows that take the Winograd path only.
--x6-taps (with --math bf16x6): the multi-tap calls Winograd does not take, and the stem's im2col GEMM, on bf16x6 too (config.x6_taps);
the weight-image split of the backward (booked as elementwise) is added to dgrad as for the pointwise rows.  --no-winograd sets
config.winograd = False for the run (every 3x3 row on the direct kernels -- or, with --x6-taps, on the multi-tap bf16x6 kernels);
--winograd-max-tile 2 is the F(2x2,3x3) cap of the "exact" setting.  --taps-only: time the rows with more than one tap only.
--x6-wgrad-tile fit (with --math bf16x6): the loader-form weight gradients on the tile that fits the layer (config.x6_wgrad_tile); the rows
whose weight gradient ran on a narrow tile are marked `fit` and summed on a line of their own.  --narrow-only: time the rows whose
(padded) channel counts pick a narrow tile only -- in any arithmetic, so the same rows can be timed in mode 0.
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diga_amd import _lib, config  # noqa: E402
from diga_amd.model import conv as dc  # noqa: E402
from diga_amd.model.conv import DigaConv2d  # noqa: E402

PEAK = 157.3          # fp32 MFMA peak; the split-bf16 mode is priced against 2500 / 3 = 833.3, bf16x6 against 2500 / 6 (see --math)
# name, count per forward, Cin, Cout, k, stride, dil, spatial (H=W)
SHAPES = [
    ("stem7x7", 1, 3, 64, 7, 2, 1, 768),
    ("l1.conv1.first", 1, 64, 64, 1, 1, 1, 193), ("l1.conv1", 2, 256, 64, 1, 1, 1, 193),
    ("l1.conv2", 3, 64, 64, 3, 1, 1, 193), ("l1.conv3", 3, 64, 256, 1, 1, 1, 193), ("l1.down", 1, 64, 256, 1, 1, 1, 193),
    ("l2.conv1.first", 1, 256, 128, 1, 2, 1, 193), ("l2.conv1", 3, 512, 128, 1, 1, 1, 97),
    ("l2.conv2", 4, 128, 128, 3, 1, 1, 97), ("l2.conv3", 4, 128, 512, 1, 1, 1, 97), ("l2.down", 1, 256, 512, 1, 2, 1, 193),
    ("l3.conv1.first", 1, 512, 256, 1, 1, 1, 97), ("l3.conv1", 22, 1024, 256, 1, 1, 1, 97),
    ("l3.conv2", 23, 256, 256, 3, 1, 2, 97), ("l3.conv3", 23, 256, 1024, 1, 1, 1, 97), ("l3.down", 1, 512, 1024, 1, 1, 1, 97),
    ("l4.conv1.first", 1, 1024, 512, 1, 1, 1, 97), ("l4.conv1", 2, 2048, 512, 1, 1, 1, 97),
    ("l4.conv2", 3, 512, 512, 3, 1, 4, 97), ("l4.conv3", 3, 512, 2048, 1, 1, 1, 97), ("l4.down", 1, 1024, 2048, 1, 1, 1, 97),
    ("aspp.1x1", 1, 2048, 256, 1, 1, 1, 97), ("aspp.d6", 1, 2048, 256, 3, 1, 6, 97), ("aspp.d12", 1, 2048, 256, 3, 1, 12, 97),
    ("aspp.d18", 1, 2048, 256, 3, 1, 18, 97), ("aspp.d24", 1, 2048, 256, 3, 1, 24, 97),
    ("aspp.bottleneck", 1, 1280, 256, 3, 1, 1, 97), ("head", 1, 256, 19, 1, 1, 1, 97),
]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def _wgrad_tile(cout, cin):
    """diga_wgrad_bf16x6_tile: the (BM, BN) tile config.x6_wgrad_tile = "fit" gives a weight gradient of these (padded) channel counts."""
    bm, bn = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("diga_wgrad_bf16x6_tile", cout, cin, ctypes.byref(bm), ctypes.byref(bn))
    return bm.value, bn.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--math", default="f32", choices=["f32", "bf16x3", "bf16x6"])
    ap.add_argument("--pointwise-only", action="store_true", help="time the 1x1 rows only (what --math bf16x6 changes)")
    ap.add_argument("--x6-split", default="pass", choices=["pass", "loader"], help="bf16x6 operand form (config.x6_split)")
    ap.add_argument("--x6-winograd", action="store_true", help="bf16x6 for the Winograd-domain GEMMs as well (config.x6_winograd)")
    ap.add_argument("--winograd-only", action="store_true", help="time the stride-1 3x3 rows of >= 128 channels only (what --x6-winograd changes)")
    ap.add_argument("--x6-taps", action="store_true", help="bf16x6 for the multi-tap calls off Winograd and the stem as well (config.x6_taps)")
    ap.add_argument("--no-winograd", action="store_true", help="config.winograd = False for the run")
    ap.add_argument("--winograd-max-tile", type=int, default=None, choices=[2, 4, 6], help="config.winograd_max_tile for the run")
    ap.add_argument("--taps-only", action="store_true", help="time the rows with more than one tap only (what --x6-taps can change)")
    ap.add_argument("--x6-wgrad-tile", default="wide", choices=["wide", "fit"], help="tile of the loader-form bf16x6 weight gradient (config.x6_wgrad_tile)")
    ap.add_argument("--narrow-only", action="store_true", help="time the rows that pick a narrow weight-gradient tile only (what --x6-wgrad-tile can change)")
    a = ap.parse_args()
    _lib.set_conv_math(a.math)
    config.active().x6_split = a.x6_split
    config.active().x6_winograd = a.x6_winograd
    config.active().x6_taps = a.x6_taps
    config.active().x6_wgrad_tile = a.x6_wgrad_tile
    if a.no_winograd:
        config.active().winograd = False
    if a.winograd_max_tile is not None:
        config.active().winograd_max_tile = a.winograd_max_tile
    global PEAK
    PEAK = {"bf16x3": 2500.0 / 3.0, "bf16x6": 2500.0 / 6.0}.get(a.math, 157.3)
    dev = "cuda"
    rows, tot = [], {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}
    pw = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}                 # the pointwise (1x1) rows alone
    wn = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}                 # the rows on the Winograd path (aspp.d24 stays direct: its ratio)
    tp = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}                 # the rows with more than one tap
    nr = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}                 # the rows that pick a narrow weight-gradient tile
    pad32 = lambda c: (c + 31) // 32 * 32  # noqa: E731
    for name, count, cin, cout, k, stride, dil, hw in SHAPES:
        wino_row = k == 3 and stride == 1 and cin >= 128 and cout >= 128 and name != "aspp.d24"
        if (a.only and a.only not in name) or (a.pointwise_only and k != 1) or (a.winograd_only and not wino_row) or (a.taps_only and k == 1):
            continue
        # the tile of the layer's weight-gradient GEMM (the stem's is the im2col GEMM: k * k * cin columns); the library's rule
        narrow = _wgrad_tile(pad32(cout), pad32(cin * k * k if cin == 3 else cin)) != (256, 128)
        if a.narrow_only and not narrow:
            continue
        pad = dil * (k - 1) // 2
        m = DigaConv2d(cin, cout, k, stride=stride, padding=pad, dilation=dil, bias=False).to(dev)
        x = torch.randn((a.images, hw, hw, cin), device=dev).permute(0, 3, 1, 2)
        need_dx = cin > 3
        x.requires_grad_(need_dx)
        y = m(x)
        gy = torch.randn_like(y)
        ho = y.shape[-1]
        flops = 2.0 * a.images * ho * ho * cout * cin * k * k

        def run_fwd():
            with torch.no_grad():
                m(x)

        t_f = timed(run_fwd, a.reps)

        # isolate the two backward kernels through the event profiler inside the library
        _lib.call("diga_prof_reset")
        dc.path_log = {}
        for _ in range(a.reps):
            m.weight.grad = None
            if need_dx:
                x.grad = None
            out = m(x)
            torch.cuda.synchronize()
            _lib.call("diga_prof_enable", 1)             # (the backward alone: the forward's own split passes are in t_f)
            out.backward(gy)
            torch.cuda.synchronize()
            _lib.call("diga_prof_enable", 0)
        nd, td = _lib.prof_query("conv_bwd_data")
        nw, tw = _lib.prof_query("conv_bwd_weight")
        t_d = td / nd if nd else 0.0
        t_w = tw / nw if nw else 0.0
        on_taps = any(arith.startswith("bf16x6") for (p, arith) in dc.path_log if p in ("dgrad", "wgrad"))
        on_fit = any(arith.endswith("/fit") for (p, arith) in dc.path_log if p == "wgrad")
        dc.path_log = None
        if a.math == "bf16x6" and (k == 1 or (a.x6_taps and on_taps)):
            # the split passes of the backward (triplet of dy, the weight image; booked as elementwise) belong to the layer's time
            ne, te = _lib.prof_query("elementwise")
            t_d += te / a.reps
        rows.append((name, count, flops, t_f, t_d, t_w, on_fit))
        tot["fwd"] += count * t_f
        tot["dgrad"] += count * t_d
        tot["wgrad"] += count * t_w
        if k == 1:
            pw["fwd"] += count * t_f
            pw["dgrad"] += count * t_d
            pw["wgrad"] += count * t_w
        if k > 1:
            tp["fwd"] += count * t_f
            tp["dgrad"] += count * t_d
            tp["wgrad"] += count * t_w
        if narrow:
            nr["fwd"] += count * t_f
            nr["dgrad"] += count * t_d
            nr["wgrad"] += count * t_w
        if wino_row:
            wn["fwd"] += count * t_f
            wn["dgrad"] += count * t_d
            wn["wgrad"] += count * t_w
        del m, x, y, gy
        torch.cuda.empty_cache()
    print(f"{'shape':18s} {'cnt':>3s} {'GFLOP':>8s} | {'fwd ms':>8s} {'TF/s':>6s} {'frac':>5s} | {'dgrad ms':>8s} {'TF/s':>6s} | "
          f"{'wgrad ms':>8s} {'TF/s':>6s} | share fwd/dgrad/wgrad")
    for name, count, flops, t_f, t_d, t_w, on_fit in rows:
        tf = lambda t: flops / (t * 1e-3) / 1e12 if t > 0 else 0.0  # noqa: E731
        print(f"{name:18s} {count:3d} {flops / 1e9:8.1f} | {t_f:8.3f} {tf(t_f):6.1f} {tf(t_f) / PEAK:5.2f} | {t_d:8.3f} {tf(t_d):6.1f} | "
              f"{t_w:8.3f} {tf(t_w):6.1f} | {100 * count * t_f / tot['fwd']:.1f}% {100 * count * t_d / max(tot['dgrad'], 1e-9):.1f}% "
              f"{100 * count * t_w / max(tot['wgrad'], 1e-9):.1f}%{' fit' if on_fit else ''}")
    print(f"sum over one forward: fwd {tot['fwd']:.1f} ms, dgrad {tot['dgrad']:.1f} ms, wgrad {tot['wgrad']:.1f} ms")
    print(f"pointwise rows, count-weighted ({a.math}{'/' + a.x6_split if a.math == 'bf16x6' else ''}): fwd {pw['fwd']:.2f} ms, dgrad {pw['dgrad']:.2f} ms, wgrad {pw['wgrad']:.2f} ms")
    print(f"winograd rows, count-weighted ({a.math}{'/x6-winograd' if a.x6_winograd else ''}): fwd {wn['fwd']:.2f} ms, dgrad {wn['dgrad']:.2f} ms, wgrad {wn['wgrad']:.2f} ms")
    setting = a.math + ("/x6-taps" if a.x6_taps else "") + ("/" + a.x6_wgrad_tile if a.math == "bf16x6" else "") + ("/no-winograd" if a.no_winograd else "") + (f"/tile{a.winograd_max_tile}" if a.winograd_max_tile else "")
    print(f"multi-tap rows, count-weighted ({setting}): fwd {tp['fwd']:.2f} ms, dgrad {tp['dgrad']:.2f} ms, wgrad {tp['wgrad']:.2f} ms")
    print(f"narrow-tile rows, count-weighted ({setting}): fwd {nr['fwd']:.2f} ms, dgrad {nr['dgrad']:.2f} ms, wgrad {nr['wgrad']:.2f} ms")


if __name__ == "__main__":
    main()
