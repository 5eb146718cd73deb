#!/usr/bin/env python3
"""The frozen translator's folded pass (bench.py::translator_leg's workload: dec_s2t(enc_s(x)), x [8,3,768,768], random-init weights,
no_grad) under three settings, in alternated rounds on one box:

    mode0      conv_math 0 (exact fp32: the direct `_opts` kernels and fp32 Winograd with the mirror in the input transform)
    x6         conv_math 2, x6_split = "loader", x6_taps, x6_winograd            (x6_opts off: the 21 calls with options stay as in mode0)
    x6+opts    ... and x6_opts: those calls on the multi-tap bf16x6 kernels and on Winograd with bf16x6 products
    x6+win     ... and x6_window (--x6-window only): the stride-1 multi-tap layers the window rule admits on the window form
    x6+up2     ... and x6_up2 (--x6-up2 only): the upsampled layers diga_conv_up2_bf16x6_plan admits on phase-collapsed weights

    python tools/bench_translator.py [--rounds 3] [--reps 3] [--batch 8] [--size 768] [--layers] [--x6-window] [--x6-up2]

Per setting: conv.path_log and the `_opts` entry points of one pass, then ms per pass of every round (device events around --reps
passes), the median and the spread.  --layers adds the five distinct folded layer shapes one by one, x6 against x6+opts (and, with
--x6-window / --x6-up2, against x6+win / x6+up2; every round's time is printed, so the settings can be compared pair by pair).  Needs the GPU."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diga_amd import _lib, config  # noqa: E402
from diga_amd.model import conv as dc  # noqa: E402
from diga_amd.model.model_noaux import ImgDecoder, ImgEncoder  # noqa: E402

X6 = dict(conv_math=2, x6_split="loader", x6_taps=True, x6_winograd=True)
SETTINGS = [("mode0", dict(conv_math=0)), ("x6", dict(X6, x6_opts=False)), ("x6+opts", dict(X6, x6_opts=True))]
# the five distinct shapes with folded options, at the sizes of an H x W crop: (name, count, Cin, Cout, k, stride, pad, source divisor,
# (reflect_pad, upsample_shift, activation))
LAYERS = [("enc 4x4/2 64->128", 1, 64, 128, 4, 2, 1, 1, (1, 0, 0)), ("enc 4x4/2 128->256", 1, 128, 256, 4, 2, 1, 2, (1, 0, 0)),
          ("res 3x3 256->256", 16, 256, 256, 3, 1, 1, 4, (1, 0, 0)), ("dec up+5x5 256->128", 1, 256, 128, 5, 1, 2, 4, (1, 1, 0)),
          ("dec up+5x5 128->64", 1, 128, 64, 5, 1, 2, 2, (1, 1, 0)), ("dec 7x7 64->3 tanh", 1, 64, 3, 7, 1, 3, 1, (1, 0, 1))]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def logged(fn):
    """One call of fn with conv.path_log and the entry points recorded."""
    calls, orig = [], _lib.call
    _lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    dc.path_log = {}
    try:
        fn()
        torch.cuda.synchronize()
        return dict(dc.path_log), calls
    finally:
        _lib.call = orig
        dc.path_log = None


def opts_calls(calls):
    names = sorted({c for c in calls if c.endswith("_opts")})
    return ", ".join(f"{calls.count(n)} x {n}" for n in names) or "none"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--x6-window", action="store_true", help="add the setting x6+win: x6+opts with config.x6_window")
    ap.add_argument("--x6-up2", action="store_true", help="add the setting x6+up2: x6+win with config.x6_up2")
    a = ap.parse_args()
    if a.x6_window:
        SETTINGS.append(("x6+win", dict(X6, x6_opts=True, x6_window=True)))
    if a.x6_up2:
        SETTINGS.append(("x6+up2", dict(X6, x6_opts=True, x6_window=True, x6_up2=True)))
    if not torch.cuda.is_available():
        sys.exit("bench_translator: needs the GPU")
    dev = "cuda"
    torch.manual_seed(3)
    enc, dec = ImgEncoder().to(dev).eval(), ImgDecoder().to(dev).eval()
    x = torch.rand((a.batch, 3, a.size, a.size), device=dev) * 2 - 1
    times = {name: [] for name, _ in SETTINGS}
    out = {}
    with torch.no_grad():
        print(f"dec_s2t(enc_s(x)), x [{a.batch},3,{a.size},{a.size}], folded (no_grad), {torch.cuda.get_device_name(0)}")
        for name, cfg in SETTINGS:                   # warm-up of every setting's kernels, and what each one launches
            with config.override(**cfg):
                log, calls = logged(lambda: out.__setitem__(name, dec(enc(x))))
            print(f"{name:8s} path_log {sorted(log.items())}\n{'':8s} `_opts` calls: {opts_calls(calls)}")
        ref = out["mode0"].double()
        for name, _ in SETTINGS[1:]:
            print(f"{name:8s} max |rec - rec(mode0)| = {float((out[name].double() - ref).abs().max()):.2e}")
        out.clear()
        for r in range(a.rounds):
            for name, cfg in SETTINGS:
                with config.override(**cfg):
                    times[name].append(timed(lambda: dec(enc(x)), a.reps))
            print(f"round {r}: " + "  ".join(f"{name} {times[name][-1]:8.2f} ms" for name, _ in SETTINGS))
        for name, _ in SETTINGS:
            t = times[name]
            print(f"{name:8s} median {statistics.median(t):8.2f} ms per {a.batch} crops (min {min(t):.2f}, max {max(t):.2f})")
        if a.layers:
            print("\nper layer (ms per call; count = calls per pass; median [path] (rounds)), x6 (the fp32 `_opts` kernel) against "
                  + " and ".join(name for name, _ in SETTINGS[2:]) + ":")
            for lname, count, cin, cout, k, stride, pad, div, opts in LAYERS:
                m = dc.DigaConv2d(cin, cout, k, stride, padding=pad, bias=True).to(dev).eval()
                xs = torch.randn((a.batch, cin, a.size // div, a.size // div), device=dev).contiguous(memory_format=torch.channels_last)
                row, logs, ts = [], {}, {name: [] for name, _ in SETTINGS[1:]}
                for name, cfg in SETTINGS[1:]:
                    with config.override(**cfg):
                        logs[name], _ = logged(lambda: m(xs, opts=opts))
                for _ in range(a.rounds):                # alternated: round r of every setting back to back
                    for name, cfg in SETTINGS[1:]:
                        with config.override(**cfg):
                            ts[name].append(timed(lambda: m(xs, opts=opts), a.reps))
                for name, _ in SETTINGS[1:]:
                    row.append(f"{name} {statistics.median(ts[name]):7.3f} ms [{', '.join(k2[1] for k2 in logs[name])}] "
                               f"({', '.join(f'{t:.3f}' for t in ts[name])})")
                print(f"{lname:22s} x{count:<3d} " + "  |  ".join(row))
                del m, xs
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
