#!/usr/bin/env python3
"""Whole-step time of the DiGA warm-up step (student + EMA teacher, ResNet-101 DeepLabV2) under each convolution arithmetic, on
synthetic data -- the figure bench.py reports for its headline leg, for arithmetics bench.py cannot select (bf16x6).

    python tools/step_time.py [--math f32 bf16x6] [--batch 8] [--size 768 768] [--steps 5] [--warmup 2] [--rounds 2] [--serial-streams]
                              [--x6-split pass loader] [--x6-winograd off on] [--x6-taps off on]
                              [--x6-wgrad-tile wide fit]
The arithmetics are run alternately, `rounds` times each, in one process; every run builds fresh models from the same seed.
--serial-streams switches the teacher / weight-gradient side streams off (kernel times add up: what the arithmetic changes by itself).
--x6-split: the operand form(s) of bf16x6 (config.x6_split; "pass" = triplet passes, "loader" = split in the GEMMs' loader waves); with both,
bf16x6 runs once per form in every round (the two must agree on the losses bit for bit).
--x6-winograd: config.x6_winograd for the bf16x6 runs ("on": the Winograd-domain GEMMs of the 3x3 layers on bf16x6 too); with both, once each.
--x6-taps: config.x6_taps for the bf16x6 runs ("on": the multi-tap calls off Winograd and the stem on bf16x6 too); with both, once each.
--x6-wgrad-tile: config.x6_wgrad_tile for the bf16x6 runs ("fit": the loader-form weight gradients of the narrow layers on the tile that
fits them); with both, once each.
Prints ms per step and crops/s per run, the run's peak allocated / reserved device memory and the last step's losses (the arithmetics
must agree on them to rounding)."""
import argparse
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diga_amd import _lib, config, synthetic  # noqa: E402
from diga_amd.model import seg_model_noaux as sm  # noqa: E402
from diga_amd.model.model_noaux import SegModel  # noqa: E402
from diga_amd.train_step import DigaTrainer  # noqa: E402

MATH = {"f32": 0, "bf16x3": 1, "bf16x6": 2}


def run(math, batch, h, w, steps, warmup, serial=False, dev="cuda", x6_split="pass", x6_winograd=False, x6_taps=False,
        x6_wgrad_tile="wide"):
    cfg = config.DEFAULTS.replace(conv_math=MATH[math], x6_split=x6_split, x6_winograd=x6_winograd, x6_taps=x6_taps,
                                  x6_wgrad_tile=x6_wgrad_tile)
    if serial:
        cfg = cfg.serial_streams()
    prev = _lib.get_conv_math()
    _lib.set_conv_math(cfg.conv_math)
    try:
        torch.manual_seed(0)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        student, teacher = SegModel(arch=sm.RESNET101).to(dev), SegModel(arch=sm.RESNET101).to(dev)
        teacher.train()
        tr = DigaTrainer(student, teacher, rng=random.Random(1234), config=cfg)
        data = synthetic.warmup_batch(1234, batch, h, w, block=32, device=dev)
        it, out = 0, None
        for _ in range(warmup):
            tr.warmup_step(it, *data)
            it += 1
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            out = tr.warmup_step(it, *data)
            it += 1
        e.record()
        torch.cuda.synchronize()
        _lib.join_side()
        mem = (torch.cuda.max_memory_allocated() / 2 ** 30, torch.cuda.max_memory_reserved() / 2 ** 30)
        return s.elapsed_time(e) / steps, {k: round(float(v), 6) for k, v in out.items()}, mem
    finally:
        _lib.set_conv_math(prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--math", nargs="+", default=["f32", "bf16x6"], choices=sorted(MATH))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=[768, 768])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--serial-streams", action="store_true")
    ap.add_argument("--x6-split", nargs="+", default=["pass"], choices=["pass", "loader"], help="bf16x6 operand form(s) (config.x6_split)")
    ap.add_argument("--x6-winograd", nargs="+", default=["off"], choices=["off", "on"], help="config.x6_winograd for the bf16x6 runs")
    ap.add_argument("--x6-taps", nargs="+", default=["off"], choices=["off", "on"], help="config.x6_taps for the bf16x6 runs")
    ap.add_argument("--x6-wgrad-tile", nargs="+", default=["wide"], choices=["wide", "fit"], help="config.x6_wgrad_tile for the bf16x6 runs")
    a = ap.parse_args()
    for r in range(a.rounds):
        for math in a.math:
            for form, xw, xt, tile in ([(f, x, t, g) for f in a.x6_split for x in a.x6_winograd for t in a.x6_taps for g in a.x6_wgrad_tile]
                                       if math == "bf16x6" else [("pass", "off", "off", "wide")]):
                ms, out, mem = run(math, a.batch, a.size[0], a.size[1], a.steps, a.warmup, a.serial_streams, x6_split=form,
                                   x6_winograd=xw == "on", x6_taps=xt == "on", x6_wgrad_tile=tile)
                torch.cuda.empty_cache()
                label = math + ("/" + form + ("+wino" if xw == "on" else "") + ("+taps" if xt == "on" else "") + ("+fit" if tile == "fit" else "") if math == "bf16x6" else "")
                print(f"round {r + 1} {label:27s}: {ms:8.2f} ms per step = {a.batch * 1e3 / ms:6.2f} crops/s | peak {mem[0]:.2f} GiB allocated, "
                      f"{mem[1]:.2f} GiB reserved | last step: {out}", flush=True)


if __name__ == "__main__":
    main()
