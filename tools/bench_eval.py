#!/usr/bin/env python3
"""The offline validation pass with and without the eval-mode BatchNorm fold (config.fold_eval_bn), at the reference geometry
(G5/evaluate_val.py:60,73-93): ResNet-101 with the deterministic test weights in eval mode, ONE seeded 1024 x 2048 image and its
512 x 1024 half through diga_amd.evaluate.evaluate_two_scale.

    python tools/bench_eval.py [--pairs 3] [--images 10] [--warmup 2] [--height 1024] [--width 2048] [--families]
                               [--math f32|bf16x3|bf16x6] [--x6-split pass|loader] [--x6-winograd] [--x6-taps] [--fold-x6]

Without the last five the run is the active configuration's (its defaults come from the environment, as everywhere).  --math,
--x6-split, --x6-winograd and --x6-taps set the convolution arithmetic of BOTH forms; --fold-x6 (config.fold_eval_bn_x6) lets the fold reach the
bf16x6 kernels under --math bf16x6, where without it only the stem and the 3x3 layers fold.

After warm-up of both forms, `--pairs` times: `--images` calls with the fold off, then `--images` calls with it on, each group
between two HIP events (the whole call: resize, both forward passes, the fused argmax / confusion kernel).  Prints ms per
validation image for both forms of every pair, the launch counts of the convolution paths (conv.path_log) and the peak allocated
memory of one call in each form.  Fold off is the code path without the feature: it is the yardstick.  Results are bit-identical
either way (tests/test_gpu_infer_fold.py); the predictions of the two forms are compared here once more.  Sets no device state.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diga_amd import config  # noqa: E402
from diga_amd import evaluate as ev  # noqa: E402
from diga_amd.model import conv as dc  # noqa: E402
from diga_amd.model import seg_model_noaux as sm  # noqa: E402
from diga_amd.model.model_noaux import SegModel  # noqa: E402
from diga_amd.util.metrics import runningScore  # noqa: E402
from oracle import deeplab as od  # noqa: E402
from oracle import detweights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--images", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--families", action="store_true", help="also time one layer per kernel family, folded against conv + BatchNorm")
    ap.add_argument("--math", choices=["f32", "bf16x3", "bf16x6"], default=None, help="conv arithmetic of both forms (default: the active configuration's)")
    ap.add_argument("--x6-split", choices=["pass", "loader"], default=None, help="bf16x6 operand form (config.x6_split)")
    ap.add_argument("--x6-winograd", action="store_true", help="bf16x6 for the Winograd-domain GEMMs (config.x6_winograd)")
    ap.add_argument("--x6-taps", action="store_true", help="bf16x6 for the multi-tap calls off Winograd and the stem (config.x6_taps)")
    ap.add_argument("--fold-x6", action="store_true", help="the fold inside the bf16x6 kernels as well (config.fold_eval_bn_x6)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on the GPU; none is visible")
    fields = {}
    if a.math is not None:
        fields["conv_math"] = {"f32": 0, "bf16x3": 1, "bf16x6": 2}[a.math]
    if a.x6_split is not None:
        fields["x6_split"] = a.x6_split
    if a.x6_winograd:
        fields["x6_winograd"] = True
    if a.x6_taps:
        fields["x6_taps"] = True
    if a.fold_x6:
        fields["fold_eval_bn_x6"] = True
    with config.override(**fields):
        run(a)


def run(a):
    dev = "cuda"
    cfg = config.active()
    math = ("fp32", "bf16x3", "bf16x6")[cfg.conv_math]
    if cfg.conv_math == 2:
        math += f" ({cfg.x6_split}{', x6_winograd' if cfg.x6_winograd else ''}{', x6_taps' if cfg.x6_taps else ''}{', fold_eval_bn_x6' if cfg.fold_eval_bn_x6 else ''})"
    m = SegModel(arch=sm.RESNET101)
    m.load_state_dict(detweights.state_dict(od.RESNET101))
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(1234)
    img = (torch.rand((1, 3, a.height, a.width), generator=g) * 2.0 - 1.0).to(dev)
    gt = torch.randint(0, 19, (1, a.height, a.width), generator=g).to(dev)
    rs = runningScore(19, verbose=False)

    def call(fold, want_pred=False):
        return ev.evaluate_two_scale(m, img, gt, rs, want_pred=want_pred, fold_bn=fold)

    preds, logs, peaks = {}, {}, {}
    for fold in (False, True):
        for _ in range(a.warmup):
            call(fold)
        torch.cuda.synchronize()
        dc.path_log = {}
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        preds[fold] = call(fold, want_pred=True)
        torch.cuda.synchronize()
        logs[fold], dc.path_log = dc.path_log, None
        peaks[fold] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    same = torch.equal(preds[False], preds[True])
    print(f"geometry 1 x 3 x {a.height} x {a.width} + half, ResNet-101, eval, {math}; predictions identical fold on/off: {same}")
    for fold in (False, True):
        fwd = {f"{k[1]}": v for k, v in sorted(logs[fold].items()) if k[0] == "fwd"}
        print(f"fold {'on ' if fold else 'off'}: conv launches per validation image {fwd} (sum {sum(fwd.values())}); "
              f"peak allocated above the resident set {peaks[fold]:.2f} GiB")

    def timed(fold):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.images):
            call(fold)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.images

    rows = []
    for p in range(a.pairs):
        off = timed(False)
        on = timed(True)
        rows.append((off, on))
        print(f"pair {p}: fold off {off:8.2f} ms / image   fold on {on:8.2f} ms / image   on/off {on / off:.4f}   ({a.images} images each)")
    off = sum(r[0] for r in rows) / len(rows)
    on = sum(r[1] for r in rows) / len(rows)
    print(f"mean  : fold off {off:8.2f} ms / image   fold on {on:8.2f} ms / image   on/off {on / off:.4f}   gain in every pair: "
          f"{all(r[1] < r[0] for r in rows)}")
    if not same:
        raise SystemExit("predictions differ between the two forms")
    if a.families:
        families(a, dev)


# per kernel family, one representative trunk layer at the full-resolution geometry (N = 1; 129 x 257 maps behind layer2, 257 x 513 in
# layer1): name, Cin, Cout, kernel, dilation, map, residual?
FAMILIES = [
    ("persistent GEMM + residual  (l3.conv3 256->1024)", 256, 1024, 1, 1, (129, 257), True),
    ("persistent GEMM             (l4.conv1 2048->512)", 2048, 512, 1, 1, (129, 257), False),
    ("LDS-DMA tiles               (l3.conv1 1024->256)", 1024, 256, 1, 1, (129, 257), False),
    ("LDS-DMA tiles + residual    (l1.conv3 64->256)  ", 64, 256, 1, 1, (257, 513), True),
    ("128 x 64 tiles, 3x3         (l1.conv2 64->64)   ", 64, 64, 3, 1, (257, 513), False),
    ("Winograd output transform   (l3.conv2 256, d 2) ", 256, 256, 3, 2, (129, 257), False),
]
# with config.fold_eval_bn_x6 under conv_math 2: one pointwise layer per column-tile width (TN) of conv_fwd_x6_kernel, each in both
# operand forms (x6_split)
X6_FAMILIES = [
    ("bf16x6 TN 1                 (l1.conv1 256->64)  ", 256, 64, 1, 1, (257, 513), False),
    ("bf16x6 TN 2                 (l3.conv1 1024->256)", 1024, 256, 1, 1, (129, 257), False),
    ("bf16x6 TN 2 + residual      (l3.conv3 256->1024)", 256, 1024, 1, 1, (129, 257), True),
]


def families(a, dev):
    """conv + diga_bn_fwd(eval) against the one folded launch, per kernel family: what decides a family's eligibility."""
    from diga_amd.model import norm as dn
    g = torch.Generator().manual_seed(4321)
    print("per kernel family, ms per layer call (two-module form / folded), warm, same tensors:")
    cases = [(f, {}) for f in FAMILIES]
    if config.active().conv_math == 2:
        print("  (conv_math 2: the pointwise rows run on bf16x6 in the active operand form; their labels name the fp32 kernels of mode 0)")
    if config.active().conv_math == 2 and config.active().fold_eval_bn_x6:
        cases += [((f"{f[0][:-1]} {split:6s}",) + f[1:], {"x6_split": split}) for f in X6_FAMILIES for split in ("pass", "loader")]
    for (name, cin, cout, k, d, (h, w), with_res), extra in cases:
        conv = dc.DigaConv2d(cin, cout, k, padding=d * (k // 2), dilation=d, bias=False).to(dev)
        bn = dn.DigaBatchNorm2d(cout).to(dev).eval()
        for p in bn.parameters():
            p.requires_grad = False
        with torch.no_grad():
            bn.running_var.copy_((0.5 + 1.5 * torch.rand(cout, generator=g)).to(dev))
            bn.running_mean.copy_((0.2 * torch.randn(cout, generator=g)).to(dev))
        x = torch.randn((1, cin, h, w), generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        res = torch.randn((1, cout, h, w), generator=g).to(dev).contiguous(memory_format=torch.channels_last) if with_res else None

        def run(fold):
            with torch.no_grad(), config.override(fold_eval_bn=fold, **extra):
                if fold:
                    assert conv.folds_eval_bn(x, bn, residual=res)
                    return conv(x, infer=(bn, res, True))
                return bn(conv(x), residual=res, relu=True)

        ms = {}
        same = torch.equal(run(False), run(True))
        for rep in range(2):                              # (alternated; the second round is reported)
            for fold in (False, True):
                run(fold)
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(20):
                    run(fold)
                e.record()
                torch.cuda.synchronize()
                ms[fold] = s.elapsed_time(e) / 20
        print(f"  {name}: {ms[False]:7.3f} / {ms[True]:7.3f} ms   folded/unfolded {ms[True] / ms[False]:.3f}   bit-identical: {same}")


if __name__ == "__main__":
    main()
