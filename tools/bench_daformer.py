#!/usr/bin/env python3
"""The DAFormer head's kernels (csrc/dwconv.hip, the resize-into-a-slice kernels of csrc/pyramid.hip) against stock torch, and the whole
head with either, on one GPU in one process:  python tools/bench_daformer.py [--rounds R] [--reps K] [--only dw,resize,head] [--no-bw] [out.txt]

Geometry: the c5 student's -- 16 maps of 192 x 192 (768 x 768 crops at 1/4 scale), 1024 channels (4 x 256 embeddings), stage widths of
MiT-B5 (64 / 128 / 320 / 512), 256 fused channels, 19 classes.  The parent commit has no such path, so the yardstick is torch on the same
device: F.conv2d(groups=C) / torch.nn.grad.conv2d_input / conv2d_weight on channels-last tensors for the depthwise passes,
F.interpolate + a copy into the slice (what torch.cat does) for the resizes, and the head with both replaced by those compositions
(tests/daformer_cases.py::composed_raw_features, daformer_head.USE_TORCH_DEPTHWISE).  Every round times torch and the kernel one after
the other (alternated pairs), `reps` calls between two device events after a warm-up of both.  Reported per row: both times of every
pair, whether the kernel won EVERY pair, the least traffic (operands read once, results written once), the achieved bytes/s at the
kernel's best time and, at the end, what the project's bandwidth kernels reach on this box (bench.bandwidth_kernels)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

N, H, W, E, CH, K = 16, 192, 192, 256, 256, 19
C = 4 * E
STAGES = (64, 128, 320, 512)
LINES = []
TBS = {}


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def compare(title, stock, kernel, rounds, reps, min_bytes=None):
    """Alternated pairs; returns True when the kernel won every one."""
    for fn in (stock, kernel):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    pairs = [(timed(stock, reps), timed(kernel, reps)) for _ in range(rounds)]
    won = all(f < c for c, f in pairs)
    lost = all(f > c for c, f in pairs)
    best = min(f for _, f in pairs)
    tail = ""
    if min_bytes is not None:
        TBS[title] = min_bytes / (best * 1e-3) / 1e12
        tail = f"   least traffic {min_bytes / 1e6:7.1f} MB -> {TBS[title]:.2f} TB/s at the best kernel time"
    say(f"{title:40s} torch / kernel ms per call: " + "  ".join(f"{c:8.3f}/{f:8.3f}" for c, f in pairs)
        + f"   kernel wins every pair: {'yes' if won else 'NO'}{' (loses every pair)' if lost else ''}" + tail)
    return won


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="dw,resize,head")
    ap.add_argument("--no-bw", action="store_true", help="skip the project's bandwidth kernels (bench.bandwidth_kernels)")
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "diag_out", "bench_daformer.txt"))
    a = ap.parse_args()
    only = set(a.only.split(","))
    import daformer_cases as dc
    from diga_amd import _lib
    from diga_amd.model.networks import daformer_head as dh
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    say(f"device {torch.cuda.get_device_name(0)}; {N} maps of {H} x {W}, {C} channels; {a.rounds} alternated rounds of {a.reps} calls ({max(2, a.reps // 2)} in the whole-head rows)")
    ok = {}
    st = _lib.stream()
    elems = N * H * W * C

    if "dw" in only:
        x = torch.randn((N, H, W, C), device=dev, generator=g)
        dy = torch.randn((N, H, W, C), device=dev, generator=g)
        w = torch.randn((C, 1, 3, 3), device=dev, generator=g) / 3.0
        w9 = dc.tap_major(w)
        y = torch.empty_like(x)
        dw9 = torch.empty((9, C), device=dev)
        nbytes = _lib.lib.diga_dwconv3x3_wgrad_workspace_bytes(N, H, W, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        xc, dyc = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)              # NCHW-shaped channels-last views: torch's operands
        for d in (6, 12, 18):
            with torch.no_grad():
                _lib.call("diga_dwconv3x3_f32", _lib.ptr(x), C, _lib.ptr(w9), _lib.ptr(y), C, N, H, W, C, d, 0, st)
                ref = F.conv2d(xc, w, None, 1, d, d, C)
                say(f"dilation {d}: max |kernel - torch| = {float((y.permute(0, 3, 1, 2) - ref).abs().max()):.2e}")
                del ref

            def t_fwd():
                with torch.no_grad():
                    F.conv2d(xc, w, None, 1, d, d, C)

            def t_dgrad():
                with torch.no_grad():
                    torch.nn.grad.conv2d_input(xc.shape, w, dyc, 1, d, d, C)

            def t_wgrad():
                with torch.no_grad():
                    torch.nn.grad.conv2d_weight(xc, w.shape, dyc, 1, d, d, C)

            ok[f"dw fwd d{d}"] = compare(f"depthwise forward, dilation {d}", t_fwd,
                                         lambda: _lib.call("diga_dwconv3x3_f32", _lib.ptr(x), C, _lib.ptr(w9), _lib.ptr(y), C, N, H, W, C, d, 0, st),
                                         a.rounds, a.reps, 8.0 * elems)
            ok[f"dw dgrad d{d}"] = compare(f"depthwise backward-data, dilation {d}", t_dgrad,
                                           lambda: _lib.call("diga_dwconv3x3_f32", _lib.ptr(dy), C, _lib.ptr(w9), _lib.ptr(y), C, N, H, W, C, d, 1, st),
                                           a.rounds, a.reps, 8.0 * elems)
            ok[f"dw wgrad d{d}"] = compare(f"depthwise weight gradient, dilation {d}", t_wgrad,
                                           lambda: _lib.call("diga_dwconv3x3_f32_wgrad", _lib.ptr(dy), C, _lib.ptr(x), C, _lib.ptr(dw9), _lib.ptr(ws),
                                                             nbytes, N, H, W, C, d, st), a.rounds, a.reps, 8.0 * elems)
        del x, dy, y, ws, xc, dyc
        torch.cuda.empty_cache()

    if "resize" in only:
        buf = torch.empty((N, H, W, C), device=dev)
        for k, r in ((1, 2), (2, 4), (3, 8)):
            h, w_ = H // r, W // r
            src = torch.randn((N, h, w_, E), device=dev, generator=g)
            sc = src.permute(0, 3, 1, 2)
            win = buf[..., k * E:(k + 1) * E]
            winc = win.permute(0, 3, 1, 2)

            def t_resize():
                with torch.no_grad():
                    winc.copy_(F.interpolate(sc, size=(H, W), mode="bilinear", align_corners=False))

            ok[f"resize x{r}"] = compare(f"resize x{r} into a slice", t_resize,
                                         lambda: _lib.call("diga_pyramid_resize_fwd", _lib.ptr(src), h, w_, _lib.ptr(win), C, H, W, N, E, st),
                                         a.rounds, a.reps, 4.0 * N * E * (H * W + h * w_))
        del buf
        torch.cuda.empty_cache()

    if "head" in only:
        head = dh.DAFormerHead(in_channels=list(STAGES), channels=CH, feature_strides=[4, 8, 16, 32], num_classes=K, in_index=[0, 1, 2, 3],
                               act_cfg=dict(type="ReLU"), dropout_ratio=0.1, norm_cfg=dict(type="BN", requires_grad=True),
                               align_corners=False).to(dev).train()
        feats = [torch.randn((N, c, H // r, W // r), device=dev, generator=g).contiguous(memory_format=torch.channels_last).requires_grad_()
                 for c, r in zip(STAGES, (1, 2, 4, 8))]
        prb = torch.randn((N, K, H, W), device=dev, generator=g)
        params = list(head.parameters())
        kernel_raw = dh.DAFormerHead.raw_features

        def form(composed):
            dh.USE_TORCH_DEPTHWISE = composed
            dh.DAFormerHead.raw_features = dc.composed_raw_features if composed else kernel_raw

        def head_fwd(composed):
            def run():
                form(composed)
                with torch.no_grad():
                    head(feats)
                form(False)
            return run

        def head_fwd_bwd(composed):
            def run():
                form(composed)
                logits, _ = head(feats)
                torch.autograd.grad([logits], params + feats, [prb], allow_unused=True)
                form(False)
            return run

        ok["head fwd"] = compare("whole head, forward (no_grad)", head_fwd(True), head_fwd(False), a.rounds, max(2, a.reps // 2))
        ok["head fwd+bwd"] = compare("whole head, forward + backward", head_fwd_bwd(True), head_fwd_bwd(False), a.rounds, max(2, a.reps // 2))
        say(f"peak memory allocated: {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
        del head, feats, prb, params
        torch.cuda.empty_cache()

    if not a.no_bw:
        import bench
        bw = bench.bandwidth_kernels(dev)
        say("the project's bandwidth kernels on this device (bench.bandwidth_kernels): "
            + ", ".join(f"{k} {v['achieved'] / 1e3:.2f} TB/s" for k, v in bw.items()))
        # (DESIGN section 16's span: ce2d at the top, the centroid weights at the bottom of the full-size bandwidth kernels)
        top, low = bw["ce2d"]["achieved"] / 1e3, bw["centroid_weights"]["achieved"] / 1e3
        for k, v in TBS.items():
            say(f"  {k:40s} {v:.2f} TB/s = {v / top:.2f} x ce2d, {v / low:.2f} x centroid_weights")
    say("kernel faster in every alternated pair: " + ", ".join(f"{k}: {'yes' if v else 'NO'}" for k, v in ok.items()))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
