#!/usr/bin/env python3
"""Backward-data of the 3x3 / stride 2 / pad 1 convolutions of HRNet-W48 (csrc/dgrad_strided.hip) against two yardsticks on the same
device and tensors, in one process:  python tools/bench_dgrad_strided.py [--rounds R] [--reps K] [--no-torch] [out.txt]

Shapes: the downsampling convolutions of HRNet-W48 at a 512 x 1024 crop, six images (Cin -> Cout of the forward conv, input extent).
Yardsticks: (a) torch.nn.grad.conv2d_input on channels-last tensors -- what a torch HRNet runs; (b) the zero-insertion composition on
this library's own stride-1 backward-data path: dy scattered into a zeroed tensor of dx's extent, then the stride-1 call DigaConv2d's
backward makes (four times the multiplications, a tensor four times dy written and re-read).
Every round times (a), (b) and the kernel one after the other (alternated), `reps` calls between two device events after a warm-up
of all three.  Reported per shape: ms per call of every round and the range over rounds; for the kernel, at its best time, achieved
bytes/s over the least traffic (dy once + dx once + weights once, at the channel counts the call runs on: padded to 32) and the
executed FLOPs (2 N Ho Wo Cout 9 Cin, the forward's count) as a fraction of the fp32 matrix peak bench.py prices against."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

N = 6
SHAPES = [(64, 64, 256, 512), (256, 96, 128, 256), (48, 48, 128, 256), (48, 96, 128, 256), (96, 192, 64, 128), (192, 384, 32, 64)]
LINES = []


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-torch", action="store_true", help="skip yardstick (a)")
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "diag_out", "bench_dgrad_strided.txt"))
    a = ap.parse_args()
    import bench
    from diga_amd import _lib
    from diga_amd.model import conv as dconv
    peak = bench.F32_MFMA_PEAK_TFLOPS * 1e12
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(24)
    _lib.set_conv_math(0)
    say(f"device {torch.cuda.get_device_name(0)}; {N} images, 3x3 / stride 2 / pad 1, conv_math 0; {a.rounds} alternated rounds of {a.reps} calls; "
        f"fp32 matrix peak {peak / 1e12:.1f} TFLOP/s")
    wins = {}
    for cin, cout, hi, wi in SHAPES:
        ho, wo = hi // 2, wi // 2
        cp, kp = dconv._pad_to(cin), dconv._pad_to(cout)
        title = f"{cin:3d} -> {cout:3d} at {hi} x {wi}"
        say(f"-- {title} (runs as {cp} -> {kp})")
        w = torch.randn((cout, cin, 3, 3), device=dev, generator=g) * (2.0 / (cout * 9)) ** 0.5
        dy = torch.randn((N, cout, ho, wo), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        w_cl = w.contiguous(memory_format=torch.channels_last)
        # the library's operands: NHWC with the channels padded to 32, the [C][R][S][K] transpose
        gyp = torch.zeros((N, ho, wo, kp), device=dev)
        gyp[..., :cout] = dy.permute(0, 2, 3, 1)
        wt = torch.zeros((cp, 3, 3, kp), device=dev)
        wt[:cin, :, :, :cout] = w.permute(1, 2, 3, 0)
        dx_new = torch.empty((N, hi, wi, cp), device=dev)
        dx_zi = torch.empty((N, hi, wi, cp), device=dev)
        st = _lib.stream()

        def new():
            _lib.call("diga_dgrad_strided_f32", _lib.ptr(gyp), kp, _lib.ptr(wt), _lib.ptr(dx_new), cp, N, hi, wi, cp, ho, wo, kp, 3, 3, 2, 2, 1, 1, st)

        def zero_insertion():
            z = torch.zeros((N, hi, wi, kp), device=dev)
            z[:, ::2, ::2] = gyp
            dconv._conv_launch(z, wt, None, dx_zi, (1, 1), (1, 1), (-1, -1), dconv._TAG_BWD_DATA)

        def stock():
            return torch.nn.grad.conv2d_input((N, cin, hi, wi), w_cl, dy, stride=2, padding=1)

        forms = [("zero-insertion (b)", zero_insertion), ("kernel", new)]
        if not a.no_torch:
            forms.insert(0, ("torch (a)", stock))
        for _, fn in forms:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        scale = float(dx_zi.abs().max())
        say(f"   max |kernel - zero-insertion| = {float((dx_new - dx_zi).abs().max()) / scale:.2e} of scale"
            + ("" if a.no_torch else f", max |kernel - torch| = "
               f"{float((dx_new[..., :cin] - stock().permute(0, 2, 3, 1)).abs().max()) / scale:.2e} of scale"))
        rounds = [[timed(fn, a.reps) for _, fn in forms] for _ in range(a.rounds)]
        for i, (name, _) in enumerate(forms):
            ts = [r[i] for r in rounds]
            say(f"   {name:20s} ms per call: " + "  ".join(f"{t:7.3f}" for t in ts) + f"   range {min(ts):.3f} .. {max(ts):.3f}")
        best = min(r[-1] for r in rounds) * 1e-3
        nbytes = 4.0 * (N * ho * wo * kp + N * hi * wi * cp + 9 * cp * kp)
        flops = 2.0 * N * ho * wo * kp * 9 * cp
        say(f"   kernel at its best time: least traffic {nbytes / 1e6:.1f} MB -> {nbytes / best / 1e12:.2f} TB/s; executed {flops / 1e9:.1f} GFLOP -> "
            f"{flops / best / 1e12:.1f} TFLOP/s = {flops / best / peak:.3f} of the fp32 matrix peak")
        for i, (name, _) in enumerate(forms[:-1]):
            wins[f"{title} vs {name}"] = all(r[-1] < r[i] for r in rounds)
        del w, dy, w_cl, gyp, wt, dx_new, dx_zi
        torch.cuda.empty_cache()
    say("kernel faster in every alternated round: " + "; ".join(f"{k}: {'yes' if v else 'NO'}" for k, v in wins.items()))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
