#!/usr/bin/env python3
"""The OCR head's two fused operations (csrc/ocr.hip) against their stock-torch compositions, and the whole head with either, on one
GPU in one process:  python tools/bench_ocr.py [--rounds R] [--reps K] [--no-bw] [out.txt]

Geometry: the student pass of the semi-supervised warm-up -- six maps (three crops, two views) of 128 x 256 at 720 / 512 / 256
channels, 19 classes.  The parent commit has no such path, so the yardstick is the composition (softmax, matmul, permute, autograd) on
the same device: every round times the composition and the fused form one after the other (alternated pairs), forward and
forward + backward, `reps` calls between two device events after a warm-up of both.  Reported per pair: both times, and per
operation whether the fused form won EVERY pair.  Also, without a gate: achieved bytes/s of each kernel-level call over the least
traffic it could have (operands read once, results written once), next to what the project's bandwidth kernels reach on this box
(bench.bandwidth_kernels, the figure of tools/bench_bw_kernels.py)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

N, H, W, CIN, C, D, K = 6, 128, 256, 720, 512, 256, 19
P = H * W
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


def compare(title, composed, fused, rounds, reps, min_bytes=None):
    """Alternated pairs; returns True when the fused form won every one."""
    for fn in (composed, fused):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    pairs = [(timed(composed, reps), timed(fused, reps)) for _ in range(rounds)]
    won = all(f < c for c, f in pairs)
    best = min(f for _, f in pairs)
    tail = ""
    if min_bytes is not None:
        tail = f"   least traffic {min_bytes / 1e6:7.1f} MB -> {min_bytes / (best * 1e-3) / 1e12:.2f} TB/s at the best fused time"
    say(f"{title:44s} composed / fused ms per call: " + "  ".join(f"{c:7.3f}/{f:7.3f}" for c, f in pairs)
        + f"   fused wins every pair: {'yes' if won else 'NO'}" + tail)
    return won


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-bw", action="store_true", help="skip the project's bandwidth kernels (bench.bandwidth_kernels)")
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "diag_out", "bench_ocr.txt"))
    a = ap.parse_args()
    import ocr_cases as oc
    from diga_amd.model.networks import ocrnet_module as om
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    say(f"device {torch.cuda.get_device_name(0)}; N = {N} maps of {H} x {W}, {CIN} / {C} / {D} channels, K = {K}; {a.rounds} alternated rounds of {a.reps} calls")
    ok = {}

    # ---- the two operations alone
    x = torch.randn((N, P, C), device=dev, generator=g).requires_grad_()
    s = (2.0 * torch.randn((N, P, K), device=dev, generator=g)).requires_grad_()
    dr = torch.randn((N, K, C), device=dev, generator=g)
    with torch.no_grad():
        d = float((om.ocr_region_gather(x, s) - oc.region_gather(x, s)).abs().max())
    say(f"region gather: max |fused - composed| = {d:.2e}")

    def fwd(fn, *t):
        def run():
            with torch.no_grad():
                fn(*t)
        return run

    def fwd_bwd(fn, gout, *t):
        ins = [u for u in t if isinstance(u, torch.Tensor)]
        return lambda: torch.autograd.grad(fn(*t), ins, gout)

    b_x, b_s = N * P * C * 4, N * P * K * 4
    ok["region fwd"] = compare("region gather, forward", fwd(oc.region_gather, x, s), fwd(om.ocr_region_gather, x, s), a.rounds, a.reps,
                               b_x + b_s)
    ok["region fwd+bwd"] = compare("region gather, forward + backward", fwd_bwd(oc.region_gather, dr, x, s),
                                   fwd_bwd(om.ocr_region_gather, dr, x, s), a.rounds, a.reps, 3 * (b_x + b_s))
    del x, s, dr
    q = torch.randn((N, P, D), device=dev, generator=g).requires_grad_()
    key = torch.randn((N, K, D), device=dev, generator=g).requires_grad_()
    val = torch.randn((N, K, D), device=dev, generator=g).requires_grad_()
    do = torch.randn((N, P, D), device=dev, generator=g)
    scale = D ** -0.5
    with torch.no_grad():
        d = float((om.ocr_object_attention(q, key, val, scale) - oc.object_attention(q, key, val, scale)).abs().max())
    say(f"object attention: max |fused - composed| = {d:.2e}")
    b_q, b_a = N * P * D * 4, N * P * K * 4
    om.FUSED_ATTENTION_NO_GRAD = True         # this row times the KERNEL without a map (the module's rule would hand back the composition)
    ok["attention fwd"] = compare("object attention, forward (no attn kept)", fwd(oc.object_attention, q, key, val, scale),
                                  fwd(om.ocr_object_attention, q, key, val, scale), a.rounds, a.reps, 2 * b_q)
    om.FUSED_ATTENTION_NO_GRAD = False        # ... and the whole head below runs as shipped
    ok["attention fwd+bwd"] = compare("object attention, forward + backward", fwd_bwd(oc.object_attention, do, q, key, val, scale),
                                      fwd_bwd(om.ocr_object_attention, do, q, key, val, scale), a.rounds, a.reps,
                                      (2 * b_q + b_a) + (3 * b_q + b_a))
    del q, key, val, do
    torch.cuda.empty_cache()

    # ---- the whole head, the callables swapped between the two forms
    head = om.OCRNet(oc.REAL_CFG).to(dev).train()
    raw = torch.randn((N, CIN, H, W), device=dev, generator=g).contiguous(memory_format=torch.channels_last).requires_grad_()
    probes = [torch.randn((N, K, H, W), device=dev, generator=g) for _ in range(2)]
    params = [p for p in head.parameters()]
    forms = {"fused": (om.ocr_region_gather, om.ocr_object_attention), "composed": (oc.region_gather, oc.object_attention)}

    def head_fwd(form):
        def run():
            om.ocr_region_gather, om.ocr_object_attention = forms[form]
            with torch.no_grad():
                head(raw)
            om.ocr_region_gather, om.ocr_object_attention = forms["fused"]
        return run

    def head_fwd_bwd(form):
        def run():
            om.ocr_region_gather, om.ocr_object_attention = forms[form]
            soft, seg, _ = head(raw)
            torch.autograd.grad([soft, seg], params + [raw], probes, allow_unused=True)
            om.ocr_region_gather, om.ocr_object_attention = forms["fused"]
        return run

    ok["head fwd"] = compare("whole head, forward (no_grad)", head_fwd("composed"), head_fwd("fused"), a.rounds, max(2, a.reps // 3))
    ok["head fwd+bwd"] = compare("whole head, forward + backward", head_fwd_bwd("composed"), head_fwd_bwd("fused"), a.rounds,
                                 max(2, a.reps // 3))
    say(f"peak memory allocated: {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    del head, raw, probes, params
    torch.cuda.empty_cache()

    if not a.no_bw:
        import bench
        bw = bench.bandwidth_kernels(dev)
        say("the project's bandwidth kernels on this device (bench.bandwidth_kernels): "
            + ", ".join(f"{k} {v['achieved'] / 1e3:.2f} TB/s" for k, v in bw.items()))
    say("fused faster in every alternated pair: " + ", ".join(f"{k}: {'yes' if v else 'NO'}" for k, v in ok.items()))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
