#!/usr/bin/env python3
"""Per-shape timing of the MiT kernels at the 16 x 768x768 sizes of MiT-B1..B5 (widths 64/128/320/512, head_dim 64) or, with
--arch b0, of MiT-B0 (widths 32/64/160/256, head_dim 32); operands cold (a 1 GB sweep between launches) when --cold:
    python tools/bench_mit_ops.py [--arch b0] [--cold] [--what gemm,wgrad,attn,ln,dw] [--sdpa]
--sdpa: every attention row is followed by torch's scaled_dot_product_attention in fp16 on the SAME tensors, measured as five
alternated warm pairs (ours, torch, ours, torch, ...; medians and all ten values), with the FLOPs / bytes / exponentials the shape
needs and the time each of the matrix, memory and vector pipes would take for them alone."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cold", action="store_true")
    ap.add_argument("--what", default="gemm,wgrad,attn,ln,dw")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--arch", default="b5", choices=["b5", "b0"], help="stage widths: b5 = 64/128/320/512 (b1..b5), b0 = 32/64/160/256")
    ap.add_argument("--sdpa", action="store_true", help="attention rows: five alternated pairs against torch SDPA (fp16)")
    a = ap.parse_args()
    import torch
    from diga_amd import _lib
    from diga_amd.model.networks.MixTransfomer import _Ops
    dev = torch.device("cuda")
    ops = _Ops(dev)
    P = _lib.ptr
    sweep = torch.empty(1 << 28, dtype=torch.float32, device=dev) if a.cold else None

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        tot = 0.0
        for _ in range(a.reps):
            if sweep is not None:
                sweep.add_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1)
        return tot / a.reps * 1e3          # us

    B = 16
    wid = {"b5": (64, 128, 320, 512), "b0": (32, 64, 160, 256)}[a.arch]
    stages = [(B * 192 * 192, wid[0], 1, 8), (B * 96 * 96, wid[1], 2, 4), (B * 48 * 48, wid[2], 5, 2), (B * 24 * 24, wid[3], 8, 1)]

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def pairs(ours, theirs, n=5):
        """n alternated warm pairs -> (median ours, median theirs, all values) in us."""
        for _ in range(2):
            ours()
            theirs()
        torch.cuda.synchronize()
        va, vb = [], []
        for _ in range(n):
            va.append(once(ours))
            vb.append(once(theirs))
        return sorted(va)[n // 2], sorted(vb)[n // 2], va, vb

    what = a.what.split(",")
    for si, (M, C, heads, sr) in enumerate(stages):
        hid = 4 * C
        print(f"== stage {si + 1}: M={M} C={C}")
        if "gemm" in what:
            shapes = [("q/proj", M, C, C, False), ("fc1", M, hid, C, False), ("fc2+res", M, C, hid, True), ("kv", B * 576, 2 * C, C, False)]
            if sr > 1:
                shapes.append(("sr", B * 576, C, sr * sr * C, True))
            for name, m, n, k, f32 in shapes:
                x = torch.randn((m, k), device=dev).half()
                w = torch.randn((n, k), device=dev).half()
                bias = torch.randn(n, device=dev)
                res = torch.randn((m, n), device=dev) if f32 else None
                out = torch.empty((m, n), device=dev, dtype=torch.float32 if f32 else torch.float16)
                us = timed(lambda: ops.gemm(x, w, bias, n, out_f32=f32, residual=res, out=out))
                byt = m * k * 2 + n * k * 2 + m * n * (8 if f32 else 2)
                print(f"  gemm {name:8s} [{m}x{n}x{k}] {us:8.1f} us  {2.0 * m * n * k / us / 1e6:7.1f} TFLOP/s  {byt / us / 1e3:7.1f} GB/s")
        if "wgrad" in what:
            for name, m, n, k in (("q/proj", M, C, C), ("fc1", M, hid, C), ("fc2", M, C, hid)):
                dy = torch.randn((m, n), device=dev).half()
                x = torch.randn((m, k), device=dev).half()
                us = timed(lambda: ops.wgrad(dy, x, 1.0, bias=True))
                print(f"  wgrad {name:7s} [{m}: {n}x{k}] {us:8.1f} us  {2.0 * m * n * k / us / 1e6:7.1f} TFLOP/s  {(m * (n + k) * 2) / us / 1e3:7.1f} GB/s")
        if "attn" in what:
            N, nk, hd = M // B, 576, C // heads
            scale = hd ** -0.5
            q = torch.randn((M, C), device=dev).half()
            kv = torch.randn((B * nk, 2 * C), device=dev).half()
            o = torch.empty_like(q)
            lse = torch.empty((B, heads, N), device=dev)

            # head_dim 64 stays on the three old entry points (the rows every earlier record was timed through); 32 needs the new ones
            def fwd():
                if hd == 64:
                    _lib.call("diga_mit_attention_fwd", P(q), C, P(kv), 2 * C, P(o), C, P(lse), B, heads, N, nk, scale, _lib.stream())
                else:
                    _lib.call("diga_mit_attention_hd_fwd", P(q), C, P(kv), 2 * C, P(o), C, P(lse), B, heads, hd, N, nk, scale, _lib.stream())

            us = timed(fwd)
            fl = 4.0 * B * heads * N * nk * hd
            print(f"  attn fwd (heads {heads}, N {N}, Nk {nk}, head_dim {hd}) {us:8.1f} us {fl / us / 1e6:7.1f} TFLOP/s")
            do = torch.randn_like(q)
            dq, dkv = torch.empty_like(q), torch.empty_like(kv)
            ws = torch.empty(_lib.lib.diga_mit_attention_hd_bwd_workspace_bytes(B, heads, hd, N, nk), dtype=torch.uint8, device=dev)

            def bwd():
                if hd == 64:
                    _lib.call("diga_mit_attention_bwd", P(q), C, P(kv), 2 * C, P(o), P(do), C, P(lse), P(dq), P(dkv), P(ws), ws.numel(),
                              B, heads, N, nk, scale, _lib.stream())
                else:
                    _lib.call("diga_mit_attention_hd_bwd", P(q), C, P(kv), 2 * C, P(o), P(do), C, P(lse), P(dq), P(dkv), P(ws), ws.numel(),
                              B, heads, hd, N, nk, scale, _lib.stream())

            us = timed(bwd)
            print(f"  attn bwd {us:8.1f} us {14.0 / 4 * fl / us / 1e6:7.1f} TFLOP/s")
            if a.sdpa:
                import torch.nn.functional as F
                # the same memory, viewed [B][heads][rows][head_dim] (strided views: no copies inside the timed region)
                tq = q.view(B, N, heads, hd).permute(0, 2, 1, 3).requires_grad_()
                tk = kv.view(B, nk, 2, heads, hd)[:, :, 0].permute(0, 2, 1, 3).requires_grad_()
                tv = kv.view(B, nk, 2, heads, hd)[:, :, 1].permute(0, 2, 1, 3).requires_grad_()
                tdo = do.view(B, N, heads, hd).permute(0, 2, 1, 3)

                def t_fwd():
                    with torch.no_grad():
                        return F.scaled_dot_product_attention(tq, tk, tv, scale=scale)

                to = F.scaled_dot_product_attention(tq, tk, tv, scale=scale)

                def t_bwd():
                    return torch.autograd.grad(to, (tq, tk, tv), tdo, retain_graph=True)

                elems = float(B) * heads * N * nk                     # scores = exponentials
                byt_f = 2.0 * (2 * M * C + B * nk * 2 * C) + 4.0 * B * heads * N
                byt_b = 2.0 * (4 * M * C + 2 * B * nk * 2 * C) + 8.0 * B * heads * N
                # chip rates: fp16 MFMA 2.5 PFLOP/s dense, HBM 6.3 TB/s measured copy, VALU 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz,
                # v_exp_f32 at a quarter of that; `valu` counts the forward's ~8 full-rate fp32 instructions per score beside the exp
                # (scale fma, max, add, cvt, and the rescales' share) -- an estimate from the source, not a counter
                lane = 256 * 4 * 16 * 2.4e9
                for name, m_ours, m_torch, flops, byt, nexp, nvalu in (("fwd", fwd, t_fwd, fl, byt_f, elems, 8 * elems),
                                                                       ("bwd", bwd, t_bwd, 3.5 * fl, byt_b, 2 * elems, 20 * elems)):
                    a_us, b_us, va, vb = pairs(m_ours, m_torch)
                    print(f"  attn {name} vs torch SDPA fp16: ours {a_us:8.1f} us  torch {b_us:8.1f} us  ratio {b_us / a_us:5.2f}x   "
                          f"ours {[round(v, 1) for v in va]} torch {[round(v, 1) for v in vb]}")
                    print(f"       needs {flops / 1e9:7.2f} GFLOP ({flops / 2.5e15 * 1e6:6.1f} us of MFMA)  {byt / 1e6:7.1f} MB "
                          f"({byt / 6.3e12 * 1e6:6.1f} us of HBM)  {nexp / 1e6:7.1f} M exp ({nexp / (lane / 4) * 1e6:6.1f} us) + "
                          f"~{nvalu / 1e6:7.1f} M fp32 VALU lane-ops ({nvalu / lane * 1e6:6.1f} us)")
        if "ln" in what:
            x = torch.randn((M, C), device=dev)
            g, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            us = timed(lambda: ops.ln_fwd(x, g, b, 1e-6))
            print(f"  ln fwd {us:8.1f} us {M * C * 6 / us / 1e3:7.1f} GB/s")
            _, _, mean, rstd = ops.ln_fwd(x, g, b, 1e-6)
            dy = torch.randn((M, C), device=dev).half()
            us = timed(lambda: ops.ln_bwd(dy, x, g, mean, rstd, x, True, True, 1.0))
            print(f"  ln bwd {us:8.1f} us {M * C * 16 / us / 1e3:7.1f} GB/s")
        if "dw" in what:
            hw = int((M // B) ** 0.5)
            x = torch.randn((B, hw, hw, hid), device=dev).half()
            wt9 = torch.randn((9, hid), device=dev)
            bias = torch.randn(hid, device=dev)
            u, h = torch.empty_like(x), torch.empty_like(x)
            us = timed(lambda: _lib.call("diga_mit_dwconv_gelu_fwd", P(x), P(wt9), P(bias), P(u), P(h), B, hw, hw, hid, _lib.stream()))
            print(f"  dwconv fwd {us:8.1f} us {M * hid * 6 / us / 1e3:7.1f} GB/s")
            du, dx = torch.empty_like(x), torch.empty_like(x)
            dw, db = torch.empty((hid, 9), device=dev), torch.empty(hid, device=dev)
            ws = torch.empty(_lib.lib.diga_mit_dwconv_bwd_workspace_bytes(B, hw, hid), dtype=torch.uint8, device=dev)
            us = timed(lambda: _lib.call("diga_mit_dwconv_gelu_bwd", P(h), P(u), P(x), P(wt9), P(du), P(dx), P(dw), P(db), 1.0, 0, P(ws),
                                         ws.numel(), B, hw, hw, hid, _lib.stream()))
            print(f"  dwconv bwd {us:8.1f} us {M * hid * 12 / us / 1e3:7.1f} GB/s")


if __name__ == "__main__":
    main()
