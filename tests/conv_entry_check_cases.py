"""Rejected calls and size queries of the convolution entry points (csrc/conv.hip, conv_bf16x6.h, winograd.hip): the cases behind
tests/test_conv_entry_checks_cpu.py and its fixture tests/golden/conv_entry_checks.json.

Every call uses fake addresses and breaks at least one argument rule, so it is answered by the host checks (EINVAL, EALIGN or
EWORKSPACE) before anything is launched; the fixture keeps (return code, message) per call, which pins the rules, their messages and
-- through the cases with two faults -- their order.  The queries' fixture keeps the value returned on a grid of valid and invalid
shapes.  Only `_lib.SIGNATURES`, `_lib.lib` and the descriptor structures are used, so the same file records from any revision:

    DIGA_LIB=<library of the revision to record> python tests/conv_entry_check_cases.py --record [--relist-valid]
    DIGA_LIB=<...> python tests/conv_entry_check_cases.py --merge <name prefix> ...   (adds entry points, keeps every recorded entry)
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_entry_checks.json")
REJECTED = (-1, -2, -3)          # DIGA_EINVAL, DIGA_EALIGN, DIGA_EWORKSPACE
A = 1 << 20                      # fake addresses: 16-byte aligned, non-null, never dereferenced
BIG = 1 << 40
BWD_DATA = 12                    # DIGA_PROF_CONV_BWD_DATA (checked against _lib.PROF_TAGS by the test)

# ------------------------------------------------------------------------------------------------------------------ signatures
# parameter names in the order of include/diga_hip.h; `?` marks a pointer that may be null
G17 = "n hi wi cin in_ld ho wo cout out_ld r s sy sx oy ox dy dx"
G16 = "n hi wi cin ho wo cout out_ld r s sy sx oy ox dy dx"
W17 = "n hi wi cin x_ld ho wo cout dy_ld r s sy sx oy ox dy dx"
W15 = "n hi wi cin ho wo cout r s sy sx oy ox dy dx"
GW = "n hi wi cin ho wo cout out_ld r s oy ox"          # the window forms: stride 1
WF = "n h w cin in_ld cout out_ld dil tile"
WB = "n h w cin x_ld cout dy_ld dil tile"
SPECS = {
    "diga_conv2d_nhwc_f32": f"in wgt bias? out {G17} stats? tag stream",
    "diga_conv2d_nhwc_f32_infer": f"in wgt bias? out {G17} infer tag stream",
    "diga_conv2d_nhwc_f32_epi": f"in wgt out {G17} epi tag stream",
    "diga_conv2d_nhwc_f32_opts": f"in wgt bias? out {G17} opts tag stream",
    "diga_conv2d_nhwc_bf16x3": f"in wgt_hi wgt_lo bias? out {G17} stats? tag stream",
    "diga_conv2d_nhwc_bf16x3_epi": f"in wgt_hi wgt_lo out {G17} epi tag stream",
    "diga_conv2d_nhwc_bf16x3_opts": f"in wgt_hi wgt_lo bias? out {G17} opts tag stream",
    "diga_conv2d_nhwc_twin": f"in img bias? out {G16} stats? tag stream",
    "diga_conv2d_nhwc_twin_epi": f"in img out {G16} epi tag stream",
    "diga_conv2d_nhwc_twin_opts": f"in img bias? out {G16} opts tag stream",
    "diga_conv2d_wgrad_nhwc_f32": f"dyp xp dw ws ws_bytes {W17} math stream",
    "diga_conv2d_wgrad_twin": f"dyp xp dw ws ws_bytes {W15} stream",
    "diga_conv2d_nhwc_bf16x6": f"in img bias? out {G16} stats? tag stream",
    "diga_conv2d_nhwc_bf16x6_epi": f"in img out {G16} epi tag stream",
    "diga_infer_conv2d_nhwc_bf16x6": f"in img bias? out {G16} infer tag stream",
    "diga_conv2d_wgrad_bf16x6": f"dyp xp dw ws ws_bytes {W15} stream",
    "diga_conv2d_nhwc_bf16x6_f32in": f"in in_ld img bias? out {G16} stats? tag stream",
    "diga_conv2d_nhwc_bf16x6_f32in_epi": f"in in_ld img out {G16} epi tag stream",
    "diga_infer_conv2d_nhwc_bf16x6_f32in": f"in in_ld img bias? out {G16} infer tag stream",
    "diga_conv2d_wgrad_bf16x6_f32in": f"dyp dy_ld xp x_ld dw ws ws_bytes {W15} stream",
    "diga_conv_taps_bf16x6_f32in": f"in in_ld img bias? out {G16} stats? tag stream",
    "diga_conv_taps_bf16x6_f32in_epi": f"in in_ld img out {G16} epi tag stream",
    "diga_infer_conv_taps_bf16x6_f32in": f"in in_ld img bias? out {G16} infer tag stream",
    "diga_conv_taps_wgrad_bf16x6_f32in": f"dyp dy_ld xp x_ld dw ws ws_bytes {W15} stream",
    "diga_conv2d_winograd_tile_table": "table n h w dil tile stream",
    "diga_conv2d_winograd_f32": f"in wgt bias? out ws ws_bytes {WF} flip stats? tile_table? tag stream",
    "diga_conv2d_winograd_f32_opts": f"in wgt bias? out ws ws_bytes {WF} opts tile_table? tag stream",
    "diga_conv2d_winograd_f32_epi": f"in wgt out ws ws_bytes {WF} flip epi tile_table? tag stream",
    "diga_conv2d_winograd_f32_infer": f"in wgt bias? out ws ws_bytes {WF} infer tile_table? tag stream",
    "diga_conv2d_winograd_f32_keep": f"in wgt bias? out v_keep ws ws_bytes {WF} stats? tile_table? tag stream",
    "diga_conv2d_wgrad_winograd_f32": f"dyp xp v_kept? dw ws ws_bytes {WB} tile_table? stream",
    "diga_conv2d_winograd_bf16x6": f"in wgt bias? out v_keep? ws ws_bytes {WF} flip stats? epi? tile_table? tag stream",
    "diga_infer_conv2d_winograd_bf16x6": f"in wgt bias? out ws ws_bytes {WF} infer tile_table? tag stream",
    "diga_conv2d_wgrad_winograd_bf16x6": f"dyp xp v_kept? dw ws ws_bytes {WB} tile_table? stream",
    "diga_gemm_batched_bf16x6_f32in": "in rows batches k img cout out stream",
    "diga_wgrad_batched_bf16x6_f32in": "dyp xp dw ws ws_bytes rows batches cout cin stream",
    "diga_wgrad_bf16x6_tiled_f32in": f"dyp dy_ld xp x_ld dw ws ws_bytes {W15} stream",
    "diga_wgrad_bf16x6_tile": "cout cin bm bn",
    "diga_conv_taps_bf16x6_f32in_opts": f"in in_ld img bias? out {G16} stats? opts tag stream",
    "diga_conv_window_bf16x6_f32in": f"in in_ld img bias? out {GW} dy dx opts? tag stream",
    "diga_conv_up2_bf16x6_f32in": f"in in_ld img img_ph bias? out {GW} opts tag stream",
    "diga_collapse_up2_weights": "wgt wc cout r s cin oy ox stream",
}
# the plan functions answer through int* results: recorded as queries, [value returned, the integers written (-7: not written)]
PLANS = {"diga_conv_window_bf16x6_plan": 3, "diga_conv_up2_bf16x6_plan": 2}
POINTERS = ("in", "wgt", "wgt_hi", "wgt_lo", "img", "bias", "out", "stats", "dyp", "xp", "dw", "ws", "table", "tile_table", "v_keep", "v_kept",
            "img_ph", "wc")
DESCRIPTORS = ("epi", "infer", "opts")
OUT_INTS = ("bm", "bn")          # results written through an int*: a real int unless the case passes null (0)


def params(name):
    return [t.rstrip("?") for t in SPECS[name].split()]


def optional(name):
    return {t[:-1] for t in SPECS[name].split() if t.endswith("?")}


def is_winograd(name):
    return "winograd" in name


def has_taps(name):
    """The entry point takes more than one tap (R, S are not pinned to 1)."""
    return "r" in params(name) and not ("bf16x6" in name and not any(k in name for k in ("taps", "tiled", "window", "up2")))


def multi_tap_form(name):
    return "conv_taps" in name or "tiled" in name or is_window(name)


def is_window(name):
    return "conv_window" in name or "conv_up2" in name


def base(name):
    """A valid call: every case below changes it in one or two places."""
    ps = params(name)
    v = {p: A + 0x1000 * (i + 1) for i, p in enumerate(POINTERS)}
    v.update({p: None for p in optional(name)})
    v.update(stream=None, tag=0, math=0, flip=0, ws_bytes=BIG, bm=1, bn=1)
    if is_winograd(name):
        v.update(n=1, h=12, w=12, cin=128, in_ld=128, x_ld=128, cout=256, out_ld=256, dy_ld=256, dil=1, tile=4)
    elif "batched" in name:
        v.update(rows=256, batches=4, k=64, cout=256, cin=128)
    else:
        rs, off = (3, -1) if has_taps(name) else (1, 0)
        v.update(n=1, hi=12, wi=12, cin=64, in_ld=64, x_ld=64, ho=12, wo=12, cout=64, out_ld=64, dy_ld=64, r=rs, s=rs, sy=1, sx=1, oy=off,
                 ox=off, dy=1, dx=1)
    for d in DESCRIPTORS:
        if d in ps:
            v[d] = None if d in optional(name) else dict(BASE_DESCRIPTOR[d])
    if "conv_up2" in name:       # 3 x 3 tiles of 8 x 16 output pixels on the 2x upsampling of 10 x 18: one interior tile, every tap of it inside
        v.update(hi=10, wi=18, ho=20, wo=36, r=5, s=5, oy=-2, ox=-2, opts=dict(upsample_shift=1))
    return v


BASE_DESCRIPTOR = {"epi": dict(addend=A + 0x100000, addend_ld=256), "infer": dict(ab=A + 0x110000, relu=1), "opts": dict(reflect_pad=0)}
E = A + 0x120000                 # further descriptor operands


def descriptor_cases(name, kind):
    """(id, descriptor or None) per rule of the descriptor; `cout` is the call's channel count."""
    if kind == "epi":
        b = BASE_DESCRIPTOR["epi"]
        yield "null", None
        yield "empty", {}
        yield "only_relu_ab", dict(relu_ab=E)
        for f, ld in (("addend", "addend_ld"), ("mask_y", "mask_ld"), ("x", "x_ld")):
            yield f"{f}_misaligned", {**b, f: E + 4, ld: 256}
            yield f"{f}_ld_small", {**b, f: E, ld: 32}
            yield f"{f}_ld_mod4", {**b, f: E, ld: 258}
        yield "mask_y_and_mask_bits", dict(b, mask_y=E, mask_ld=256, mask_bits=E + 64, mask_bits_ld=32)
        yield "mask_y_and_relu_ab", dict(b, mask_y=E, mask_ld=256, x=E + 64, x_ld=256, relu_ab=E + 128)
        yield "mask_bits_and_relu_ab", dict(b, mask_bits=E, mask_bits_ld=32, x=E + 64, x_ld=256, relu_ab=E + 128)
        yield "mask_bits_ld_small", dict(b, mask_bits=E, mask_bits_ld=7)
        yield "relu_ab_without_x", dict(b, relu_ab=E)
        yield "relu_ab_misaligned", dict(b, x=E, x_ld=256, relu_ab=E + 68)
        full = dict(b, x=E, x_ld=256, mean=E + 64, invstd=E + 128, partials=E + 192)
        for drop in ("x", "mean", "invstd"):
            yield f"partials_without_{drop}", {k: v for k, v in full.items() if k != drop}
        yield "partials_mean_misaligned", dict(full, mean=E + 68)
        yield "partials_invstd_misaligned", dict(full, invstd=E + 132)
        # two faults: the first rule in the list answers
        yield "empty+bad_ld", dict(addend_ld=2)
        yield "bad_addend+bad_x", dict(b, addend_ld=32, x=E + 4, x_ld=256)
        yield "bad_mask_y+two_masks", dict(b, mask_y=E + 4, mask_ld=256, mask_bits=E, mask_bits_ld=32)
        yield "two_masks+partials_without_mean", dict(b, mask_y=E, mask_ld=256, mask_bits=E, mask_bits_ld=32, x=E, x_ld=256, partials=E)
    elif kind == "infer":
        b = BASE_DESCRIPTOR["infer"]
        yield "null", None
        yield "null_ab", dict(b, ab=None)
        yield "ab_misaligned", dict(b, ab=E + 4)
        yield "residual_misaligned", dict(b, residual=E + 4, residual_ld=256)
        yield "residual_ld_small", dict(b, residual=E, residual_ld=32)
        yield "residual_ld_mod4", dict(b, residual=E, residual_ld=258)
        yield "residual_is_out", dict(b, residual=A + 0x1000 * (POINTERS.index("out") + 1), residual_ld=256)
        if name == "diga_conv2d_nhwc_f32_infer":
            yield "residual_ld_2^32", dict(b, residual=E, residual_ld=1 << 32)
        yield "null_ab+bad_residual", dict(b, ab=None, residual=E + 4, residual_ld=2)
    else:
        yield "null", None
        for f, bad in (("reflect_pad", (2, -1)), ("upsample_shift", (3, -1)), ("activation", (2, -1))):
            for x in bad:
                yield f"{f}={x}", {f: x}
        if is_winograd(name):
            yield "upsample_shift=1", dict(upsample_shift=1)
            yield "activation=1", dict(activation=1)
            yield "reflect_tile2", dict(reflect_pad=1)           # (with tile = 2, below)
        elif "bf16x3" in name:
            yield "reflect_beyond_2^31", dict(reflect_pad=1)     # (bf16x3: with an in_ld that leaves the 32-bit kernel, below)


def variants(name):
    """(case id prefix, changes to the base call): the tiled weight gradient is walked once per family of answers -- a narrow tile
    with taps, a narrow tile at 1x1 (Cin % 8 is enough, the tap coordinates are still checked), and the 256 x 128 tile with taps and at
    1x1, whose rejections past the shape rule come in the words of the wide entry points."""
    if name != "diga_wgrad_bf16x6_tiled_f32in":
        return [("", {})]
    pw, wide = dict(r=1, s=1, oy=0, ox=0), dict(cout=512, cin=256, dy_ld=512, x_ld=256)
    return [("", {}), ("1x1:", pw), ("wide:", wide), ("wide1x1:", {**wide, **pw})]


def cases(valid=False):
    """(case id, entry point, argument values) of every rejected call (valid: and of the generated calls that break no rule)."""
    for name, (prefix, over) in ((n, v) for n in SPECS for v in variants(n)):
        b, ps, opt = {**base(name), **over}, params(name), optional(name)

        def one(cid, **kw):
            # a case changes parameters the entry point has (None: the generated case does not apply to it)
            return (f"{name}::{prefix}{cid}", name, {**b, **kw}) if all(k in b and k in ps for k in kw) else None

        out = []
        for p in ps:
            if p in POINTERS:
                if p not in opt:
                    out.append(one(f"{p}=null", **{p: 0}))
                for off in (2, 4, 8):
                    out.append(one(f"{p}+{off}", **{p: A + 0x1000 * (POINTERS.index(p) + 1) + off}))
            elif p in OUT_INTS:
                out.append(one(f"{p}=null", **{p: 0}))
            elif p in ("n", "hi", "wi", "ho", "wo", "h", "w", "cout", "cin", "r", "s", "rows", "batches", "k", "dil", "tile"):
                if p in ("cin", "cout") and "wgrad_winograd" in name:
                    continue                                     # (the weight-gradient split-K plan divides by the tile count: not a call to make)
                out.append(one(f"{p}=0", **{p: 0}))
                out.append(one(f"{p}=-4", **{p: -4}))
            elif p in ("in_ld", "out_ld", "x_ld", "dy_ld"):
                for x in (32, 66, 258, -1) + ((1 << 31,) if "f32in" in name and p != "out_ld" else ()):
                    out.append(one(f"{p}={x}", **{p: x}))
            elif p in ("sy", "sx"):
                for x in (0, -1) + ((1 << 30, 1 << 31) if multi_tap_form(name) else ()):
                    out.append(one(f"{p}={x}", **{p: x}))
            elif p in ("oy", "ox", "dy", "dx") and multi_tap_form(name):
                for x in (1 << 30, -(1 << 30), 1 << 31, -(1 << 31)):
                    out.append(one(f"{p}={x}", **{p: x}))
            elif p == "ws_bytes":
                out += [one("ws_bytes=0", ws_bytes=0), one("ws_bytes=64", ws_bytes=64), one("ws=null+ws_bytes=0", ws=0, ws_bytes=0)]
            elif p == "math":
                out += [one("math=2", math=2), one("math=-1", math=-1)]
            elif p in DESCRIPTORS:
                for did, d in descriptor_cases(name, p):
                    if d is None and p in opt:
                        continue
                    extra = {}
                    if did == "reflect_tile2":
                        extra = dict(tile=2)
                    elif did == "reflect_beyond_2^31":
                        extra = dict(in_ld=1 << 24)
                    out.append(one(f"{p}:{did}", **{p: d}, **extra))
        out.append(one("cin=48", cin=48))
        have = lambda **kw: {k: v for k, v in kw.items() if k in ps}          # (the leading dimensions this entry point has)
        out.append(one("cin=48+ld", **have(cin=48, in_ld=48, x_ld=48)))
        out.append(one("cout=62", cout=62))
        out.append(one("cout=66+ld", **have(cout=66, out_ld=68, dy_ld=68)))
        if is_winograd(name):
            px = dict(n=1 << 12, h=1 << 10, w=1 << 9)
            out += [one("2^31_pixels", **px), one("tile=3", tile=3), one("tile=8", tile=8), one("dil=4096", dil=4096), one("cout=64", cout=64),
                    one("too_many_tiles", n=1 << 10, h=1 << 10, w=1 << 10, tile=2, ws_bytes=BIG)]
            if "v_kept" in ps:
                out += [one("cin=64", cin=64), one("cout=128", cout=128), one("xp=null+v_kept=null", xp=0, v_kept=0), one("v_kept+4", v_kept=A + 4),
                        one("v_kept+4+dyp=null", v_kept=A + 4, dyp=0)]
            if "stats" in ps:
                out += [one("stats_tile2", stats=A, tile=2), one("stats+2", stats=A + 2), one("stats_tile2+ws_bytes=0", stats=A, tile=2, ws_bytes=0)]
            if "infer" in ps:
                out += [one("infer_tile2", tile=2), one("infer_tile2+in=null", tile=2, **{"in": 0})]
            if "opts" in ps:
                out += [one("reflect_dil=12", opts=dict(reflect_pad=1), dil=12), one("reflect_tile2+in=null", opts=dict(reflect_pad=1), tile=2, **{"in": 0})]
            if "v_keep" in ps and "epi" in ps:
                e = dict(BASE_DESCRIPTOR["epi"])
                out += [one("v_keep_flip", v_keep=A, flip=1), one("v_keep_epi", v_keep=A, epi=e), one("epi_bias", epi=e, bias=A),
                        one("epi_stats", epi=e, stats=A), one("epi_bias+empty", epi={}, bias=A), one("v_keep+2+flip", v_keep=A + 2, flip=1)]
            two = [dict(tile=3, cin=48), dict(ws_bytes=0, cin=48), dict(ws_bytes=0, **px), dict(tile=3, **px), dict(ws=0, tile=0)]
            first = "in" if "in" in ps else "dyp"
            two += [{first: 0, "n": 0}, {first: A + 4, "ws_bytes": 0}, {first: A + 4, "cin": 48}]
        elif "batched" in name:
            out += [one("2^31_rows", rows=1 << 31), one("rows=100", rows=100), one("batches=65536", batches=65536), one("cout=64", cout=64)]
            two = [{"rows": 100, params(name)[0]: 0}, {"rows": 100, params(name)[0]: A + 4}, {"cout": 0, "ws_bytes": 0}]
        else:
            out += [one("2^31_input_pixels", n=1 << 12, hi=1 << 10, wi=1 << 9), one("2^31_output_pixels", n=1 << 12, ho=1 << 10, wo=1 << 9),
                    one("rs=65", r=5, s=13), one("r=65", r=65, s=1)]
            if not has_taps(name):
                out.append(one("rs=9", r=3, s=3))
            if multi_tap_form(name):
                out += [one("rs_wraps", r=1 << 32, s=1 << 32), one("ho*sy=2^30", ho=1 << 10, sy=1 << 20), one("wo*sx=2^30", wo=1 << 10, sx=1 << 20),
                        one("r*dy=2^30", r=3, dy=1 << 29), one("s*dx=2^30", s=3, dx=-(1 << 29))]
            if "infer" in ps:
                out += [one("infer_bwd_data", tag=BWD_DATA) if "bf16x6" in name else None, one("infer_cout=18", cout=18, out_ld=20), one("infer_bias+4", bias=A + 4),
                        one("null_ab+cout=18", infer=dict(relu=1), cout=18, out_ld=20),
                        one("cout=18+bad_residual", cout=18, out_ld=20, infer=dict(BASE_DESCRIPTOR["infer"], residual=E + 4, residual_ld=256))]
            if "epi" in ps:
                out += [one("empty+cout=62", epi={}, cout=62), one("cout=62+bad_addend", cout=62, epi=dict(addend=E + 4, addend_ld=8)),
                        one("out_ld=66+bad_x", out_ld=66, epi=dict(BASE_DESCRIPTOR["epi"], x=E + 4, x_ld=256))]
            if "opts" in ps:
                out += [one("bad_opts+in=null", opts=dict(activation=2), **{"in": 0}), one("bad_opts+2^31", opts=dict(activation=2), n=1 << 12, ho=1 << 10, wo=1 << 9)]
            first = "in" if "in" in ps else "dyp"
            two = [{first: 0, "n": 0}, {first: 0, "cin": 48}, {first: A + 4, "cin": 48}, {first: A + 4, "n": 1 << 12, "ho": 1 << 10, "wo": 1 << 9},
                   {"cin": 48, "r": 65, "s": 1}, {"sy": 0, "r": 0}, {"oy": 1 << 31, "cin": 48}, {"n": 0, "r": 65}]
            if is_window(name):
                up2 = "conv_up2" in name
                refl = dict(BASE_DESCRIPTOR["opts"], upsample_shift=int(up2), reflect_pad=1)
                out += [one("rs=1", r=1, s=1), one("out_ld=2^31", out_ld=1 << 31), one("hi=2^30", hi=1 << 30), one("dy=4097", dy=4097),
                        one("window_too_large", r=7, s=7, dy=8, dx=8),
                        # a mirror reaches at most the far border (the collapsed form's own rule refuses these calls first)
                        one("reflect_oy", opts=refl, oy=-12), one("reflect_ox", opts=refl, ox=-12), one("reflect_far_y", opts=refl, dy=7),
                        one("reflect_far_x", opts=refl, dx=7), one("reflect_up1_oy", opts=dict(refl, upsample_shift=1), oy=-24),
                        one("reflect_far_y_ho", opts=refl, ho=40), one("reflect_far_x_wo", opts=refl, wo=72),
                        one("too_many_tiles", n=1 << 12, hi=1 << 8, wi=1 << 8, ho=1 << 9, wo=1 << 9, cout=1 << 16, out_ld=1 << 16)]
                if up2:          # what the collapsed form does not take (diga_conv_up2_bf16x6_plan), one reason each
                    out += [one("up_shift=0", opts={}), one("up_shift=2", opts=dict(upsample_shift=2)), one("cout=16", cout=16),
                            one("two_tile_rows", ho=16), one("two_tile_columns", wo=32), one("r=8", r=8), one("r=1", r=1), one("oy=1", oy=1),
                            one("interior_tap_outside", ho=28), one("oy=-9", oy=-9), one("img_ph+4+bad_opts", img_ph=A + 4, opts=dict(activation=2))]
                # two faults, rule by rule in the order of the checks
                taken = dict(cout=16) if up2 else dict(r=7, s=7, dy=8, dx=8)
                chain = [{"in": 0}, {"n": 0}] + ([] if up2 else [{"r": 65, "s": 1}]) + \
                    [{"cin": 48}, {"in_ld": 66}, {"in": A + 4}, {"opts": dict(activation=2)}, {"oy": 1 << 31}, taken, {"n": 1 << 12, "hi": 1 << 10, "wi": 1 << 9}]
                two += [{**a, **b} for a, b in zip(chain, chain[1:])]
                two += [{"opts": refl, "oy": -12, "n": 1 << 12, "hi": 1 << 10, "wi": 1 << 9}, {"opts": refl, "oy": -12, "in": A + 4},
                        {"opts": refl, "oy": -12, "cout": 1 << 16, "out_ld": 1 << 16, "n": 1 << 12, "hi": 1 << 8, "wi": 1 << 8, "ho": 1 << 9, "wo": 1 << 9}]
            if "opts" in ps and "stats" in ps:                   # a folded input map comes without statistics
                chain = [{"in": 0}, {"n": 0}, {"in_ld": -1}, {"r": 65, "s": 1}, {"sy": 0}, {"stats": A}, {"opts": dict(activation=2)},
                         {"oy": 1 << 31}, {"cin": 48}, {"in": A + 4}, {"n": 1 << 12, "ho": 1 << 10, "wo": 1 << 9}]
                out += [one("stats", stats=A), one("stats+4", stats=A + 4), one("hi=2^30", hi=1 << 30), one("hi=2^29_up_shift=1", hi=1 << 29, opts=dict(upsample_shift=1)),
                        one("too_many_tiles", n=1 << 10, ho=1 << 10, wo=1 << 10, cout=1 << 16, out_ld=1 << 16)]
                two += [{**a, **b} for a, b in zip(chain, chain[1:]) if not set(a) & set(b)]
            if name == "diga_collapse_up2_weights":
                out += [one("r=1", r=1), one("r=8", r=8), one("s=1", s=1), one("s=8", s=8), one("oy=1", oy=1), one("ox=1", ox=1),
                        one("oy=-2^30", oy=-(1 << 30)), one("ox=-2^30", ox=-(1 << 30)), one("2^40_elements", cout=1 << 31)]
                two += [{"wgt": A + 4, "r": 1}, {"wc": A + 4, "oy": 1}, {"wgt": 0, "wc": A + 4}]
            if "tiled" in name:
                # Cin % 8 is the rule at 1x1, Cin % 32 with taps; the tap coordinates answer before pitch, alignment, pixel count, workspace
                out += [one("cin=72+ld+ws_bytes=64", cin=72, x_ld=72, ws_bytes=64), one("cin=44+ld", cin=44, x_ld=44)]
                two += [{"oy": 1 << 31, "dy_ld": 66}, {"oy": 1 << 31, "dyp": A + 4}, {"oy": 1 << 31, "n": 1 << 12, "hi": 1 << 10, "wi": 1 << 9},
                        {"oy": 1 << 31, "ws_bytes": 0}, {"dy_ld": 66, "dyp": A + 4}, {"dyp": A + 4, "n": 1 << 12, "hi": 1 << 10, "wi": 1 << 9}]
            if "bm" in ps:
                two += [{"bm": 0, "cout": 0}, {"bm": 0, "bn": 0}]
            if "ws_bytes" in ps:
                two += [{"ws_bytes": 0, first: A + 4}, {"ws_bytes": 0, "n": 1 << 12, "ho": 1 << 10, "wo": 1 << 9}, {"ws_bytes": 0, "cin": 48},
                        {"ws_bytes": 0, "math": 2}, {"ws": 0, "n": 0}]
        out += [one("+".join(f"{k}={v}" if not isinstance(v, dict) else k + ":" + ",".join(f"{f}={x}" for f, x in v.items()) for k, v in kw.items()), **kw)
                for kw in two]
        seen = set()
        for c in out:
            if c is not None and c[0] not in seen and (valid or c[0] not in VALID_CALLS):
                seen.add(c[0])
                yield c


# Generated calls that break no rule of their entry point (a misaligned pointer where the kernels ask for less than 16 bytes, a
# parameter the entry point does not read, a shape that merely is another valid one): they would be launched, so they are no cases.
# The fixture lists them ("valid_calls"); the recorder refuses a call that is neither rejected nor listed.
def load_fixture():
    """The fixture, expanded: {"calls": {case id: [code, message]}, "queries": {query id: value}, "valid_calls": [case id]}.  On disk it
    is compact: the distinct (code, message) answers once, per entry point {case: answer index}, per query its values in grid order."""
    with open(FIXTURE) as fh:
        d = json.load(fh)
    grids = {}
    for qid, name, _ in queries():
        grids.setdefault(name, []).append(qid)
    assert all(len(grids[n]) == len(v) for n, v in d["queries"].items()), "the query grid changed: record again"
    return {"calls": {f"{n}::{c}": d["answers"][i] for n, per in d["calls"].items() for c, i in per.items()},
            "queries": {qid: v for n, vals in d["queries"].items() for qid, v in zip(grids[n], vals)},
            "valid_calls": [f"{n}::{c}" for n, cs in d["valid_calls"].items() for c in cs]}


def dump_fixture(data):
    answers = sorted({tuple(a) for a in data["calls"].values()})
    index = {a: i for i, a in enumerate(answers)}
    calls, valid, qs = {}, {}, {}
    for cid, a in data["calls"].items():
        calls.setdefault(cid.split("::")[0], {})[cid.split("::", 1)[1]] = index[tuple(a)]
    for cid in data["valid_calls"]:
        valid.setdefault(cid.split("::")[0], []).append(cid.split("::", 1)[1])
    for qid, name, _ in queries():
        qs.setdefault(name, []).append(data["queries"][qid])
    row = lambda v: json.dumps(v, separators=(",", ":"))
    block = lambda d: "{\n" + ",\n".join(f"{json.dumps(k)}:{row(d[k])}" for k in sorted(d)) + "\n}"
    with open(FIXTURE, "w") as fh:
        fh.write('{"answers":[\n' + ",\n".join(row(list(a)) for a in answers) + '\n],\n"calls":' + block(calls) + ',\n"queries":' + block(qs) +
                 ',\n"valid_calls":' + block(valid) + "\n}\n")


VALID_CALLS = set()              # (filled from the fixture below, once queries() is defined)


def call(_lib, name, vals):
    """Runs one case; (return code, message)."""
    held, args = [], []
    for p in params(name):
        x = vals[p]
        if p in DESCRIPTORS and x is not None:
            d = {"epi": _lib.BwdEpilogue, "infer": _lib.InferEpilogue, "opts": _lib.ConvOptions}[p]()
            for k, val in x.items():
                setattr(d, k, val)
            held.append(d)
            x = ctypes.byref(d)
        if p in OUT_INTS:
            held.append(ctypes.c_int(-7))
            x = ctypes.byref(held[-1]) if x else None
        args.append(x)
    assert len(args) == len(_lib.SIGNATURES[name][1]), name
    rc = getattr(_lib.lib, name)(*args)
    return rc, _lib.last_error()


# ------------------------------------------------------------------------------------------------------------------ queries
def is_query(name):
    return name in PLANS or name.endswith(("_workspace_bytes", "_stats_floats", "_stats_records", "_v_floats", "_tile_table_bytes", "_image_bytes")) or \
        name in ("diga_conv2d_stats_chunk_rows", "diga_conv2d_epi_chunk_rows")


ENTRY_PREFIXES = ("diga_conv2d_", "diga_conv_taps_", "diga_conv_window_", "diga_conv_up2_", "diga_collapse_up2_", "diga_infer_conv",
                  "diga_wgrad_bf16x6_")
QUERY_PREFIXES = ENTRY_PREFIXES + ("diga_split_bf16",)           # (of the weight-image functions only the size queries)


def in_scope(name, restype_is_int):
    """By name alone: an entry point or query that joins `_lib.SIGNATURES` under one of these names is in scope whether or not a case
    was written for it (the coverage test then fails until one is)."""
    if is_query(name):
        return name.startswith(QUERY_PREFIXES) or "batched_bf16x6" in name
    return restype_is_int and (name.startswith(ENTRY_PREFIXES) or "batched_bf16x6" in name)


def query(_lib, name, args):
    """The answer of one query: the value returned; for a plan function [value returned, the integers written]."""
    outs = [ctypes.c_int(-7) for _ in range(PLANS.get(name, 0))]
    got = getattr(_lib.lib, name)(*args, *[ctypes.byref(o) for o in outs])
    return [got] + [o.value for o in outs] if outs else got


def queries():
    """(query id, name, arguments): a grid of valid and invalid shapes per size / row query."""
    n_, hw, ch = (0, 1, 2, 1 << 12), (0, 12, 97, 1 << 10), (0, 48, 64, 128, 256, 320)
    wino = [(n, h, w, ci, co, d, t) for n, h, w in ((1, 12, 12), (2, 33, 29), (0, 12, 12), (1, 0, 12), (1 << 12, 1 << 10, 1 << 9), (2, 97, 97))
            for ci, co in ((128, 256), (64, 64), (48, 256), (128, 62), (0, 256), (256, 0), (256, 512))
            for d, t in ((1, 2), (1, 4), (2, 6), (12, 4), (0, 4), (4096, 4), (1, 3), (1, 0))]
    direct = [(n, h, w, co, ci, r, s) for n, h, w in ((1, 12, 12), (2, 33, 29), (2, 193, 193), (0, 12, 12), (1 << 12, 1 << 10, 1 << 9))
              for co, ci in ((64, 64), (256, 128), (512, 1024), (62, 64), (64, 48), (0, 64), (64, 0), (19, 256))
              for r, s in ((1, 1), (3, 3), (7, 7), (0, 3), (5, 13), (65, 1))]
    # (the queries that do not check their shape -- they divide by the tile count -- see valid shapes only)
    # the tiled weight gradient: the grid above (64 x 64, the wide tile, refused shapes) and one shape per further tile
    tiled = direct + [(n, h, w, co, ci, r, s) for n, h, w in ((2, 33, 29), (2, 193, 193))
                      for co, ci in ((64, 256), (128, 512), (256, 64), (128, 64), (40, 72), (320, 72)) for r, s in ((1, 1), (3, 3))]
    plain = [g for g in direct if g[0] == 1 or g[0] == 2 if g[3] > 0 and g[4] > 0 and g[5] > 0 and g[5] * g[6] <= 64]
    grids = {
        "diga_conv2d_winograd_workspace_bytes": wino, "diga_conv2d_winograd_bf16x6_workspace_bytes": wino,
        "diga_conv2d_wgrad_winograd_workspace_bytes": [g + (k,) for g in wino for k in (0, 1)],
        "diga_conv2d_wgrad_winograd_bf16x6_workspace_bytes": [g + (k,) for g in wino for k in (0, 1)],
        "diga_conv2d_winograd_tile_table_bytes": sorted({(n, h, w, d, t) for n, h, w, _, _, d, t in wino}),
        "diga_conv2d_winograd_stats_records": sorted({(n, h, w, co, d, t) for n, h, w, _, co, d, t in wino}),
        "diga_conv2d_winograd_stats_floats": sorted({(n, h, w, co, d, t) for n, h, w, _, co, d, t in wino}),
        "diga_conv2d_winograd_v_floats": sorted({(n, h, w, ci, d, t) for n, h, w, ci, _, d, t in wino}),
        "diga_conv2d_wgrad_workspace_bytes": plain, "diga_conv2d_wgrad_twin_workspace_bytes": plain,
        "diga_conv2d_wgrad_bf16x6_workspace_bytes": plain, "diga_conv_taps_wgrad_bf16x6_workspace_bytes": direct,
        "diga_wgrad_bf16x6_tiled_workspace_bytes": tiled,
        "diga_conv2d_stats_floats": list(itertools.product(n_, hw, (12, 29), ch)),
        "diga_split_bf16_image_bytes": list(itertools.product((0, 19, 64, 65, 256), (0, 1, 9, 49), (0, 32, 48, 64, 160))),
        "diga_split_bf16x6_image_bytes": list(itertools.product((0, 19, 64, 65, 256), (0, 1, 9, 49), (0, 32, 48, 64, 160))),
        "diga_wgrad_batched_bf16x6_workspace_bytes": list(itertools.product((0, 64, 100, 2304, 1 << 31), (0, 4, 16, 36, 65536), (0, 256, 320, 512),
                                                                            (0, 128, 192, 256))),
    }
    rows = [(n, h, w, ci, ho, wo, co, r, s, sy, sx, oy, ox, m)
            for n, h, w, ho, wo in ((2, 193, 193, 193, 193), (2, 97, 97, 97, 97), (4, 193, 193, 97, 97), (1, 12, 12, 12, 12), (16, 256, 256, 256, 256))
            for ci, co in ((64, 256), (256, 128), (48, 128), (64, 64), (2048, 512))
            for r, s, sy, sx, oy, ox in ((1, 1, 1, 1, 0, 0), (1, 1, 2, 2, 0, 0), (3, 3, 1, 1, -1, -1), (1, 1, 1, 1, 0, 1))
            for m in (0, 1, 2, 3)]
    grids["diga_conv2d_stats_chunk_rows"] = rows
    grids["diga_conv2d_epi_chunk_rows"] = rows
    # (Hi, Wi, Cin, Cout, R, S, dil_y, dil_x, upsample_shift)
    grids["diga_conv_window_bf16x6_plan"] = [(h, w, ci, co, r, s, dy, dx, up) for h, w in ((12, 12), (97, 33), (0, 12), (12, -1))
                                             for ci, co in ((64, 64), (32, 3), (64, 16), (64, 17), (48, 64), (0, 64), (64, 0))
                                             for r, s, dy, dx in ((3, 3, 1, 1), (5, 5, 1, 1), (7, 7, 1, 1), (3, 3, 2, 2), (3, 3, 14, 14), (7, 7, 4, 4),
                                                                  (7, 7, 8, 8), (9, 9, 1, 1), (1, 1, 1, 1), (1, 2, 1, 1), (65, 1, 1, 1), (8, 8, 1, 1),
                                                                  (3, 3, 0, 1), (3, 3, 1, 4097), (3, 1, 4096, 1))
                                             for up in (0, 1, 2, 3, -1)]
    # (Hi, Wi, Cin, Cout, Ho, Wo, R, S, off_y0, off_x0, dil_y, dil_x, upsample_shift, reflect_pad)
    grids["diga_conv_up2_bf16x6_plan"] = [(h, w, ci, co, ho, wo, r, s, oy, ox, dy, dx, up, refl)
                                          for h, w, ho, wo in ((10, 18, 20, 36), (12, 24, 24, 48), (96, 96, 192, 192), (8, 16, 16, 32), (10, 18, 20, 32),
                                                               (10, 18, 24, 36), (10, 18, 20, 52), (0, 18, 20, 36), (1 << 29, 18, 20, 36), (10, 18, 0, 36))
                                          for ci, co in ((32, 72), (64, 64), (64, 16), (48, 72))
                                          for r, s, oy, ox in ((5, 5, -2, -2), (3, 3, -1, -1), (7, 7, -3, -3), (4, 4, -1, -2), (2, 2, 0, 0), (5, 5, -3, -2),
                                                               (8, 8, -3, -3), (1, 3, 0, -1), (3, 3, 1, -1), (5, 5, -2, -9), (5, 5, -9, -2))
                                          for dy, dx, up, refl in ((1, 1, 1, 0), (1, 1, 1, 1), (2, 1, 1, 0), (1, 2, 1, 0), (1, 1, 0, 0), (1, 1, 2, 0),
                                                                   (1, 1, 1, 2), (1, 1, 1, -1))]
    for name, grid in grids.items():
        for g in grid:
            yield f"{name}{tuple(g)}", name, tuple(g)


if os.path.exists(FIXTURE):
    VALID_CALLS = set(load_fixture()["valid_calls"])


def record(_lib, relist, only=""):
    """relist: rewrite the list of valid calls from what this library accepts (to be read through before it is committed).
    only: the entry points and queries whose names start with it (for --merge)."""
    got, accepted = {}, []
    for cid, name, vals in cases(valid=relist):
        if not name.startswith(only):
            continue
        rc, msg = call(_lib, name, vals)
        if rc in REJECTED:
            got[cid] = [rc, msg]
        else:
            accepted.append(cid)
    if accepted and not relist:
        raise SystemExit("calls that no argument check rejects and that are not listed as valid calls:\n" + "\n".join(accepted))
    q = {qid: query(_lib, name, args) for qid, name, args in queries() if name.startswith(only)}
    return {"calls": got, "queries": q, "valid_calls": sorted(accepted) if relist else sorted(VALID_CALLS)}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from diga_amd import _lib
    if "--merge" in sys.argv:
        # entry points that join the fixture later: their answers are recorded (valid calls relisted), every other entry is kept as it is
        data = load_fixture()
        for only in sys.argv[sys.argv.index("--merge") + 1:]:
            new = record(_lib, True, only)
            assert not (set(new["calls"]) | set(new["queries"])) & (set(data["calls"]) | set(data["queries"])), "already recorded: " + only
            data["calls"].update(new["calls"])
            data["queries"].update(new["queries"])
            data["valid_calls"] = sorted(set(data["valid_calls"]) | set(new["valid_calls"]))
            print(f"{only}: {len(new['calls'])} calls, {len(new['queries'])} queries, {len(new['valid_calls'])} valid calls merged into {FIXTURE}")
        dump_fixture(data)
    elif "--record" in sys.argv:
        data = record(_lib, "--relist-valid" in sys.argv)
        dump_fixture(data)
        print(f"{len(data['calls'])} calls, {len(data['queries'])} queries, {len(data['valid_calls'])} valid calls -> {FIXTURE}")
