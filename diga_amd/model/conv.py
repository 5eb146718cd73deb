"""Conv2d on the MI355X fp32 matrix cores (diga_conv2d_nhwc_f32 and friends).

`DigaConv2d` is a drop-in for the nn.Conv2d layers of the reference model
(G5/model/seg_model_noaux.py:57-101,140-172): same constructor, same parameter names and [Cout,Cin,R,S]
shapes in the state_dict.  Inside, weights live in channels_last memory ([Cout][R][S][Cin]) and
activations travel NHWC; tensors handed to / returned from the module are NCHW-shaped views of that
memory (torch's channels_last format), so neighbouring torch ops see ordinary 4-D tensors.
Channel counts that are not multiples of 32 (the 3-channel image, the 19-class head) are zero-padded.
"""
import ctypes
import os
import sys
from typing import NamedTuple

import torch
import torch.nn as nn

_pkg = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(_pkg) not in sys.path:
    sys.path.append(os.path.dirname(_pkg))
from diga_amd import _lib, config  # noqa: E402

_TAG_FWD, _TAG_BWD_DATA = _lib.PROF_TAGS.index("conv_fwd"), _lib.PROF_TAGS.index("conv_bwd_data")


def _pad_to(c, q=32):
    return (c + q - 1) // q * q


def _pad_last(t, c_to):
    """Zero-pad the last (channel) dimension of a contiguous tensor to c_to."""
    c = t.shape[-1]
    if c == c_to:
        return t
    out = t.new_zeros(t.shape[:-1] + (c_to,))
    out[..., :c] = t
    return out



def _bias_grad(gy):
    """Bias gradient of a convolution = column sums of the NHWC output gradient (torch: grad_output.sum((0, 2, 3))), on
    diga_colsum_nhwc.  gy: [N,H,W,K] (a channel slice of a contiguous NHWC tensor is fine)."""
    k = gy.shape[-1]
    ld = gy.stride(2)
    m = gy.shape[0] * gy.shape[1] * gy.shape[2]
    dense = gy.stride(3) == 1 and gy.stride(1) == gy.shape[2] * ld and gy.stride(0) == gy.shape[1] * gy.stride(1)
    if not dense or ((k % 4 != 0 or ld % 4 != 0) and k > 64):
        return gy.sum(dim=(0, 1, 2))                          # (layouts no model of this repository produces)
    out = torch.empty(k, dtype=torch.float32, device=gy.device)
    ws = _lib.workspace(_lib.lib.diga_norm_workspace_bytes(m, 1, k), gy.device, "norm")
    _lib.call("diga_colsum_nhwc", _lib.ptr(gy), ld, _lib.ptr(out), m, k, _lib.ptr(ws), ws.numel(), _lib.stream())
    return out


def _use_twin(cin, k, taps, shared):
    """The staging-free kernel (both operands pre-split, LDS-DMA) needs one extra pass over the activations to build
    their split twin (read 4 B + write 4 B per element).  That pays when the tensor is read by many tiles: convs with
    more than one tap, or several convs on one input (`shared`, the ASPP branches).  DIGA_CONV_TWIN=0 switches the
    path off, =1 forces it for every eligible conv."""
    mode = config.active().conv_twin
    if mode == "0" or cin % 32 != 0 or k <= 64:
        return False
    return mode == "1" or taps > 1 or shared


def _use_x6(cin, r, s):
    """bf16x6 eligibility of a layer (conv_math = 2; csrc/conv_bf16x6.h): a 1x1 convolution (groups = 1 is all DigaConv2d builds) whose
    PADDED input channel count is a multiple of 32 -- any stride, any output channel count (the kernels clamp ragged channel tiles,
    the backward passes see channel counts padded to 32), with or without bias, BatchNorm statistics or a backward-data epilogue.
    Not eligible: multi-tap layers (Winograd / direct fp32), the stem's im2col GEMM (its backward has its own path) and calls with a
    folded input map / activation (`opts`) -- the callers pass those as pointwise_ok=False to _layer_math.  (config.x6_taps, _x6_taps
    below, is the opt-in that sends the multi-tap calls left on the direct fp32 kernels, and the stem, to bf16x6 too.)"""
    return r == 1 and s == 1 and cin % 32 == 0


def _x6_taps():
    """True when config.x6_taps is in force (conv_math = 2; both read per call): a multi-tap call that _plan / _wgrad_plan would leave
    on the direct fp32 kernels runs on the multi-tap bf16x6 kernels instead (family "x6rs", the `diga_conv_taps_*` entry points), and
    the stem's im2col GEMM on the pointwise ones ("x6ls") -- the loader form whatever x6_split says: fp32 tensors read in place, no
    triplets.  Winograd keeps every call it takes."""
    return _lib.get_conv_math() == 2 and config.active().x6_taps


def _x6_opts():
    """True when config.x6_opts is in force (conv_math = 2; both read per call): a call with a folded input map / activation (`opts`:
    the frozen translator's reflection padding, nearest upsampling and tanh) is planned by the rules of a call without -- _taps_ok
    admits it, and a "winograd_reflect" call asks _wino_x6.  Nothing else reads it; pointwise calls with options stay exact fp32."""
    return _lib.get_conv_math() == 2 and config.active().x6_opts


def _taps_ok(cin, r, s, copt):
    """Eligibility of a call for the "x6rs" family: more than one tap (at most 64: the live-tap mask), padded Cin % 32 == 0, no folded
    input map / activation -- unless config.x6_opts admits those (the `_opts` entry point)."""
    return 1 < r * s <= 64 and cin % 32 == 0 and (not copt or _x6_opts())


def _x6_window(hi, wi, cin, k, r, s, doff, shift):
    """True when config.x6_window is in force (conv_math = 2 with x6_taps; read per call) AND the library's window rule
    (diga_conv_window_bf16x6_plan, the one place that decides) takes a stride-1 forward of r x s taps at dilation doff on the
    2^shift upsampling of an hi x wi x cin image with k output channels: the call then runs on the window form ("x6win",
    diga_conv_window_bf16x6_f32in).  Only _plan asks, for a forward without statistics and without an epilogue."""
    if not (_x6_taps() and config.active().x6_window) or doff[0] < 1 or doff[1] < 1:
        return False
    th, tw, cols = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    return _lib.lib.diga_conv_window_bf16x6_plan(hi, wi, cin, k, r, s, doff[0], doff[1], shift, ctypes.byref(th), ctypes.byref(tw),
                                                 ctypes.byref(cols)) == 1


def _x6_up2(hi, wi, cin, k, ho, wo, r, s, off0, doff, opts):
    """True when config.x6_up2 is in force (conv_math = 2 with x6_taps, x6_opts and x6_window; read per call) AND the library's rule
    (diga_conv_up2_bf16x6_plan, the one place that decides) takes the call: a window-form forward of the 2x nearest upsampling of an
    hi x wi x cin image whose interior tiles then run on phase-collapsed weights ("x6up2", diga_conv_up2_bf16x6_f32in).  Only _plan
    asks, for a call it would otherwise answer "x6win" with options."""
    if not (_x6_opts() and config.active().x6_up2):
        return False
    rc, sc = ctypes.c_int(0), ctypes.c_int(0)
    return _lib.lib.diga_conv_up2_bf16x6_plan(hi, wi, cin, k, ho, wo, r, s, off0[0], off0[1], doff[0], doff[1], int(opts[1]),
                                              int(opts[0]), ctypes.byref(rc), ctypes.byref(sc)) == 1


def _x6_fit(kp, cp):
    """True when config.x6_wgrad_tile = "fit" is in force (conv_math = 2; both read per call) AND the library's tile rule
    (diga_wgrad_bf16x6_tile, the one place that decides) gives a layer with kp (padded) output and cp input channels something other
    than the 256 x 128 tile: its loader-form weight gradient ("x6ls" / "x6rs") then runs on diga_wgrad_bf16x6_tiled_f32in.  The pass
    form ("x6"), Winograd and every forward / backward-data call never ask."""
    if _lib.get_conv_math() != 2 or config.active().x6_wgrad_tile != "fit":
        return False
    bm, bn = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("diga_wgrad_bf16x6_tile", kp, cp, ctypes.byref(bm), ctypes.byref(bn))
    return (bm.value, bn.value) != (256, 128)


def _x6_loader():
    """bf16x6 operand form of the active configuration (config.x6_split, read per call): True = "loader", the GEMMs' loader waves
    split the fp32 tensors themselves (the `_f32in` entry points: no triplet pass, no triplet buffer, channel slices read in place);
    False = "pass", diga_make_triplet + the triplet entry points.  Bit-identical results."""
    return config.active().x6_split == "loader"


def _nhwc_ld(t):
    """Row pitch (floats between pixels) of an NHWC tensor the `_f32in` kernels can read in place -- unit channel stride, dense pixel
    order, pitch % 4 == 0, 16-byte aligned base: a contiguous tensor or a channel slice of one -- else None."""
    ld = t.stride(2)
    ok = (t.dtype == torch.float32 and t.stride(3) == 1 and ld >= t.shape[3] and ld % 4 == 0 and t.stride(1) == t.shape[2] * ld
          and t.stride(0) == t.shape[1] * t.stride(1) and t.data_ptr() % 16 == 0)
    return ld if ok else None


def _layer_math(r, s, cin, pointwise_ok=True):
    """The arithmetic ONE layer runs in under the active conv_math: 0 / 1 as set; in mode 2 (bf16x6) 2 for an eligible layer
    (_use_x6) and 0 -- the exact-fp32 paths, Winograd included -- for every other one.  Every path decision and every `math`
    argument handed to the library reads this, never the process-wide mode."""
    m = _lib.get_conv_math()
    if m != 2:
        return m
    return 2 if (pointwise_ok and _use_x6(cin, r, s)) else 0


def takes_twin_only_input(conv, pointwise_ok=False):
    """True when `conv` (a DigaConv2d) reads its input exclusively through split twins -- forward on the twin kernel and
    backward-weight on the twin kernel -- so that its producer may write the twin instead of the fp32 tensor.
    pointwise_ok: also for 1x1 layers (worth it only when both of its twins are free, i.e. under autograd where the
    weight gradient gains 35-39 %; the forward kernel alone gains nothing on 8-step tiles)."""
    taps = conv.kernel_size[0] * conv.kernel_size[1]
    cfg = config.active()
    return (cfg.conv_math == 1 and cfg.conv_twin != "0" and cfg.twin_only
            and (taps > 1 or pointwise_ok) and conv.in_channels % 32 == 0 and conv.in_channels > 64 and conv.out_channels >= 256 and conv.out_channels % 8 == 0
            and tuple(conv.stride) == (1, 1) and conv.groups == 1)


def _wino_x6():
    """_layer_math's sibling for the layers it sends to 0 in mode 2: True when a call that takes the fp32 Winograd path runs its
    Winograd-domain GEMMs on bf16x6 instead (conv_math = 2 and config.x6_winograd, both read per call; the `_bf16x6` Winograd entry
    points -- same tile table, transforms, keep-V, statistics and backward epilogue).  Path selection itself never reads this: only
    the arithmetic of the products changes, and a kept V is fp32 either way, so forward and backward may differ."""
    return _lib.get_conv_math() == 2 and config.active().x6_winograd


INLINE_WGRAD = "inline"       # `uses` of a functional _Conv2dFn call whose weight is a non-leaf tensor (see backward)
_WINO_CACHE = {}
# bench.py sets this to a dict to learn what the convolutions of a step multiply: name -> [FLOPs of the direct
# convolution (the algorithmic work), FLOPs the matrix cores execute (16/36 of it per 2x2 tile on the Winograd path)]
flop_log = None


# a test or tool sets this to a dict to learn which kernels ran: (pass, arithmetic) -> launches, pass in "fwd" / "dgrad" / "wgrad",
# arithmetic in "f32" / "bf16x3" / "bf16x6" / "bf16x6/ls" (bf16x6 with the operands split by the loader waves, config.x6_split = "loader") /
# "winograd" / "winograd/x6" (the Winograd path with its products on bf16x6, config.x6_winograd); "f32+bn" / "winograd+bn": a forward with the eval-mode BatchNorm behind it
# folded into its epilogue (config.fold_eval_bn); "bf16x6+bn" / "bf16x6/ls+bn" / "winograd/x6+bn": the same on the bf16x6 kernels
# (config.fold_eval_bn_x6); "bf16x6/taps" / "bf16x6/taps+bn": a multi-tap call on the bf16x6 kernels (config.x6_taps);
# "bf16x6/ls/fit" / "bf16x6/taps/fit" (wgrad only): the loader-form weight gradient on a narrow tile (config.x6_wgrad_tile = "fit");
# "f32/s2" (dgrad only): the phase-split backward-data of a stride-2 multi-tap conv (diga_dgrad_strided_f32; exact fp32 in every mode)
path_log = None


def _log_path(tag, arith):
    if path_log is not None:
        key = (tag if isinstance(tag, str) else ("dgrad" if tag == _TAG_BWD_DATA else "fwd"), arith)
        path_log[key] = path_log.get(key, 0) + 1


def _strided_dgrad_ok(r, s, stride, padding, dilation):
    """True where a strided conv's input gradient runs on diga_dgrad_strided_f32 (the phase-split kernel, path_log arithmetic "f32/s2"):
    stride (2, 2), dilation (1, 1), more than one tap, padding smaller than the kernel.  A strided 1x1 keeps its GEMM + scatter route."""
    return (tuple(stride) == (2, 2) and tuple(dilation) == (1, 1) and r * s > 1
            and 0 <= padding[0] < r and 0 <= padding[1] < s)


def _log_flops(name, direct, executed):
    if flop_log is not None:
        e = flop_log.setdefault(name, [0.0, 0.0])
        e[0] += direct
        e[1] += executed


# Path switches live in diga_amd/config.py (StepConfig: winograd, winograd_ratio, winograd_max_tile, winograd_keep_v, winograd_stats,
# keep_v_max_gb, keep_v_min_device_gb; environment variables give their DEFAULTS, read once at import); a convolution call reads the
# active configuration, makes no environment or driver query.  winograd_max_tile = 2 keeps every layer on F(2x2,3x3).
_DEVICE_TOTAL = {}
_KEEP_OFF = set()             # devices on which a keep-V allocation failed: the recompute path from then on (reset_keep_decisions())


def reset_keep_decisions():
    """Forget that a kept-transform allocation ran out of memory (e.g. after the caller freed a second model)."""
    _KEEP_OFF.clear()


def _room_for(nbytes, device):
    """Keeping a layer's transformed input V alive until its weight gradient is a memory-for-bandwidth trade (the backward-weight
    pass skips one input transform: a bandwidth pass over the input + V; 26 layers, ~4 ms of a 424 ms C2 step).  Decision:
    `winograd_keep_v` on (default), the layer's V <= `keep_v_max_gb` (8 GiB; the largest C2 layer keeps 2.2 GB) and the device
    has >= `keep_v_min_device_gb` of memory in total (160 GiB: an MI355X has 288 GB; the C2 step keeps ~21 GB of V and peaks at
    the figure bench.py reports as peak_mem_gb) -- shape and static device properties only, no free-memory query.  If the
    allocation itself fails, `_alloc_keep_v` switches the device to the recompute path."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    cfg = config.active()
    if not cfg.winograd_keep_v or idx in _KEEP_OFF or nbytes > int(cfg.keep_v_max_gb * (1 << 30)):
        return False
    total = _DEVICE_TOTAL.get(idx)
    if total is None:
        total = _DEVICE_TOTAL[idx] = torch.cuda.get_device_properties(idx).total_memory
    return total >= int(cfg.keep_v_min_device_gb * (1 << 30))


def _alloc_keep_v(nfloats, device):
    """The kept transform's buffer, or None when the policy says recompute or the allocation fails (out of memory: the device is
    switched to the recompute path instead of failing the step)."""
    if not _room_for(nfloats * 4, device):
        return None
    try:
        return torch.empty(nfloats, dtype=torch.float32, device=device)
    except torch.cuda.OutOfMemoryError:
        _KEEP_OFF.add(device.index if device.index is not None else torch.cuda.current_device())
        return None


def _wino_plan(hi, wi, d):
    """(tile, ratio): the Winograd output-tile edge for a stride-1 3x3 layer with dilation d on an hi x wi map and the share of the
    direct convolution's multiplications it executes.  The d*d sub-images {(a + d i, b + d j)} are cut into m x m tiles of
    (m + 2)^2 products each: F(2x2,3x3) 16 per 4 outputs, F(4x4,3x3) 36 per 16, F(6x6,3x3) 64 per 36; the smallest count wins, the
    smaller tile on a tie (97 x 97 map: dilation 1 / 2 / 4 / 18 -> 0.218 / 0.218 / 0.218 / 0.245 with 6x6 tiles, where 4x4 tiles
    give 0.266 / 0.266 / 0.266 / 0.551; dilation 12 / 24 -> 0.266 with 4x4 tiles, 0.435 with 6x6; direct = 1)."""
    max_tile = config.active().winograd_max_tile
    key = (hi, wi, d, max_tile)
    plan = _WINO_CACHE.get(key)
    if plan is None:
        def tiles(length, m):
            return sum((((length - a + d - 1) // d if length > a else 0) + m - 1) // m for a in range(d))
        plan = None
        for m in (2, 4, 6):
            if m > max_tile:
                continue
            ratio = float((m + 2) ** 2) * tiles(hi, m) * tiles(wi, m) / (9.0 * hi * wi)
            if plan is None or ratio < plan[1] - 1e-9:
                plan = (m, ratio)
        _WINO_CACHE[key] = plan
    return plan


_TILE_TABLES = {}


def _tile_table(n, hi, wi, d, tile, device):
    """The Winograd tile table of a geometry (a function of (N, H, W, dilation, tile) only: image and top-left output pixel of every
    tile), built once per device and reused by every call on that geometry -- forward, backward-data and backward-weight of all
    layers that share it (layer3's 23 conv2 layers: 4 calls each per step) -- instead of one wino_tiles_kernel launch per call (136
    per C2 step).  The one-time build is followed by a stream synchronisation: the table is read from several streams (student,
    teacher, weight-gradient side stream).  Not inside a stream capture (no sync there): the call then builds its own."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, n, hi, wi, d, tile)
    tab = _TILE_TABLES.get(key)
    if tab is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        tab = torch.empty(_lib.lib.diga_conv2d_winograd_tile_table_bytes(n, hi, wi, d, tile), dtype=torch.uint8, device=device)
        _lib.call("diga_conv2d_winograd_tile_table", _lib.ptr(tab), n, hi, wi, d, tile, _lib.stream())
        torch.cuda.current_stream(device).synchronize()
        # never evicted: a table is a few KB, its device pointer may be baked into captured HIP graphs and kernels on the side /
        # teacher streams may still be reading it (clearing the cache at 256 geometries freed tables in use)
        _TILE_TABLES[key] = tab
    return tab


def _wino_ratio(hi, wi, d):
    return _wino_plan(hi, wi, d)[1]


def _winograd_ok(n, hi, wi, cin, k, r, s, stride, off0, doff, ho, wo):
    """Exact-fp32 mode: stride-1 'same' 3x3 layers (dilation d = padding, forward or backward-data geometry) go through
    Winograd (csrc/winograd.hip; tile from _wino_plan) when cutting the d*d sub-images into tiles leaves few enough
    multiplications: share of the direct convolution <= `winograd_ratio` (default 0.62; dilation 24 on a 97x97 map has 5x5
    sub-images -> 0.98 and stays direct, where the kernel also skips the dead taps).  `winograd = False` switches the path off."""
    cfg = config.active()
    if not cfg.winograd:
        return False
    d = abs(doff[0])
    if not (r == 3 and s == 3 and tuple(stride) == (1, 1) and doff[0] == doff[1] and d >= 1 and off0[0] == -doff[0]
            and off0[1] == -doff[1] and hi == ho and wi == wo and cin % 32 == 0 and cin >= 128 and k % 4 == 0 and k >= 128):
        return False
    ratio = _wino_ratio(hi, wi, d)
    # (the batched GEMM indexes its products * tiles rows as a [rows / 256][256] image with 15-bit row coordinates)
    return ratio <= cfg.winograd_ratio and n * hi * wi * ratio * 9.0 / 256.0 < 32000


class _Path(NamedTuple):
    """Which kernel ONE convolution call runs on.  _plan (forward / backward-data) and _wgrad_plan (weight gradient) decide it, once
    per call, from the call's geometry, the features it wants and the active configuration; everything else -- the launch, the
    statistics buffer DigaConv2d allocates, infer_kernel, winograd_stats_plan, what a forward saves for its backward -- reads it."""
    family: str                # "x6ls" (bf16x6, operands split by the loader waves) / "x6" (bf16x6 on triplets) / "x6rs" (multi-tap bf16x6) /
    #                            "x6win" (multi-tap bf16x6 from an LDS window: config.x6_window) / "x6up2" (... of a 2x upsampled input, the
    #                            interior on phase-collapsed weights: config.x6_up2) / "twin" / "bf16x3" /
    #                            "winograd" / "winograd_reflect" (reflection padding folded into the input transform) / "f32"
    variant: str               # "" / "epi" (backward-data epilogue) / "opts" / "infer" / "keep" (Winograd forward that keeps V)
    math: int                  # the layer's arithmetic (_layer_math): the `math` argument the library is given
    arith: str                 # the arithmetic under which path_log counts the call
    tile: int = 0              # Winograd: output-tile edge and the share of the direct convolution's multiplications (_wino_plan)
    ratio: float = 1.0
    x6w: bool = False          # Winograd: the Winograd-domain products run on bf16x6 (_wino_x6)
    flops: bool = True         # counted in flop_log (all but the bf16x3 forward / backward-data kernels, the twin weight gradient, the stem's)
    fit: bool = False          # weight gradient of "x6ls" / "x6rs": on the narrow tile of diga_wgrad_bf16x6_tiled_f32in (_x6_fit)


def _plan(n, hi, wi, cin, k, r, s, stride, off0, doff, ho, wo, tag=_TAG_FWD, stats=None, epi=False, opts=None, infer=False,
          shared=False, must_twin=False, x6_ok=True, keep=False):
    """The _Path of a forward (tag = _TAG_FWD, doff = dilation) or backward-data (_TAG_BWD_DATA, doff = -dilation) call on an
    [n,hi,wi,cin] input (cin padded) with tap offsets off0 + i * doff, or a RuntimeError where the library has no kernel for the
    combination.  Pure: no tensor, no device; the switches are read from the active configuration now, nothing is remembered.
    stats: None / "chunks" (equal-sized partial sums for the BatchNorm behind the conv) / "records" (the Winograd output transform's);
    epi / infer: the call carries a backward-data / inference epilogue; opts: (reflect_pad, upsample_shift, activation) or None;
    shared: a twin / triplet box comes with the input; must_twin: the input holds split-twin bytes; x6_ok=False keeps a pointwise
    call off bf16x6 (the stem); keep: the caller wants the weight gradient, so a Winograd forward with Cout % 256 == 0 and
    Cin % 128 == 0 keeps its transformed input for it (config.winograd_keep_v)."""
    copt = opts is not None and any(opts)
    if copt and (stats is not None or epi):
        raise RuntimeError("DigaConv2d: folded padding / upsampling / activation cannot be combined with BN statistics or a backward epilogue")
    stem_x6 = not x6_ok and _x6_taps()                         # the stem's im2col GEMM: on bf16x6 only under config.x6_taps
    math = _layer_math(r, s, cin, (x6_ok or stem_x6) and not copt)
    fold_x6 = infer and config.active().fold_eval_bn_x6        # the bf16x6 kernels' inference epilogue is a switch of its own
    if infer and ((math != 0 and not (math == 2 and fold_x6)) or copt or stats is not None or epi or tag != _TAG_FWD or k % 4 != 0):
        raise RuntimeError("DigaConv2d: no kernel with the inference epilogue for this call (exact-fp32 forward -- or, with "
                           "config.fold_eval_bn_x6, bf16x6 -- without statistics, Cout % 4 == 0; check infer_kernel / folds_eval_bn first)")
    variant = "infer" if infer else "epi" if epi else "opts" if copt else ""
    if math == 2:
        # bf16x6: the weights as a pre-split image; the activations read as fp32 and split by the loader waves, or pre-split into
        # three bf16 planes and copied global -> LDS by LDS-DMA (csrc/conv_bf16x6.h)
        bn = "+bn" if infer else ""
        return _Path("x6ls", variant, 2, "bf16x6/ls" + bn) if (_x6_loader() or stem_x6) else _Path("x6", variant, 2, "bf16x6" + bn)
    if math == 1 and _use_twin(cin, k, r * s, shared) and n * hi * wi * cin * 4 < (1 << 40):
        # split-bf16 arithmetic without register staging: both operands pre-split, copied global -> LDS by LDS-DMA
        return _Path("twin", variant, 1, "bf16x3", flops=False)
    if must_twin:
        raise RuntimeError("DigaConv2d: the input holds split-twin bytes but the twin kernel is not selected "
                           "(conv math or config.conv_twin changed since the producer ran)")
    if math == 1:
        # split-bf16 arithmetic: the weights are split once per call (two bf16 arrays), the activations inside the kernel
        return _Path("bf16x3", variant, 1, "bf16x3", flops=False)
    if copt:
        # reflection padding folded into the Winograd input transform (the translator's 3x3 ResBlock convs; round 5)
        if (opts[0] and not opts[1] and not opts[2] and 0 < doff[0] < min(hi, wi)
                and _winograd_ok(n, hi, wi, cin, k, r, s, stride, off0, doff, ho, wo)):
            tile, ratio = _wino_plan(hi, wi, doff[0])
            if tile >= 4:
                # (the mirror lives in the input transform only: under config.x6_opts the products behind it take _wino_x6's answer)
                x6w = _x6_opts() and _wino_x6()
                return _Path("winograd_reflect", "opts", 0, "winograd/x6" if x6w else "winograd", tile, ratio, x6w)
    elif stats != "chunks" and _winograd_ok(n, hi, wi, cin, k, r, s, stride, off0, doff, ho, wo):
        tile, ratio = _wino_plan(hi, wi, abs(doff[0]))
        if stats is not None and (tile < 4 or epi or doff[0] < 0):
            raise RuntimeError("DigaConv2d: Winograd statistics come with the forward output transform of 4x4 / 6x6 tiles")
        if infer and tile < 4:
            raise RuntimeError("DigaConv2d: the inference epilogue comes with Winograd tiles of 4x4 / 6x6 (winograd_max_tile = 2)")
        x6w = (not infer or fold_x6) and _wino_x6()    # (without config.fold_eval_bn_x6 the inference epilogue stays exact fp32)
        if keep and variant == "" and doff[0] > 0 and k % 256 == 0 and cin % 128 == 0 and config.active().winograd_keep_v:
            variant = "keep"
        arith = ("winograd/x6+bn" if x6w else "winograd+bn") if infer else "winograd/x6" if x6w else "winograd"
        return _Path("winograd", variant, 0, arith, tile, ratio, x6w)
    if _x6_taps() and _taps_ok(cin, r, s, copt):
        # what Winograd left of the multi-tap calls: bf16x6 with the tap walk in the loader waves (config.x6_taps)
        if infer and not fold_x6:
            raise RuntimeError("DigaConv2d: the multi-tap bf16x6 kernels' inference epilogue needs config.fold_eval_bn_x6 (check "
                               "infer_kernel / folds_eval_bn first)")
        if (tag == _TAG_FWD and stats is None and not epi and not infer and tuple(stride) == (1, 1)
                and _x6_window(hi, wi, cin, k, r, s, doff, opts[1] if copt else 0)):
            # a stride-1 plain forward the window rule admits: the tile's input window split into LDS once (config.x6_window)
            if copt and _x6_up2(hi, wi, cin, k, ho, wo, r, s, off0, doff, opts):
                # ... of a 2x upsampled input: the interior tiles on phase-collapsed weights, the border ring as "x6win" (config.x6_up2)
                return _Path("x6up2", variant, 2, "bf16x6/up2")
            return _Path("x6win", variant, 2, "bf16x6/window")
        return _Path("x6rs", variant, 2, "bf16x6/taps+bn" if infer else "bf16x6/taps")
    return _Path("f32", variant, 0, "f32+bn" if infer else "f32")


def _wgrad_plan(n, hi, wi, cp, kp, r, s, stride, padding, dilation, ho, wo, x_twin=False, stem=False):
    """_plan's sibling for the weight gradient of a layer with (padded) cp input and kp output channels.  x_twin: the forward left
    the split twin of its input and the layer may use it (bf16x3); stem: the im2col GEMM of _StemConvFn, which stays off bf16x6
    unless config.x6_taps is on.  A loader-form bf16x6 answer ("x6ls" / "x6rs") carries fit = _x6_fit(kp, cp), read now: nothing the
    forward saved depends on it."""
    stem_x6 = stem and _x6_taps()
    math = _layer_math(r, s, cp, not stem or stem_x6)
    if math == 2:
        if _x6_loader() or stem_x6:
            return _Path("x6ls", "", 2, "bf16x6/ls/fit", fit=True) if _x6_fit(kp, cp) else _Path("x6ls", "", 2, "bf16x6/ls")
        return _Path("x6", "", 2, "bf16x6")
    if math == 1 and x_twin:
        return _Path("twin", "", 1, "bf16x3", flops=False)
    if (math == 0 and kp % 256 == 0 and cp % 128 == 0
            and _winograd_ok(n, hi, wi, cp, kp, r, s, stride, (-padding[0], -padding[1]), dilation, ho, wo)):
        tile, ratio = _wino_plan(hi, wi, dilation[0])
        x6w = _wino_x6()                               # (read per call: a kept V is fp32 whichever arithmetic the forward ran)
        return _Path("winograd", "", 0, "winograd/x6" if x6w else "winograd", tile, ratio, x6w)
    if math == 0 and _x6_taps() and _taps_ok(cp, r, s, False):
        return _Path("x6rs", "", 2, "bf16x6/taps/fit", fit=True) if _x6_fit(kp, cp) else _Path("x6rs", "", 2, "bf16x6/taps")
    return _Path("f32", "", math, "bf16x3" if math == 1 else "f32", flops=not stem)


def _stats_plan(n, hi, wi, cin, k, r, s, stride, padding, dilation, ho, wo, opts=None, x6_ok=True):
    """(form, _Path): the statistics a forward with emit_bn_stats hands the BatchNorm behind it, from the kernel the call will run on --
    "chunks" of equal size, or (round 5) the "records" of unequal size that the Winograd output transform of 4x4 / 6x6 tiles leaves
    (diga_bn_fwd_records); None: F(2x2)-only runs and config.winograd_stats = False keep the BatchNorm's own statistics pass."""
    path = _plan(n, hi, wi, cin, k, r, s, stride, (-padding[0], -padding[1]), dilation, ho, wo, opts=opts, x6_ok=x6_ok)
    if path.family != "winograd":
        return "chunks", path
    return ("records" if config.active().winograd_stats and path.tile >= 4 and k % 4 == 0 else None), path


def winograd_stats_plan(n, hi, wi, cin_padded, k, r, s, stride, padding, dilation, ho, wo):
    """(floats, records) of the statistics buffer a forward DigaConv2d on the fp32 Winograd path with 4x4 / 6x6 tiles fills for the
    BatchNorm behind it (diga_conv2d_winograd_stats_floats / _records), or None when the layer is not on that path."""
    path = _plan(n, hi, wi, cin_padded, k, r, s, stride, (-padding[0], -padding[1]), tuple(dilation), ho, wo)
    if path.family != "winograd" or path.tile < 4 or k % 4 != 0:
        return None
    return (_lib.lib.diga_conv2d_winograd_stats_floats(n, hi, wi, k, dilation[0], path.tile),
            _lib.lib.diga_conv2d_winograd_stats_records(n, hi, wi, k, dilation[0], path.tile))


def infer_kernel(n, hi, wi, cin, k, r, s, stride, padding, dilation, ho, wo, pointwise_ok=True):
    """The forward kernel family with the inference epilogue (diga_infer_epilogue_t) a layer would run on under the active
    configuration -- "f32+bn" (direct / LDS-DMA / persistent GEMM) or "winograd+bn" (4x4 / 6x6 tiles); with config.fold_eval_bn_x6
    under conv_math 2 also "bf16x6+bn" / "bf16x6/ls+bn" (pointwise layers, by config.x6_split), "winograd/x6+bn" (config.x6_winograd)
    and "bf16x6/taps+bn" (config.x6_taps: the multi-tap calls off Winograd; the stem then answers "bf16x6/ls+bn")
    -- or None where there is none: conv_math 1; pointwise layers in mode 2 without fold_eval_bn_x6; Cout % 4 != 0; Winograd capped at
    2x2 tiles.  cin: the padded input channel count."""
    try:
        return _plan(n, hi, wi, cin, k, r, s, stride, (-padding[0], -padding[1]), tuple(dilation), ho, wo, infer=True,
                     x6_ok=pointwise_ok).arith
    except RuntimeError:                               # (the planner's refusal of an inference epilogue IS the answer)
        return None


def _infer_epilogue(infer, out):
    """(coefficients [2][K], residual NCHW-shaped or None, relu) -> (_lib.InferEpilogue, the tensors it points to)."""
    ab, residual, relu = infer
    e = _lib.InferEpilogue()
    e.ab = _lib.ptr(ab)
    rn = None
    e.residual, e.residual_ld = None, 0
    if residual is not None:
        rn = residual.detach().permute(0, 2, 3, 1)
        if tuple(rn.shape) != tuple(out.shape):
            raise RuntimeError(f"DigaConv2d: residual {tuple(rn.shape)} does not match the output {tuple(out.shape)}")
        if rn.dtype != torch.float32:
            rn = rn.float()
        ld = rn.stride(2)
        if not (rn.stride(3) == 1 and ld >= rn.shape[3] and ld % 4 == 0 and rn.stride(1) == rn.shape[2] * ld
                and rn.stride(0) == rn.shape[1] * rn.stride(1) and rn.data_ptr() % 16 == 0):
            rn = rn.contiguous()
            ld = rn.shape[3]
        e.residual, e.residual_ld = _lib.ptr(rn), ld
    e.relu = 1 if relu else 0
    return e, (ab, rn)


def _make_split(src, ld, rows, ch, triplet):
    """The pre-split copy of a [rows][ch] fp32 matrix with row pitch ld that the LDS-DMA kernels read: its split twin (bf16 hi / lo
    planes, 4 bytes per element) or, for bf16x6, its three-plane triplet (6 bytes)."""
    out = torch.empty(rows * ch * (6 if triplet else 4), dtype=torch.uint8, device=src.device)
    _lib.call("diga_make_triplet" if triplet else "diga_make_twin", _lib.ptr(src), ld, _lib.ptr(out), rows, ch, _lib.stream())
    return out


# (family, variant) -> entry point.  The implicit-GEMM families share one argument layout (_conv_launch) up to: the leading operand
# pointers (_operands), an input pitch (the two families that read fp32 activations through the ordinary loads), a bias slot (all
# but `_epi`) and the one trailing pointer (statistics, or the variant's struct).  The Winograd entry points have their own layout
# (_winograd_launch); with the products on bf16x6 one entry point serves every variant but "infer" and "opts", which have their own.
# ("x6rs", "opts") keeps the (null) statistics slot of its sibling in front of the options.
_ENTRY = {
    ("x6ls", ""): "diga_conv2d_nhwc_bf16x6_f32in", ("x6ls", "epi"): "diga_conv2d_nhwc_bf16x6_f32in_epi",
    ("x6ls", "infer"): "diga_infer_conv2d_nhwc_bf16x6_f32in",
    ("x6rs", ""): "diga_conv_taps_bf16x6_f32in", ("x6rs", "epi"): "diga_conv_taps_bf16x6_f32in_epi",
    ("x6rs", "infer"): "diga_infer_conv_taps_bf16x6_f32in", ("x6rs", "opts"): "diga_conv_taps_bf16x6_f32in_opts",
    ("x6win", ""): "diga_conv_window_bf16x6_f32in", ("x6win", "opts"): "diga_conv_window_bf16x6_f32in",
    ("x6up2", "opts"): "diga_conv_up2_bf16x6_f32in",
    ("x6", ""): "diga_conv2d_nhwc_bf16x6", ("x6", "epi"): "diga_conv2d_nhwc_bf16x6_epi", ("x6", "infer"): "diga_infer_conv2d_nhwc_bf16x6",
    ("twin", ""): "diga_conv2d_nhwc_twin", ("twin", "epi"): "diga_conv2d_nhwc_twin_epi", ("twin", "opts"): "diga_conv2d_nhwc_twin_opts",
    ("bf16x3", ""): "diga_conv2d_nhwc_bf16x3", ("bf16x3", "epi"): "diga_conv2d_nhwc_bf16x3_epi",
    ("bf16x3", "opts"): "diga_conv2d_nhwc_bf16x3_opts",
    ("f32", ""): "diga_conv2d_nhwc_f32", ("f32", "epi"): "diga_conv2d_nhwc_f32_epi", ("f32", "opts"): "diga_conv2d_nhwc_f32_opts",
    ("f32", "infer"): "diga_conv2d_nhwc_f32_infer",
    ("winograd", ""): "diga_conv2d_winograd_f32", ("winograd", "epi"): "diga_conv2d_winograd_f32_epi",
    ("winograd", "infer"): "diga_conv2d_winograd_f32_infer", ("winograd", "keep"): "diga_conv2d_winograd_f32_keep",
    ("winograd_reflect", "opts"): "diga_conv2d_winograd_f32_opts",
}
_WINOGRAD_X6 = "diga_conv2d_winograd_bf16x6"
_WINOGRAD_X6_INFER = "diga_infer_conv2d_winograd_bf16x6"
_WINOGRAD_X6_OPTS = "diga_conv_winograd_bf16x6_opts"         # ("winograd_reflect", "opts") with x6w: the fp32 `_opts` form's argument list


def _up2_phase_images(w_krsc, hi, wi, ho, wo, off0, opts):
    """The four phase images of "x6up2": the collapsed weights [phi_y][phi_x][K][R'][S'][C] (diga_collapse_up2_weights; R' x S' is the
    rule's answer) and diga_split_bf16x6_image of each, consecutive in one buffer."""
    k, r, s, cin = w_krsc.shape
    rc, sc = ctypes.c_int(0), ctypes.c_int(0)
    if _lib.lib.diga_conv_up2_bf16x6_plan(hi, wi, cin, k, ho, wo, r, s, off0[0], off0[1], 1, 1, int(opts[1]), int(opts[0]),
                                          ctypes.byref(rc), ctypes.byref(sc)) != 1:
        raise RuntimeError("DigaConv2d: diga_conv_up2_bf16x6_plan does not take a call planned as 'x6up2'")
    rs = rc.value * sc.value
    wc = torch.empty((4, k, rc.value, sc.value, cin), dtype=torch.float32, device=w_krsc.device)
    _lib.call("diga_collapse_up2_weights", _lib.ptr(w_krsc), _lib.ptr(wc), k, r, s, cin, off0[0], off0[1], _lib.stream())
    size = _lib.lib.diga_split_bf16x6_image_bytes(k, rs, cin)
    imgs = torch.empty(4 * size, dtype=torch.uint8, device=w_krsc.device)
    for ph in range(4):
        _lib.call("diga_split_bf16x6_image", _lib.ptr(wc[ph]), _lib.ptr(imgs[ph * size:]), k, rs, cin, _lib.stream())
    return wc, imgs


def _operands(path, x, w_krsc, twin_box, up2=None):
    """The operands of an implicit-GEMM call in the form its family reads -> (the leading arguments up to the weights, the tensors
    behind them, the twin / triplet of x to hand back).  The weight image / split lives until the launch returns.  up2: (ho, wo, off0,
    opts) of the call ("x6up2" alone reads them: its phase images depend on the first tap's offsets)."""
    n, hi, wi, cin = x.shape
    k, r, s, _ = w_krsc.shape
    if path.family in ("x6ls", "x6rs", "x6win", "x6up2"):
        # loader form: the activations are read as fp32 in place (contiguous or a channel slice) -- no triplet is built, returned or
        # looked for in the box
        split, ld = None, _nhwc_ld(x)
        if ld is None:
            x, ld = x.contiguous(), cin
        act = [_lib.ptr(x), ld]
    elif path.family in ("x6", "twin"):
        split = twin_box[0] if twin_box is not None else None
        if split is None:
            split = _make_split(x if x.is_contiguous() else x.contiguous(), cin, n * hi * wi, cin, path.family == "x6")
            if twin_box is not None:
                twin_box[0] = split
        act = [_lib.ptr(split)]
    if path.family in ("x6ls", "x6rs", "x6win", "x6up2", "x6", "twin"):
        size, fill = ((_lib.lib.diga_split_bf16_image_bytes, "diga_split_bf16_image") if path.family == "twin" else
                      (_lib.lib.diga_split_bf16x6_image_bytes, "diga_split_bf16x6_image"))
        img = torch.empty(size(k, r * s, cin), dtype=torch.uint8, device=x.device)
        _lib.call(fill, _lib.ptr(w_krsc), _lib.ptr(img), k, r * s, cin, _lib.stream())
        if path.family == "x6up2":                     # the full image for the ring of border tiles + one image per output phase
            wc, imgs = _up2_phase_images(w_krsc, hi, wi, *up2)
            return act + [_lib.ptr(img), _lib.ptr(imgs)], (x, split, img, wc, imgs), split
        return act + [_lib.ptr(img)], (x, split, img), split
    if path.family == "bf16x3":
        nel = w_krsc.numel()
        w_hi = torch.empty(nel, dtype=torch.int16, device=w_krsc.device)
        w_lo = torch.empty(nel, dtype=torch.int16, device=w_krsc.device)
        _lib.call("diga_split_bf16", _lib.ptr(w_krsc), _lib.ptr(w_hi), _lib.ptr(w_lo), nel, _lib.stream())
        return [_lib.ptr(x), _lib.ptr(w_hi), _lib.ptr(w_lo)], (w_hi, w_lo), None
    return [_lib.ptr(x), _lib.ptr(w_krsc)], (), None


def _winograd_launch(path, x, w_krsc, bias, out, d, flip, tag, stats, struct, keep_v):
    """The Winograd entry points: workspace, tile table and (variant "keep") the kept transform, then one call.  d: |dilation|;
    flip: 1 for backward-data; keep_v: a one-element list -- the transformed input stays alive for this layer's weight gradient."""
    n, hi, wi, cin = x.shape
    k, tile = out.shape[3], path.tile
    size = _lib.lib.diga_conv2d_winograd_bf16x6_workspace_bytes if path.x6w else _lib.lib.diga_conv2d_winograd_workspace_bytes
    ws = _lib.workspace(size(n, hi, wi, cin, k, d, tile), x.device, "winograd")
    tab = _tile_table(n, hi, wi, d, tile, x.device)
    variant, vk = path.variant, None
    if variant == "keep":
        vk = keep_v[0] = _alloc_keep_v(_lib.lib.diga_conv2d_winograd_v_floats(n, hi, wi, cin, d, tile), x.device)
        if vk is None:                                 # policy or memory said recompute
            variant = ""
    lead = [_lib.ptr(x), _lib.ptr(w_krsc)] + ([] if variant == "epi" and not path.x6w else [_lib.ptr(bias)]) + [_lib.ptr(out)]
    shape = (_lib.ptr(ws), ws.numel(), n, hi, wi, cin, x.stride(2), k, out.stride(2), d, tile)
    if path.x6w and variant in ("infer", "opts"):
        _lib.call(_WINOGRAD_X6_INFER if variant == "infer" else _WINOGRAD_X6_OPTS, *lead, *shape, struct, _lib.ptr(tab), tag, _lib.stream())
        return
    if path.x6w:
        # one entry point for the plain forward / backward-data, the forward with statistics, the forward that keeps V and
        # backward-data with the epilogue
        _lib.call(_WINOGRAD_X6, *lead, _lib.ptr(vk), *shape, flip, _lib.ptr(stats), struct, _lib.ptr(tab), tag, _lib.stream())
        return
    if variant == "keep":
        lead.append(_lib.ptr(vk))
    _lib.call(_ENTRY[(path.family, variant)], *lead, *shape, *((flip,) if variant in ("", "epi") else ()),
              struct if struct is not None else _lib.ptr(stats), _lib.ptr(tab), tag, _lib.stream())


def _conv_launch(x, w_krsc, bias, out, stride, off0, doff, tag, stats=None, twin_box=None, must_twin=False, epi=None,
                 opts=None, keep_v=None, x6_ok=True, infer=None, path=None):
    """x [N,Hi,Wi,Cin] (contiguous or a channel slice of a contiguous tensor), w_krsc [K,R,S,Cin],
    out [N,Ho,Wo,K] (same rule).  twin_box: a one-element list shared by the convs that read the very same x.
    (In bf16x6 mode the box holds the three-plane triplet of x instead.)  x6_ok=False keeps a pointwise call off bf16x6 (the stem).
    infer: (ab, residual, relu) -- forward only: the `_infer` entry points apply the eval-mode BatchNorm behind the conv (+ residual,
    + ReLU) in the epilogue (diga_infer_epilogue_t); a layer without such a kernel (infer_kernel is None) raises.
    epi: a _lib.BwdEpilogue (backward-data only, bias-free): the `_epi` entry points finish the gradient in the epilogue.
    opts: (reflect_pad, upsample_shift, activation) = a diga_conv_options_t handed to the `_opts` entry points -- x is then the SOURCE tensor of the
    (virtually) upsampled / mirrored input.  path: the call's _Path where the caller has planned it already (_Conv2dFn.forward: statistics
    records and keep_v come with it).
    Returns the twin / triplet of x the call read (built here or taken from the box), None on the other families."""
    n, hi, wi, cin = x.shape
    _, ho, wo, k = out.shape
    _, r, s, _ = w_krsc.shape
    if path is None:
        path = _plan(n, hi, wi, cin, k, r, s, stride, off0, doff, ho, wo, tag, None if stats is None else "chunks", epi is not None,
                     opts, infer is not None, twin_box is not None, must_twin, x6_ok)
    struct = inf_held = None
    if path.variant == "epi":
        struct = ctypes.byref(epi)
    elif path.variant == "opts":
        struct = ctypes.byref(_lib.ConvOptions(int(opts[0]), int(opts[1]), int(opts[2])))
    elif path.variant == "infer":
        inf, inf_held = _infer_epilogue(infer, out)
        struct = ctypes.byref(inf)
    direct = 2.0 * n * ho * wo * k * r * s * cin
    _log_path(tag, path.arith)
    if path.flops:
        _log_flops("conv_bwd_data" if tag == _TAG_BWD_DATA else "conv_fwd", direct, direct * path.ratio)
    if path.family in ("winograd", "winograd_reflect"):
        _winograd_launch(path, x, w_krsc, bias, out, abs(doff[0]), 1 if doff[0] < 0 else 0, tag, stats, struct, keep_v)
        return None
    lead, held, split = _operands(path, x, w_krsc, twin_box, (ho, wo, off0, opts))      # (`held`, `inf_held`: alive until the kernel is enqueued)
    if path.family == "x6up2":
        # stride 1, dilation 1 and the options (upsample_shift = 1) are the entry point's signature
        _lib.call(_ENTRY[(path.family, path.variant)], *lead, _lib.ptr(bias), _lib.ptr(out), n, hi, wi, cin, ho, wo, k, out.stride(2), r, s,
                  off0[0], off0[1], struct, tag, _lib.stream())
        return split
    if path.family == "x6win":
        # stride 1 is the entry point's signature; the options are nullable (variant "": a plain zero-padded convolution)
        _lib.call(_ENTRY[(path.family, path.variant)], *lead, _lib.ptr(bias), _lib.ptr(out), n, hi, wi, cin, ho, wo, k, out.stride(2), r, s,
                  off0[0], off0[1], doff[0], doff[1], struct, tag, _lib.stream())
        return split
    _lib.call(_ENTRY[(path.family, path.variant)], *lead, *(() if path.variant == "epi" else (_lib.ptr(bias),)), _lib.ptr(out),
              n, hi, wi, cin, *((x.stride(2),) if path.family in ("bf16x3", "f32") else ()), ho, wo, k, out.stride(2), r, s,
              stride[0], stride[1], off0[0], off0[1], doff[0], doff[1],
              *((_lib.ptr(stats),) if (path.family, path.variant) == ("x6rs", "opts") else ()),
              struct if struct is not None else _lib.ptr(stats), tag, _lib.stream())
    return split


# weight gradient: family -> (entry point, its workspace query); Winograd by the arithmetic of its products
_WGRAD = {
    "x6ls": ("diga_conv2d_wgrad_bf16x6_f32in", _lib.lib.diga_conv2d_wgrad_bf16x6_workspace_bytes),
    "x6rs": ("diga_conv_taps_wgrad_bf16x6_f32in", _lib.lib.diga_conv_taps_wgrad_bf16x6_workspace_bytes),
    "x6": ("diga_conv2d_wgrad_bf16x6", _lib.lib.diga_conv2d_wgrad_bf16x6_workspace_bytes),
    "twin": ("diga_conv2d_wgrad_twin", _lib.lib.diga_conv2d_wgrad_twin_workspace_bytes),
    "f32": ("diga_conv2d_wgrad_nhwc_f32", _lib.lib.diga_conv2d_wgrad_workspace_bytes),
}
_WGRAD_FIT = ("diga_wgrad_bf16x6_tiled_f32in", _lib.lib.diga_wgrad_bf16x6_tiled_workspace_bytes)      # _Path.fit ("x6ls" / "x6rs")
_WGRAD_WINOGRAD = {
    False: ("diga_conv2d_wgrad_winograd_f32", _lib.lib.diga_conv2d_wgrad_winograd_workspace_bytes),
    True: ("diga_conv2d_wgrad_winograd_bf16x6", _lib.lib.diga_conv2d_wgrad_winograd_bf16x6_workspace_bytes),
}


def _wgrad_launch(path, gy, x, dwp, r, s, stride, padding, dilation, splits=None, wino_v=None):
    """dwp [Kp,R,S,Cp] = the weight gradient of gy [N,Ho,Wo,Kp] and x [N,Hi,Wi,Cp] on the kernel `path` (_wgrad_plan) names.
    splits: (twin / triplet of gy, of x) for the families that read those; wino_v: the forward's kept Winograd transform of x."""
    n, hi, wi, cp = x.shape
    _, ho, wo, kp = gy.shape
    _log_path("wgrad", path.arith)
    if path.flops:
        direct = 2.0 * n * ho * wo * kp * r * s * cp
        _log_flops("conv_bwd_weight", direct, direct * path.ratio)
    if path.family == "winograd":
        name, size = _WGRAD_WINOGRAD[path.x6w]
        ws = _lib.workspace(size(n, hi, wi, cp, kp, dilation[0], path.tile, 1 if wino_v is not None else 0), x.device, "winograd_wgrad")
        tab = _tile_table(n, hi, wi, dilation[0], path.tile, x.device)
        _lib.call(name, _lib.ptr(gy), _lib.ptr(x), _lib.ptr(wino_v), _lib.ptr(dwp), _lib.ptr(ws), ws.numel(), n, hi, wi, cp, x.stride(2),
                  kp, gy.stride(2), dilation[0], path.tile, _lib.ptr(tab), _lib.stream())
        return
    name, size = _WGRAD_FIT if path.fit else _WGRAD[path.family]
    ws = _lib.workspace(size(n, ho, wo, kp, cp, r, s), x.device, "wgrad")
    f32 = path.family == "f32"                         # (reads pitched fp32 tensors and takes the layer's arithmetic)
    if path.family in ("x6ls", "x6rs"):                # fp32 dy and x as they are (a saved triplet of x, if any, is ignored)
        lead = (_lib.ptr(gy), gy.stride(2), _lib.ptr(x), x.stride(2))
    else:
        lead = (_lib.ptr(gy), _lib.ptr(x)) if f32 else (_lib.ptr(splits[0]), _lib.ptr(splits[1]))
    _lib.call(name, *lead, _lib.ptr(dwp), _lib.ptr(ws), ws.numel(), n, hi, wi, cp, *((x.stride(2),) if f32 else ()), ho, wo, kp,
              *((gy.stride(2),) if f32 else ()), r, s, stride[0], stride[1], -padding[0], -padding[1], dilation[0], dilation[1],
              *((path.math,) if f32 else ()), _lib.stream())


class _Call(NamedTuple):
    """What one call of the autograd functions below carries besides x, weight and bias."""
    stride: tuple = (1, 1)
    padding: tuple = (0, 0)
    dilation: tuple = (1, 1)
    stats: object = None       # the statistics buffer the kernel fills for the BatchNorm behind it; (buffer, "records"): Winograd records
    uses: object = None        # [weight-gradient calls of the current backward pass], or INLINE_WGRAD
    twin_box: object = None    # a one-element list shared by the convs that read the very same x
    x_is_twin: bool = False    # x holds split-twin bytes
    dy_is_twin: bool = False   # the output gradient will arrive as a split twin
    bn_box: object = None      # the BatchNorm that produced x (norm._BnFn): its gradient is finished in this conv's backward-data epilogue
    opts: object = None        # (reflect_pad, upsample_shift, activation)
    chain: object = None       # the convs on one tensor that chain their input gradients
    infer: object = None       # (ab, residual, relu): the inference epilogue


class _StemConvFn(torch.autograd.Function):
    """Few-channel conv (the 7x7/2 stem on the 3-channel image): im2col into rows of R*S*C (padded to 32)
    floats, then a 1x1 conv on the GEMM kernels.  No gradient wrt the input (it is the image)."""

    @staticmethod
    def forward(ctx, x, weight, bias, call):
        _lib.require_gpu(x, weight)
        stride, padding = call.stride, call.padding
        xc = x.detach().float().contiguous()                      # NCHW
        n, c, h, w_ = xc.shape
        k, _, r, s = weight.shape
        ho = (h + 2 * padding[0] - (r - 1) - 1) // stride[0] + 1
        wo = (w_ + 2 * padding[1] - (s - 1) - 1) // stride[1] + 1
        kk = r * s * c
        kp = _pad_to(kk)
        # student and teacher read the very same image batch (train_step.py: both get `cat`): the gathered rows depend on
        # the images and the geometry only, so the second stem to arrive reuses them (the entry rides on the input tensor
        # and dies with it; an event orders the two streams)
        key = (r, s, stride[0], padding[0], kp, x._version, x.data_ptr())
        hit = getattr(x, "_diga_xcol", None)
        cur = torch.cuda.current_stream(x.device)
        if hit is not None and hit[0] == key:
            xcol = hit[1]
            cur.wait_event(hit[2])
            xcol.record_stream(cur)
        else:
            xcol = torch.empty((n, ho, wo, kp), dtype=torch.float32, device=x.device)
            _lib.call("diga_im2col_nchw", _lib.ptr(xc), _lib.ptr(xcol), n, c, h, w_, r, s, stride[0], padding[0], ho, wo, kp,
                      _lib.stream())
            ev = torch.cuda.Event()
            ev.record(cur)
            x._diga_xcol = (key, xcol, ev)
        w2 = _pad_last(weight.detach().permute(0, 2, 3, 1).reshape(k, 1, 1, kk).contiguous(), kp)
        out = torch.empty((n, ho, wo, k), dtype=torch.float32, device=x.device)
        b = None if bias is None else bias.detach().float().contiguous()
        _conv_launch(xcol, w2, b, out, (1, 1), (0, 0), (1, 1), _TAG_FWD, call.stats, x6_ok=False, infer=call.infer)     # (bf16x6 mode: the stem stays exact fp32 unless config.x6_taps)
        ctx.save_for_backward(xcol)
        ctx.geom = (k, c, r, s, kk, kp, bias is not None, weight.stride())
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        (xcol,) = ctx.saved_tensors
        k, c, r, s, kk, kp, has_bias, w_strides = ctx.geom
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("the stem conv path does not produce a gradient wrt its (image) input")
        n, ho, wo, _ = xcol.shape
        gy = grad_out.permute(0, 2, 3, 1)
        if not gy.is_contiguous():
            gy = gy.contiguous()
        kq = _pad_to(k)
        gyp = _pad_last(gy, kq)
        dw = db = None
        if ctx.needs_input_grad[1]:
            dwp = torch.empty((kq, 1, 1, kp), dtype=torch.float32, device=xcol.device)
            path = _wgrad_plan(n, ho, wo, kp, kq, 1, 1, (1, 1), (0, 0), (1, 1), ho, wo, stem=True)
            _wgrad_launch(path, gyp, xcol, dwp, 1, 1, (1, 1), (0, 0), (1, 1))
            dw = torch.empty_strided((k, c, r, s), w_strides, dtype=torch.float32, device=xcol.device)
            dw.copy_(dwp[:k, 0, 0, :kk].reshape(k, r, s, c).permute(0, 3, 1, 2))
        if has_bias and ctx.needs_input_grad[2]:
            db = _bias_grad(gy)
        return None, dw, db, None


def _set_mask(epi, box, xn, cp):
    """ReLU mask of a BatchNorm with residual for the backward epilogue: its bit mask when the forward wrote one
    (norm._BnFn, `mask_bits`), else its output (= this conv's input xn)."""
    if not box["has_res"]:
        epi.mask_y, epi.mask_ld = None, 0
    elif box.get("mask_bits") is not None:
        epi.mask_y, epi.mask_ld = None, 0
        epi.mask_bits, epi.mask_bits_ld = _lib.ptr(box["mask_bits"]), cp // 8
    else:
        epi.mask_y, epi.mask_ld = _lib.ptr(xn), cp


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, call):
        # x: NCHW-shaped; weight: [K,C,R,S] (any dense layout); returns an NCHW-shaped channels_last tensor
        _lib.require_gpu(x, weight)
        stride, padding, dilation, stats, uses, twin_box, x_is_twin, dy_is_twin, bn_box, opts, chain, infer = call
        if x_is_twin:          # the producer wrote the split twin instead of fp32 (same bytes per element): hand it on
            xt = x.detach().permute(0, 2, 3, 1)
            if not (xt.is_contiguous() and xt.dtype == torch.float32):
                raise RuntimeError("DigaConv2d: a twin-only input must be a dense NHWC float32-shaped buffer")
            twin_box = [xt.reshape(-1).view(torch.uint8)]
        if opts is not None and any(opts) and (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)):
            raise RuntimeError("DigaConv2d: folded reflect padding / upsampling / tanh are inference-only (no backward)")
        xn = x.detach().permute(0, 2, 3, 1)
        n, hi, wi, _ = xn.shape
        k, c, r, s = weight.shape
        cp = _pad_to(c)
        up = int(opts[1]) if opts is not None else 0
        ho = ((hi << up) + 2 * padding[0] - dilation[0] * (r - 1) - 1) // stride[0] + 1
        wo = ((wi << up) + 2 * padding[1] - dilation[1] * (s - 1) - 1) // stride[1] + 1
        wino_stats = isinstance(stats, tuple)         # (buffer, "records"): the Winograd output transform fills it (DigaConv2d.forward)
        if wino_stats:
            stats = stats[0]
        # exact-fp32 Winograd layers whose weight gradient is wanted keep their transformed input (4x the input's bytes, HBM
        # is 288 GB): the backward-weight pass then skips a bandwidth pass of 5x the input (config.winograd_keep_v = False: recompute)
        path = _plan(n, hi, wi, cp, k, r, s, stride, (-padding[0], -padding[1]), dilation, ho, wo, _TAG_FWD,
                     None if stats is None else "records" if wino_stats else "chunks", opts=opts, infer=infer is not None,
                     shared=twin_box is not None, must_twin=bool(x_is_twin),
                     keep=ctx.needs_input_grad[1])
        # bf16x6 with the split in the loader waves reads a channel slice of a wider NHWC buffer in place (and saves that view for the
        # weight gradient); every other path gets a dense copy
        in_place = (cp == c and not x_is_twin and bn_box is None and chain is None and path.family == "x6ls"
                    and _nhwc_ld(xn) is not None)
        if not in_place and (not xn.is_contiguous() or xn.dtype != torch.float32):
            xn = xn.contiguous().float()
        xn = _pad_last(xn, cp)
        w = weight.detach().permute(0, 2, 3, 1)
        if not w.is_contiguous():
            w = w.contiguous()
        w = _pad_last(w, cp)
        out = torch.empty((n, ho, wo, k), dtype=torch.float32, device=x.device)
        b = None if bias is None else bias.detach().float().contiguous()
        keep_v = [None] if path.variant == "keep" else None
        x_twin = _conv_launch(xn, w, b, out, stride, (-padding[0], -padding[1]), dilation, _TAG_FWD, stats, twin_box, opts=opts,
                              keep_v=keep_v, infer=infer, path=path)
        ctx.wino_v = keep_v[0] if keep_v is not None else None
        ctx.max_tile = config.active().winograd_max_tile      # (the kept transform's layout is the forward's tile: checked in backward)
        ctx.save_for_backward(xn, w)
        # the split twin of the input serves the weight gradient too (multi-tap / shared-input layers, Cout >= 256)
        ctx.x_twin = x_twin if (path.math != 2 and ctx.needs_input_grad[1] and k >= 256 and k % 8 == 0 and cp == c) else None
        # bf16x6: the three-plane triplet of the (padded) input serves the weight gradient of every eligible layer
        ctx.x_trip = x_twin if (path.math == 2 and ctx.needs_input_grad[1]) else None
        ctx.dy_is_twin = bool(dy_is_twin)
        if dy_is_twin and ctx.x_twin is None and ctx.needs_input_grad[1]:
            raise RuntimeError("DigaConv2d: twin_grad=True on a layer whose weight gradient is not on the twin kernel")
        if x_is_twin and (x_twin is None or (ctx.needs_input_grad[1] and ctx.x_twin is None)):
            raise RuntimeError("DigaConv2d: got a twin-only input but this layer is not on the twin kernels "
                               "(check takes_twin_only_input before asking the producer for a twin)")
        ctx.geom = (stride, padding, dilation, c, bias is not None, weight.stride())
        ctx.uses = uses
        # data-parallel runs: the parameter offers its slice of the all-reduce bucket as the gradient's home (ddp.GradReducer.grad_view)
        ctx.grad_view = getattr(weight, "_diga_grad_view", None) if isinstance(weight, nn.Parameter) else None
        ctx.weight_param = weight if ctx.grad_view is not None else None
        # the arithmetic / twin decisions of this forward bind its backward: saved tensors may hold twin bytes
        ctx.math = _lib.get_conv_math()
        ctx.x_is_twin = bool(x_is_twin)
        # the BatchNorm that produced x lets this conv's backward-data epilogue finish its incoming gradient (norm._BnFn)
        ctx.bn_box = None
        if (bn_box is not None and ctx.needs_input_grad[0] and stride == (1, 1) and cp == c and c % 4 == 0
                and "claimed" not in bn_box and bn_box.get("rows") == n * hi * wi and bn_box.get("C") == c
                and (not bn_box["has_res"] or not x_is_twin)):
            bn_box["claimed"] = True
            bn_box["consumer_ready"] = True
            ctx.bn_box = bn_box
        # several convs on one tensor (the ASPP branches): their input gradients are summed by chaining the running sum
        # through the backward-data epilogues (`addend`) instead of autograd adds; the last one to run also finishes the
        # gradient of the BatchNorm that produced the tensor.  All members must be eligible, else the chain is off.
        ctx.chain = chain
        if chain is not None:
            if not (ctx.needs_input_grad[0] and stride == (1, 1) and cp == c and c % 4 == 0 and not x_is_twin):
                chain["disabled"] = True
            box = chain.get("box")
            if box is not None and ("claimed" in box or box.get("rows") != n * hi * wi or box.get("C") != c):
                chain["box"] = None
            elif box is not None:
                chain["box_ok"] = True
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        xn, w = ctx.saved_tensors
        stride, padding, dilation, c_true, has_bias, w_strides = ctx.geom
        x_trip = getattr(ctx, "x_trip", None)
        if (ctx.x_is_twin or ctx.dy_is_twin or ctx.x_twin is not None or x_trip is not None) and _lib.get_conv_math() != ctx.math:
            raise RuntimeError("DigaConv2d: the conv arithmetic (_lib.set_conv_math) changed between forward and backward of a graph that "
                               "holds split-twin tensors (their bytes are only readable by the twin kernels)")
        if ctx.x_is_twin and ctx.needs_input_grad[1] and ctx.x_twin is None:
            raise RuntimeError("DigaConv2d: twin-only input saved for backward but the weight gradient is off the twin kernel")
        n, hi, wi, cp = xn.shape
        k, r, s, _ = w.shape
        gy = grad_out.permute(0, 2, 3, 1)
        if not gy.is_contiguous():
            gy = gy.contiguous()
        _, ho, wo, _ = gy.shape
        kp = _pad_to(k)
        gyp = _pad_last(gy, kp)
        dx = dw = db = None
        st = _lib.stream()
        x_twin = getattr(ctx, "x_twin", None)
        use_tw = x_twin is not None and ctx.needs_input_grad[1] and _lib.get_conv_math() == 1 and kp == k
        dy_box = [None] if use_tw else None            # the twin of dy: built once, read by backward-data and -weight
        wpath = _wgrad_plan(n, hi, wi, cp, kp, r, s, stride, padding, dilation, ho, wo, x_twin=use_tw)
        # The two passes decide their arithmetic separately: a layer may have a Winograd backward-data (0) and a multi-tap bf16x6
        # weight gradient (2; config.x6_taps).  dm: what the backward-data call's planner (_plan, in _conv_launch) will be given --
        # 2 for the pointwise layers of bf16x6 mode, whose dy triplet (pass form) the two passes share.
        dm = _layer_math(r, s, kp)
        use_x6 = wpath.math == 2                       # the weight gradient runs on bf16x6 ...
        x6_ls = wpath.family in ("x6ls", "x6rs")       # ... with the operands split by the loader waves: no triplets (read per call)
        if use_x6 or dm == 2:
            dy_box = [None]                            # the triplet of dy, shared the same way (stays empty in the loader form)
        if ctx.dy_is_twin:          # the BatchNorm after this conv wrote its dx as a twin (same bytes per element)
            if not (kp == k and _lib.get_conv_math() == 1 and cp > 64 and (use_tw or not ctx.needs_input_grad[1])):
                raise RuntimeError("DigaConv2d: twin gradient on a layer that is not on the twin kernels")
            dy_box = [gyp.reshape(-1).view(torch.uint8)]
        if ctx.needs_input_grad[0]:
            # backward-data = stride-1 correlation of dy with the [C][R][S][K] transpose, tap offsets negated
            if kp == k:
                wt = torch.empty((cp, r, s, kp), dtype=torch.float32, device=w.device)
                _lib.call("diga_weight_transpose", _lib.ptr(w), _lib.ptr(wt), k, r * s, cp, st)
            else:                                   # 19-class head only: tiny, padded with torch ops
                wt = torch.zeros((cp, r, s, kp), dtype=torch.float32, device=w.device)
                wt[..., :k] = w.permute(3, 1, 2, 0)
            if stride == (1, 1):
                dxn = torch.empty((n, hi, wi, cp), dtype=torch.float32, device=w.device)
                epi, box = None, ctx.bn_box
                # rows per partial-sum record of the backward-data epilogue this call will run (the Winograd form writes one
                # record per tile group: any divisor of the row count the finaliser is told works, 128 as before)
                epi_chunk = _lib.lib.diga_conv2d_epi_chunk_rows(n, ho, wo, kp, hi, wi, cp, r, s, 1, 1, padding[0], padding[1],
                                                                  dm)
                chain = ctx.chain if (ctx.chain is not None and not ctx.chain.get("disabled")) else None
                last_of_chain = False
                if chain is not None:
                    # `remaining` counts the members whose backward has not run yet IN THIS backward pass.  The running sum
                    # only reaches autograd through the member that brings it to 0, so a pass in which a member never runs
                    # (its output unused / detached) or a second pass over a retained graph would hand the trunk a missing
                    # or stale sum: both are refused loudly instead.
                    if chain.get("done"):
                        raise RuntimeError("DigaConv2d: a second backward pass through convolutions that chain their input "
                                           "gradients (retain_graph) is not supported; run the forward again")
                    chain["remaining"] -= 1
                    if chain["remaining"] < 0:
                        raise RuntimeError("DigaConv2d: gradient chain ran more members than it has")
                    last_of_chain = chain["remaining"] == 0
                    if last_of_chain:
                        chain["done"] = True
                    prev = chain.get("acc")
                    cbox = chain.get("box") if (last_of_chain and chain.get("box_ok")) else None
                    if prev is not None or cbox is not None:
                        epi = _lib.BwdEpilogue()
                        epi.addend, epi.addend_ld = _lib.ptr(prev), cp
                        if cbox is not None:
                            m_rows = n * hi * wi
                            part = torch.empty(((m_rows + 63) // 64) * 2 * cp, dtype=torch.float32, device=w.device)      # (the size include/diga_hip.h asks for; the epilogue writes 128-row records into its first half)
                            _set_mask(epi, cbox, xn, cp)
                            epi.x, epi.x_ld = _lib.ptr(cbox["x"]), cp
                            epi.relu_ab = _lib.ptr(cbox["relu_ab"]) if not cbox["has_res"] else None
                            epi.mean, epi.invstd, epi.partials = _lib.ptr(cbox["mean"]), _lib.ptr(cbox["invstd"]), _lib.ptr(part)
                            cbox["claimed"] = True
                            cbox["premasked"] = (dxn.data_ptr(), part, dxn, prev, dxn._version, epi_chunk)
                    chain["acc"] = dxn
                elif box is not None:
                    # finish the gradient of the BatchNorm in front of this conv in the epilogue: + residual-branch
                    # gradient, ReLU mask, sum g / sum g*xhat per 128-row chunk (include/diga_hip.h, diga_bwd_epilogue_t)
                    m_rows = n * hi * wi
                    part = torch.empty(((m_rows + 63) // 64) * 2 * cp, dtype=torch.float32, device=w.device)      # (the size include/diga_hip.h asks for; the epilogue writes 128-row records into its first half)
                    # the residual-branch gradient of the tensor this conv reads, left by the BatchNorm that took it as
                    # residual -- whether or not the producing BN itself had a residual (the epilogue combines `addend`
                    # with either mask form)
                    add = box.pop("dres", None)
                    box["consumed"] = True          # a residual gradient arriving from now on must go through autograd
                    epi = _lib.BwdEpilogue()
                    epi.addend, epi.addend_ld = _lib.ptr(add), cp
                    _set_mask(epi, box, xn, cp)
                    epi.x, epi.x_ld = _lib.ptr(box["x"]), cp
                    epi.relu_ab = _lib.ptr(box["relu_ab"]) if not box["has_res"] else None
                    epi.mean, epi.invstd, epi.partials = _lib.ptr(box["mean"]), _lib.ptr(box["invstd"]), _lib.ptr(part)
                    box["premasked"] = (dxn.data_ptr(), part, dxn, add, dxn._version, epi_chunk)
                _conv_launch(gyp, wt, None, dxn, (1, 1), (padding[0], padding[1]), (-dilation[0], -dilation[1]),
                             _TAG_BWD_DATA, None, dy_box if (((use_tw or ctx.dy_is_twin) and cp > 64) or dm == 2) else None,
                             must_twin=ctx.dy_is_twin, epi=epi)
            elif _strided_dgrad_ok(r, s, stride, padding, dilation):
                # stride 2 with more than one tap: the four phases of dx in one launch, exact fp32 under every conv_math (no split
                # form of this kernel exists).  The forward claims a bn_box and keeps a chain enabled for stride 1 only, so neither
                # can be live here; a twin dy would be bytes this kernel cannot read.  All three are refused rather than ignored.
                if ctx.dy_is_twin or ctx.bn_box is not None or (ctx.chain is not None and not ctx.chain.get("disabled")):
                    raise RuntimeError("DigaConv2d: backward-data of a stride-2 multi-tap conv takes no twin gradient (twin_grad), no "
                                       "BatchNorm-backward epilogue (bn_box) and no gradient chain")
                dxn = torch.empty((n, hi, wi, cp), dtype=torch.float32, device=w.device)
                _lib.call("diga_dgrad_strided_f32", _lib.ptr(gyp), kp, _lib.ptr(wt), _lib.ptr(dxn), cp, n, hi, wi, cp, ho, wo, kp, r, s,
                          stride[0], stride[1], padding[0], padding[1], st)
                _log_path(_TAG_BWD_DATA, "f32/s2")
                direct = 2.0 * n * ho * wo * kp * r * s * cp
                _log_flops("conv_bwd_data", direct, direct)
            else:
                if (r, s) != (1, 1) or padding != (0, 0):
                    raise NotImplementedError("backward-data of strided convs is built for 1x1 without padding (any stride) and for stride "
                                              f"(2, 2), dilation (1, 1), padding < kernel; got kernel {(r, s)}, stride {tuple(stride)}, "
                                              f"padding {tuple(padding)}, dilation {tuple(dilation)}")
                dense = torch.empty((n, ho, wo, cp), dtype=torch.float32, device=w.device)
                _conv_launch(gyp, wt, None, dense, (1, 1), (0, 0), (1, 1), _TAG_BWD_DATA, twin_box=dy_box if dm == 2 else None)
                dxn = torch.zeros((n, hi, wi, cp), dtype=torch.float32, device=w.device)
                dxn[:, ::stride[0], ::stride[1]] = dense
            dx = dxn[..., :c_true].permute(0, 3, 1, 2)
            if ctx.chain is not None and not ctx.chain.get("disabled") and ctx.chain["remaining"] > 0:
                dx = None                           # the running sum travels on through the chain; the last member returns it
        if ctx.needs_input_grad[1]:
            # A weight that entered the graph more than once (the self-training step runs the student twice) gets its
            # contributions summed by autograd on the main stream: only the first one of a backward pass may still be
            # in flight on the side stream when it is handed over, the later ones run in line after a join.
            # A weight that is NOT a leaf (uses == INLINE_WGRAD: the folded matrices of the SegFormer head, whose gradient the next
            # autograd node reads at once) is computed in line on the main stream.
            later = False
            inline = isinstance(ctx.uses, str)
            if ctx.uses is not None and not inline:
                later = ctx.uses[0] > 0
                ctx.uses[0] += 1
            # data-parallel runs: the gradient is written straight into the parameter's slice of its all-reduce bucket
            # (ddp.GradReducer.grad_view: a fresh tensor of the weight's shape and strides over that slice) -- nothing packs it
            gv = getattr(ctx, "grad_view", None)
            dw = gv() if (gv is not None and not later and not inline and kp == k and cp == c_true) else None
            if dw is not None:
                # ... unless the slice already IS the parameter's gradient: a second graph differentiated before reduce() (the
                # overlapped self-training step's student(cross_mix), gradient accumulation under GradReducer.hold()) would overwrite
                # the first graph's result and AccumulateGrad would then add the slice to itself (this check replaced a
                # module-global switch the step driver had to flip around the second forward)
                held = ctx.weight_param.grad
                if held is not None and held.data_ptr() == dw.data_ptr():
                    dw = None
            if dw is None or tuple(dw.stride()) != tuple(w_strides) or dw.device != w.device:
                dw = torch.empty_strided((k, c_true, r, s), w_strides, dtype=torch.float32, device=w.device)
            # the kernels write [K][R][S][C]: for an unpadded channels_last weight that IS dw's memory (no copy afterwards)
            alias = kp == k and cp == c_true and dw.permute(0, 2, 3, 1).is_contiguous()
            dwp = dw.permute(0, 2, 3, 1) if alias else torch.empty((kp, r, s, cp), dtype=torch.float32, device=w.device)

            # the pre-split operands of the twin / triplet kernels: dy's is shared with backward-data, x's comes from the forward
            splits = None
            if use_tw or (use_x6 and not x6_ls):
                dy_split, x_split = dy_box[0], x_twin if use_tw else x_trip
                if dy_split is None:                # backward-data did not build it (no input gradient, strided, narrow)
                    dy_split = _make_split(gyp, kp, n * ho * wo, kp, use_x6)
                if x_split is None:                 # (bf16x6) the forward ran in another arithmetic and saved none
                    x_split = _make_split(xn, xn.stride(2), n * hi * wi, cp, True)      # (xn may be a channel slice saved by the loader form)
                splits = (dy_split, x_split)
            ctx.x_trip = None

            wino_v = getattr(ctx, "wino_v", None)
            ctx.wino_v = None
            if wino_v is not None and config.active().winograd_max_tile != ctx.max_tile:
                raise RuntimeError("DigaConv2d: the Winograd tile cap changed between this layer's forward and its backward "
                                   f"({ctx.max_tile} -> {config.active().winograd_max_tile}): the kept input transform has the forward's "
                                   "layout (set_conv_math(..., exact=) belongs between steps, not inside one)")

            def run():
                _wgrad_launch(wpath, gyp, xn, dwp, r, s, stride, padding, dilation, splits, wino_v)
                if not alias:
                    dw.copy_(dwp[:k, :, :, :c_true].permute(0, 3, 1, 2))

            # The weight gradient is a leaf of the backward graph: under the step driver it runs on a second stream
            # next to the backward-data / BatchNorm chain (the driver joins the streams before the optimizer step);
            # `later` / `inline` (above) keep the exceptions in line.
            if later:
                _lib.join_side()
            side = None if (later or inline) else _lib.side_stream(w.device)
            if side is None:
                run()
            else:
                side.wait_stream(torch.cuda.current_stream(w.device))
                with torch.cuda.stream(side):
                    run()
                dw.record_stream(side)          # (a returned gradient: never held, see _lib.release_to_side)
                _lib.release_to_side(side, (gyp, xn) + (() if alias else (dwp,)) + (splits or ()) + ((wino_v,) if wino_v is not None else ()))
        if has_bias and ctx.needs_input_grad[2]:
            db = _bias_grad(gy)
        return dx, dw, db, None


class DigaConv2d(nn.Conv2d):
    """nn.Conv2d whose compute is the HIP implicit-GEMM kernel; weights kept in channels_last memory."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.groups != 1 or self.padding_mode != "zeros":
            raise NotImplementedError("DigaConv2d: groups=1 and zero padding only")
        self.emit_bn_stats = False      # set by the model on convs that feed a train-mode BatchNorm
        self._bw_seen = [0]
        self.share_twin = False         # set by the model on convs that share their input with other convs (ASPP branches)
        self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)

    def _apply(self, fn, *a, **k):
        super()._apply(fn, *a, **k)
        if self.weight.dim() == 4 and not self.weight.data.is_contiguous(memory_format=torch.channels_last):
            self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)
        return self

    def _stem_path(self, x):
        """image-like input: the few channels of all taps are gathered into the K dimension (_StemConvFn)"""
        return (self.in_channels < 8 and not x.requires_grad and tuple(self.dilation) == (1, 1)
                and self.stride[0] == self.stride[1] and self.padding[0] == self.padding[1])

    def folds_eval_bn(self, x, bn, residual=None):
        """True when this conv on `x` may run as conv + eval-mode BatchNorm `bn` (+ residual, + ReLU) in ONE kernel
        (forward(..., infer=)): config.fold_eval_bn is on; nothing here is differentiated (grad mode off, or neither the input, the
        residual nor this conv's parameters require grad); `bn` is in eval mode with running statistics; the layer runs on a kernel
        that has the inference epilogue (infer_kernel: exact fp32, or bf16x6 with config.fold_eval_bn_x6); Cout % 4 == 0; and neither module carries forward or
        forward-pre hooks (a hook would see a tensor that no longer exists).  Bit-identical to the two-module form either way."""
        if not config.active().fold_eval_bn:
            return False
        if torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad) or self.weight.requires_grad
                                        or (self.bias is not None and self.bias.requires_grad)):
            return False
        if (not isinstance(bn, nn.BatchNorm2d) or bn.training or bn.running_mean is None or bn.running_var is None or not bn.affine
                or bn.num_features != self.out_channels or self.out_channels % 4 != 0):
            return False
        if self._forward_hooks or self._forward_pre_hooks or bn._forward_hooks or bn._forward_pre_hooks:
            return False
        if self.share_twin or getattr(x, "_diga_is_twin", False) or x.dim() != 4 or not x.is_cuda:
            return False
        n, _, h, w = x.shape
        r, s = self.kernel_size
        ho = (h + 2 * self.padding[0] - self.dilation[0] * (r - 1) - 1) // self.stride[0] + 1
        wo = (w + 2 * self.padding[1] - self.dilation[1] * (s - 1) - 1) // self.stride[1] + 1
        if self._stem_path(x):           # the im2col GEMM: a pointwise layer that stays exact fp32 in bf16x6 mode
            return infer_kernel(n, ho, wo, _pad_to(r * s * self.in_channels), self.out_channels, 1, 1, (1, 1), (0, 0), (1, 1), ho, wo,
                                pointwise_ok=False) is not None
        return infer_kernel(n, h, w, _pad_to(self.in_channels), self.out_channels, r, s, tuple(self.stride), tuple(self.padding),
                            tuple(self.dilation), ho, wo) is not None

    def forward(self, x, twin_grad=False, opts=None, chain=None, infer=None):
        """twin_grad: the gradient of this conv's output will arrive as a split twin (the BatchNorm that consumes the
        output was called with dx_twin=True).  opts = (reflect_pad, upsample_shift, activation): inference-only input
        map / output activation folded into the kernel (diga_conv_options_t, the `_opts` entry points).
        infer = (bn_module, residual_or_None, relu): returns relu(bn(conv(x)) + residual) of an eval-mode BatchNorm from one kernel
        (the `_infer` entry points; the caller has checked folds_eval_bn)."""
        fn = _Conv2dFn
        if self._stem_path(x):
            fn = _StemConvFn           # image-like input: gather the few channels of all taps into the K dimension
        stride, padding, dilation = tuple(self.stride), tuple(self.padding), tuple(self.dilation)
        stats = wino_records = None
        if infer is not None:
            from diga_amd.model.norm import eval_coefficients
            if twin_grad or chain is not None or (opts is not None and any(opts)) or getattr(x, "_diga_is_twin", False):
                raise RuntimeError("DigaConv2d: infer= is a plain forward (no twin gradient, chain, options or twin input)")
            bn, residual, relu = infer
            call = _Call(stride, padding, dilation, infer=(eval_coefficients(bn), residual, bool(relu)))
        else:
            if self.emit_bn_stats and self.training and self.out_channels % 4 == 0:
                n, _, h, w = x.shape
                r, s = self.kernel_size
                cp = _pad_to(self.in_channels)
                ho = (h + 2 * padding[0] - dilation[0] * (r - 1) - 1) // stride[0] + 1
                wo = (w + 2 * padding[1] - dilation[1] * (s - 1) - 1) // stride[1] + 1
                form, path = _stats_plan(n, h, w, cp, self.out_channels, r, s, stride, padding, dilation, ho, wo, opts, fn is _Conv2dFn)
                if form == "chunks":
                    stats = torch.empty(_lib.lib.diga_conv2d_stats_floats(n, ho, wo, self.out_channels), dtype=torch.float32,
                                        device=x.device)
                elif form == "records":
                    floats, wino_records = winograd_stats_plan(n, h, w, cp, self.out_channels, r, s, stride, padding, dilation, ho, wo)
                    stats = (torch.empty(floats, dtype=torch.float32, device=x.device), "records")
            uses = None
            if torch.is_grad_enabled() and self.weight.requires_grad:
                if self._bw_seen[0] > 0:          # a backward pass has consumed the previous graph(s)
                    self._bw_seen[0] = 0
                uses = self._bw_seen              # [weight-gradient calls of the current backward pass]
            twin_box = None
            if self.share_twin:                   # several convs read this very tensor: the first one builds its split twin
                twin_box = getattr(x, "_diga_twin_box", None)
                if twin_box is None:
                    twin_box = x._diga_twin_box = [None]
            x_is_twin = bool(getattr(x, "_diga_is_twin", False))
            if x_is_twin and fn is not _Conv2dFn:
                raise RuntimeError("DigaConv2d: twin-only input on the stem path")
            bn_box = getattr(x, "_diga_bn_box", None)
            if bn_box is not None and (self.share_twin or chain is not None or fn is not _Conv2dFn or not torch.is_grad_enabled()):
                bn_box = None                     # several convs read this tensor (the chain carries the box) / no backward
            if opts is not None and any(opts):
                if fn is not _Conv2dFn or stats is not None:
                    raise RuntimeError("DigaConv2d: folded padding / upsampling / activation need the implicit-GEMM path without BN statistics")
                call = _Call(stride, padding, dilation, None, uses, twin_box, opts=tuple(int(v) for v in opts))
            else:
                if (x_is_twin or twin_grad or bn_box is not None or chain is not None) and (fn is not _Conv2dFn or (self.bias is not None and twin_grad)):
                    if chain is None:
                        raise RuntimeError("DigaConv2d: twin gradient needs a bias-free conv on the implicit-GEMM path")
                    chain["disabled"] = True
                call = _Call(stride, padding, dilation, stats, uses, twin_box, x_is_twin, bool(twin_grad), bn_box, None, chain)
        with torch.set_grad_enabled(infer is None and torch.is_grad_enabled()):       # (infer=: nothing is differentiated)
            y = fn.apply(x, self.weight, self.bias, call)
        if wino_records is not None:
            y._diga_bn_partials = (stats[0], ("records", wino_records))
        elif stats is not None:
            chunk = _lib.lib.diga_conv2d_stats_chunk_rows(n, h, w, cp, ho, wo, self.out_channels, r, s, stride[0], stride[1],
                                                          -padding[0], -padding[1], path.math)
            y._diga_bn_partials = (stats, chunk)     # picked up by the DigaBatchNorm2d that consumes y
        return y
