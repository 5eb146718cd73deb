"""The convolution-dispatch scenarios: the smallest shapes at which every kernel path of diga_amd/model/conv.py is still taken, each
under every configuration that switches paths.  tests/test_gpu_conv_dispatch.py runs them on the GPU against the recorded launch
sequences (tests/golden/conv_dispatch.json), tests/test_conv_plan_cpu.py asks the planner about the single layers without a device.
Only the public surface is used (DigaConv2d and the models), so the same file records the fixture from any revision."""
import torch

N, HW, STEM_HW = 2, (12, 10), (33, 31)

# name, Cin, Cout, kernel, stride, padding, dilation, bias, with a second run that emits BatchNorm statistics
LAYERS = [
    ("pw_64_256", 64, 256, 1, 1, 0, 1, False, True),
    ("pw_256_64", 256, 64, 1, 1, 0, 1, False, True),
    ("pw_96_320_ragged", 96, 320, 1, 1, 0, 1, False, True),
    ("pw_256_128_stride2", 256, 128, 1, 2, 0, 1, False, True),
    ("pw_256_19_bias", 256, 19, 1, 1, 0, 1, True, False),             # (Cout % 4 != 0: no statistics form)
    ("c3_64_64_direct", 64, 64, 3, 1, 1, 1, False, False),
    ("c3_128_128_winograd", 128, 128, 3, 1, 1, 1, False, True),
    ("c3_128_256_d2_keep_v", 128, 256, 3, 1, 2, 2, False, True),
    ("c3_128_256_d12_bias_direct", 128, 256, 3, 1, 12, 12, True, False),
    ("stem_7x7", 3, 64, 7, 2, 3, 1, False, False),
]

# name, configuration fields
CONFIGS = [
    ("f32", dict(conv_math=0)),
    ("f32_tile2", dict(conv_math=0, winograd_max_tile=2)),
    ("f32_no_winograd", dict(conv_math=0, winograd=False)),
    ("f32_no_keep_v", dict(conv_math=0, winograd_keep_v=False)),
    ("bf16x3_twin0", dict(conv_math=1, conv_twin="0")),
    ("bf16x3", dict(conv_math=1)),
    ("bf16x3_twin1", dict(conv_math=1, conv_twin="1")),
    ("bf16x6_pass", dict(conv_math=2, x6_split="pass")),
    ("bf16x6_loader", dict(conv_math=2, x6_split="loader")),
    ("bf16x6_pass_wino", dict(conv_math=2, x6_split="pass", x6_winograd=True)),
    ("bf16x6_loader_wino", dict(conv_math=2, x6_split="loader", x6_winograd=True)),
]
MATHS = [c for c in CONFIGS if c[0] in ("f32", "bf16x3", "bf16x6_pass")]

# what conv.py itself launches: the rest of a model's calls (BatchNorm, pooling, losses) is not this fixture's business, and the
# Winograd tile table appears only on the first call of a process on a geometry
_HELPERS = {"diga_make_twin", "diga_make_triplet", "diga_split_bf16", "diga_split_bf16_image", "diga_split_bf16x6_image",
            "diga_weight_transpose", "diga_im2col_nchw"}


def is_conv_call(name):
    return (name.startswith("diga_conv2d_") or name in _HELPERS) and name != "diga_conv2d_winograd_tile_table"


def single_layer_ids():
    """(scenario id, layer, emit_bn_stats, configuration fields) of every single-layer scenario."""
    for cname, fields in CONFIGS:
        for layer in LAYERS:
            for stats in ((False, True) if layer[8] else (False,)):
                yield f"{layer[0]}{'+stats' if stats else ''}@{cname}", layer, stats, fields


_modules = {}


def _cached(key, make):
    if key not in _modules:
        torch.manual_seed(len(_modules))
        _modules[key] = make().cuda()
    for p in _modules[key].parameters():
        p.grad = None
    return _modules[key]


def _finish():
    from diga_amd import _lib
    _lib.join_side()
    torch.cuda.synchronize()


def _image(c, hw, grad=True, n=N):
    return torch.randn((n, c) + tuple(hw), device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(grad)


def run_layer(layer, stats):
    from diga_amd.model.conv import DigaConv2d
    name, cin, cout, k, stride, pad, dil, bias, _ = layer
    conv = _cached(name, lambda: DigaConv2d(cin, cout, k, stride=stride, padding=pad, dilation=dil, bias=bias)).train()
    conv.emit_bn_stats = stats
    stem = name.startswith("stem")
    y = conv(_image(cin, STEM_HW if stem else HW, grad=not stem))
    y.backward(torch.ones_like(y))
    _finish()


def run_bottleneck():
    """ResNet-101 widths (layer3 geometry): the BN-box epilogue, the chain, the twin-only input."""
    from diga_amd.model import seg_model_noaux as sm
    blk = _cached("bottleneck", lambda: sm.Bottleneck(1024, 256, 1, dilation=2)).train()
    y = blk(_image(1024, HW, n=1))
    y.backward(torch.ones_like(y))
    _finish()


def _tiny():
    from diga_amd.model import seg_model_noaux as sm
    from diga_amd.model.model_noaux import SegModel
    return _cached("tiny", lambda: SegModel(arch=sm.TINY))


def run_tiny_train():
    """The shared ASPP input."""
    outs = _tiny().train()(_image(3, (96, 128), grad=False))
    (outs[2].sum() + outs[3].sum()).backward()
    _finish()


def run_tiny_eval():
    with torch.no_grad():
        _tiny().eval()(_image(3, (96, 128), grad=False))
    _finish()


def run_translator():
    """The `_opts` forms: reflect, upsample, tanh."""
    from diga_amd.model.model_noaux import ImgDecoder, ImgEncoder
    enc, dec = _cached("enc", ImgEncoder).eval(), _cached("dec", ImgDecoder).eval()
    with torch.no_grad():
        dec(enc(_image(3, (32, 24), grad=False, n=1)))
    _finish()


def run_segformer_pointwise():
    """The functional INLINE_WGRAD convolution of the SegFormer head: a weight that is not a leaf."""
    from diga_amd.model.networks import segformer_head as sh
    a = torch.randn((96, 32), device="cuda", requires_grad=True)
    b = torch.randn((32, 64), device="cuda", requires_grad=True)
    bias = torch.randn(96, device="cuda", requires_grad=True)
    y = sh._pointwise(_image(64, (6, 5)), a @ b, bias)
    y.backward(torch.ones_like(y))
    _finish()


def scenarios():
    """(scenario id, configuration fields, callable) of every scenario, single layers first."""
    for sid, layer, stats, fields in single_layer_ids():
        yield sid, fields, (lambda layer=layer, stats=stats: run_layer(layer, stats))
    for cname, fields in MATHS:
        yield f"bottleneck@{cname}", fields, run_bottleneck
        yield f"tiny_train@{cname}", fields, run_tiny_train
    yield "bottleneck@bf16x6_loader", dict(conv_math=2, x6_split="loader"), run_bottleneck      # (the loader form's `_epi` entry point)
    for fold in (True, False):
        yield f"tiny_eval@fold_{'on' if fold else 'off'}", dict(conv_math=0, fold_eval_bn=fold), run_tiny_eval
    for cname, fields in MATHS[:2]:
        yield f"translator@{cname}", fields, run_translator
    yield "segformer_pointwise@f32", dict(conv_math=0), run_segformer_pointwise


def record(run, fields, on_call=None):
    """Run one scenario under its configuration -> (the conv entry points it launched, in order; its path_log as sorted
    [pass, arithmetic, launches] rows; its flop_log).  on_call(name, args) sees every library call."""
    from diga_amd import _lib, config
    from diga_amd.model import conv as dc
    names, real = [], _lib.call

    def tracing(name, *args):
        if is_conv_call(name):
            names.append(name)
        if on_call is not None:
            on_call(name, args)
        return real(name, *args)

    with config.override(**fields):
        _lib.call, dc.path_log, dc.flop_log = tracing, {}, {}
        try:
            run()
            paths, flops = dc.path_log, dc.flop_log
        finally:
            _lib.call, dc.path_log, dc.flop_log = real, None, None
    return names, sorted([p, a, c] for (p, a), c in paths.items()), flops
