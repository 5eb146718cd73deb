"""The convolution planner (diga_amd/model/conv.py: _plan and the helpers that read it) without a device: for every single-layer
scenario of conv_dispatch_scenarios the forward entry point it names equals the one recorded on the GPU
(tests/golden/conv_dispatch.json), and infer_kernel / winograd_stats_plan answer what the planner answers."""
import json
import os

import pytest

import conv_dispatch_scenarios as sc
from conftest import GOLDEN
from diga_amd import config
from diga_amd.model import conv as dc

SINGLE = list(sc.single_layer_ids())


def _geometry(layer):
    """(n, h, w, padded Cin, Cout, r, s, stride, padding, dilation, ho, wo) of the layer's forward as DigaConv2d sees it."""
    name, cin, cout, k, stride, pad, dil, _, _ = layer
    h, w = sc.STEM_HW if name.startswith("stem") else sc.HW
    ho, wo = ((v + 2 * pad - dil * (k - 1) - 1) // stride + 1 for v in (h, w))
    return sc.N, h, w, dc._pad_to(cin), cout, k, k, (stride, stride), (pad, pad), (dil, dil), ho, wo


def _forward_path(layer, stats):
    """The _Path of the layer's training forward, asked the way DigaConv2d.forward and the autograd functions ask."""
    n, h, w, cp, cout, r, s, stride, pad, dil, ho, wo = g = _geometry(layer)
    if layer[0].startswith("stem"):         # the im2col GEMM: a pointwise layer over R*S*C gathered channels that stays off bf16x6
        return dc._plan(n, ho, wo, dc._pad_to(r * s * layer[1]), cout, 1, 1, (1, 1), (0, 0), (1, 1), ho, wo, x6_ok=False)
    form = dc._stats_plan(*g)[0] if stats else None
    return dc._plan(n, h, w, cp, cout, r, s, stride, (-pad[0], -pad[1]), dil, ho, wo, stats=form, keep=True)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "conv_dispatch.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("sid,layer,stats,fields", SINGLE, ids=[s[0] for s in SINGLE])
def test_planner_names_the_forward_entry_point_the_gpu_launched(sid, layer, stats, fields, recorded):
    with config.override(**fields):
        path = _forward_path(layer, stats)
    entry = dc._WINOGRAD_X6 if path.x6w else dc._ENTRY[(path.family, path.variant)]
    assert entry == next(n for n in recorded[sid]["names"] if n.startswith("diga_conv2d_")), path
    assert ["fwd", path.arith, 1] in recorded[sid]["path_log"], path


def _gives(**features):
    """The planner's _Path for a call with these features, None where it refuses the combination."""
    try:
        return dc._plan(**features)
    except RuntimeError:
        return None


@pytest.mark.parametrize("sid,layer,stats,fields", [s for s in SINGLE if not s[2]], ids=[s[0] for s in SINGLE if not s[2]])
def test_infer_kernel_and_winograd_stats_plan_answer_from_the_planner(sid, layer, stats, fields):
    n, h, w, cp, cout, r, s, stride, pad, dil, ho, wo = g = _geometry(layer)
    call = dict(n=n, hi=h, wi=w, cin=cp, k=cout, r=r, s=s, stride=stride, off0=(-pad[0], -pad[1]), doff=dil, ho=ho, wo=wo)
    with config.override(**fields):
        inf = _gives(infer=True, **call)
        assert (dc.infer_kernel(*g) is not None) == (inf is not None and inf.variant == "infer")
        rec = _gives(stats="records", **call)
        assert (dc.winograd_stats_plan(*g) is not None) == (rec is not None and rec.family == "winograd")


def test_infer_kernel_known_answers():
    """(not through the planner: what the layers of the scenarios are known to run on)"""
    by_name = {layer[0]: _geometry(layer) for layer in sc.LAYERS}
    with config.override(conv_math=0):
        assert dc.infer_kernel(*by_name["pw_64_256"]) == "f32+bn"
        assert dc.infer_kernel(*by_name["c3_128_128_winograd"]) == "winograd+bn"
        assert dc.infer_kernel(*by_name["c3_128_256_d12_bias_direct"]) == "f32+bn"
        assert dc.infer_kernel(*by_name["pw_256_19_bias"]) is None                    # Cout % 4
        assert dc.winograd_stats_plan(*by_name["c3_128_128_winograd"]) is not None
        assert dc.winograd_stats_plan(*by_name["c3_64_64_direct"]) is None
    with config.override(conv_math=0, winograd_max_tile=2):
        assert dc.infer_kernel(*by_name["c3_128_128_winograd"]) is None
        assert dc.winograd_stats_plan(*by_name["c3_128_128_winograd"]) is None
    for math in (1, 2):
        with config.override(conv_math=math):
            assert dc.infer_kernel(*by_name["pw_64_256"]) is None
            assert dc.infer_kernel(*by_name["c3_128_128_winograd"]) == (None if math == 1 else "winograd+bn")


def test_the_plan_follows_a_patched_wino_plan(monkeypatch):
    """_wino_plan is looked up per call: the tile of the plan (forward and weight gradient) is the patched one, and nothing is kept."""
    layer = next(x for x in sc.LAYERS if x[0] == "c3_128_256_d2_keep_v")
    n, h, w, cp, cout, r, s, stride, pad, dil, ho, wo = _geometry(layer)
    with config.override(conv_math=0):
        before = _forward_path(layer, False)
        for tile in (4, 2):
            monkeypatch.setattr(dc, "_wino_plan", lambda hi, wi, d, tile=tile: (tile, 0.5))
            path = _forward_path(layer, False)
            assert (path.family, path.variant, path.tile, path.ratio) == ("winograd", "keep", tile, 0.5)
            assert dc._wgrad_plan(n, h, w, cp, cout, r, s, stride, pad, dil, ho, wo).tile == tile
        monkeypatch.undo()
        assert _forward_path(layer, False) == before
