"""Which kernels the convolutions launch: every scenario of conv_dispatch_scenarios (each kernel path of diga_amd/model/conv.py at its
smallest shape, under every configuration that switches paths) must launch the recorded sequence of entry points and count the
recorded `path_log` (tests/golden/conv_dispatch.json: names only, no sizes).  A change of dispatch is then a change of the fixture
that a review sees, never a side effect."""
import json
import os

import pytest

import conv_dispatch_scenarios as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def test_every_scenario_launches_the_recorded_entry_points():
    with open(os.path.join(GOLDEN, "conv_dispatch.json")) as f:
        want = json.load(f)
    todo = list(sc.scenarios())
    assert sorted(sid for sid, _, _ in todo) == sorted(want)
    bad = []
    for sid, fields, run in todo:
        names, paths, _ = sc.record(run, fields)
        if names != want[sid]["names"] or paths != want[sid]["path_log"]:
            bad.append(f"{sid}:\n  launched {names}\n  recorded {want[sid]['names']}\n  path_log {paths}\n  recorded {want[sid]['path_log']}")
    assert not bad, "\n".join(bad)


def test_the_scenarios_reach_every_convolution_entry_point():
    """Every diga_conv2d_* kernel entry point the binding declares is launched by some scenario (the size queries apart, and the
    tile table, which the fixture leaves out)."""
    from diga_amd import _lib
    with open(os.path.join(GOLDEN, "conv_dispatch.json")) as f:
        seen = {name for v in json.load(f).values() for name in v["names"]}
    declared = {n for n, (res, _) in _lib.SIGNATURES.items() if n.startswith("diga_conv2d_") and res is _lib.INT and sc.is_conv_call(n)}
    assert declared - {"diga_conv2d_stats_chunk_rows", "diga_conv2d_epi_chunk_rows"} <= seen            # (those two are row-count queries)
