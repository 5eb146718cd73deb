"""The host checks of the convolution entry points (csrc/conv.hip, conv_bf16x6.h, winograd.hip) answer as recorded: for every rejected call
of tests/conv_entry_check_cases.py the return code and the message of tests/golden/conv_entry_checks.json -- which rule answers, in which
words, and, in the cases with two faults, which rule answers first -- and for every size / row query the recorded value.

The fixture was recorded from the library of the commit before the launch layer moved onto call records (ConvCall, csrc/conv_call.h); the
tiled weight gradient (diga_wgrad_bf16x6_tile, diga_wgrad_bf16x6_tiled_f32in and its workspace query) joined it from the last commit with
a launcher of its own, before the bf16x6 weight gradients shared one -- a 256 x 128 shape answers there in the wide entry points' words; the
multi-tap forward with options, the window and collapsed-upsampling forwards, their two plan functions (recorded as queries: the value
returned and the integers written) and diga_collapse_up2_weights joined from the last commit before the two window forms shared their checks.  Every
recorded call was rejected by an argument check, so none can reach a launch; the subject is host code, and where a device is visible
the test skips itself rather than hand fake addresses to a library that could launch on them."""
import pytest
import torch

import conv_entry_check_cases as cc

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host checks only: run where no device is visible")


@pytest.fixture(scope="module")
def recorded():
    return cc.load_fixture()


def test_every_entry_point_and_query_in_scope_is_covered(recorded):
    from diga_amd import _lib
    assert _lib.PROF_TAGS.index("conv_bwd_data") == cc.BWD_DATA
    entries = {n for n, (res, _) in _lib.SIGNATURES.items() if cc.in_scope(n, res is _lib.INT) and not cc.is_query(n)}
    queries = {n for n, (res, _) in _lib.SIGNATURES.items() if cc.in_scope(n, res is _lib.INT) and cc.is_query(n)}
    # in_scope goes by the name alone, so an entry point that joins the library under one of the families' names is missed by no one
    assert {"diga_conv_window_bf16x6_f32in", "diga_conv_up2_bf16x6_f32in", "diga_collapse_up2_weights"} <= entries
    assert set(cc.PLANS) <= queries
    assert entries == set(cc.SPECS), entries ^ set(cc.SPECS)
    assert queries == {name for _, name, _ in cc.queries()}, queries ^ {name for _, name, _ in cc.queries()}
    for name in cc.SPECS:
        assert len(cc.params(name)) == len(_lib.SIGNATURES[name][1]), name
    # the fixture holds exactly the generated cases, every one of them a rejection; the calls that break no rule are listed, not run
    ids = [cid for cid, _, _ in cc.cases()]
    assert len(ids) == len(set(ids)) and set(ids) == set(recorded["calls"])
    assert all(rc in cc.REJECTED for rc, _ in recorded["calls"].values())
    assert not set(recorded["valid_calls"]) & set(recorded["calls"])
    assert {cid.split("::")[0] for cid in ids} == set(cc.SPECS)
    assert {qid for qid, _, _ in cc.queries()} == set(recorded["queries"])


@pytest.mark.parametrize("name", sorted(cc.SPECS))
def test_rejected_calls_answer_as_recorded(name, recorded):
    from diga_amd import _lib
    wrong = []
    for cid, entry, vals in cc.cases():
        if entry != name:
            continue
        got = list(cc.call(_lib, entry, vals))
        if got != recorded["calls"][cid]:
            wrong.append((cid, got, recorded["calls"][cid]))
    assert not wrong, wrong[:5]


def test_queries_answer_as_recorded(recorded):
    from diga_amd import _lib
    wrong = [(qid, got, recorded["queries"][qid]) for qid, name, args in cc.queries()
             for got in [cc.query(_lib, name, args)] if got != recorded["queries"][qid]]
    assert not wrong, wrong[:5]
