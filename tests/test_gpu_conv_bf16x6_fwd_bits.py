"""The bits of the bf16x6 forward kernels (csrc/conv_bf16x6.h) against a recording: for each case of tests/x6_fwd_bits_cases.py the
SHA-256 of every buffer the call writes (out, statistics partials, the epilogue's records; the triplet and the weight images of the
elementwise kernels) equals the one in tests/golden/x6_fwd_bits.json, which was recorded on an MI355X from the library of the commit the
fixture names -- the last one in which the forward, window and weight-gradient kernels each spelled out the six-product chain and
the split-and-pack of eight channels themselves.  The comparisons of the other bf16x6 tests (one form against another, every form
against float64) have the same source on both sides; this one does not."""
import pytest

import x6_fwd_bits_cases as bc

CASES = bc.cases()


@pytest.fixture(scope="module")
def recorded():
    return bc.load_fixture()


def test_fixture_holds_exactly_the_cases_and_they_reach_every_instantiation(recorded):
    """(needs the library, no device)"""
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)) and recorded["recorded_from"] and set(recorded["sha256"]) == set(ids)
    # the launchers' selection rule over the cases: kX6 [form][tn][variant] (18), kX6Opt [tn] (2), the weight-batch form, the four forms
    # of conv_win_x6_kernel and the three elementwise kernels
    reached = set().union(*(bc.kernels(c) for c in CASES))
    assert reached == bc.ALL_KERNELS, reached ^ bc.ALL_KERNELS
    assert len(bc.ALL_KERNELS) == 18 + 2 + 1 + 4 + 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bits_equal_the_recording(case, recorded):
    import torch
    got = bc.run(case)
    want = recorded["sha256"][case[0]]
    assert set(got) == set(want)
    for name, t in got.items():
        if name == "out":
            assert not torch.isnan(t).any(), f"{case[0]}: output elements left unwritten"
        assert bc.sha256(t) == want[name], f"{case[0]}: {name} differs from the bits recorded from {recorded['recorded_from']}"
