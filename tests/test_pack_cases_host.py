"""CPU checks of the packed-weight byte pin's inputs (tests/pack_cases.py): the generator is deterministic (every input has the
sha256 the fixture recorded on the MI355X), every planted value is in every weight, and the fixture has exactly the cases."""
import json
import os

import pytest
import torch

from tests import pack_cases as PC

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_weight_hashes.json")


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_has_exactly_the_cases(fixture):
    assert sorted(fixture["cases"]) == sorted(PC.case_ids())
    assert len(set(PC.case_ids())) == len(PC.case_ids())
    assert len(fixture["recorded_from"]) >= 7      # the commit the recording library was built from
    for e in fixture["cases"].values():
        assert sorted(e) == ["bias_sha256", "fields", "input_sha256", "w_sha256"] and sorted(e["fields"]) == sorted(PC.FIELDS)


@pytest.mark.parametrize("case,form", PC.params(), ids=PC.case_ids())
def test_input_is_deterministic(case, form, fixture):
    w = PC.make_weight(case, form)
    assert w.device.type == "cpu" and w.dtype == PC.torch_dtype(form) and tuple(w.shape) == case.shape
    assert PC.sha(w) == PC.sha(PC.make_weight(case, form)) == fixture["cases"][f"{case.name}-{form}"]["input_sha256"]


@pytest.mark.parametrize("case,form", PC.params(), ids=PC.case_ids())
def test_planted_values(case, form):
    w = PC.make_weight(case, form)
    v = (w if case.packer != "pack_weight_batched" else w.movedim(0, -1)).float()      # [co, ci, ...]
    neg0 = v[0, 1].reshape(-1)
    assert bool((neg0 == 0).all()) and bool(torch.signbit(neg0).all())                 # -0.0, every tap
    assert bool((v[1] == 0).all()) and not bool(torch.signbit(v[1]).any())             # the all-zero row, +0.0
    if v.shape[1] >= 16:                                                               # the e3m2 spread inside one 16-channel group
        grp = v[2, :16].reshape(16, -1).abs()
        assert bool((grp[5] == 0.75).all())
        assert float(grp[[1, 3, 7, 9, 11, 13, 15]].max()) <= 2.0 ** -10 and 0 < float(grp[0::2].max()) <= 2.0 ** -6
    if PC.has_ties(case):
        u = PC.tie_ulp(form)
        rt = torch.tensor([1.0, u / 2, u / 1024])
        assert torch.equal(v[0, 0], rt.reshape(3, 1, 1).expand(3, 3, 3)) and torch.equal(v[0, 2], rt.reshape(1, 1, 3).expand(3, 3, 3))
        t = PC.torch_dtype(form) if form in PC.HALF else torch.float16                # the type the fold sum is rounded to
        one, up = torch.tensor(1.0), torch.tensor(1.0 + u)
        assert (one + u / 2).to(t).float() == one                                      # two taps: a tie, to even
        assert ((one + u / 2) + u / 1024).to(t).float() == up                          # three, summed in fp32, rounded once
        assert ((one + u / 2).to(t).float() + u / 1024).to(t).float() == one           # ... and not when rounded tap by tap


def test_odd_tap_runs_are_packed_in_the_fast_forms():
    """runs of 9 taps (kH * kW = 9) end on a tap without a partner; the fast-fp32 forms must meet one, alone and after other runs"""
    runs = {dict(c.kw)["k"] for c in PC.CASES if c.packer == "pack_weight" and "f32q" in c.forms and "f32q6" in c.forms}
    assert {(1, 3, 3), (3, 3, 3)} <= runs
