"""Kernel choice, GroupNorm record counts and weight-gradient workspace sizes of the conv launch path, over the corpus of
tests/conv_selection_cases.py and under every knob variant it lists, against tests/golden/conv_selection.json -- recorded by the
library as it was BEFORE any of the launch path's host code was folded (the weight gradient's workspace layout and knob table).
No GPU: the library answers these from the host."""
import json

import pytest

from tests import conv_selection_cases as SC


@pytest.fixture(scope="module")
def golden():
    with open(SC.GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def summary():
    return SC.summary(SC.recorded())


@pytest.mark.parametrize("name,corpus", [(n, c) for n, _, c in SC.VARIANTS])
def test_selection_and_sizes_match_the_recorded_ones(golden, summary, name, corpus):
    want, got = golden["hashes"][corpus][name], summary["hashes"][corpus][name]
    assert sorted(got) == sorted(want)
    bad = [fam for fam in want if got[fam] != want[fam]]
    assert not bad, (f"{corpus} / {name}: families {bad} differ from the record; print the rows of both libraries with "
                     "`python -m tests.conv_selection_cases " + corpus + " --rows` under the variant's environment and diff them")


def test_the_corpus_is_the_recorded_one(golden, summary):
    assert summary["rows"] == golden["rows"]


def test_the_corpus_reaches_the_recorded_kernels(golden, summary):
    # (dtype, kernel) pairs the default variant selects: a plain five-family sweep reached 80, and families are only ever added
    assert len(golden["pairs"]) >= 80
    assert summary["pairs"] == golden["pairs"]
