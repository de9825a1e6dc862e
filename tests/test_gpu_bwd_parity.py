"""The backward passes that are not convolutions keep their BITS (csrc/bwd_kernels.hip: one GroupNorm-backward element, one
per-channel fold, one finish kernel): every output of every non-raising case of the edge tables, in each of its dtypes, has the
sha256 that tests/golden/bwd_pass_digests.json recorded with the library as it stood before the passes were gathered into one file
(tests/bwd_parity.py lists the cases and the two it adds).  The fp64 bounds of tests/test_gpu_pass_edges.py,
tests/test_gpu_wgrad_edges.py and tests/test_gpu_boundary_edges.py leave room for another FMA contraction or another order of
summation; this does not.  A case that differs means the arithmetic moved: find the expression, do not re-record."""
import json
import os

import pytest

import bwd_parity as P

pytestmark = pytest.mark.gpu

CASES = P.keys()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "bwd_pass_digests.json")) as f:
        return json.load(f)


def test_the_inputs_are_the_recorded_ones(golden):
    """asserted first: digests of other inputs say nothing about the passes"""
    assert P.input_digests() == golden["inputs"], (
        "the inputs of the edge tables (tests/pass_ref.py, tests/wgrad_ref.py, tests/boundary_ref.py) are no longer the ones the "
        "digests were recorded on: re-record tests/golden/bwd_pass_digests.json with the library of the commit BEFORE the change "
        "under test")


@pytest.fixture(scope="module")
def got():
    return P.pass_digests()


def test_the_cases_are_the_recorded_ones(golden, got):
    # 60 + 2 GroupNorm backward, 54 row softmax, 24 temporal attention, 76 channel sums, 22 folds, 25 2x2 sums, 2 LayerNorm
    assert set(got) == set(golden["passes"]) == set(CASES) and len(CASES) == len(set(CASES)) == 265


@pytest.mark.parametrize("case", CASES)
def test_pass_writes_the_recorded_bits(golden, got, case):
    assert got[case] == golden["passes"][case], case
