"""The passes of the training loss keep their BITS (csrc/loss_kernels.hip: one group walk, one reduce pair over operand sources):
every output of every case of tests/loss_parity.py has the sha256 that tests/golden/loss_pass_digests.json recorded with the library
as it stood before the six kernel templates were folded into four.  The fp64 bands of tests/test_gpu_loss.py and
tests/test_gpu_loss_domain_frame_maps.py leave room for another FMA contraction or another order of summation; this does not.
A case that differs means the arithmetic moved: find the expression, do not re-record."""
import json
import os

import pytest

import loss_parity as P

pytestmark = pytest.mark.gpu

CASES = P.keys()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "loss_pass_digests.json")) as f:
        return json.load(f)


def test_the_inputs_are_the_recorded_ones(golden):
    """asserted first: digests of other inputs say nothing about the passes"""
    assert P.input_digests() == golden["inputs"], (
        "the inputs of tests/loss_parity.py are no longer the ones the digests were recorded on: re-record "
        "tests/golden/loss_pass_digests.json with the library of the commit BEFORE the change under test")


@pytest.fixture(scope="module")
def got():
    return P.pass_digests()


def test_the_cases_are_the_recorded_ones(golden, got):
    # reduce_sum: 24 op x dtype, 18 dtype pairs, 14 element counts, 7 views, 1 grid stride; 54 frame maps; 12 Gaussian posteriors
    assert set(got) == set(golden["passes"]) == set(CASES) and len(CASES) == len(set(CASES)) == 130


@pytest.mark.parametrize("case", CASES)
def test_pass_writes_the_recorded_bits(golden, got, case):
    assert got[case] == golden["passes"][case], case
