"""The multi-tensor update passes keep their BITS (csrc/optim_kernels.hip: one chunk walk, one AdamW template): every buffer a pass may
write, on the edge lists of tests/optim_ref.py and tests/master_ref.py, has the sha256 that tests/golden/update_pass_digests.json
recorded with the library as it stood before the passes were folded together (tests/update_parity.py lists the cases).  The fp64
bounds of tests/test_gpu_optim.py leave room for another FMA contraction or another order of summation; this does not.  A case that
differs means the arithmetic moved: find the expression, do not re-record."""
import json
import os

import pytest

from tests import update_parity as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "update_pass_digests.json")) as f:
        return json.load(f)


def test_the_inputs_are_the_recorded_ones(golden):
    """asserted first: digests of other inputs say nothing about the passes"""
    assert U.input_digests() == golden["inputs"], (
        "the edge lists of tests/optim_ref.py / tests/master_ref.py are no longer the ones the digests were recorded on: "
        "re-record tests/golden/update_pass_digests.json with the library of the commit BEFORE the change under test")


@pytest.fixture(scope="module")
def got():
    return U.pass_digests()


def test_the_cases_are_the_recorded_ones(golden, got):
    assert set(got) == set(golden["passes"]) == set(CASES) and len(CASES) == 12


CASES = (["adamw_nocoef", "adamw_coef"] + [f"adamw_master_{d}_{c}" for d in ("bf16", "fp16") for c in ("nocoef", "coef")]
         + ["ema", "scale", "grad_norm_1", "grad_norm_1e6", "sumsq_norm_finish_mixed", "pack"])


@pytest.mark.parametrize("case", CASES)
def test_pass_writes_the_recorded_bits(golden, got, case):
    assert got[case] == golden["passes"][case], case
