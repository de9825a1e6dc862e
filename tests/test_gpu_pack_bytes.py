"""The packed-weight bytes, pinned: every public packer of cvvae_amd.ops on the inputs of tests/pack_cases.py must write the same
buffer (sha256 of all of it, read-ahead tail included), the same padded bias and the same PackedConv fields as the recording in
tests/golden/packed_weight_hashes.json.  The packed format is read by conv_fwd_kernel only, so the convolution tests see a wrong
packer through their tolerances at best; this one sees a single byte.  The fixture was recorded from the library of the commit it
names, before the packers moved into csrc/pack_kernels.hip, and passes unchanged on both."""
import json
import os

import pytest
import torch

from tests import pack_cases as PC

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_weight_hashes.json")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case,form", PC.params(), ids=PC.case_ids())
def test_packed_bytes(case, form, recorded):
    from cvvae_amd import ops
    pw, win = PC.run_case(ops, case, form)
    torch.cuda.synchronize()
    got, want = PC.summarise(pw, win), recorded[f"{case.name}-{form}"]
    assert got["input_sha256"] == want["input_sha256"], "the generated input differs from the recorded one"
    assert got["fields"] == want["fields"]
    assert got["bias_sha256"] == want["bias_sha256"]
    assert got["w_sha256"] == want["w_sha256"]
