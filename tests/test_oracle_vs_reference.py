"""Pin of the CPU oracle against the reference's OWN unmodified modules: the oracle's restatement runs on the same seeded
weights and inputs the reference ran on when tests/golden/ref_oracle_pins.npz was written (python -m oracle.make_golden pins)."""
import os

import numpy as np
import pytest
import torch

from oracle import cvvae_oracle as O
from oracle.golden_cases import PIN_CASES, PIN_FIXTURE, PIN_WSEED, PIN_XSEED, pin_key
from oracle.seeded import seeded_input, seeded_state_dict
from oracle.shapes import state_dict_shapes


@pytest.mark.parametrize("family,shape", PIN_CASES)
def test_oracle_equals_reference_modules(family, shape, golden_dir):
    gold = np.load(os.path.join(golden_dir, PIN_FIXTURE + ".npz"))
    sd = seeded_state_dict(state_dict_shapes(family), PIN_WSEED)
    x = seeded_input(shape, PIN_XSEED)
    with torch.no_grad():
        mom = O.encode_moments(x, sd, {}, family)
        rec_o = O.decode_sample(O.posterior_mode(mom), sd, {}, family)
    ref_mom = torch.from_numpy(gold[pin_key(family, shape) + "_moments"])
    ref_rec = torch.from_numpy(gold[pin_key(family, shape) + "_recon"])
    assert mom.shape == ref_mom.shape and rec_o.shape == ref_rec.shape
    assert (mom - ref_mom).abs().max() <= 2e-5
    assert (rec_o - ref_rec).abs().max() <= 1e-4
