"""The conv input gradients against fp64 at their borders (needs the MI355X).

Every case of tests/dgrad_edge_cases.py runs in each of its dtypes through the product's own functions -- grad3d.dgrad333,
backward.conv_dgrad, backward.dgrad1x1, grad3d.sd3_upsample_backward (grads = None) over a WeightCache -- and the result is compared
PER ELEMENT with fp64 autograd of the forward op (tests/dgrad_ref.py, from the dtype-rounded operands) under that element's own
bound: worst err / bound <= 1.  Besides: the stated shape and dtype, stored pad channels exactly zero, exact zeros where no window
reaches, a second call gives the same bits, and the operands are left as they were.  A line per (case, dtype) reports the worst
ratio and where (appended to dgrad_edges_parity.txt under CVVAE_TEST_LOG_DIR when that is set).

tests/test_dgrad_edges_host.py checks the table, the yardstick and the bound themselves on the CPU."""
import os

import pytest
import torch

import dgrad_edge_cases as DC
import dgrad_ref as DR

pytestmark = pytest.mark.gpu

CASES = DC.cases()
PARAMS = [(c, dt) for c in CASES for dt in c.dtypes]


def _log(line):
    print("\n" + line)
    d = os.environ.get("CVVAE_TEST_LOG_DIR", "")          # a directory that receives the figures of a run; unset: printed only
    if d and os.path.isdir(d):
        with open(os.path.join(d, "dgrad_edges_parity.txt"), "a") as f:
            f.write(line + "\n")


def test_the_table_is_complete():
    assert len(CASES) == 54 and len(PARAMS) == 3 * 54


@pytest.mark.parametrize("case,dt", PARAMS, ids=[f"{c.name}-{dt}" for c, dt in PARAMS])
def test_input_gradient(case, dt):
    from cvvae_amd.engine import WeightCache
    t = DR.inputs(case, dt)
    with torch.cuda.device(0):
        dev = {k: v.cuda() for k, v in t.items()}
        wc = WeightCache(DR.holder(dev["w"]))
        got = DR.call(case, dev, wc)
        again = DR.call(case, dev, wc)
        torch.cuda.synchronize()
    for k in ("g", "add", "residual"):
        assert k not in t or torch.equal(dev[k].cpu(), t[k]), f"{case.name} {dt}: the call modified {k}"
    got, again = got.cpu(), again.cpu()
    dead = DR.check_result(case, dt, got)
    w, at, bad = DR.worst(case, dt, got)
    same = got.dtype == again.dtype and got.shape == again.shape and torch.equal(got.view(torch.uint8), again.view(torch.uint8))
    _log(f"DGRAD-EDGE {case.name} {dt}: n = {DR.n_stored(case)}, worst err/bound = {w:.4f} at {at}, {dead} unreached elements"
         f"{'' if same else '  NOT REPRODUCIBLE'}")
    assert w <= 1.0, f"{case.name} {dt}: worst err/bound = {w:.4f} at (b, t, y, x, c) = {at} ({bad} elements beyond their bound)"
    assert same, f"{case.name} {dt}: two calls on the same inputs differ"
