"""The two attention blocks and their backward against fp64 at the edges (needs the MI355X).

Every case of tests/attn_block_cases.py runs `engine.spatial_attention` / `engine.v3_attn_spatial_temporal` untaped and taped and
`grad.attention_backward` (+ `grad3d.temporal_attention_backward`) with parameter gradients on the HIP kernels, in each dtype, twice
on the same inputs.  The output, the input gradient and every parameter gradient are compared with the fp64 yardstick of
tests/attn_block_ref.py in that file's measures (worst token row of an activation; ||.|| / ||S|| of a parameter gradient) under
MARGIN x the noise of the CPU restatement that rounds where the product path stores -- nothing measured here enters a bound.  A line
per (case, dtype) reports `err / bound` of every tensor; any ratio above 1 fails.  profiles/attn_block_edges_parity.log holds those lines
from one run (pytest -s).

Without a band: the two runs and the taped and untaped outputs are bit-identical; the frozen backward (`grads=None`, as the 2-D
constraint decoder calls it) returns the trainable one's dx bits; the q / k gradients at one token (q_t / k_t at one frame) are exactly
zero; the padding columns of the taped `p` are exactly zero; every output is finite -- with NaN-filled device memory freed in front
of every product call, so that a padding element nobody writes is read as NaN and not as a stale zero.  16-bit models with 512
channels run with the fused kernel and with CVVAE_FUSED_ATTENTION=0, forward and backward under both.

tests/test_attn_block_edges_host.py checks the references, recipes, bound and seeded defects themselves on the CPU.
"""
import os

import pytest
import torch

import attn_block_cases as AC
import attn_block_ref as AR
from attn_block_cases import F32

pytestmark = pytest.mark.gpu

CASES = AC.all_cases()


def _log(line):
    """printed (pytest -s), and appended to $CVVAE_PARITY_LOG_DIR/attn_block_edges_parity.txt when that names a directory"""
    print("\n" + line)
    d = os.environ.get("CVVAE_PARITY_LOG_DIR", "")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "attn_block_edges_parity.txt"), "a") as f:
            f.write(line + "\n")


def _poison():
    """64 MB (more than a call's intermediates) and a run of sub-megabyte blocks (the allocator's small pool) filled with NaN and
    handed back to the caching allocator: what the next call allocates and does not write reads as NaN"""
    big = torch.full((16 << 20,), float("nan"), dtype=torch.float32, device="cuda")
    small = [torch.full((192 << 10,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(16)]
    del big, small


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8),
                                                                     b.contiguous().view(-1).view(torch.uint8))


def _one(case, dt, tag=""):
    """both runs of one (case, dtype) under the current switches -> its failures"""
    bwd = not case.get("fwd_only")
    got = AR.run_product(case, dt, "cuda", backward_pass=bwd, frozen=True, before=_poison)
    again = AR.run_product(case, dt, "cuda", backward_pass=bwd, frozen=True, before=_poison)
    torch.cuda.synchronize()
    got, again = {k: v.cpu() for k, v in got.items()}, {k: v.cpu() for k, v in again.items()}
    fails = []
    rows = AR.compare(case, dt, got)
    worst = max(rows, key=lambda r: r[1] / r[2])
    ch = max((r for r in rows if r[3] is not None), key=lambda r: r[3] / r[2], default=None)
    _log(f"ATTN-BLOCK-EDGE {case.name} {dt}{tag}: worst err/bound = {worst[1] / worst[2]:.4f} at {worst[0]}"
         + (f"; worst channel {ch[3] / ch[2]:.4f} of {ch[0]}" if ch else "") + " | "
         + " ".join(f"{k}={m / b:.3f}" for k, m, b, _ in rows))
    fails += [f"{k}: err/bound = {m / b:.3f} ({m:.3e} > {b:.3e})" for k, m, b, _ in rows if not m <= b]
    fails += [f"{k} is not finite" for k, v in got.items() if not bool(torch.isfinite(v.float()).all())]
    fails += [f"{k}: two runs on the same inputs differ" for k in got if not _same(got[k], again[k])]
    if bwd:
        if not _same(got["y"], got["y_taped"]):
            fails.append("the taped pass does not return the untaped pass's bits")
        if case.op != AC.V3ST and not _same(got["dx"], got["dx_frozen"]):
            fails.append("the frozen backward's dx differs from the trainable one's")
        p = got["p"].view(-1, got["p"].shape[-1])
        if bool((p[:, AC.tokens(case):] != 0).any()):
            fails.append("padding columns of the taped p are not zero")
        fails += [f"{k} is not exactly zero" for k in AR.exact_zero(case) if bool((got[k] != 0).any())]
    return [f"{dt}{tag}: {f}" for f in fails]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_attention_block(case, monkeypatch):
    if case.raises:   # the taped backward over more than 8 frames: what ops.temporal_attention_bwd documents
        for dt in case.dtypes:
            with pytest.raises(NotImplementedError):
                AR.run_product(case, dt, "cuda")
            _log(f"ATTN-BLOCK-EDGE {case.name} {dt}: raises (unsupported shape)")
        return
    failures = []
    for dt in case.dtypes:
        monkeypatch.setenv("CVVAE_FUSED_ATTENTION", "1")
        failures += _one(case, dt)
        if case["C"] == 512 and dt != F32:
            monkeypatch.setenv("CVVAE_FUSED_ATTENTION", "0")
            failures += _one(case, dt, " five-launch")
    assert not failures, f"{case.name}: " + "; ".join(failures)

