"""engine.master_weights() on a real MI355X (cvvae_amd/autoencoder.py): the `latent` engine of tests/engine_cases.py at the shape of
tests/test_gpu_train_engine.py, bf16 networks on fp32 master weights, three iterations of each optimizer.

Conditions, not bands.  After every iteration each cast parameter is its master rounded to bf16, bit for bit.  The first iteration's
gradients are bit-identical to those of an engine prepared with engine_cases.to_device(..., bfloat16): the bf16 weights are the same
bits (fp32 rounded once, on either path), so the forward and the backward must be untouched by the feature.  And after the first
iteration of each optimizer nothing synchronises with the host: the remaining iterations and their EMA updates run with torch's
synchronisation check on "error"."""
import copy

import pytest
import torch

from oracle.seeded import seeded_input
from tests import engine_cases as EC

pytestmark = pytest.mark.gpu
SHAPE = (1, 3, 5, 32, 32)
INDICES = [0, 2]


def _prepare(e, seen):
    """seeded draws; `seen` receives {name: gradient} as the backward left them (a plain bf16 engine's clip scales them in place)"""
    e.sample_generator = torch.Generator("cuda").manual_seed(5)
    e.frame_indices = INDICES
    backward = e.manual_backward

    def recording(loss):
        backward(loss)
        seen.append({n: p.grad.clone() for n, p in e.named_parameters() if p.grad is not None})
    e.manual_backward = recording
    return e


def test_three_iterations_of_each_optimizer_on_master_weights():
    built = EC.build("latent", True, ema_decay=0.999)
    fp32 = {n: p.detach().clone() for n, p in built.named_parameters()}
    seen_a, seen_b = [], []
    a = _prepare(copy.deepcopy(built).cuda().master_weights(), seen_a)
    b = _prepare(EC.to_device(copy.deepcopy(built), torch.bfloat16), seen_b)
    x = seeded_input(SHAPE, 12).to(torch.bfloat16).cuda()
    names = [n for n, p in a.named_parameters() if p.requires_grad]
    cast = [n for n in names if a.get_parameter(n).dtype == torch.bfloat16]
    assert cast and all(n.startswith("loss.logvar") for n in set(names) - set(cast))
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert p.dtype == q.dtype and torch.equal(p, q), n                  # the same weights, bit for bit
    for n in cast:
        assert torch.equal(a.master_of(a.get_parameter(n)).cpu(), fp32[n])
    assert all(s.dtype == torch.float32 and s.is_cuda for s in a.model_ema.buffers() if s.is_floating_point())

    def check(it):
        for n in cast:
            p = a.get_parameter(n)
            m = a.master_of(p)
            assert m.dtype == torch.float32 and m.is_cuda and torch.equal(p.detach(), m.to(torch.bfloat16)), (it, n)

    for it in range(2):                                                     # the first iteration of each optimizer
        loss_a = a.training_step({"frames": x}, it)
        loss_b = b.training_step({"frames": x}, it)
        if it == 0:
            assert torch.equal(loss_a, loss_b)
            assert sorted(seen_a[0]) == sorted(seen_b[0]) and len(seen_a[0]) > len(cast) // 2
            for n, g in seen_a[0].items():
                assert g.dtype == seen_b[0][n].dtype and torch.equal(g, seen_b[0][n]), n
        a.on_train_batch_end()
        b.on_train_batch_end()
        check(it)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for it in range(2, 6):
            loss = a.training_step({"frames": x}, it)
            a.on_train_batch_end()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check(5)
    assert a.global_step == 6 and bool(torch.isfinite(loss))
    opts = a.optimizers()
    assert all(float(st["step"]) == 3.0 for o in opts for st in o.state.values())
    moved = [n for n in cast if not torch.equal(a.master_of(a.get_parameter(n)).cpu(), fp32[n])]
    assert len(moved) > 0.8 * len(cast), (len(moved), len(cast))
    # the plain bf16 engine's state is what torch's 16-bit step leaves: bf16 moments, no masters; ours: fp32 state, fp32 shadows
    st_b = next(iter(b.optimizers()[1].state.values()))
    st_a = next(iter(opts[1].state.values()))
    assert st_b["exp_avg"].dtype == torch.bfloat16 and "master" not in st_b
    assert st_a["exp_avg"].dtype == st_a["master"].dtype == torch.float32
    msd = a.master_state_dict()
    assert list(msd) == list(a.state_dict()) and all(msd[n].dtype == torch.float32 for n in names)
