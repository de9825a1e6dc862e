"""CPU checks of the 3-D PatchGAN discriminator module (cvvae_amd/discriminator.py):

  * the yardstick itself: tests/disc_ref.py in fp64 equals the REFERENCE's own module (tests/golden/disc_net_ref.npz, written by
    tools/make_disc_fixture.py from the unmodified models/discriminator.py) -- logits and dL/dx to 1e-12 relative, the parameter
    gradients' stored sums, norms and entries to 1e-10;
  * the module's CPU path in fp64 equals the same;
  * the HOST logic of the GPU path -- launch program, tape and backward walker -- on plain-PyTorch emulations of the ops
    (tests/emu_ops.py, the four of tests/test_disc_ops_host_logic.py, and the gn_out forms and the new input-gradient kernel defined
    here) against fp64 autograd of disc_ref: 1e-5 relative (fp32 emulation against fp64, the figure of the other host-logic tests)
    for the logits, dL/dx and every parameter gradient; no statistics pass anywhere, no first-layer input gradient for a detached
    input, equal gradients from two backward calls."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import disc_ref, emu_ops
from tests.test_disc_ops_host_logic import emu_avgpool3d_down, emu_avgpool3d_down_bwd, emu_gn_leaky_apply, emu_leaky_bwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "disc_net_ref.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind == "f" else [str(s) for s in z[k]]) for k in z.files}


@pytest.fixture(scope="module")
def ref64(fixture):
    """fp64 disc_ref at the fixture's input with the seeded weights, computed once: (state, logits, dL/dx, parameter gradients)"""
    state = disc_ref.seeded_state()
    y, dx, gp = disc_ref.run(state, fixture["x"], fixture["c"])
    return state, y, dx, gp


def _check_summaries(fixture, grads, tol):
    assert sorted(fixture["pnames"]) == sorted(k for k, g in grads.items() if g is not None)
    for i, k in enumerate(fixture["pnames"]):
        g = grads[k].detach().double().reshape(-1)
        n = float(fixture["pl2"][i])
        assert abs(float(g.norm()) - n) <= tol * n, k
        assert abs(float(g.sum()) - float(fixture["psum"][i])) <= tol * n * g.numel() ** 0.5, k
        e = g[(torch.arange(8) * g.numel()) // 8]
        assert float((e - fixture["pentries"][i]).abs().max()) <= tol * float(g.abs().max()), k


def test_disc_ref_fp64_equals_the_reference_module(fixture, ref64):
    _, y, dx, gp = ref64
    assert tuple(y.shape) == (1, 1, 1, 4, 4)
    assert _rel(y, fixture["logits"]) <= 1e-12 and _rel(dx, fixture["dx"]) <= 1e-12
    assert all(gp[k] is None for k in gp if ".temb_proj." in k)
    _check_summaries(fixture, gp, 1e-10)


def test_module_cpu_path_fp64_equals_the_reference_module(fixture):
    from cvvae_amd.discriminator import get_cvvae_discriminator
    net = get_cvvae_discriminator()
    net.load_state_dict(disc_ref.seeded_state())
    net = net.double().train()
    x = fixture["x"].clone().requires_grad_(True)
    y = net(x)
    (y * fixture["c"]).sum().backward()
    assert _rel(y.detach(), fixture["logits"]) <= 1e-12 and _rel(x.grad, fixture["dx"]) <= 1e-12
    _check_summaries(fixture, {k: p.grad for k, p in net.named_parameters()}, 1e-10)


# ---- emulations of the launches tests/emu_ops.py and tests/test_disc_ops_host_logic.py do not have ----
def emu_gn_leaky_apply_out(x, gn, slope=0.2, out=None, gn_out=0):
    y = emu_gn_leaky_apply(x, gn, slope, out)
    return (y, emu_ops.FakePart(y, x.shape[0], x.shape[-1], gn_out)) if gn_out else y


def emu_avgpool3d_down_out(x, gn_out=0):
    y = emu_avgpool3d_down(x)
    return (y, emu_ops.FakePart(y, x.shape[0], x.shape[-1], gn_out)) if gn_out else y


def emu_conv333_s2_dgrad_small(gy, w, in_shape, cin):
    """include/cvvae.h: the input gradient of conv3d(x, w, stride 2, zero padding 1), 8 channels, those >= cin zero"""
    B, T, H, W = in_shape
    if w.dim() == 3:   # the [27, Cout, 8] table
        w = w[:, :, :cin].reshape(3, 3, 3, w.shape[1], cin).permute(3, 4, 0, 1, 2)
    cout = w.shape[0]
    x = torch.zeros(B, cin, T, H, W, requires_grad=True)
    with torch.enable_grad():
        y = F.conv3d(x, w.detach().float(), None, stride=2, padding=1)
        assert tuple(y.shape[2:]) == tuple(gy.shape[1:4])
        (y * gy.float()[..., :cout].permute(0, 4, 1, 2, 3)).sum().backward()
    out = torch.zeros(B, T, H, W, 8, dtype=gy.dtype)
    out[..., :cin] = x.grad.permute(0, 2, 3, 4, 1).to(gy.dtype)
    return out


@pytest.fixture
def emulated(monkeypatch):
    from cvvae_amd import ops
    calls = []

    def rec(name, fn):
        def f(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return f
    with emu_ops.patched(whole_model=True):
        monkeypatch.setattr(ops, "_need_gpu", lambda t: None)
        for n, fn in (("avgpool3d_down", emu_avgpool3d_down_out), ("avgpool3d_down_bwd", emu_avgpool3d_down_bwd),
                      ("gn_leaky_apply", emu_gn_leaky_apply_out), ("leaky_bwd", emu_leaky_bwd),
                      ("conv333_s2_dgrad_small", emu_conv333_s2_dgrad_small)):
            monkeypatch.setattr(ops, n, rec(n, fn))
        for n in ("gn_stats", "gn_finalize", "conv", "conv_wgrad", "gn_bwd_input", "gn_bwd_input_params", "gn_silu_apply", "pad_fold"):
            monkeypatch.setattr(ops, n, rec(n, getattr(ops, n)))
        yield calls
        monkeypatch.undo()  # before patched() restores its own


def _net():
    from cvvae_amd.discriminator import get_cvvae_discriminator
    net = get_cvvae_discriminator()
    net.load_state_dict(disc_ref.seeded_state())
    return net.train()


def _run(net, x, c, attached=True):
    from cvvae_amd.discriminator import DiscFn
    named = list(net.named_parameters())
    xa = x.clone().requires_grad_(attached)
    y = DiscFn.apply(xa, net, tuple(n for n, _ in named), *[p for _, p in named])
    return xa, y, named


def test_gpu_program_and_walker_on_emulated_ops_match_fp64_autograd(fixture, ref64, emulated):
    _, yr, dxr, gpr = ref64
    net = _net()
    x, c = fixture["x"].float(), fixture["c"].float()
    xa, y, named = _run(net, x, c)
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(yr.shape) and y.requires_grad
    assert _rel(y.detach(), yr) <= TOL
    fwd = list(emulated)
    assert "gn_stats" not in fwd                                     # every Normalize reads its producer's records
    assert fwd.count("gn_finalize") == 4 * 2 + 4 and fwd.count("gn_leaky_apply") == 5 and fwd.count("avgpool3d_down") == 4
    assert fwd.count("conv") == 1 + 4 * 2 + 3 + 1                     # main.0, conv1 / conv2, three nin_shortcuts, main.14
    # two backward calls over one graph (the loss's last-layer probe, then backward()): equal gradients
    ps = [p for _, p in named if ".temb_proj." not in _]
    L = (y * c).sum()
    first = torch.autograd.grad(L, [xa] + ps, retain_graph=True)
    del emulated[:]
    L.backward()
    bwd = list(emulated)
    assert "gn_stats" not in bwd and "pad_fold" not in bwd
    assert bwd.count("conv333_s2_dgrad_small") == 1
    assert bwd.count("conv_wgrad") == 1 + 4 * 2 + 3 + 1 and bwd.count("gn_bwd_input_params") == 4 * 2 + 4
    assert torch.equal(first[0], xa.grad) and all(torch.equal(a, p.grad) for a, p in zip(first[1:], ps))
    assert _rel(xa.grad, dxr) <= TOL
    for n, p in named:
        if ".temb_proj." in n:
            assert p.grad is None and gpr[n] is None, n
        else:
            assert p.grad.dtype == p.dtype and p.grad.shape == p.shape and _rel(p.grad, gpr[n]) <= TOL, (n, _rel(p.grad, gpr[n]))


def test_detached_input_and_frozen_parameters_skip_their_launches(fixture, emulated):
    net = _net()
    x, c = fixture["x"].float(), fixture["c"].float()
    xa, y, named = _run(net, x, c)
    (y * c).sum().backward()
    want = {n: p.grad.clone() for n, p in named if p.grad is not None}
    net.zero_grad(set_to_none=True)
    del emulated[:]
    xd, y, named = _run(net, x, c, attached=False)                   # the discriminator step: the input is detached
    (y * c).sum().backward()
    assert "conv333_s2_dgrad_small" not in emulated and xd.grad is None
    assert all(torch.equal(p.grad, want[n]) for n, p in named if n in want)
    # the generator step through a frozen discriminator: the input gradient alone
    net.requires_grad_(False)
    net.zero_grad(set_to_none=True)
    del emulated[:]
    xa2, y, named = _run(net, x, c)
    (y * c).sum().backward()
    assert torch.equal(xa2.grad, xa.grad) and all(p.grad is None for _, p in named)
    assert not {"conv_wgrad", "gn_bwd_input_params", "gn_silu_apply"} & set(emulated) and emulated.count("conv333_s2_dgrad_small") == 1


def test_no_grad_and_eval_run_without_a_tape(fixture, monkeypatch, emulated):
    from cvvae_amd import discriminator as D
    net = _net()
    x = fixture["x"].float()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))   # route the CPU tensor to the (emulated) GPU path
    taped = net(x)
    assert taped.requires_grad
    with torch.no_grad():
        a = net(x)
    b = net.eval()(x)
    assert not a.requires_grad and not b.requires_grad and torch.equal(a, taped.detach()) and torch.equal(b, a)
    with pytest.raises(ValueError):
        net(x[:, :2])
    with pytest.raises(RuntimeError, match="without a tape"):     # eval() must not drop an input gradient silently
        net(x.clone().requires_grad_(True))
    assert D.DIRECT_FIRST_DGRAD is True
