"""CPU check of the HOST logic of cvvae_amd/disc_ops.py: with the four new ops wrappers replaced by plain-PyTorch emulations of their
documented arithmetic (defined here) and the GroupNorm statistics / backward wrappers by those of tests/emu_ops.py, the two
differentiable functions must reproduce torch.autograd over the fp64 yardstick -- F.avg_pool3d after the reference's torch.cat, and
F.leaky_relu(F.group_norm(...)) -- forward and every gradient.  That pins which tables go to which launch, what is saved, the output
mask of the activation's backward and the autograd.Function wiring.  (The kernels themselves: tests/test_gpu_disc_ops.py.)
Tolerance 1e-5 relative: fp32 emulation against fp64 over a few dozen terms."""
import pytest
import torch
import torch.nn.functional as F

from tests import emu_ops

TOL = 1e-5


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-30))


# ---- the documented arithmetic of the four entry points (include/cvvae.h), fp32 ----
def emu_avgpool3d_down(x):
    B, T, H, W, C = x.shape
    To, Ho, Wo = (T + (T & 1)) // 2, H // 2, W // 2
    stored = lambda p: p if T % 2 == 0 else max(p - 1, 0)  # noqa: E731  (padded frame -> stored frame)
    out = torch.zeros(B, To, Ho, Wo, C, dtype=torch.float32)
    for to in range(To):
        for dt in (0, 1):
            f = x[:, stored(2 * to + dt)].float()
            for dy in (0, 1):
                for dx in (0, 1):
                    out[:, to] += f[:, dy:2 * Ho:2, dx:2 * Wo:2]
    return (out * 0.125).to(x.dtype)


def emu_avgpool3d_down_bwd(gy, shape):
    B, T, H, W, C = shape
    Ho, Wo = H // 2, W // 2
    gx = torch.zeros(B, T, H, W, C, dtype=torch.float32)
    for t in range(T):
        to = (t + (T & 1)) // 2
        k = 0.25 if (T % 2 == 1 and t == 0) else 0.125
        up = gy[:, to].float().repeat_interleave(2, 1).repeat_interleave(2, 2)
        gx[:, t, :2 * Ho, :2 * Wo] = k * up
    return gx.to(gy.dtype)


def emu_gn_leaky_apply(x, gn, slope=0.2, out=None):
    v = x.float()
    if gn is not None:
        sc, sh = gn
        assert sc.dtype == torch.float32 and tuple(sc.shape) == (x.shape[0], x.shape[-1]) and sh.shape == sc.shape
        v = v * sc[:, None, None, None, :] + sh[:, None, None, None, :]
    y = torch.where(v > 0, v, slope * v).to(x.dtype)
    return y if out is None else out.copy_(y)


def emu_leaky_bwd(y, gy, slope=0.2, out=None):
    g = torch.where(y.float() > 0, gy.float(), slope * gy.float()).to(gy.dtype)
    return g if out is None else out.copy_(g)


@pytest.fixture
def emulated(monkeypatch):
    from cvvae_amd import ops
    calls = []

    def rec(name, fn):
        def f(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return f
    with emu_ops.patched(whole_model=True):  # the GroupNorm wrappers + torch.cuda.device, as tests/test_grad3d_host_logic.py
        monkeypatch.setattr(ops, "_need_gpu", lambda t: None)
        for n, fn in (("avgpool3d_down", emu_avgpool3d_down), ("avgpool3d_down_bwd", emu_avgpool3d_down_bwd),
                      ("gn_leaky_apply", emu_gn_leaky_apply), ("leaky_bwd", emu_leaky_bwd)):
            monkeypatch.setattr(ops, n, rec(n, fn))
        for n in ("gn_stats", "gn_bwd_input", "gn_bwd_input_params"):
            monkeypatch.setattr(ops, n, rec(n, getattr(ops, n)))
        yield calls
        monkeypatch.undo()  # before patched() restores its own


def _seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("T", [1, 2, 5])
def test_avg_pool_down3d_matches_autograd_of_cat_and_avg_pool3d(emulated, T):
    from cvvae_amd import disc_ops
    x = _seeded((2, T, 5, 4, 16), T)                     # odd H: the last row is dropped
    xr = x.double().permute(0, 4, 1, 2, 3).clone().requires_grad_(True)   # the reference's NCDHW
    h = torch.cat([xr[:, :, :1], xr], 2) if T % 2 else xr
    yr = F.avg_pool3d(h, kernel_size=2, stride=2)
    cot = _seeded(tuple(yr.shape), 10 + T)
    (yr * cot.double()).sum().backward()
    xa = x.clone().requires_grad_(True)
    ya = disc_ops.avg_pool_down3d(xa)
    assert ya.requires_grad and tuple(ya.shape) == (2, (T + 1) // 2, 2, 2, 16)
    assert _rel(ya.detach().permute(0, 4, 1, 2, 3), yr.detach()) < TOL
    (ya * cot.permute(0, 2, 3, 4, 1)).sum().backward()
    gr = xr.grad.permute(0, 2, 3, 4, 1)
    assert _rel(xa.grad, gr) < TOL
    assert torch.equal(xa.grad[:, :, 4], torch.zeros_like(xa.grad[:, :, 4]))    # the dropped row
    assert emulated == ["avgpool3d_down", "avgpool3d_down_bwd"]
    # no graph without a gradient to compute
    assert not disc_ops.avg_pool_down3d(x).requires_grad


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("train_affine", [True, False])
@pytest.mark.parametrize("C,groups", [(64, 32), (16, 4)])
def test_group_norm_leaky_matches_autograd_of_group_norm_and_leaky_relu(emulated, T, train_affine, C, groups):
    from cvvae_amd import disc_ops
    x = _seeded((2, T, 5, 4, C), 20 + T) * 1.5 + 0.3
    w = 1.0 + 0.2 * _seeded((C,), 31)
    b = 0.3 * _seeded((C,), 32)
    xr = x.double().permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = F.leaky_relu(F.group_norm(xr, groups, wr, br, 1e-6), 0.2)
    cot = _seeded(tuple(yr.shape), 40 + T)
    (yr * cot.double()).sum().backward()
    xa = x.clone().requires_grad_(True)
    wa, ba = w.clone().requires_grad_(train_affine), b.clone().requires_grad_(train_affine)
    kw = {} if groups == 32 else dict(num_groups=groups)   # 32 groups and eps 1e-6 are the defaults (the reference's Normalize)
    ya = disc_ops.group_norm_leaky(xa, wa, ba, **kw)
    assert ya.requires_grad and _rel(ya.detach().permute(0, 4, 1, 2, 3), yr.detach()) < TOL
    (ya * cot.permute(0, 2, 3, 4, 1)).sum().backward()
    assert _rel(xa.grad, xr.grad.permute(0, 2, 3, 4, 1)) < TOL
    if train_affine:
        assert wa.grad.shape == w.shape and _rel(wa.grad, wr.grad) < TOL and _rel(ba.grad, br.grad) < TOL
        assert emulated == ["gn_stats", "gn_leaky_apply", "leaky_bwd", "gn_bwd_input_params"]
    else:
        assert wa.grad is None and ba.grad is None
        assert emulated == ["gn_stats", "gn_leaky_apply", "leaky_bwd", "gn_bwd_input"]   # a frozen norm: no affine sums


def test_group_norm_leaky_with_a_frozen_input_still_trains_the_affine(emulated):
    from cvvae_amd import disc_ops
    C, groups = 16, 4
    x = _seeded((1, 2, 3, 4, C), 5)
    w, b = (1.0 + 0.2 * _seeded((C,), 6)), 0.3 * _seeded((C,), 7)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = F.leaky_relu(F.group_norm(x.double().permute(0, 4, 1, 2, 3).contiguous(), groups, wr, br, 1e-5), 0.1)
    yr.sum().backward()
    wa, ba = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ya = disc_ops.group_norm_leaky(x, wa, ba, num_groups=groups, eps=1e-5, slope=0.1)
    ya.sum().backward()
    assert _rel(ya.detach().permute(0, 4, 1, 2, 3), yr.detach()) < TOL
    assert _rel(wa.grad, wr.grad) < TOL and _rel(ba.grad, br.grad) < TOL


@pytest.mark.parametrize("T", [1, 2, 5])
def test_bare_leaky_relu_takes_its_mask_from_the_output(emulated, T):
    from cvvae_amd import disc_ops
    x = _seeded((2, T, 5, 4, 16), 50 + T)
    x.view(-1)[::7] = 0.0                                # exact zeros: y = 0 there, the gradient is slope * gy
    xr = x.double().clone().requires_grad_(True)
    yr = F.leaky_relu(xr, 0.2)
    cot = _seeded(tuple(x.shape), 60 + T)
    (yr * cot.double()).sum().backward()
    xa = x.clone().requires_grad_(True)
    ya = disc_ops.group_norm_leaky(xa)
    assert _rel(ya.detach(), yr.detach()) < TOL and bool((ya.detach().view(-1)[::7] == 0).all())
    (ya * cot).sum().backward()
    assert _rel(xa.grad, xr.grad) < TOL
    assert torch.equal(xa.grad.view(-1)[::7], (0.2 * cot.view(-1)[::7]))
    assert emulated == ["gn_leaky_apply", "leaky_bwd"]   # no statistics, no GroupNorm backward
