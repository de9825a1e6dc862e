"""CPU check of the HOST logic of cvvae_amd/lpips.py: with every kernel replaced by a plain-PyTorch emulation of its documented
arithmetic (tests/emu_ops.py for the convolutions; the LPIPS passes of include/cvvae.h ABI 14 are emulated below), the module's
forward must reproduce the restatement of the reference's LPIPS.forward (tests/lpips_ref.py) and its autograd node
torch.autograd's gradient -- i.e. both images go through the trunk in the right order, the right ReLU outputs are taped, the right
half of the batch is back-propagated and every launch is fed the right operand.  (The kernels themselves are measured on the GPU:
tests/test_gpu_lpips.py.)"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from tests import emu_ops, lpips_ref


# ---- emulations of the LPIPS passes (fp32 arithmetic, one rounding to the storage dtype) ----
def lpips_scale_in(x, shift, scale, cpad, dtype, out=None):
    N, C, H, W = x.shape
    o = torch.zeros(N, H, W, cpad, dtype=dtype)
    o[..., :3] = ((x.float() - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1)).permute(0, 2, 3, 1).to(dtype)
    if out is None:
        return o
    assert tuple(out.shape) == (N, H, W, cpad) and out.is_contiguous()
    out.copy_(o)
    return out


def lpips_scale_in_bwd(g, scale, dtype):
    return (g.float()[..., :3] / scale.view(1, 1, 1, 3)).permute(0, 3, 1, 2).contiguous().to(dtype)


def relu_(x):
    return x.clamp_(min=0)


def _nchw(x):
    H, W, C = x.shape[-3:]
    return x.float().reshape(-1, H, W, C).permute(0, 3, 1, 2)


def maxpool2x2(x):
    H, W, C = x.shape[-3:]
    y = F.max_pool2d(_nchw(x), 2, 2).permute(0, 2, 3, 1)
    return y.reshape(*x.shape[:-3], H // 2, W // 2, C).contiguous().to(x.dtype)


def relu_pool_bwd(y, g_tap, g_pool):
    assert g_tap is not None or g_pool is not None
    g = torch.zeros_like(y, dtype=torch.float32) if g_tap is None else g_tap.float().clone()
    if g_pool is not None:
        t = _nchw(y).clone().requires_grad_(True)
        with torch.enable_grad():
            (F.max_pool2d(t, 2, 2) * _nchw(g_pool)).sum().backward()
        g = g + t.grad.permute(0, 2, 3, 1).reshape(y.shape)
    return (g * (y.float() > 0)).to(y.dtype)


def _head(f0, f1, w):
    def nrm(f):
        return f / (torch.sqrt((f * f).sum(-1, keepdim=True) + 1e-10) + 1e-10)
    d = ((nrm(f0) - nrm(f1)) ** 2 * w).sum(-1)
    return d.reshape(d.shape[0], -1).mean(1)


def lpips_head(f0, f1, w, out):
    out += _head(f0.float(), f1.float(), w)
    return out


def lpips_head_bwd(f0, f1, w, gout, g0, g1):
    a, b = f0.float().clone().requires_grad_(True), f1.float().clone().requires_grad_(True)
    with torch.enable_grad():
        (_head(a, b, w) * gout).sum().backward()
    if g0 is not None:
        g0.copy_(a.grad.to(g0.dtype))
    if g1 is not None:
        g1.copy_(b.grad.to(g1.dtype))


_LPIPS_OPS = dict(lpips_scale_in=lpips_scale_in, lpips_scale_in_bwd=lpips_scale_in_bwd, relu_=relu_, maxpool2x2=maxpool2x2,
                  relu_pool_bwd=relu_pool_bwd, lpips_head=lpips_head, lpips_head_bwd=lpips_head_bwd)


@contextlib.contextmanager
def emulated(monkeypatch):
    """emu_ops.patched() + the LPIPS passes above + CPU tensors let through the module's device guard"""
    from cvvae_amd import ops
    with emu_ops.patched(whole_model=True), monkeypatch.context() as mp:
        for n, f in _LPIPS_OPS.items():
            mp.setattr(ops, n, f)
        mp.setattr(ops, "_need_gpu", lambda t: None)
        yield


def _module(seed=3):
    from cvvae_amd.lpips import LPIPS
    sd = lpips_ref.lpips_state_dict(seed)
    m = LPIPS().eval()
    m.load_state_dict(sd, strict=True)
    return m, sd


def _images(shape, seed):
    from oracle.seeded import seeded_input
    x = seeded_input(shape, seed)
    return x, (x + 0.3 * seeded_input(shape, seed + 1)).clamp(-1, 1)


def test_seeded_features_stay_alive():
    """the yardstick's weights: relu5_3 of the seeded trunk must neither die nor blow up (He scaling, tests/lpips_ref.py)"""
    sd = lpips_ref.lpips_state_dict(3)
    x, _ = _images((2, 3, 64, 64), 11)
    p = {k: v.double() for k, v in sd.items()}
    taps = lpips_ref.vgg_taps((x.double() - p["scaling_layer.shift"]) / p["scaling_layer.scale"], p)
    for k, t in enumerate(taps):
        frac, mx = float((t > 0).double().mean()), float(t.abs().max())
        print(f"relu tap {k}: non-zero fraction {frac:.3f}, max {mx:.3f}")
        assert 0.2 < frac < 0.8 and 1e-2 < mx < 1e2, (k, frac, mx)


@pytest.mark.parametrize("shape", [(2, 3, 32, 48), (1, 3, 50, 50)])
@pytest.mark.parametrize("wrt", [(False, True), (True, False), (True, True)])
def test_lpips_forward_and_gradient_wiring(monkeypatch, shape, wrt):
    m, sd = _module()
    x0, x1 = _images(shape, 5)
    from oracle.seeded import seeded_input
    cot = 0.5 + seeded_input((shape[0], 1, 1, 1), 8).abs()
    ref, r0, r1 = lpips_ref.lpips_with_grads(x0, x1, sd, cot, torch.float64, wrt)
    a, b = x0.clone().requires_grad_(wrt[0]), x1.clone().requires_grad_(wrt[1])
    with emulated(monkeypatch):
        val = m(a, b)
        (val * cot).sum().backward()
        with torch.no_grad():
            plain = m(x0, x1)
    assert tuple(val.shape) == (shape[0], 1, 1, 1) and val.dtype == torch.float32
    assert torch.allclose(val.detach().double(), ref, rtol=1e-4, atol=0), float((val.detach().double() - ref).abs().max())
    assert torch.equal(plain, val.detach())
    for got, want, need in ((a.grad, r0, wrt[0]), (b.grad, r1, wrt[1])):
        if not need:
            assert got is None
            continue
        assert got.shape == want.shape and got.dtype == torch.float32
        err = float((got.double() - want).norm() / want.norm())
        assert err < 1e-4, err


def test_nothing_is_taped_without_grad(monkeypatch):
    """no_grad / inputs that need no gradient: the plain forward, no autograd node and no tape"""
    from cvvae_amd import lpips
    m, _ = _module()
    x0, x1 = _images((1, 3, 32, 32), 2)
    tapes = []
    real = lpips._forward

    def spy(mod, a, b, tape):
        tapes.append(tape)
        return real(mod, a, b, tape)

    monkeypatch.setattr(lpips, "_forward", spy)
    with emulated(monkeypatch):
        with torch.no_grad():
            v = m(x0.clone().requires_grad_(True), x1)
        assert v.grad_fn is None and not v.requires_grad and tapes == [None]
        v = m(x0, x1)
        assert v.grad_fn is None and tapes == [None, None]
        v = m(x0, x1.clone().requires_grad_(True))
        assert v.grad_fn is not None and isinstance(tapes[-1], list) and len(tapes[-1]) == 5
        assert [len(t) for t in tapes[-1]] == [2, 2, 3, 3, 3]


def test_only_the_needed_half_is_back_propagated(monkeypatch):
    """gradient into `target` alone (the training step: reconstructions): every backward launch sees N frames, not 2N"""
    from cvvae_amd import ops
    m, _ = _module()
    x0, x1 = _images((2, 3, 32, 32), 4)
    seen = []
    with emulated(monkeypatch):
        real = ops.relu_pool_bwd
        monkeypatch.setattr(ops, "relu_pool_bwd", lambda y, gt, gp: (seen.append(y.shape[1]), real(y, gt, gp))[1])
        b = x1.clone().requires_grad_(True)
        m(x0, b).sum().backward()
    assert len(seen) == 13 and set(seen) == {2}
