"""The discriminator passes (csrc/disc_kernels.hip, cvvae_amd/disc_ops.py) on a real MI355X against torch on the CPU in fp64:
F.avg_pool3d after the reference's torch.cat, and F.leaky_relu(F.group_norm(...)).

Bounds are derived from the number formats, not measured:
  pool forward     fp32 sums of 8 values scaled by 0.125: |err| <= 8 * 2^-24 * mean|x_i| of the window; 16-bit adds half an ulp of the result
  pool backward    0.125 gy / 0.25 gy are exact: BIT-EQUAL to the fp64 gradient rounded to the dtype (inputs kept out of the subnormals)
  gn_leaky_apply   one fma and one multiply: 2 fp32 ulps of |x scale| + |shift|, plus half an ulp of a 16-bit storage dtype
  leaky_bwd        one multiply rounded once: BIT-EQUAL to torch.where(y > 0, gy, slope * gy) evaluated in fp32
group_norm_leaky end to end is held against the same function built from the launches the project already had (cvvae_gn_stats,
cvvae_gn_silu_apply without SiLU, torch's leaky_relu on the GPU, cvvae_gn_bwd_input_params): the new path's error against fp64 may
be at most 1.5x the old path's (the project's factor for box-to-box differences), and at most the absolute band of
tests/golden/disc_ops_bands.json (1.5x the figure measured on the MI355X; both measured figures are recorded next to it).
Every figure is printed before it is asserted (`pytest -s` shows the `[disc band]` lines the band file is made from)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = os.path.join(ROOT, "tests", "golden", "disc_ops_bands.json")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
POOL_SHAPES = [(2, 1, 2, 2, 8),      # odd T = 1: both padded frames are frame 0
               (1, 2, 4, 6, 16),     # even T
               (1, 5, 7, 6, 40),     # odd T, the odd row is dropped, five 8-channel vectors per pixel
               (1, 9, 16, 16, 128)]  # more than one workgroup
SLOPE = 0.2
SLOPE32 = float(torch.tensor(SLOPE, dtype=torch.float32))   # the value the kernels multiply by
# significant bits and smallest normal exponent of the storage formats
FMT = {torch.float16: (11, -14), torch.bfloat16: (8, -126), torch.float32: (24, -126)}


def _ulp(mag, dtype):
    """unit in the last place of `dtype` at magnitude `mag` (fp64 tensor)"""
    p, emin = FMT[dtype]
    e = torch.floor(torch.log2(mag.clamp_min(1e-300))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - (p - 1))


def _randn(shape, seed, dtype):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _away_from_zero(t):
    """|t| >= 2^-6, signs kept: an eighth of it is a normal number in every dtype"""
    return torch.where(t >= 0, t.float().clamp_min(2.0 ** -6), t.float().clamp_max(-2.0 ** -6)).to(t.dtype)


def _ncdhw64(t):
    return t.double().permute(0, 4, 1, 2, 3).contiguous()


def _ref_pool(x64):
    """the reference's lines on an fp64 NCDHW tensor (models/discriminator.py:240-243)"""
    if x64.shape[2] % 2 == 1:
        x64 = torch.cat([x64[:, :, :1], x64], dim=2)
    return F.avg_pool3d(x64, kernel_size=2, stride=2)


_POOL_REF = {}


def _pool_case(shape, dtype):
    """inputs and the fp64 yardstick of one (shape, dtype), computed once and shared by the tests below (never modified)"""
    key = (shape, dtype)
    if key not in _POOL_REF:
        x = _randn(shape, 1 + len(_POOL_REF), dtype)
        xr = _ncdhw64(x).requires_grad_(True)
        yr = _ref_pool(xr)
        mean_abs = _ref_pool(_ncdhw64(x).abs())
        gy = _away_from_zero(_randn(tuple(yr.permute(0, 2, 3, 4, 1).shape), 101 + len(_POOL_REF), dtype))
        (yr * _ncdhw64(gy)).sum().backward()
        _POOL_REF[key] = (x, gy, yr.detach().permute(0, 2, 3, 4, 1), mean_abs.permute(0, 2, 3, 4, 1), xr.grad.permute(0, 2, 3, 4, 1))
    return _POOL_REF[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool3d_down_forward(shape, dtype):
    from cvvae_amd import ops
    x, _, yr, mean_abs, _ = _pool_case(shape, dtype)
    xd = x.cuda()
    y = ops.avgpool3d_down(xd)
    B, T, H, W, C = shape
    assert tuple(y.shape) == (B, (T + 1) // 2, H // 2, W // 2, C) and y.dtype == dtype and y.is_contiguous()
    assert torch.equal(y, ops.avgpool3d_down(xd))                       # the same bits on every run
    bound = 8 * 2.0 ** -24 * mean_abs
    if dtype != torch.float32:
        bound = bound + 0.5 * _ulp(yr.abs() + bound, dtype)
    err = (y.cpu().double() - yr).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n[disc pool fwd] {shape} {dtype}: worst |err| / bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool3d_down_backward_is_bit_equal(shape, dtype):
    from cvvae_amd import ops
    x, gy, _, _, gr = _pool_case(shape, dtype)
    B, T, H, W, C = shape
    gyd = gy.cuda()
    gx = ops.avgpool3d_down_bwd(gyd, shape)
    assert tuple(gx.shape) == shape and gx.dtype == dtype
    assert torch.equal(gx, ops.avgpool3d_down_bwd(gyd, shape))
    gx = gx.cpu()
    assert torch.equal(gx, gr.to(dtype))                                 # every element, the fp64 gradient rounded once
    if H % 2:
        assert torch.equal(gx[:, :, H - 1], torch.zeros_like(gx[:, :, H - 1]))     # the dropped row: exactly 0
    if W % 2:
        assert torch.equal(gx[:, :, :, W - 1], torch.zeros_like(gx[:, :, :, W - 1]))
    if T % 2:                                                            # frame 0 of an odd T went into output frame 0 twice
        up = gy[:, 0].float().repeat_interleave(2, 1).repeat_interleave(2, 2)
        assert torch.equal(gx[:, 0, :2 * (H // 2), :2 * (W // 2)], (0.25 * up).to(dtype))
    # the differentiable function on top: the same launches
    from cvvae_amd import disc_ops
    xa = x.cuda().requires_grad_(True)
    ya = disc_ops.avg_pool_down3d(xa)
    ya.backward(gyd)
    assert torch.equal(ya.detach(), ops.avgpool3d_down(x.cuda())) and torch.equal(xa.grad.cpu(), gx)


def _apply_case(shape, dtype, seed):
    B, T, H, W, C = shape
    x = _randn(shape, seed, dtype)
    g = torch.Generator().manual_seed(seed + 50)
    scale = (1.0 + 0.3 * torch.randn(B, C, generator=g)).float()
    shift = (0.5 * torch.randn(B, C, generator=g)).float()
    shift[:, 3] = 0.0
    x[:, :, ::2, :, 3] = 0.0          # v = fma(0, scale, 0): exact zeros in the pre-activation
    return x, scale, shift


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 32), (1, 1, 3, 3, 8)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("bare", [False, True], ids=["affine", "bare"])
def test_gn_leaky_apply(shape, dtype, bare):
    from cvvae_amd import ops
    x, scale, shift = _apply_case(shape, dtype, 7)
    x64 = x.double()
    if bare:
        v, mag, tabs = x64, x64.abs(), None
    else:
        sc, sh = scale.double()[:, None, None, None, :], shift.double()[:, None, None, None, :]
        v, mag, tabs = x64 * sc + sh, (x64 * sc).abs() + sh.abs(), (scale.cuda(), shift.cuda())
    ref = torch.where(v > 0, v, SLOPE32 * v)
    bound = 2 * _ulp(mag, torch.float32)
    if dtype != torch.float32:
        bound = bound + 0.5 * _ulp(ref.abs() + bound, dtype)
    xd = x.cuda()
    y = ops.gn_leaky_apply(xd, tabs, SLOPE)
    assert y.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), x)    # out of place leaves x alone
    assert torch.equal(y, ops.gn_leaky_apply(xd, tabs, SLOPE))
    err = (y.cpu().double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n[disc gn_leaky_apply] {shape} {dtype} {'bare' if bare else 'affine'}: worst |err| / bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst
    zeros = v == 0
    assert int(zeros.sum()) > 0 and bool((y.cpu()[zeros] == 0).all())    # exact zeros stay zero
    xin = xd.clone()
    assert ops.gn_leaky_apply(xin, tabs, SLOPE, out=xin) is xin and torch.equal(xin, y)    # in place: the same bits


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 32), (1, 1, 3, 3, 8), (3, 7, 11)], ids=lambda s: "x".join(map(str, s)))
def test_leaky_bwd_is_bit_equal(shape, dtype):
    """(3, 7, 11): 231 elements, not a multiple of 8 -- the last group goes element by element"""
    from cvvae_amd import ops
    y = _randn(shape, 21, dtype)
    y.view(-1)[::5] = 0.0                                                 # y == 0: the gradient is slope * gy there
    gy = _randn(shape, 22, dtype)
    want = torch.where(y > 0, gy.float(), SLOPE * gy.float()).to(dtype)
    assert torch.equal(want.view(-1)[::5], (SLOPE * gy.float()).to(dtype).view(-1)[::5])
    yd, gd = y.cuda(), gy.cuda()
    gv = ops.leaky_bwd(yd, gd, SLOPE)
    assert torch.equal(gv.cpu(), want) and torch.equal(gd.cpu(), gy)
    assert torch.equal(gv, ops.leaky_bwd(yd, gd, SLOPE))
    gin = gd.clone()
    assert ops.leaky_bwd(yd, gin, SLOPE, out=gin) is gin and torch.equal(gin, gv)           # gv == gy


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref).norm() / ref.norm())


def _bands_hold(figures):
    """figures: [(key, new, base)].  Print them all, then hold each new figure to 1.5x the old path's and to the recorded band"""
    for key, new, base in figures:
        print(f"\n[disc band] {key}: new {new:.6e} base {base:.6e}")
    bands = json.load(open(BANDS)) if os.path.isfile(BANDS) else {}
    missed = []
    for key, new, base in figures:
        if not (new == new and new <= 1.5 * base):
            missed.append(f"{key}: new {new:.3e} > 1.5 x base {base:.3e}")
        if key + "_band" not in bands:
            missed.append(f"no recorded band for {key} (measured {new:.3e})")
        elif not new <= bands[key + "_band"]:
            missed.append(f"{key}: measured {new:.3e}, band {bands[key + '_band']:.3e}")
    assert not missed, missed


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_group_norm_leaky_end_to_end(dtype):
    """[1,5,8,8,64] with 32 groups (two channels per group: the discriminator's Normalize(64)), forward, dx, dweight, dbias"""
    from cvvae_amd import disc_ops, ops
    shape, G, eps = (1, 5, 8, 8, 64), 32, 1e-6
    C = shape[-1]
    x = (1.5 * _randn(shape, 31, dtype).float() + 0.4).to(dtype)
    w = (1.0 + 0.2 * _randn((C,), 32, torch.float32))
    b = 0.3 * _randn((C,), 33, torch.float32)
    cot = _randn(shape, 34, dtype)
    # fp64 yardstick
    xr = _ncdhw64(x).requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = F.leaky_relu(F.group_norm(xr, G, wr, br, eps), SLOPE32)
    (yr * _ncdhw64(cot)).sum().backward()
    ref = dict(y=yr.detach().permute(0, 2, 3, 4, 1), dx=xr.grad.permute(0, 2, 3, 4, 1), dw=wr.grad, db=br.grad)
    # the new path
    xa = x.cuda().requires_grad_(True)
    wa, ba = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    ya = disc_ops.group_norm_leaky(xa, wa, ba, num_groups=G, eps=eps, slope=SLOPE)
    ya.backward(cot.cuda())
    new = dict(y=ya, dx=xa.grad, dw=wa.grad, db=ba.grad)
    assert ya.dtype == dtype and xa.grad.dtype == dtype and wa.grad.dtype == torch.float32 and wa.grad.shape == (C,)
    # the same function from the launches that existed before: GroupNorm-apply without SiLU, torch's leaky_relu, GroupNorm backward
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    v = ops.gn_silu_apply(xd, ops.gn_stats(xd, wd, bd, eps, groups=G), silu=False).detach().requires_grad_(True)
    yb = F.leaky_relu(v, SLOPE)
    yb.backward(cot.cuda())
    unit = ops.gn_stats(xd, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), eps, groups=G)
    gxb, dwb, dbb = ops.gn_bwd_input_params(xd, v.grad, unit, wd, bd, silu=False, groups=G)
    base = dict(y=yb, dx=gxb, dw=dwb, db=dbb)
    name = str(dtype)[6:]
    _bands_hold([(f"gnl_1x5x8x8x64_g32_{name}_{k}", _rel(new[k], ref[k]), _rel(base[k], ref[k])) for k in ("y", "dx", "dw", "db")])
    # the same bits on every run
    xa2 = x.cuda().requires_grad_(True)
    wa2, ba2 = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    ya2 = disc_ops.group_norm_leaky(xa2, wa2, ba2, num_groups=G, eps=eps, slope=SLOPE)
    ya2.backward(cot.cuda())
    assert torch.equal(ya2, ya) and torch.equal(xa2.grad, xa.grad) and torch.equal(wa2.grad, wa.grad) and torch.equal(ba2.grad, ba.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_bare_group_norm_leaky_is_the_leaky_relu(dtype):
    from cvvae_amd import disc_ops
    x = _randn((1, 2, 3, 3, 8), 41, dtype)
    x.view(-1)[::4] = 0.0
    cot = _randn(tuple(x.shape), 42, dtype)
    xa = x.cuda().requires_grad_(True)
    ya = disc_ops.group_norm_leaky(xa)
    ya.backward(cot.cuda())
    assert torch.equal(ya.detach().cpu(), torch.where(x > 0, x.float(), SLOPE * x.float()).to(dtype))
    assert torch.equal(xa.grad.cpu(), torch.where(x > 0, cot.float(), SLOPE * cot.float()).to(dtype))
