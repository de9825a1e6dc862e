"""LPIPS on a real MI355X: every new C-ABI entry (include/cvvae.h ABI 14) against its torch formula evaluated in fp64 on the
CPU, and the whole module (cvvae_amd/lpips.py), forward and input gradient, against the fp64 restatement of the reference's
LPIPS.forward (tests/lpips_ref.py) on seeded weights.

Per-kernel bounds come from the number formats alone: every kernel computes in fp32 and rounds ONCE to the storage dtype, so
an element is within half an ulp of the storage type (2^-9 relative for bf16, 2^-12 for fp16 -- half the subnormal spacing, 2^-25,
for fp16 values below 6.1e-5: _round_bound; relative L2 norms a little below that) plus fp32 rounding noise of the arithmetic
(a few 1e-7 per operation); selections (ReLU, max pooling, the routing of the pooled gradient) are exact.

Whole-path bounds for 16-bit modules are not fixed numbers: the same test runs the restatement itself in that dtype with torch on
the CPU and measures ITS error against fp64; the HIP path must stay within 1.5x of it (the project's rule: the reference's own
16-bit noise at the same shapes, 1.5x for seed-to-seed spread).  fp32 modules: within 1.5x of the figures measured on the first GPU
run (tests/golden/lpips_bands.json) AND below a tenth of the fp16 CPU-noise figure of the same case."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from oracle.seeded import seeded_input
from tests import lpips_ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# relative L2 bound of a tensor rounded once to the storage dtype (half an ulp worst case per element), fp32: arithmetic noise
ROUND_L2 = {torch.float32: 2e-6, torch.float16: 2.0 ** -12, torch.bfloat16: 2.0 ** -9}
BANDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_bands.json")


def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


def _round_bound(ref, dtype):
    """relative L2 bound of `ref` rounded once to `dtype`: per element half an ulp, i.e. 2^-(p+1) |x| in the normal range and half the
    subnormal spacing below it (fp16: 2^-25 -- gradients of a spatial mean are often below fp16's smallest normal 6.1e-5), plus
    1e-5 for the fp32 arithmetic in front of the rounding"""
    u, tiny = {torch.float32: (2.0 ** -24, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25), torch.bfloat16: (2.0 ** -8, 0.0)}[dtype]
    r = ref.double().abs()
    return float(torch.maximum(u * r, torch.full_like(r, tiny)).norm() / r.norm()) + 1e-5


def _rand(shape, seed, dtype):
    return seeded_input(shape, seed).to(dtype)


# ------------------------------------------------------------------------------------------------------------
# per-kernel
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", DTYPES)
@pytest.mark.parametrize("dst", DTYPES)
def test_scale_in_and_its_adjoint(src, dst):
    from cvvae_amd import ops
    N, H, W = 3, 7, 9
    x = _rand((N, 3, H, W), 1, src)
    shift, scale = torch.tensor(lpips_ref.SHIFT), torch.tensor(lpips_ref.SCALE)
    y = ops.lpips_scale_in(x.cuda(), shift.cuda(), scale.cuda(), 32, dst)
    ref = ((x.double() - shift.double().view(1, 3, 1, 1)) / scale.double().view(1, 3, 1, 1)).permute(0, 2, 3, 1)
    assert tuple(y.shape) == (N, H, W, 32) and y.dtype == dst
    assert _rel(y[..., :3], ref) < ROUND_L2[dst] and float(y[..., 3:].abs().max()) == 0.0
    g = _rand((N, H, W, 8), 2, dst)
    gx = ops.lpips_scale_in_bwd(g.cuda(), scale.cuda(), src)
    gref = (g.double()[..., :3] / scale.double()).permute(0, 3, 1, 2)
    assert tuple(gx.shape) == (N, 3, H, W) and gx.dtype == src and _rel(gx, gref) < ROUND_L2[src]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_relu_and_maxpool_are_exact(dtype, C):
    from cvvae_amd import ops
    N, H, W = 3, 7, 9  # odd extents; N*H*W*C/8 is not a multiple of 256
    x = _rand((1, N, H, W, C), C, dtype)
    y = ops.relu_(x.cuda().clone())
    assert torch.equal(y.cpu(), torch.relu(x.float()).to(dtype))
    p = ops.maxpool2x2(x.cuda())
    ref = F.max_pool2d(x[0].float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).to(dtype)
    assert tuple(p.shape) == (1, N, H // 2, W // 2, C) and torch.equal(p[0].cpu(), ref)


def _pool_bwd_ref(y, g_tap, g_pool):
    """(g_tap + max_pool2d's backward of g_pool on the SAME stored values) * (y > 0): fp32 sum, one rounding"""
    g = torch.zeros(y.shape, dtype=torch.float32) if g_tap is None else g_tap.float()
    if g_pool is not None:
        t = y.permute(0, 3, 1, 2).clone().requires_grad_(True)  # the storage dtype itself: ATen routes ties to the first maximum
        with torch.enable_grad():
            F.max_pool2d(t, 2, 2).backward(g_pool.permute(0, 3, 1, 2).contiguous())
        g = g + t.grad.float().permute(0, 2, 3, 1)
    return (g * (y.float() > 0)).to(y.dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("shape", [(3, 7, 9, 64), (2, 8, 6, 128), (1, 5, 5, 256), (2, 4, 7, 512)])
def test_relu_pool_bwd_routes_ties_as_aten(dtype, shape):
    from cvvae_amd import ops
    N, H, W, C = shape
    # values on a coarse grid: most 2x2 windows hold equal maxima (and many zeros, as a ReLU output does)
    y = torch.relu(torch.round(seeded_input(shape, 3) * 2) / 2).to(dtype)
    ties = F.max_pool2d(y.float().permute(0, 3, 1, 2), 2, 2)
    assert float((F.unfold(y.float().permute(0, 3, 1, 2).reshape(N * C, 1, H, W), 2, stride=2) ==
                  ties.reshape(N * C, 1, -1)).sum(1).float().mean()) > 1.5  # on average more than one maximum per window
    gt, gp = _rand(shape, 4, dtype), _rand((N, H // 2, W // 2, C), 5, dtype)
    for a, b in ((gt, gp), (None, gp), (gt, None)):
        got = ops.relu_pool_bwd(y.cuda(), a.cuda() if a is not None else None, b.cuda() if b is not None else None)
        assert torch.equal(got.cpu(), _pool_bwd_ref(y, a, b)), (a is None, b is None)


def _head_ref(f0, f1, w):
    def nrm(f):
        return f / (torch.sqrt((f * f).sum(-1, keepdim=True) + 1e-10) + 1e-10)
    d = ((nrm(f0) - nrm(f1)) ** 2 * w).sum(-1)
    return d.reshape(d.shape[0], -1).mean(1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,H,W", [(64, 7, 9), (128, 13, 11), (256, 5, 5), (512, 3, 3), (512, 9, 7)])
def test_lpips_head_forward_and_backward(dtype, C, H, W):
    from cvvae_amd import ops
    N = 3
    f0 = torch.relu(_rand((N, H, W, C), 6, torch.float32) * 3).to(dtype)
    f1 = torch.relu(_rand((N, H, W, C), 7, torch.float32) * 3 + 0.2).to(dtype)
    f0[0, 0, 0] = 0  # an all-zero feature vector: m = 1e-5 + 1e-10
    w = _rand((C,), 8, torch.float32).abs()
    gout = 0.5 + _rand((N,), 9, torch.float32).abs()
    a, b = f0.double().requires_grad_(True), f1.double().requires_grad_(True)
    ref = _head_ref(a, b, w.double())
    (ref * gout.double()).sum().backward()
    d0, d1, dw = f0.cuda(), f1.cuda(), w.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((N,), 0.25, dtype=torch.float32, device="cuda")  # accumulates: out += level
        ops.lpips_head(d0, d1, dw, out)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    assert _rel(outs[0] - 0.25, ref.detach()) < 1e-5  # fp32 arithmetic on exactly representable inputs
    grads = []
    for _ in range(2):
        g0, g1 = torch.empty_like(d0), torch.empty_like(d1)
        ops.lpips_head_bwd(d0, d1, dw, gout.cuda(), g0, g1)
        grads.append((g0.cpu(), g1.cpu()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert _rel(grads[0][0], a.grad) < _round_bound(a.grad, dtype) and _rel(grads[0][1], b.grad) < _round_bound(b.grad, dtype)
    only0, only1 = torch.full_like(d0, 7.0), torch.full_like(d1, 7.0)
    ops.lpips_head_bwd(d0, d1, dw, gout.cuda(), only0, None)
    ops.lpips_head_bwd(d0, d1, dw, gout.cuda(), None, only1)
    assert torch.equal(only0.cpu(), grads[0][0]) and torch.equal(only1.cpu(), grads[0][1])


# ------------------------------------------------------------------------------------------------------------
# whole path
# ------------------------------------------------------------------------------------------------------------
def _module(dtype, seed=3):
    from cvvae_amd.lpips import LPIPS
    m = LPIPS().eval()
    m.load_state_dict(lpips_ref.lpips_state_dict(seed), strict=True)
    m = m.to(dtype)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}  # what the module holds (rounded to its dtype), on the CPU
    return m.cuda(), sd


def _images(shape, seed, dtype):
    """two images in [-1, 1] whose values the module's dtype holds exactly: every evaluation sees the same inputs"""
    x0 = seeded_input(shape, seed)
    x1 = (x0 + 0.3 * seeded_input(shape, seed + 1)).clamp(-1, 1)
    return x0.to(dtype).float(), x1.to(dtype).float()


def _ref64(x0, x1, sd, cot, wrt, chunk=4):
    """the fp64 restatement (frames are independent: evaluated `chunk` pairs at a time to bound the autograd tape)"""
    vals, g0, g1 = [], [], []
    for i in range(0, x0.shape[0], chunk):
        v, a, b = lpips_ref.lpips_with_grads(x0[i:i + chunk], x1[i:i + chunk], sd, cot[i:i + chunk], torch.float64, wrt)
        vals.append(v), g0.append(a), g1.append(b)
    return torch.cat(vals), (torch.cat(g0) if wrt[0] else None), (torch.cat(g1) if wrt[1] else None)


def _errors(val, grads, ref, refgrads):
    e = {"value": float((val.double() - ref).abs().max() / ref.abs().max())}
    for name, g, r in zip(("grad_input", "grad_target"), grads, refgrads):
        if r is not None:
            e[name] = float((g.double() - r).norm() / r.norm())
    return e


def measure(dtype, shape, wrt=(False, True), seed=5, noise_dtype=None):
    """-> (errors of the HIP module, errors of the CPU restatement evaluated in noise_dtype), both against the fp64 restatement"""
    m, sd = _module(dtype)
    x0, x1 = _images(shape, seed, dtype)
    cot = 0.5 + seeded_input((shape[0], 1, 1, 1), seed + 2).abs()
    ref, r0, r1 = _ref64(x0, x1, sd, cot, wrt)
    a, b = x0.cuda().requires_grad_(wrt[0]), x1.cuda().requires_grad_(wrt[1])
    val = m(a, b)
    assert tuple(val.shape) == (shape[0], 1, 1, 1) and val.dtype == dtype
    (val.float() * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    hip = _errors(val.detach().cpu(), (a.grad.cpu() if wrt[0] else None, b.grad.cpu() if wrt[1] else None), ref, (r0, r1))
    noise = None
    if noise_dtype is not None:
        nsd = {k: v.to(noise_dtype) for k, v in sd.items()}
        nv, n0, n1 = lpips_ref.lpips_with_grads(x0, x1, nsd, cot, noise_dtype, wrt)
        noise = _errors(nv, (n0, n1), ref, (r0, r1))
        assert all(v == v and v < float("inf") for v in noise.values()), noise  # the yardstick itself must be finite
    return hip, noise


SHAPES = [(5, 3, 64, 64), (5, 3, 80, 48), (5, 3, 50, 50)]


def _key(shape, wrt):
    return "x".join(map(str, shape)) + "_" + "".join("yn"[not w] for w in wrt)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_whole_path_16bit_within_the_references_own_noise(dtype, shape):
    hip, noise = measure(dtype, shape, noise_dtype=dtype)
    print(f"\nLPIPS {str(dtype)[6:]} {shape}: HIP {hip}  CPU {str(dtype)[6:]} restatement {noise}")
    for k in hip:
        assert hip[k] <= 1.5 * noise[k], (k, hip[k], noise[k])


@pytest.mark.parametrize("shape", SHAPES)
def test_whole_path_fp32(shape):
    hip, noise = measure(torch.float32, shape, noise_dtype=torch.float16)
    band = json.load(open(BANDS))["fp32"][_key(shape, (False, True))]
    print(f"\nLPIPS float32 {shape}: HIP {hip}  recorded {band}  CPU float16 restatement {noise}")
    for k in hip:
        assert hip[k] <= 1.5 * band[k], (k, hip[k], band[k])
        assert hip[k] < 0.1 * noise[k], (k, hip[k], noise[k])


@pytest.mark.parametrize("wrt", [(True, False), (True, True)])
def test_gradient_into_input_and_into_both(wrt):
    hip, noise = measure(torch.bfloat16, (5, 3, 64, 64), wrt=wrt, noise_dtype=torch.bfloat16)
    print(f"\nLPIPS bfloat16 wrt {wrt}: HIP {hip}  CPU bfloat16 restatement {noise}")
    assert set(hip) == {"value"} | {n for n, w in zip(("grad_input", "grad_target"), wrt) if w}
    for k in hip:
        assert hip[k] <= 1.5 * noise[k], (k, hip[k], noise[k])


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_grad_forward_is_bit_equal_to_the_taped_forward(dtype):
    m, _ = _module(dtype)
    x0, x1 = _images((3, 3, 50, 50), 9, dtype)
    a, b = x0.cuda(), x1.cuda()
    with torch.no_grad():
        plain = m(a, b.clone().requires_grad_(True))
    taped = m(a, b.clone().requires_grad_(True))
    assert plain.grad_fn is None and taped.grad_fn is not None
    assert torch.equal(plain, taped.detach()) and torch.equal(plain, m(a, b))


def test_training_sized_call_bf16():
    """2N = 34 frames of 256x256 (one training step's `perceptual_loss(inputs, reconstructions)` with gradient into the
    reconstructions).  The CPU runs of the restatement at this very shape (bf16, and fp64 in chunks) take about a minute."""
    shape = (17, 3, 256, 256)
    hip, noise = measure(torch.bfloat16, shape, noise_dtype=torch.bfloat16)
    print(f"\nLPIPS bfloat16 {shape}: HIP {hip}  CPU bfloat16 restatement {noise}")
    assert all(v == v and v < float("inf") for v in hip.values())
    assert hip["grad_target"] <= 1.5 * noise["grad_target"], (hip, noise)
    assert hip["value"] <= 1.5 * noise["value"], (hip, noise)
