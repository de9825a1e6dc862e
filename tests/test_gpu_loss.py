"""The training-loss kernels (csrc/loss_kernels.hip) and modules (cvvae_amd/loss.py) on a real MI355X, against fp64 on the CPU.

Exact where the arithmetic is one fp32 operation rounded once: the gradients of ABS_DIFF / IDENT / the hinges are
`coef * {-1, 0, 1}` and must equal torch's `(coef * sign).to(dtype)` bit for bit; masks and selections are exact; every launch
repeated on the same inputs must return the same bits, and so must a strided view and its contiguous copy.

Banded where fp32 sums or exp are involved (sums, z, SOFTPLUS_*, SQ_DIFF / SQ gradients, d logvar, the whole loss in fp32):
tests/golden/loss_bands.json holds the error measured on the MI355X against the fp64 yardstick; the test allows 1.5x that (the
project's convention for fp32 bands: the margin covers box-to-box compiler differences only; the summation order is fixed, so a
recorded 0 stays 0).  16-bit elementwise outputs (z, g_moments, the SQ / SQ_DIFF / SOFTPLUS gradients) are NOT banded: they are one
rounding of an fp32 result and are held to the format's half ulp (HALF_ULP per element, ROUND_L2 over a tensor), bounds fixed by
choice from the number formats, not measured.  16-bit whole-loss runs are held to 1.5x the
error of the restatement itself evaluated in that dtype on the CPU, as tests/test_gpu_lpips.py does.
Every figure is printed before it is asserted (`pytest -s` shows the `[loss band] key: value` lines the band file is made from)."""
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.seeded import seeded_input, seeded_state_dict
from tests import loss_ref, lpips_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = os.path.join(ROOT, "tests", "golden", "loss_bands.json")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# one rounding of an fp32 result to a 16-bit dtype, per element: half a unit in the last place, relative (fp16 has 11 significant
# bits, bf16 8), plus 1e-6 for the fp32 arithmetic in front of it.  Over a tensor the relative L2 norm of such errors is bounded by
# half of that again in practice (ROUND_L2, as tests/test_gpu_lpips.py).  These 16-bit bounds are fixed by the formats, not measured.
HALF_ULP = {torch.float16: 2.0 ** -11 + 1e-6, torch.bfloat16: 2.0 ** -8 + 1e-6}
ROUND_L2 = {torch.float16: 2.0 ** -12, torch.bfloat16: 2.0 ** -9}
SPAN = 256 * 8            # elements of one workgroup pass
GRID_SPAN = 2048 * SPAN   # elements of one pass of the whole (capped) stage-1 grid


_MISSED = []


def _band(key, err):
    """print `err`, then hold it to 1.5x the recorded figure.  A miss is noted and raised when the
    test ends (_bands_hold), so that one run prints every figure of a test"""
    print(f"\n[loss band] {key}: {err:.6e}")
    bands = json.load(open(BANDS)) if os.path.isfile(BANDS) else {}
    if key not in bands:
        _MISSED.append(f"no recorded band for {key} (measured {err:.3e})")
    elif not (err == err and err <= 1.5 * bands[key]):
        _MISSED.append(f"{key}: measured {err:.3e}, recorded {bands[key]:.3e}")


@pytest.fixture(autouse=True)
def _bands_hold():
    _MISSED.clear()
    yield
    assert not _MISSED, _MISSED


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    n = float(ref.norm())
    return float((got - ref).norm()) / n if n > 0 else float(got.norm())


def _ops():
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    return L, ops


def _term64(L, op, a, b):
    return {L.RED_ABS_DIFF: lambda: (a - b).abs(), L.RED_SQ_DIFF: lambda: (a - b) ** 2, L.RED_SQ: lambda: a * a,
            L.RED_IDENT: lambda: a, L.RED_HINGE_NEG: lambda: F.relu(1.0 - a), L.RED_HINGE_POS: lambda: F.relu(1.0 + a),
            L.RED_SOFTPLUS_NEG: lambda: F.softplus(-a), L.RED_SOFTPLUS_POS: lambda: F.softplus(a)}[op]()


def _twice(fn):
    """run a launch twice on the same inputs: identical bits"""
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert (x is None and y is None) or torch.equal(x, y), "not reproducible"
    return a


# ------------------------------------------------------------------------------------------------------------
# cvvae_reduce_sum / _bwd
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, SPAN - 1, SPAN, SPAN + 1, GRID_SPAN + 1])
def test_reduce_sum_element_counts(n):
    L, ops = _ops()
    a, b = seeded_input((n,), 1), seeded_input((n,), 2)
    got = _twice(lambda: ops.reduce_sum(L.RED_ABS_DIFF, a.cuda(), b.cuda()))
    assert got.dtype == torch.float32 and got.dim() == 0
    _band(f"sum_abs_diff_n{n}", _rel(got, (a.double() - b.double()).abs().sum()))
    if n <= SPAN + 1:
        coef = torch.tensor(0.37, device="cuda")
        ga, gb = _twice(lambda: ops.reduce_sum_bwd(L.RED_ABS_DIFF, a.cuda(), b.cuda(), coef, True, True))
        want = 0.37 * torch.sign(a - b)
        assert torch.equal(ga.cpu(), torch.tensor(0.37) * torch.sign(a - b)) and torch.equal(gb.cpu(), -want)


def test_inner_run_not_a_multiple_of_8_and_misaligned_base_give_the_bits_of_the_contiguous_copy():
    L, ops = _ops()
    big = seeded_input((3, 5, 16), 3).cuda()
    other = seeded_input((3 * 5 * 13 + 1,), 4).cuda()
    view = big[..., :13]                       # runs of 13 elements
    off = other[1:].view(3, 5, 13)             # base 4 bytes past a 16-byte boundary
    assert not view.is_contiguous() and off.data_ptr() % 16 == 4
    ref = (view.double().cpu() - off.double().cpu()).abs().sum()
    got = _twice(lambda: ops.reduce_sum(L.RED_ABS_DIFF, view, off))
    assert torch.equal(got, ops.reduce_sum(L.RED_ABS_DIFF, view.contiguous(), off.clone()))
    _band("sum_abs_diff_runs_of_13_misaligned", _rel(got, ref))
    coef = torch.tensor(-1.25, device="cuda")
    ga, gb = ops.reduce_sum_bwd(L.RED_ABS_DIFF, view, off, coef, True, True)
    want = (-1.25 * torch.sign(view - off)).cpu()
    assert ga.is_contiguous() and torch.equal(ga.cpu(), want) and torch.equal(gb.cpu(), -want)
    # 16-bit operand at an odd element offset
    h = seeded_input((4099,), 5).to(torch.bfloat16).cuda()
    assert torch.equal(ops.reduce_sum(L.RED_SQ, h[3:]), ops.reduce_sum(L.RED_SQ, h[3:].clone()))


def test_strided_frame_view_is_read_in_place_bit_equal_to_its_copy():
    L, ops = _ops()
    clip = seeded_input((2, 3, 9, 16, 16), 6).cuda()
    rec2d = (clip[:, :, ::4] + 0.25 * seeded_input((2, 3, 3, 16, 16), 7).cuda()).to(torch.bfloat16)
    view = clip[:, :, ::4]
    assert not view.is_contiguous()
    for op in (L.RED_ABS_DIFF, L.RED_SQ_DIFF):
        got = _twice(lambda: ops.reduce_sum(op, rec2d, view))
        assert torch.equal(got, ops.reduce_sum(op, rec2d, view.contiguous()))
        ref = _term64(L, op, rec2d.double().cpu(), view.double().cpu()).sum()
        _band(f"sum_op{op}_frame_slice_bf16_f32", _rel(got, ref))
        coef = torch.tensor(0.5, device="cuda")
        g1 = ops.reduce_sum_bwd(op, rec2d, view, coef, True, True)
        g2 = ops.reduce_sum_bwd(op, rec2d, view.contiguous(), coef, True, True)
        assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1]) and g1[1].shape == view.shape and g1[1].is_contiguous()


@pytest.mark.parametrize("da", DTYPES)
@pytest.mark.parametrize("db", DTYPES)
def test_abs_diff_every_dtype_pair(da, db):
    L, ops = _ops()
    n = 3 * SPAN + 5
    a = seeded_input((n,), 8)
    a[::7] = torch.round(a[::7] * 64) / 64  # multiples of 1/64 below 1: exact in all three dtypes ...
    a = a.to(da)
    b = (a.float() + 0.5 * seeded_input((n,), 9)).to(db)
    b[::7] = a[::7].to(db)                  # ... so a - b is exactly 0 there for every pair
    d = a.float() - b.float()
    assert int((d == 0).sum()) > 0
    got = _twice(lambda: ops.reduce_sum(L.RED_ABS_DIFF, a.cuda(), b.cuda()))
    _band(f"sum_abs_diff_{str(da)[6:]}_{str(db)[6:]}", _rel(got, (a.double() - b.double()).abs().sum()))
    coef = torch.tensor(0.0123, device="cuda")
    ga, gb = _twice(lambda: ops.reduce_sum_bwd(L.RED_ABS_DIFF, a.cuda(), b.cuda(), coef, True, True))
    want = torch.tensor(0.0123) * torch.sign(d)
    assert ga.dtype == da and gb.dtype == db
    assert torch.equal(ga.cpu(), want.to(da)) and torch.equal(gb.cpu(), (-want).to(db))
    only_b = ops.reduce_sum_bwd(L.RED_ABS_DIFF, a.cuda(), b.cuda(), coef, False, True)
    assert only_b[0] is None and torch.equal(only_b[1], gb)


@pytest.mark.parametrize("op", range(8))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_op_forward_and_adjoint(op, dtype):
    L, ops = _ops()
    n = 2 * SPAN + 77
    a = (2.5 * seeded_input((n,), 10 + op)).to(dtype)
    a[:6] = torch.tensor([1.0, -1.0, 0.0, 25.0, -25.0, 1.0]).to(dtype)  # logits exactly at the hinges' kinks, softplus past its threshold
    two = op in ops.TWO_OPERAND_OPS
    b = (a.float() + seeded_input((n,), 30)).to(dtype) if two else None
    if two:
        b[:4] = a[:4]
    a64 = a.double().requires_grad_(True)
    ref = _term64(L, op, a64, b.double() if two else None).sum()
    (gref,) = torch.autograd.grad(0.75 * ref, a64)
    got = _twice(lambda: ops.reduce_sum(op, a.cuda(), b.cuda() if two else None))
    _band(f"sum_op{op}_{str(dtype)[6:]}", _rel(got, ref))
    coef = torch.tensor(0.75, device="cuda")
    ga, gb = _twice(lambda: ops.reduce_sum_bwd(op, a.cuda(), b.cuda() if two else None, coef, True, two))
    if op in (L.RED_ABS_DIFF, L.RED_IDENT, L.RED_HINGE_NEG, L.RED_HINGE_POS):
        f = a.float()
        sign = {L.RED_ABS_DIFF: lambda: torch.sign(f - b.float()), L.RED_IDENT: lambda: torch.ones_like(f),
                L.RED_HINGE_NEG: lambda: -((1.0 - f) > 0).float(), L.RED_HINGE_POS: lambda: ((1.0 + f) > 0).float()}[op]()
        assert torch.equal(ga.cpu(), (torch.tensor(0.75) * sign).to(dtype))
    else:
        err = _rel(ga, gref)
        if dtype == torch.float32:
            _band(f"grad_op{op}_float32", err)
        else:  # one rounding to bf16 (half an ulp = 2^-9 relative per element) on top of the fp32 arithmetic
            print(f"\n[loss] grad op {op} bf16 rel {err:.3e}")
            assert err <= ROUND_L2[dtype]
    if two:
        assert torch.equal(gb, -ga)


def test_logical_index_past_2_to_the_31():
    """a broadcast row (stride 0): 2^31 + 4096 logical elements over 16 KiB of memory; every index is 64-bit"""
    L, ops = _ops()
    rows, run = (1 << 19) + 1, 4096
    row = seeded_input((run,), 12).abs() + 0.5
    a = row.cuda().view(1, run).expand(rows, run)
    assert a.numel() > 2 ** 31
    got = _twice(lambda: ops.reduce_sum(L.RED_IDENT, a))
    _band("sum_ident_2p31_broadcast", _rel(got, row.double().sum() * rows))


# ------------------------------------------------------------------------------------------------------------
# cvvae_gauss_reg / _bwd
# ------------------------------------------------------------------------------------------------------------
def _moments(shape, dtype, seed, ends=(-31.0, -30.0)):
    """moments whose first raw logvars sit outside and exactly on an end of the clamp.  The lower end goes into every banded figure;
    the upper end (exp(20) = 4.9e8 would drown every other term of a sum) is compared on its own: kl, and z / d mean / d logvar
    element by element at the two positions."""
    m = (1.5 * seeded_input(shape, seed)).to(dtype)
    C = shape[1] // 2
    flat = m.view(shape[0], shape[1], -1)
    flat[0, C, :2] = torch.tensor(ends).to(dtype)
    return m


def _gauss64(m, noise, g_z, coef):
    p = m.double().requires_grad_(True)
    z, kl_loss = loss_ref.gauss_reg_ref(p, noise)
    kl_sum = kl_loss * m.shape[0]
    obj = coef * kl_sum + ((z * g_z.double()).sum() if g_z is not None else 0.0)
    (g,) = torch.autograd.grad(obj, p)
    return z.detach(), kl_sum.detach(), g


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 6, 1, 5, 5), (1, 32, 2, 4, 4), (3, 8, 33, 31)], ids=["cs75", "cs512", "4d_odd"])
@pytest.mark.parametrize("sample", [True, False])
def test_gauss_reg_forward_and_adjoint(dtype, shape, sample):
    L, ops = _ops()
    m = _moments(shape, dtype, 20)
    zshape = (shape[0], shape[1] // 2, *shape[2:])
    noise = seeded_input(zshape, 21).to(dtype) if sample else None
    g_z = seeded_input(zshape, 22).to(dtype)
    key = f"gauss_{'x'.join(map(str, shape))}_{str(dtype)[6:]}_{'sample' if sample else 'mode'}"
    md, nd = m.cuda(), (noise.cuda() if sample else None)
    z, kl = _twice(lambda: ops.gauss_reg(md, nd))
    z64, kl64, g64 = _gauss64(m, noise, g_z, 0.3)
    assert z.shape == zshape and z.dtype == dtype and kl.dtype == torch.float32 and kl.dim() == 0
    _band(key + "_kl", _rel(kl, kl64))
    if not sample:
        assert torch.equal(z.cpu(), m[:, :shape[1] // 2])
    elif dtype == torch.float32:
        _band(key + "_z", _rel(z, z64))
    else:  # one rounding of an fp32 result: half an ulp per element
        assert _rel(z, z64) <= ROUND_L2[dtype]
    coef = torch.tensor(0.3, device="cuda")
    g = _twice(lambda: ops.gauss_reg_bwd(md, nd, g_z.cuda(), coef))
    C = shape[1] // 2
    assert g.shape == m.shape and g.dtype == dtype
    # clamp's inclusive mask: raw logvar -31 / 21 get exactly 0, -30 / 20 do not
    gl = g.view(shape[0], shape[1], -1)[0, C, :2].float().cpu()
    mh = _moments(shape, dtype, 20, (20.0, 21.0))
    hi = ops.gauss_reg_bwd(mh.cuda(), nd, g_z.cuda(), coef)
    gh = hi.view(shape[0], shape[1], -1)[0, C, :2].float().cpu()
    assert float(gl[0]) == 0.0 and float(gl[1]) != 0.0 and float(gh[0]) != 0.0 and float(gh[1]) == 0.0
    # the clamp's upper end against the yardstick: kl (its sum is then exp(20) twice: a clamp at another bound changes it by a
    # factor), and z, d mean and d logvar element by element at the two positions (raw logvar 20, and 21 which must act as 20)
    zh, klh = _twice(lambda: ops.gauss_reg(mh.cuda(), nd))
    zh64, klh64, gh64 = _gauss64(mh, noise, g_z, 0.3)
    _band(key + "_kl_upper", _rel(klh, klh64))

    def at(t, c0):
        return t.detach().reshape(shape[0], t.shape[1], -1)[0, c0, :2].double().cpu()

    def worst(got, ref):
        return float(((got - ref).abs() / ref.abs()).max())

    e_z, e_dm = worst(at(zh, 0), at(zh64, 0)), worst(at(hi, 0), at(gh64, 0))
    if not sample:
        assert e_z == 0.0
    if dtype == torch.float32:
        if sample:
            _band(key + "_z_upper", e_z)
        _band(key + "_dmean_upper", e_dm)
        _band(key + "_dlogvar_upper", worst(at(hi, C)[:1], at(gh64, C)[:1]))
    else:
        assert e_z <= HALF_ULP[dtype] and e_dm <= HALF_ULP[dtype], (e_z, e_dm)
        if dtype == torch.bfloat16:
            assert worst(at(hi, C)[:1], at(gh64, C)[:1]) <= HALF_ULP[dtype]
        else:  # coef 0.5 (exp(20) - 1) = 7.3e7 is past fp16's range: the rounding of the fp32 result is an infinity of its sign
            assert float(at(hi, C)[0]) == float("inf") * (1.0 if float(at(gh64, C)[0]) > 0 else -1.0)
    if dtype == torch.float32:
        _band(key + "_dmean", _rel(g[:, :C], g64[:, :C]))
        _band(key + "_dlogvar", _rel(g[:, C:], g64[:, C:]))
    else:
        assert _rel(g, g64) <= ROUND_L2[dtype]
    # only the KL term back-propagated: g_z = NULL
    gk = _twice(lambda: ops.gauss_reg_bwd(md, nd, None, coef))
    _, _, gk64 = _gauss64(m, noise, None, 0.3)
    if dtype == torch.float32:
        _band(key + "_kl_only", _rel(gk, gk64))
    else:
        assert _rel(gk, gk64) <= ROUND_L2[dtype]


# ------------------------------------------------------------------------------------------------------------
# the whole loss
# ------------------------------------------------------------------------------------------------------------
class Disc(nn.Module):
    """elementwise stand-in (no convolution): 5-D clip -> 5-D logits in [-1.5, 1.7], both hinge kinks inside the range.
    Its parameter gradients are sums over all logits, computed by torch in the clip's dtype.  The summands are kept of one sign
    (tanh^2, |x|): with summands of both signs those gradients are small differences of large sums, whose relative error in a 16-bit
    dtype is a random draw -- in the path under test and in the 16-bit yardstick alike -- and says nothing about either."""

    def __init__(self, dtype=torch.float32):
        super().__init__()
        self.gain = nn.Parameter(torch.tensor(1.7, dtype=dtype))
        self.bias = nn.Parameter(torch.tensor(-1.5, dtype=dtype))

    def forward(self, x):
        return self.gain.to(x.dtype) * torch.tanh(2.0 * x[:, :1]) ** 2 + self.bias.to(x.dtype) * x[:, 1:2].abs()


def _whole(dtype, optimizer_idx, device, ref_dtype=None):
    """one evaluation of LPIPSWithDiscriminatorAndDomainConstraint + the regulariser -> dict of 0-dim values and gradients.
    device "cuda": the modules under test; "cpu": the restatement in ref_dtype (fp64: the yardstick; a 16-bit dtype: its own noise).
    The glue that stands for the decoder (xhat from the `base` and `last` leaves and z) is not under test: it runs in fp32 with one
    cast to `dtype` in every path, so a 16-bit comparison holds the loss's own arithmetic against the restatement's, not two orders
    of torch's 16-bit sums in the glue's backward (the 3-element `last` gradient is a sum of 15360 terms of both signs)."""
    sd = {k: v.to(dtype).float() for k, v in lpips_ref.lpips_state_dict(3).items()}  # what a module of `dtype` holds
    x = seeded_input((1, 3, 5, 32, 32), 40)
    base = (x + 0.3 * seeded_input((1, 3, 5, 32, 32), 41)).clamp(-1, 1).to(dtype)
    x2 = (x[:, :, ::4] + 0.2 * seeded_input((1, 3, 2, 32, 32), 42)).clamp(-1, 1).to(dtype)
    mom = _moments((1, 32, 2, 4, 4), dtype, 43)
    noise = seeded_input((1, 16, 2, 4, 4), 44).to(dtype)
    feat = seeded_input((1, 3, 5, 32, 32), 45).to(dtype)
    last0 = torch.tensor([0.05, -0.04, 0.03])
    cfg = dict(disc_start=10, logvar_init=3.0, perceptual_weight=0.7, disc_factor=0.8, disc_weight=0.6, rec2d_weight=0.5)
    if device == "cuda":
        from cvvae_amd.loss import DiagonalGaussianRegularizer, LPIPSWithDiscriminatorAndDomainConstraint
        m = LPIPSWithDiscriminatorAndDomainConstraint(dims=3, learn_logvar=True, regularization_weights={"kl_loss": 1e-3},
                                                      discriminator=Disc(), **cfg)
        m.perceptual_loss.load_state_dict(lpips_ref.lpips_state_dict(3), strict=True)
        m.perceptual_loss.to(dtype)
        m = m.cuda().train()
        lv = {"base": base.float().cuda().requires_grad_(True), "xhat2d": x2.float().cuda().requires_grad_(True),
              "moments": mom.cuda().requires_grad_(True), "last": last0.cuda().requires_grad_(True)}
        z, rlog = DiagonalGaussianRegularizer()(lv["moments"], noise=noise.cuda())
        xhat = (lv["base"] + lv["last"].view(1, 3, 1, 1, 1) * feat.float().cuda() + 0.01 * z.float()[:, :3, :1, :1, :1]).to(dtype)
        loss, log = m(x.cuda(), xhat, lv["xhat2d"].to(dtype), regularization_log=rlog, optimizer_idx=optimizer_idx, global_step=20,
                      last_layer=lv["last"])
        loss.backward()
        torch.cuda.synchronize()
        params = {"logvar": m.logvar, "logvar_2d": m.logvar_2d, "disc.gain": m.discriminator.gain, "disc.bias": m.discriminator.bias}
    else:
        rd = ref_dtype
        gd = torch.float64 if rd == torch.float64 else torch.float32  # the glue's dtype
        lv = {"base": base.to(gd).requires_grad_(True), "xhat2d": x2.to(gd).requires_grad_(True),
              "moments": mom.to(rd).requires_grad_(True), "last": last0.to(gd).requires_grad_(True)}
        disc = Disc(rd)
        params = {"logvar": torch.tensor(3.0, dtype=rd, requires_grad=True), "logvar_2d": torch.tensor(3.0, dtype=rd, requires_grad=True),
                  "disc.gain": disc.gain, "disc.bias": disc.bias}
        z, kl = loss_ref.gauss_reg_ref(lv["moments"], noise, rd)
        xhat = (lv["base"] + lv["last"].view(1, 3, 1, 1, 1) * feat.to(gd) + 0.01 * z.to(gd)[:, :3, :1, :1, :1]).to(rd)
        loss, log = loss_ref.loss_ref(
            x.to(rd), xhat, lv["xhat2d"].to(rd), logvar=params["logvar"], logvar_2d=params["logvar_2d"], discriminator=disc,
            perceptual=lambda a, b: lpips_ref.lpips_forward(a, b, sd, rd), perceptual_weight=cfg["perceptual_weight"],
            disc_start=10, disc_factor=cfg["disc_factor"], disc_weight=cfg["disc_weight"], rec2d_weight=cfg["rec2d_weight"],
            regularization_weights={"kl_loss": 1e-3}, regularization_log={"kl_loss": kl}, optimizer_idx=optimizer_idx,
            global_step=20, last_layer=lv["last"], dtype=rd)
        loss.backward()
    out = {"loss": loss.detach(), **{"log:" + k: v.detach() for k, v in log.items()}}
    for n, t in {**lv, **params}.items():
        if t.grad is not None:
            out["grad:" + n] = t.grad
    return {k: v.detach().double().cpu() for k, v in out.items()}


_REF = {}


def _ref64(dtype, idx):
    """the fp64 yardstick, computed once per case and shared"""
    if (dtype, idx) not in _REF:
        _REF[(dtype, idx)] = _whole(dtype, idx, "cpu", torch.float64)
    return _REF[(dtype, idx)]


def _errs(got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return {k: _rel(got[k], ref[k]) for k in ref}


@pytest.mark.parametrize("idx", [0, 1], ids=["generator", "discriminator"])
def test_whole_loss_fp32(idx):
    e = _errs(_whole(torch.float32, idx, "cuda"), _ref64(torch.float32, idx))
    assert ("grad:base" in e) == (idx == 0) and "grad:disc.gain" in e
    for k, v in e.items():
        _band(f"whole_fp32_idx{idx}_{k}", v)


@pytest.mark.parametrize("idx", [0, 1], ids=["generator", "discriminator"])
def test_whole_loss_bf16_within_the_restatements_own_noise(idx):
    ref = _ref64(torch.bfloat16, idx)
    hip = _errs(_whole(torch.bfloat16, idx, "cuda"), ref)
    noise = _errs(_whole(torch.bfloat16, idx, "cpu", torch.bfloat16), ref)
    print(f"\n[loss] whole bf16 idx {idx}: HIP {hip}\n  CPU bf16 restatement {noise}")
    assert all(v == v and v < float("inf") for v in noise.values()), noise
    for k in hip:
        assert hip[k] <= 1.5 * noise[k], (k, hip[k], noise[k])


def test_adaptive_weight_probe_through_the_decoder_tail_node():
    """calculate_adaptive_weight's two torch.autograd.grad(..., retain_graph=True) calls run through the reduce nodes and the
    conv_out tail node of a real Decoder3D (cvvae_amd/grad3d.py), then the step's backward still fills every parameter; the
    weight equals the ratio formed from the same two probes taken by hand"""
    import cvvae_amd
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    from cvvae_amd.loss import GeneralLPIPSWithDiscriminator
    dtype = torch.bfloat16
    net = cvvae_amd.CVVAESD3Model(block_out_channels=[128, 256, 512], layers_per_block=1)
    net.load_state_dict(seeded_state_dict({k: v.shape for k, v in net.state_dict().items()}, 8), strict=True)
    dec = net.decoder.to(dtype).cuda().train()
    z = seeded_input((1, 16, 3, 8, 12), 13).to(dtype).cuda().requires_grad_(True)
    m = GeneralLPIPSWithDiscriminator(disc_start=0, dims=3, perceptual_weight=0.0, disc_weight=0.5, logvar_init=6.0,
                                      discriminator=Disc()).cuda().train()
    y = dec(z)
    x = (y.detach().float() + 0.2 * seeded_input(tuple(y.shape), 5).cuda()).contiguous()
    loss, log = m(x, y, regularization_log={}, optimizer_idx=0, global_step=1, last_layer=dec.get_last_layer())
    n = y.shape[0] * y.shape[2]
    gy = (torch.sign(y.detach().float() - x) / (float(torch.exp(torch.tensor(6.0))) * n)).to(dtype)
    g_nll = torch.autograd.grad(y, dec.get_last_layer(), grad_outputs=gy, retain_graph=True)[0]
    g_g = torch.autograd.grad(-m.discriminator(y).float().mean(), dec.get_last_layer(), retain_graph=True)[0]
    want = torch.clamp(g_nll.float().norm() / (g_g.float().norm() + 1e-4), 0.0, 1e4) * 0.5
    got = log["train/scalars/d_weight"]
    print(f"\n[loss] adaptive weight through the decoder tail: {float(got):.6e} (by hand {float(want):.6e})")
    assert 0.0 < float(want) < 0.5e4
    # the hand probe differs in the discriminator's mean (torch's, on bf16 logits) and in fp32 rounding of the cotangent: bf16 noise
    assert abs(float(got) - float(want)) <= 2.0 ** -7 * float(want)
    loss.backward()
    assert z.grad is not None and bool(torch.isfinite(z.grad).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in dec.parameters())
    assert torch.equal(ops.reduce_sum(L.RED_SQ, g_nll), ops.reduce_sum(L.RED_SQ, g_nll))
