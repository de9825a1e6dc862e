"""cvvae_conv333_s2_dgrad_small on the MI355X: the direct stride-2 input gradient of a few-channel 3x3x3 conv against fp64
torch.autograd of F.conv3d(stride=2, padding=1) on the CPU.

Bound per element, from the formats alone: half an ulp of the storage dtype at the result (the one rounding; fp32 storage: none) plus
n 2^-24 sum|terms| for the fp32 accumulation of n <= 8 Cout products (an input pixel gathers from at most 8 output pixels), with
sum|terms| the same gradient over |gy| and |W|.  The zero-stuffed grad3d.dgrad333 path is held to the same bound on the same
operands: it is one the existing path satisfies.  Extents: (5,6,7) and (4,9,6) put both parities on every axis; (2,3,131) has 66
column pairs (a second, ragged wave chunk); (5,420,3) with B = 2 has more row chunks than the capped grid has waves (the stride
loop)."""
import os

import pytest
import torch

from lossnet_ref import dgrad_bound as _bound  # the reference and the bound live with the edge tests' references (tests/lossnet_ref.py)
from lossnet_ref import dgrad_ref as _ref

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16, torch.float32]


def _log(line):
    print("\n" + line)
    d = os.environ.get("CVVAE_TEST_LOG_DIR", "")          # a directory that receives the figures of a run; unset: printed only
    if d and os.path.isdir(d):
        with open(os.path.join(d, "disc_dgrad_parity.txt"), "a") as f:
            f.write(line + "\n")


def _operands(dtype, cout, in_shape, seed):
    B, T, H, W = in_shape
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(cout, 3, 3, 3, 3, generator=g) * 0.1).to(dtype)
    gy = torch.randn(B, (T - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1, cout, generator=g).to(dtype)
    return gy, w


def _check(got, gy, w, in_shape, dtype, what):
    ref = _ref(gy, w, in_shape)
    terms = _ref(gy.abs(), w.abs(), in_shape)
    bound = _bound(ref, terms, dtype, w.shape[0])
    got = got.cpu()
    assert tuple(got.shape) == (*in_shape, 8) and got.dtype == dtype
    assert torch.equal(got[..., 3:], torch.zeros_like(got[..., 3:])), what                    # pad channels exactly zero
    err = (got[..., :3].double() - ref).abs()
    worst = float((err / bound).max())
    _log(f"[{what} {str(dtype)[6:]} {in_shape} Cout {w.shape[0]}] max err / bound {worst:.3f}; max |err| {float(err.max()):.3e}")
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cout", [8, 64])
@pytest.mark.parametrize("thw", [(5, 6, 7), (4, 9, 6)])
def test_direct_dgrad_and_the_zero_stuffed_path_meet_the_format_bound(dtype, cout, thw):
    from cvvae_amd import grad3d, ops
    from cvvae_amd.engine import P1, ZERO, WeightCache
    in_shape = (2, *thw)
    gy, w = _operands(dtype, cout, in_shape, 100 + cout + thw[0])
    with torch.cuda.device(0):
        a = ops.conv333_s2_dgrad_small(gy.cuda(), w.cuda(), in_shape, 3)
        b = ops.conv333_s2_dgrad_small(gy.cuda(), w.cuda(), in_shape, 3)
        assert torch.equal(a, b)                                                               # two runs: the same bits
        _check(a, gy, w, in_shape, dtype, "direct")
        # the existing path on the same operands (its K chunk is 16 channels: Cout = 8 goes in with eight zero channels behind it)
        holder = torch.nn.Module()
        holder.c = torch.nn.Conv3d(3, cout, 3, stride=2, padding=1).to(dtype).cuda()
        with torch.no_grad():
            holder.c.weight.copy_(w.cuda())
        g16 = torch.zeros(*gy.shape[:4], max(cout, 16), dtype=dtype)
        g16[..., :cout] = gy
        z = grad3d.dgrad333(WeightCache(holder), g16.cuda(), "c", P1, ZERO, ZERO, in_shape, stride=(2, 2, 2))
        _check(z, gy, w, in_shape, dtype, "zero-stuffed")


def test_pixel_stride_larger_than_cout_and_nan_in_the_unused_channels():
    from cvvae_amd import ops
    dtype, cout, in_shape = torch.bfloat16, 64, (2, 5, 6, 7)
    gy, w = _operands(dtype, cout, in_shape, 7)
    wide = torch.full((*gy.shape[:4], cout + 8), float("nan"), dtype=dtype)
    wide[..., :cout] = gy
    with torch.cuda.device(0):
        a = ops.conv333_s2_dgrad_small(wide.cuda(), w.cuda(), in_shape, 3)
        b = ops.conv333_s2_dgrad_small(gy.cuda(), w.cuda(), in_shape, 3)
    assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    _check(a, gy, w, in_shape, dtype, "strided")


@pytest.mark.parametrize("in_shape,cout", [((1, 2, 3, 131), 64), ((2, 5, 420, 3), 8)])
def test_second_wave_chunk_and_the_grid_stride_loop(in_shape, cout):
    from cvvae_amd import ops
    dtype = torch.bfloat16
    gy, w = _operands(dtype, cout, in_shape, 11)
    with torch.cuda.device(0):
        a = ops.conv333_s2_dgrad_small(gy.cuda(), w.cuda(), in_shape, 3)
    _check(a, gy, w, in_shape, dtype, "chunks")


def test_eight_input_channels_take_the_wide_table():
    from cvvae_amd import ops
    dtype, in_shape = torch.float16, (1, 3, 4, 5)
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(16, 8, 3, 3, 3, generator=g) * 0.1).to(dtype)
    gy = torch.randn(1, 2, 2, 3, 16, generator=g).to(dtype)
    with torch.cuda.device(0):
        got = ops.conv333_s2_dgrad_small(gy.cuda(), w.cuda(), in_shape, 8).cpu()
    ref, terms = _ref(gy, w, in_shape), _ref(gy.abs(), w.abs(), in_shape)
    assert float(((got.double() - ref).abs() / _bound(ref, terms, dtype, 16)).max()) <= 1.0
