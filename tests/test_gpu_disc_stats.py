"""cvvae_gn_leaky_apply_stats and cvvae_avgpool3d_down_stats (csrc/disc_kernels.hip) on a real MI355X: the passes that leave the
GroupNorm records of the tensor they store, so that the discriminator's Normalize layers need no statistics pass of their own.

  * the stored tensor is BIT-EQUAL to the plain entry point's (cvvae_gn_leaky_apply / cvvae_avgpool3d_down), also with out_partials
    NULL (through the C entry) and in place;
  * the (scale, shift) tables cvvae_gn_finalize makes of the new records are compared with fp64 statistics of the ROUNDED stored tensor.
    The yardstick is cvvae_gn_stats run on that same stored tensor: the new tables' error (relative L2 over the table) may be at most
    2x that entry's own error against fp64 -- both compute Chan merges in fp32 and differ in the order only.  Every pair of figures is
    printed before it is asserted (`pytest -s`: the `[disc stats]` lines); the figures measured on the MI355X are recorded in
    tests/golden/disc_net_bands.json;
  * two runs give identical record bits.

Shapes: the 2-, 4-, 8- and 16-channel groups of the network's Normalize(64 ... 512) at sizes of one workgroup per sample, plus, beyond
that list, runs of several workgroups per sample with a ragged last one, and channel counts whose 8-channel vectors do not divide the
workgroup (C = 40 as 4 groups of 10: pairs; C = 96 as 8 groups of 12: quads)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
EPS, SLOPE = 1e-6, 0.2
# (NDHWC shape of the pass's INPUT, groups)
LEAKY_CASES = [((2, 3, 6, 5, 64), 32), ((1, 2, 4, 4, 128), 32), ((2, 1, 3, 7, 512), 32), ((2, 2, 5, 9, 256), 32),
               ((1, 9, 24, 24, 64), 32), ((2, 3, 21, 19, 512), 32), ((3, 3, 5, 7, 40), 4), ((1, 5, 9, 11, 96), 8)]
POOL_CASES = [((2, 3, 6, 5, 64), 32), ((1, 4, 5, 6, 256), 32), ((2, 1, 4, 6, 128), 32), ((1, 7, 34, 35, 128), 32),
              ((1, 4, 12, 10, 512), 32), ((2, 3, 6, 10, 40), 4)]


def _id(case):
    return "x".join(map(str, case[0])) + f"g{case[1]}"


def _randn(shape, seed, dtype):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.3 * torch.randn(C, generator=g)).float(), (0.4 * torch.randn(C, generator=g)).float()


def _tables64(y, G, gamma, beta):
    """fp64 GroupNorm tables [B, C] of the stored tensor y [B,T,H,W,C] (CPU)"""
    B, C = y.shape[0], y.shape[-1]
    v = y.double().reshape(B, -1, G, C // G)
    mean = v.mean(dim=(1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rstd = (var + EPS).rsqrt()
    scale = gamma.double()[None] * rstd.repeat_interleave(C // G, 1)
    shift = beta.double()[None] - mean.repeat_interleave(C // G, 1) * scale
    return scale, shift


def _rel(got, ref):
    return float((got.cpu().double() - ref).norm() / ref.norm())


def _records_hold(tag, y, part, G):
    """y: the stored tensor (GPU), part: its GNPartials from the pass under test"""
    from cvvae_amd import ops
    B, C = y.shape[0], y.shape[-1]
    assert part.rows == B and part.groups == G and part.C == C and part.slabs >= 1
    assert tuple(part.buf.shape) == (B, G, part.slabs, 3) and part.buf.dtype == torch.float32
    n = part.buf[..., 0].double().sum(-1).cpu()
    assert bool((n == y[0].numel() // G).all()), "every stored element is counted once"
    gamma, beta = _affine(C, 5)
    s64, h64 = _tables64(y.cpu(), G, gamma, beta)
    gd, bd = gamma.cuda(), beta.cuda()
    new = ops.gn_finalize(part, gd, bd, EPS)
    base = ops.gn_stats(y, gd, bd, EPS, groups=G)
    figs = [("scale", _rel(new[0], s64), _rel(base[0], s64)), ("shift", _rel(new[1], h64), _rel(base[1], h64))]
    for k, a, b in figs:
        print(f"\n[disc stats] {tag} {k}: new {a:.6e} gn_stats {b:.6e}")
    for k, a, b in figs:
        assert a == a and a <= 2.0 * b, f"{tag} {k}: new {a:.3e} > 2 x gn_stats {b:.3e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("bare", [False, True], ids=["affine", "bare"])
@pytest.mark.parametrize("case", LEAKY_CASES, ids=_id)
def test_gn_leaky_apply_stats(case, bare, dtype):
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    shape, G = case
    B, T, H, W, C = shape
    x = (1.3 * _randn(shape, 11, dtype).float() + 0.25).to(dtype).cuda()
    tabs = None
    if not bare:
        g = torch.Generator().manual_seed(12)
        tabs = ((1.0 + 0.3 * torch.randn(B, C, generator=g)).float().cuda(), (0.5 * torch.randn(B, C, generator=g)).float().cuda())
    plain = ops.gn_leaky_apply(x, tabs, SLOPE)
    y, part = ops.gn_leaky_apply(x, tabs, SLOPE, gn_out=G)
    assert torch.equal(y, plain)
    y2, part2 = ops.gn_leaky_apply(x, tabs, SLOPE, gn_out=G)
    assert torch.equal(y2, y) and torch.equal(part2.buf.view(torch.int32), part.buf.view(torch.int32))   # the same record bits
    xin = x.clone()
    yin, part3 = ops.gn_leaky_apply(xin, tabs, SLOPE, out=xin, gn_out=G)                                  # in place
    assert yin is xin and torch.equal(xin, y) and torch.equal(part3.buf.view(torch.int32), part.buf.view(torch.int32))
    # out_partials = NULL with groups given, and out_groups = 0 with a buffer: the plain pass
    lib = L.load()
    for groups, buf in ((G, None), (0, part.buf.data_ptr())):
        out = torch.full_like(x, 7.0)
        rc = lib.cvvae_gn_leaky_apply_stats(ops._dt(dtype), x.data_ptr(), tabs[0].data_ptr() if tabs else None,
                                            tabs[1].data_ptr() if tabs else None, out.data_ptr(), B, T * H * W, C, SLOPE, groups, buf,
                                            ops._stream(x))
        assert rc == 0 and torch.equal(out, plain)
    _records_hold(f"leaky {_id(case)} {str(dtype)[6:]} {'bare' if bare else 'affine'}", y, part, G)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case", POOL_CASES, ids=_id)
def test_avgpool3d_down_stats(case, dtype):
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    shape, G = case
    B, T, H, W, C = shape
    x = (1.3 * _randn(shape, 21, dtype).float() + 0.25).to(dtype).cuda()
    plain = ops.avgpool3d_down(x)
    y, part = ops.avgpool3d_down(x, gn_out=G)
    assert tuple(y.shape) == ops.avgpool3d_down_shape(shape) and torch.equal(y, plain)
    y2, part2 = ops.avgpool3d_down(x, gn_out=G)
    assert torch.equal(y2, y) and torch.equal(part2.buf.view(torch.int32), part.buf.view(torch.int32))
    lib = L.load()
    for groups, buf in ((G, None), (0, part.buf.data_ptr())):
        out = torch.full_like(plain, 7.0)
        rc = lib.cvvae_avgpool3d_down_stats(ops._dt(dtype), x.data_ptr(), out.data_ptr(), B, T, H, W, C, groups, buf,
                                            ops._stream(x))
        assert rc == 0 and torch.equal(out, plain)
    _records_hold(f"pool {_id(case)} {str(dtype)[6:]}", y, part, G)


def test_the_slab_counts_of_the_cases_cover_one_and_several_workgroups_per_sample():
    """what the shape lists above are chosen for (host code, asserted here so that a change of the slab rule does not empty the cover)"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    f = L.load().cvvae_pass_gn_slabs
    leaky = [f(s[0], s[1] * s[2] * s[3], s[4], g) for s, g in LEAKY_CASES]
    pool = [f(s[0], o[1] * o[2] * o[3], s[4], g) for s, g in POOL_CASES for o in [ops.avgpool3d_down_shape(s)]]
    assert min(leaky) == 1 and max(leaky) > 4 and min(pool) == 1 and max(pool) > 4, (leaky, pool)
