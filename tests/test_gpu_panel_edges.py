"""cvvae_recon_panels on the MI355X against the eager torch expression of log_images in the same dtype (tests/panel_ref.py `panels`,
evaluated on the device), for every case of tests/panel_edge_cases.py and every boost factor.  Each call goes through the C ABI
with its four outputs inside larger poisoned buffers, and is held to:
  all four panels bit for bit equal to eager torch's;
  two runs give identical bits; the in-place view gives the bits of its .contiguous() copy;
  no byte outside the four outputs is written.
NaN is outside the contract."""
import ctypes

import pytest
import torch

import panel_edge_cases as PC
import panel_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes in front of and behind every output (keeps the outputs on a 16-byte boundary)
POISON = 0xA5
NAMES = ("inputs", "reconstructions", "diff", "diff_boost")


def _call(x, xrec, boost, shift=0):
    """one call through the C ABI on device operands (views read in place) -> the four panels on the CPU; asserts the guard bytes.
    shift: the outputs start `shift` elements behind the 16-byte boundary"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    lib = L.load()
    B, T, H, W = ops.check_panel_operands(x, xrec)
    x, vx = ops._clip_view(x)
    xrec, vr = ops._clip_view(xrec)
    esz = x.element_size()
    nbytes = B * T * 3 * H * W * esz
    off = GUARD + shift * esz
    bufs = [torch.full((off + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda") for _ in NAMES]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    L.check(lib.cvvae_recon_panels(x.data_ptr(), ctypes.byref(vx), xrec.data_ptr(), ctypes.byref(vr), B, T, H, W, float(boost),
                                   *[b.data_ptr() + off for b in bufs], ops._stream(x)), "cvvae_recon_panels")
    torch.cuda.synchronize()
    out = []
    for name, b in zip(NAMES, bufs):
        h = b.cpu()
        assert bool((h[:off] == POISON).all()) and bool((h[off + nbytes:] == POISON).all()), f"bytes around {name} were written"
        out.append(h[off:off + nbytes].clone().view(x.dtype).reshape(B * T, 3, H, W))
    return out


@pytest.mark.parametrize("case", PC.CASES, ids=[c.name for c in PC.CASES])
def test_panels_are_the_eager_expression_bit_for_bit(case):
    bx, br = PC.bases(case)
    dx, dr = PC.view_of(case, bx.cuda()), br.cuda()
    assert torch.equal(dx, bx.cuda())
    if case.view != "none":
        assert not dx.is_contiguous() or dx.storage_offset()
    failures = []
    for f in PC.BOOSTS:
        want = [t.cpu() for t in R.panels(dx, dr, f)]
        got = _call(dx, dr, f)
        for name, g, w in zip(NAMES, got, want):
            if not R.same_bits(g, w):
                bad = (g.float() != w.float()) | (g.float().signbit() != w.float().signbit())
                i = int(bad.flatten().nonzero()[0])
                failures.append(f"f={f} {name}: {int(bad.sum())} of {g.numel()} elements differ, first at {i}: "
                                f"{float(g.flatten()[i])!r} != {float(w.flatten()[i])!r}")
        if not all(R.same_bits(a, b) for a, b in zip(got, _call(dx, dr, f))):
            failures.append(f"f={f}: two runs on the same inputs differ")
    if case.view != "none" and not all(R.same_bits(a, b) for a, b in zip(_call(dx, dr, 2.5), _call(dx.contiguous(), dr, 2.5))):
        failures.append("the in-place view and its .contiguous() copy differ")
    assert not failures, f"{case.name}: " + "; ".join(failures)


@pytest.mark.parametrize("dtype", list(PC.DTYPES.values()), ids=list(PC.DTYPES))
def test_outputs_off_the_16_byte_boundary_and_both_operands_as_views(dtype):
    """outputs based 1 and 3 elements past a 16-byte boundary (the head moves); xrec a view too, on another alignment than x"""
    case = PC.Case("shifted", dtype, (2, 3, 3, 7, 16), "crop")
    bx, br = PC.bases(case, seed=5)
    dx = PC.view_of(case, bx.cuda())
    dr = PC.view_of(PC.Case("r", dtype, case.shape, "frames"), br.cuda())
    want = [t.cpu() for t in R.panels(dx, dr, 3.0)]
    for shift in (0, 1, 3):
        got = _call(dx, dr, 3.0, shift=shift)
        assert all(R.same_bits(g, w) for g, w in zip(got, want)), shift


def test_public_wrapper_gives_the_same_bits_without_a_host_sync():
    from cvvae_amd import ops
    case = PC.Case("wrapper", torch.bfloat16, (1, 3, 5, 32, 32), "frames")
    bx, br = PC.bases(case, seed=9)
    dx, dr = PC.view_of(case, bx.cuda()), br.cuda()
    ops.recon_panels(dx, dr, 3.0)        # (first call: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = ops.recon_panels(dx, dr, 3.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = R.panels(dx, dr, 3.0)
    assert all(g.is_contiguous() and tuple(g.shape) == (5, 3, 32, 32) for g in got)
    assert all(R.same_bits(g.cpu(), w.cpu()) for g, w in zip(got, want))
    with pytest.raises(ValueError, match="one dtype"):
        ops.recon_panels(dx, dr.float(), 3.0)
    with pytest.raises(ValueError, match="shapes"):
        ops.recon_panels(dx, dr[:, :, :4], 3.0)
