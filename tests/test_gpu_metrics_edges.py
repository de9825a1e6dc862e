"""cvvae_frame_metrics on the MI355X against the fp64 restatement of tests/metrics_ref.py, for every case of
tests/metrics_edge_cases.py.  Each case is called through the C ABI with its three outputs and the workspace inside larger poisoned
buffers, and is held to:
  sse    equal to the restatement's when both operands are on integer values, else within 1e-12 relative (fp64 accumulation);
  psnr   within one fp32 ulp of float32(10 log10(65025 * 3HW / sse)) evaluated in fp64 on the host; +inf exactly where sse == 0;
  ssim   within 1e-6 ABSOLUTE of the restatement (metrics_ref.SSIM_ATOL: the issue's condition, not a band fitted to the kernel);
         x against x gives 1.0 exactly;
  two runs give identical bits; an in-place view gives the bits of its .contiguous() copy; quantize=True on float clips gives the bits
  of the uint8 path on ops.ncdhw_to_frames_u8 of the same clips; no byte outside the outputs and the workspace is written.
A line per case reports the worst ssim error (pytest -s); tests/golden/metrics_bands.json keeps the overall worst of one run, for
the record."""
import ctypes
import math

import numpy as np
import pytest
import torch

import metrics_edge_cases as MC
import metrics_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes in front of and behind every output
POISON = 0xA5


def _call(a, b, quantize, want_ssim=True):
    """one call through the C ABI on device operands (views read in place) -> (sse, psnr, ssim) on the CPU; asserts the guard bytes"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    lib = L.load()
    B, T, H, W = ops.check_metric_operands(a, b, want_ssim)
    a, va = ops._clip_view(a)
    b, vb = ops._clip_view(b)
    n = B * T
    sizes = {"sse": 8 * n, "psnr": 4 * n, "ssim": 4 * n, "ws": int(lib.cvvae_frame_metrics_workspace_bytes(B, T, H, W, int(want_ssim)))}
    assert sizes["ws"] > 0
    bufs = {k: torch.full((GUARD + s + GUARD,), POISON, dtype=torch.uint8, device="cuda") for k, s in sizes.items()}
    ptr = {k: v.data_ptr() + GUARD for k, v in bufs.items()}
    L.check(lib.cvvae_frame_metrics(a.data_ptr(), ctypes.byref(va), b.data_ptr(), ctypes.byref(vb), B, T, H, W, int(quantize), int(want_ssim),
                                    ptr["sse"], ptr["psnr"], ptr["ssim"] if want_ssim else None, ptr["ws"], ops._stream(a)),
            "cvvae_frame_metrics")
    torch.cuda.synchronize()
    host = {k: v.cpu() for k, v in bufs.items()}
    for k, h in host.items():
        assert bool((h[:GUARD] == POISON).all()) and bool((h[GUARD + sizes[k]:] == POISON).all()), f"bytes around {k} were written"
    if not want_ssim:
        assert bool((host["ssim"] == POISON).all()), "ssim written though not wanted"
    cut = {k: host[k][GUARD:GUARD + sizes[k]] for k in ("sse", "psnr", "ssim")}
    return (cut["sse"].view(torch.float64).reshape(B, T), cut["psnr"].view(torch.float32).reshape(B, T),
            cut["ssim"].view(torch.float32).reshape(B, T) if want_ssim else None)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(x, y):
    return all(torch.equal(_bits(p), _bits(q)) for p, q in zip(x, y))


@pytest.mark.parametrize("case", MC.CASES, ids=[c.name for c in MC.CASES])
def test_frame_metrics_against_the_fp64_restatement(case):
    from cvvae_amd import ops
    ba, bb = MC.bases(case)
    ca, cb = MC.apply(case, ba, bb)
    want_sse, want_psnr, want_ssim = R.frame_metrics(ca, cb, case.quantize)
    da, db = MC.apply(case, ba.cuda(), bb.cuda())
    if case.view != "none":
        assert not (da.is_contiguous() and db.is_contiguous()) or da.storage_offset() or db.storage_offset()
    got = _call(da, db, case.quantize)
    sse, psnr, ssim = got
    H, W = case.H, case.W
    err = float((ssim.double() - want_ssim).abs().max())
    print(f"METRICS-EDGE {case.name}: worst |ssim - fp64| = {err:.3e}  (condition {R.SSIM_ATOL:.0e})")
    failures = []
    if R.integer_valued(ca, cb, case.quantize):
        if not torch.equal(sse, want_sse):
            failures.append(f"sse {sse.tolist()} != {want_sse.tolist()} on integer-valued operands")
    elif not bool(((sse - want_sse).abs() <= R.SSE_RTOL * want_sse).all()):
        failures.append(f"sse off by {float(((sse - want_sse).abs() / want_sse).max()):.3e} relative")
    for i in range(case.B):
        for t in range(case.T):
            s = float(sse[i, t])
            if s == 0.0:
                if not (math.isinf(float(psnr[i, t])) and float(psnr[i, t]) > 0):
                    failures.append(f"psnr[{i},{t}] = {float(psnr[i, t])} where sse == 0")
            else:
                w = float(np.float32(10.0 * math.log10(65025.0 * 3 * H * W / s)))
                if not abs(float(psnr[i, t]) - w) <= R.ulp32(w):
                    failures.append(f"psnr[{i},{t}] = {float(psnr[i, t])!r}, host fp64 gives {w!r}")
    if not err <= R.SSIM_ATOL:
        failures.append(f"ssim off by {err:.3e} > {R.SSIM_ATOL:.0e}")
    if case.content == "same" and not bool((ssim == 1.0).all()):
        failures.append(f"x against x: ssim = {ssim.tolist()}, not exactly 1.0")
    if case.content == "inverse" and case.ka == case.kb == "u8" and not bool((ssim < -0.9).all()):
        failures.append(f"x against 255 - x: ssim = {ssim.tolist()}")
    if not _same_bits(got, _call(da, db, case.quantize)):
        failures.append("two runs on the same inputs differ")
    if case.view != "none" and not _same_bits(got, _call(da.contiguous(), db.contiguous(), case.quantize)):
        failures.append("the in-place view and its .contiguous() copy differ")
    if case.quantize and "u8" != case.ka and "u8" != case.kb and case.B == 1:
        ua, ub = ops.ncdhw_to_frames_u8(da.contiguous()), ops.ncdhw_to_frames_u8(db.contiguous())
        if not _same_bits(got, _call(ua, ub, True)):
            failures.append("quantize=True differs from the uint8 path on ncdhw_to_frames_u8 of the same clips")
    only_psnr = _call(da, db, case.quantize, want_ssim=False)
    if R.integer_valued(ca, cb, case.quantize):   # (the two passes tile the frame differently: another order of summation otherwise)
        if not _same_bits(got[:2], only_psnr[:2]):
            failures.append("sse / psnr differ between the SSIM pass and the PSNR-only pass")
    elif not bool(((only_psnr[0] - want_sse).abs() <= R.SSE_RTOL * want_sse).all()):
        failures.append("sse of the PSNR-only pass is off")
    assert not failures, f"{case.name}: " + "; ".join(failures)


def test_quantize_on_batched_float_clips_is_the_u8_path_clip_by_clip():
    from cvvae_amd import ops
    g = torch.Generator().manual_seed(11)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        x = ((torch.rand((2, 3, 2, 27, 43), generator=g) * 2.4 - 1.2).to(dt)).cuda()
        y = ((torch.rand((2, 3, 2, 27, 43), generator=g) * 2.4 - 1.2).to(dt)).cuda()
        got = _call(x, y, True)
        for i in range(2):
            ux, uy = ops.ncdhw_to_frames_u8(x[i:i + 1].contiguous()), ops.ncdhw_to_frames_u8(y[i:i + 1].contiguous())
            one = _call(ux, uy, True)
            assert _same_bits([t[i:i + 1] for t in got], one), (dt, i)


def test_public_layer_does_not_synchronise_the_host():
    from cvvae_amd import metrics
    g = torch.Generator().manual_seed(3)
    a = torch.randint(0, 256, (3, 27, 43, 3), generator=g, dtype=torch.uint8).cuda()
    x = (torch.rand((1, 3, 3, 27, 43), generator=g) * 2 - 1).to(torch.bfloat16).cuda()
    meter = metrics.ReconstructionMeter()
    metrics.frame_metrics(a, x)          # (first call: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m = metrics.frame_metrics(a, x)
        p = metrics.psnr(a[1:], x[:, :, 1:], quantize=False)
        s = metrics.ssim(x, x)
        meter.update(a, x)
        meter.update(a, a)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = meter.compute()
    assert out["frames"] == 6 and out["identical_frames"] == 3 and math.isfinite(out["psnr"])
    assert tuple(m["ssim"].shape) == (1, 3) and tuple(p.shape) == (1, 2) and bool((s == 1.0).all())
    want = R.frame_metrics(a.cpu(), x.cpu())
    assert torch.equal(m["sse"].cpu(), want[0]) and float((m["ssim"].cpu().double() - want[2]).abs().max()) <= R.SSIM_ATOL
    assert out["ssim"] == pytest.approx((float(m["ssim"].double().sum()) + 3.0) / 6, rel=1e-12)
