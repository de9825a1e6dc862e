"""What holds of the reconstruction metrics without a GPU: the fp64 restatement of tests/metrics_ref.py against three independent
routes (scipy's gaussian_filter as skimage builds SSIM from it, the closed form for flat frames, a direct 11 x 11 double loop), the
8-bit mapping against the scripts' torch expression over every 16-bit pattern in [-1.5, 1.5], the case list's own coverage, the
fp32 arithmetic a user would write the metric in (the reason the kernel's moments are fp64), and the Python layer (cvvae_amd/metrics.py, the
view handling of ops.frame_metrics) with the kernel call replaced by the restatement."""
import math

import numpy as np
import pytest
import torch

import metrics_edge_cases as MC
import metrics_ref as R


def _pair(H, W, seed=0, T=2):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8))


def test_restatement_agrees_with_scipys_gaussian_filter():
    import scipy.ndimage as ndi
    worst = 0.0
    for H, W, seed in ((11, 11, 0), (12, 13, 1), (27, 43, 2), (43, 75, 3)):
        a, b = _pair(H, W, seed)
        u, v = R.to_scale8(a)[0], R.to_scale8(b)[0]          # [3,T,H,W]

        def filt(x):
            return ndi.gaussian_filter(x, sigma=(0, 0, 1.5, 1.5), truncate=3.5, mode="reflect")
        mx, my = filt(u), filt(v)
        vx, vy, cxy = filt(u * u) - mx * mx, filt(v * v) - my * my, filt(u * v) - mx * my
        S = ((2 * mx * my + R.C1) * (2 * cxy + R.C2)) / ((mx * mx + my * my + R.C1) * (vx + vy + R.C2))
        want = S[..., 5:H - 5, 5:W - 5].mean(axis=(0, 2, 3))
        got = R.frame_metrics(a, b)[2][0].numpy()
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"METRICS-HOST restatement vs scipy gaussian_filter: worst |d| = {worst:.3e}")
    assert worst <= 1e-12


def test_restatement_agrees_with_the_closed_form_on_flat_frames():
    for x, y in ((255, 254), (0, 1)):
        a = torch.full((1, 13, 12, 3), x, dtype=torch.uint8)
        b = torch.full((1, 13, 12, 3), y, dtype=torch.uint8)
        sse, psnr, ssim = R.frame_metrics(a, b)
        want = (2.0 * x * y + R.C1) / (x * x + y * y + R.C1)
        err = abs(float(ssim[0, 0]) - want)
        print(f"METRICS-HOST flat {x}/{y}: ssim {float(ssim[0, 0]):.15f} closed form {want:.15f} |d| {err:.3e}")
        assert err <= 1e-11
        assert float(sse[0, 0]) == 13 * 12 * 3 and float(psnr[0, 0]) == np.float32(10 * math.log10(65025.0))


def test_restatement_agrees_with_a_direct_double_loop():
    a, b = _pair(14, 17, 5, T=1)
    u, v = R.to_scale8(a)[0, :, 0], R.to_scale8(b)[0, :, 0]   # [3,H,W]
    g = R.window()
    S = R.ssim_map(u, v)
    for c, y, x in ((0, 0, 0), (1, 3, 6), (2, 2, 0), (0, 3, 6), (1, 1, 4)):
        m = {"x": 0.0, "y": 0.0, "xx": 0.0, "yy": 0.0, "xy": 0.0}
        for i in range(11):
            for j in range(11):
                w, p, q = g[i] * g[j], u[c, y + i, x + j], v[c, y + i, x + j]
                m["x"] += w * p
                m["y"] += w * q
                m["xx"] += w * p * p
                m["yy"] += w * q * q
                m["xy"] += w * p * q
        vx, vy, cxy = m["xx"] - m["x"] ** 2, m["yy"] - m["y"] ** 2, m["xy"] - m["x"] * m["y"]
        want = ((2 * m["x"] * m["y"] + R.C1) * (2 * cxy + R.C2)) / ((m["x"] ** 2 + m["y"] ** 2 + R.C1) * (vx + vy + R.C2))
        assert abs(S[c, y, x] - want) <= 1e-12, (c, y, x)
    assert abs(R.window().sum() - 1.0) <= 2e-16 and R.window()[5] == R.window().max()


def test_sse_and_psnr_of_the_restatement():
    a, b = _pair(11, 13, 7, T=3)
    sse, psnr, _ = R.frame_metrics(a, b)
    d = a.long() - b.long()
    assert torch.equal(sse[0], (d * d).sum(dim=(1, 2, 3)).double())
    assert psnr.dtype == torch.float32 and sse.dtype == torch.float64
    same = R.frame_metrics(a, a.clone())
    assert torch.all(same[0] == 0) and torch.all(torch.isinf(same[1])) and torch.all(same[1] > 0) and torch.all(same[2] == 1.0)
    inv = R.frame_metrics(a, 255 - a)[2]
    assert torch.all(inv < -0.9)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_eight_bit_mapping_is_the_scripts_expression_bit_for_bit(dt):
    dtype = MC.DTYPE[dt]
    if dt == "f32":
        g = torch.Generator().manual_seed(0)
        x = torch.cat([(torch.rand(1 << 16, generator=g) * 3 - 1.5), torch.arange(256) / 127.5 - 1.0,
                       torch.tensor([-1.5, -1.0, -0.0, 0.0, 1.0, 1.5, 1.0 - 2 ** -24, -1.0 + 2 ** -24])])
    else:
        x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)   # every bit pattern
        x = x[torch.isfinite(x.float()) & (x.float().abs() <= 1.5)]
        assert x.numel() > 30000
    want = ((torch.clamp(x, -1.0, 1.0) + 1.0) * 127.5).to(torch.uint8)
    got = R.quantize_u8(x)
    assert torch.equal(got, want)
    assert int(got.min()) == 0 and int(got.max()) == 255
    raw = R.to_scale8(x.view(1, 1, 1, 1, -1), quantize=False)
    assert raw.min() == 0.0 and raw.max() == 255.0


def test_case_list_covers_what_the_issue_names():
    cs = MC.CASES
    assert len({c.name for c in cs}) == len(cs)
    hw = {(c.H, c.W) for c in cs}
    TH, TW = MC.TILE_H, MC.TILE_W
    assert {c.H for c in cs} >= {11, 12, 13} and {c.W for c in cs} >= {11, 12, 13}
    assert {h - 10 for h, _ in hw} >= {TH - 1, TH, TH + 1, 2 * TH + 1} and {w - 10 for _, w in hw} >= {TW - 1, TW, TW + 1, 2 * TW + 1}
    assert any(-(-(h - 10) // TH) >= 3 and -(-(w - 10) // TW) >= 3 for h, w in hw)
    assert {c.T for c in cs} >= {1, 3} and {c.B for c in cs} >= {1, 2}
    assert {c.content for c in cs} == set(MC.CONTENTS) and {c.view for c in cs} == set(MC.VIEWS)
    kinds = {(c.ka, c.kb, c.quantize) for c in cs}
    assert ("u8", "u8", True) in kinds and ("u8", "bf16", True) in kinds and ("f16", "f32", True) in kinds
    assert all((d, d, q) in kinds for d in ("f16", "bf16", "f32") for q in (True, False))
    assert any(c.view == "frame_slice" and c.ka == "u8" and (c.H * c.W * 3) % 2 == 1 for c in cs)
    for c in cs:
        a, b = MC.apply(c, *MC.bases(c))
        ea, eb = ((1,) + tuple(t.shape[:3]) if t.dtype == torch.uint8 else (t.shape[0],) + tuple(t.shape[2:]) for t in (a, b))
        assert ea == eb == (c.B, c.T, c.H, c.W), c.name
        assert a.dtype == MC.DTYPE[c.ka] and b.dtype == MC.DTYPE[c.kb]
        assert a.numel() <= 6 * 43 * 75 * 3, c.name
        if c.view != "none":
            assert not (a.is_contiguous() and b.is_contiguous()) or a.storage_offset() or b.storage_offset(), c.name


def test_the_fp32_expression_misses_the_kernels_condition_by_orders_of_magnitude():
    """the arithmetic choice of csrc/metrics_kernels.hip: 255 against 254 through the 11 x 11 window with every operation in fp32 (the taps
    added one by one, so the figure does not depend on a convolution library's order of summation) is off by about 1e-3; the same
    operations in fp64 are the closed form to 1e-13"""
    g64 = torch.tensor(R.window())
    want = (2.0 * 255 * 254 + R.C1) / (255.0 ** 2 + 254.0 ** 2 + R.C1)

    def ssim_flat(dtype):
        g = g64.to(dtype)
        x, y = torch.tensor(255.0, dtype=dtype), torch.tensor(254.0, dtype=dtype)
        m = {k: torch.zeros((), dtype=dtype) for k in ("x", "y", "xx", "yy", "xy")}
        for i in range(11):
            for j in range(11):
                w = g[i] * g[j]
                for k, v in (("x", x), ("y", y), ("xx", x * x), ("yy", y * y), ("xy", x * y)):
                    m[k] = m[k] + w * v
        c1, c2 = torch.tensor(R.C1, dtype=dtype), torch.tensor(R.C2, dtype=dtype)
        vx, vy, cxy = m["xx"] - m["x"] * m["x"], m["yy"] - m["y"] * m["y"], m["xy"] - m["x"] * m["y"]
        return float(((2 * m["x"] * m["y"] + c1) * (2 * cxy + c2)) / ((m["x"] * m["x"] + m["y"] * m["y"] + c1) * (vx + vy + c2)))
    e32, e64 = abs(ssim_flat(torch.float32) - want), abs(ssim_flat(torch.float64) - want)
    print(f"METRICS-HOST SSIM of 255 vs 254, every operation in fp32: |d| = {e32:.3e}; in fp64: |d| = {e64:.3e}")
    assert e64 <= 1e-12 and e32 > 100 * R.SSIM_ATOL


# ---- the Python layer, with the kernel call replaced by the restatement ----
@pytest.fixture
def emulated(monkeypatch):
    from cvvae_amd import ops
    seen = []

    def fake(a, b, quantize=True, want_ssim=True):
        seen.append((a, b, quantize, want_ssim))
        sse, psnr, ssim = R.frame_metrics(a, b, quantize, want_ssim)
        return sse, psnr, (ssim.float() if want_ssim else None)
    monkeypatch.setattr(ops, "frame_metrics", fake)
    return seen


def test_public_functions_shapes_dtypes_and_pass_through(emulated):
    import cvvae_amd
    from cvvae_amd import metrics
    assert cvvae_amd.metrics is metrics and cvvae_amd.ReconstructionMeter is metrics.ReconstructionMeter
    a, b = _pair(12, 13, 1, T=3)
    m = metrics.frame_metrics(a, b)
    assert set(m) == {"sse", "psnr", "ssim"}
    assert m["sse"].dtype == torch.float64 and m["psnr"].dtype == torch.float32 and m["ssim"].dtype == torch.float32
    assert all(tuple(v.shape) == (1, 3) for v in m.values())
    x = torch.rand(2, 3, 4, 12, 13) * 2 - 1
    w = x[:, :, 1:]                                        # a window: handed on as it is, strides and all
    p = metrics.psnr(w, w.to(torch.bfloat16), quantize=False)
    assert tuple(p.shape) == (2, 3) and emulated[-1][0] is w and emulated[-1][2:] == (False, False)
    s = metrics.ssim(a[1:], x[:1, :, 2:].half())           # uint8 frames against a float clip
    assert tuple(s.shape) == (1, 2) and emulated[-1][2:] == (True, True)
    assert emulated[-1][0].data_ptr() == a[1:].data_ptr()
    small = torch.zeros(1, 10, 40, 3, dtype=torch.uint8)
    assert tuple(metrics.psnr(small, small).shape) == (1, 1)    # PSNR alone has no minimum size


def test_public_functions_raise_value_errors(emulated):
    from cvvae_amd import metrics
    u = torch.zeros(3, 12, 13, 3, dtype=torch.uint8)
    f = torch.zeros(1, 3, 3, 12, 13)
    bad = [
        (u, torch.zeros(3, 12, 14, 3, dtype=torch.uint8)),          # W differs
        (u, torch.zeros(1, 3, 4, 12, 13)),                           # T differs
        (u, torch.zeros(2, 3, 3, 12, 13)),                           # uint8 frames against B = 2
        (f, torch.zeros(1, 3, 3, 12, 13, dtype=torch.float64)),      # dtype without a kernel
        (f, torch.zeros(1, 3, 3, 12, 13, dtype=torch.int32)),
        (f, torch.zeros(1, 1, 3, 12, 13)),                           # not 3 channels
        (u, torch.zeros(3, 12, 13, 4, dtype=torch.uint8)),
        (u, torch.zeros(3, 12, 13, dtype=torch.uint8)),              # rank
        (f, torch.zeros(3, 3, 12, 13)),
        (torch.zeros(0, 12, 13, 3, dtype=torch.uint8), torch.zeros(0, 12, 13, 3, dtype=torch.uint8)),
    ]
    for fn in (metrics.frame_metrics, metrics.psnr, metrics.ssim):
        for a, b in bad:
            with pytest.raises(ValueError):
                fn(a, b)
            with pytest.raises(ValueError):
                fn(b, a)
    for hw in ((10, 40), (40, 10)):
        s = torch.zeros(1, 3, 1, *hw)
        with pytest.raises(ValueError, match="11"):
            metrics.ssim(s, s)
        with pytest.raises(ValueError, match="11"):
            metrics.frame_metrics(s, s)
    assert emulated == []                                    # nothing reached the kernel call


def test_views_are_described_in_place_and_other_layouts_copied_once():
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    x = torch.zeros(4, 3, 5, 14, 13, dtype=torch.bfloat16)
    for v in (x, x[:, :, 1:], x[2:], x[:, :, :, 2:13], x[:, :, :, :, 1:12], x[:, :, ::2]):
        t, cv = ops._clip_view(v)
        assert t.data_ptr() == v.data_ptr() and t.stride() == v.stride()
        assert (cv.layout, cv.dtype) == (L.CLIP_NCTHW, L.BF16) and (cv.sb, cv.sc, cv.st, cv.sy) == v.stride()[:4]
    for v in (x.permute(0, 1, 2, 4, 3), x[..., ::2], x[:, :, :, :1].expand(4, 3, 5, 14, 13)):
        t, cv = ops._clip_view(v)
        assert t.is_contiguous() and t.data_ptr() != v.data_ptr() and torch.equal(t, v) and cv.sy == v.shape[4]
    f = torch.zeros(5, 14, 13, 3, dtype=torch.uint8)
    for v in (f, f[1:], f[:, 2:13], f[:, :, 1:12], f[::2]):
        t, cv = ops._clip_view(v)
        assert t.data_ptr() == v.data_ptr() and cv.layout == L.CLIP_THWC_U8 and (cv.st, cv.sy) == v.stride()[:2]
    for v in (f[..., [2, 1, 0]].permute(0, 1, 2, 3), f.permute(0, 2, 1, 3), f[:, :, ::2]):
        t, cv = ops._clip_view(v)
        assert t.is_contiguous() and torch.equal(t, v) and (cv.st, cv.sy) == t.stride()[:2]
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.frame_metrics(f, f)                              # CPU tensors: no fallback


def test_meter_pools_frames_and_keeps_identical_frames_out_of_the_psnr_mean(emulated):
    from cvvae_amd.metrics import ReconstructionMeter
    a, b = _pair(12, 13, 3, T=3)
    b[1] = a[1]                                              # one identical frame
    c, d = _pair(12, 13, 4, T=2)
    meter = ReconstructionMeter()
    with pytest.raises(RuntimeError):
        meter.compute()
    got1 = meter.update(a, b)
    assert torch.isinf(got1["psnr"][0, 1]) and float(got1["ssim"][0, 1]) == 1.0
    meter.update(c, d)
    out = meter.compute()
    r1, r2 = R.frame_metrics(a, b), R.frame_metrics(c, d)
    psnrs = [float(v) for v in torch.cat([r1[1].flatten(), r2[1].flatten()]) if math.isfinite(float(v))]
    ssims = torch.cat([r1[2].float().flatten(), r2[2].float().flatten()]).double()
    assert out["frames"] == 5 and out["identical_frames"] == 1 and out["lpips"] is None
    assert out["psnr"] == pytest.approx(sum(psnrs) / 4, rel=1e-12) and out["ssim"] == pytest.approx(float(ssims.mean()), rel=1e-12)
    assert all(type(out[k]) is float for k in ("psnr", "ssim")) and type(out["frames"]) is int
    meter.reset()
    meter.update(a[1:2], b[1:2])
    out = meter.compute()
    assert out["frames"] == 1 and out["identical_frames"] == 1 and math.isnan(out["psnr"]) and out["ssim"] == 1.0


def test_meter_feeds_lpips_the_same_frames_in_unit_range(emulated):
    from cvvae_amd.metrics import ReconstructionMeter

    class FakeLPIPS:
        compute_dtype = torch.float32

        def __call__(self, x, y):
            assert x.shape == y.shape and x.shape[1] == 3 and x.dim() == 4
            self.last = (x, y)
            return (x - y).abs().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)
    lp = FakeLPIPS()
    meter = ReconstructionMeter(lp)
    a, _ = _pair(16, 17, 5, T=2)
    x = torch.rand(1, 3, 2, 16, 17) * 2 - 1
    m = meter.update(a, x)
    assert torch.equal(lp.last[0], a.permute(0, 3, 1, 2).float() / 127.5 - 1.0)
    assert torch.equal(lp.last[1], x[0].permute(1, 0, 2, 3))
    assert tuple(m["lpips"].shape) == (1, 2)
    assert meter.compute()["lpips"] == pytest.approx(float(m["lpips"].double().mean()), rel=1e-12)
