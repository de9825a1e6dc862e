"""Time the per-frame metrics pass on an MI355X: PSNR + SSIM of two clips of [1,3,17,512,512] as
  (a) `hip`:      cvvae_amd.ops.frame_metrics (csrc/metrics_kernels.hip: one pass over both operands + a one-wave-per-frame finish),
                  uint8 frames against uint8 frames and a bf16 clip against a bf16 clip;
  (b) `conv2d64`: the same metric as a user writes it today -- the operands to the 8-bit scale, five depthwise F.conv2d in fp64 with the
                  11 x 11 window, the SSIM map, the means -- on the same GPU (fp64 because the fp32 expression is wrong by 1e-3);
the two taking turns call by call in ONE process, on the same inputs.

    timeout -k 10 600 python tools/metrics_step.py                 # writes profiles/metrics_step.json

Each figure is the median over `--iters` calls of the time between two device events around the call (host time that the device does
not hide is in it), after `--warmup` untimed calls.  `bytes_read` is what the metric has to read (both operands, once) and
`read_bytes_per_s` is that over the median time, against 6.3e12 bytes/s of achievable HBM bandwidth; `fma_per_s` counts the pass's
fp64 FMAs (5 sums x 11 taps x 2 passes per map position).  The results of the two paths are compared before anything is timed.
There is no CPU path.  No speed bar is asserted; the figures are recorded."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvvae_amd import _lib, ops  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SHAPE = (1, 3, 17, 512, 512)


def window64(device):
    g = torch.exp(-((torch.arange(11, dtype=torch.float64, device=device) - 5.0) ** 2) / 4.5)
    g = g / g.sum()
    return (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()


def conv2d64(a, b, k):
    """PSNR and SSIM per frame as written with torch ops, fp64: operands uint8 [T,H,W,3] or float [1,3,T,H,W] (quantized as the scripts do)"""
    def scale8(x):
        if x.dtype == torch.uint8:
            return x.permute(0, 3, 1, 2).double()
        return ((torch.clamp(x, -1.0, 1.0) + 1.0) * 127.5).to(torch.uint8)[0].permute(1, 0, 2, 3).double()
    u, v = scale8(a), scale8(b)                       # [T,3,H,W]
    mse = ((u - v) ** 2).mean(dim=(1, 2, 3))
    psnr = 10.0 * torch.log10(65025.0 / mse)
    mx, my = F.conv2d(u, k, groups=3), F.conv2d(v, k, groups=3)
    vx, vy, cxy = F.conv2d(u * u, k, groups=3) - mx * mx, F.conv2d(v * v, k, groups=3) - my * my, F.conv2d(u * v, k, groups=3) - mx * my
    c1, c2 = 2.55 * 2.55, 7.65 * 7.65
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return psnr, s.mean(dim=(1, 2, 3))


def timed(fns, warmup, iters):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "iters": iters} for k, v in ts.items()}


def measure(kind, warmup, iters):
    B, C, T, H, W = SHAPE
    g = torch.Generator().manual_seed(7)
    base = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8)
    noisy = torch.clamp(base.int() + torch.randint(-6, 7, base.shape, generator=g), 0, 255).to(torch.uint8)
    if kind == "u8":
        a, b = base.cuda(), noisy.cuda()
    else:
        a, b = ((x.permute(3, 0, 1, 2)[None].float() / 127.5 - 1.0).to(torch.bfloat16).cuda() for x in (base, noisy))
    k = window64("cuda")
    sse, psnr, ssim = ops.frame_metrics(a, b)
    psnr_t, ssim_t = conv2d64(a, b, k)
    d_psnr = float((psnr[0].double() - psnr_t).abs().max())
    d_ssim = float((ssim[0].double() - ssim_t).abs().max())
    assert d_psnr < 1e-4 and d_ssim < 1e-6, (d_psnr, d_ssim)
    run = timed({"hip": lambda: ops.frame_metrics(a, b), "conv2d64": lambda: conv2d64(a, b, k)}, warmup, iters)
    nbytes = 2 * a.numel() * a.element_size()
    fmas = 3 * T * (H - 10) * (W - 10) * 5 * 11 * 2
    out = {"operands": f"{kind} against {kind}", "bytes_read": nbytes, "fp64_fma": fmas, "max_abs_diff_psnr": d_psnr, "max_abs_diff_ssim": d_ssim}
    for name, r in run.items():
        r["read_bytes_per_s"] = nbytes / (r["median_ms"] * 1e-3)
        r["frac_of_hbm"] = r["read_bytes_per_s"] / HBM_BYTES_PER_S
        out[name] = r
    out["hip"]["fp64_fma_per_s"] = fmas / (out["hip"]["median_ms"] * 1e-3)
    out["conv2d64_over_hip"] = out["conv2d64"]["median_ms"] / out["hip"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/metrics_step.py measures on an MI355X; no GPU found (there is no CPU path)")
    torch.cuda.set_device(0)
    res = {"pass": "per-frame SSE + PSNR + SSIM of two clips, quantize=True", "shape": list(SHAPE), "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "kernel_sources": _lib.source_fingerprint(), "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "timing": "device events around each call, paths interleaved in one process", "runs": {}}
    for kind in ("u8", "bf16"):
        res["runs"][kind] = measure(kind, a.warmup, a.iters)
        print(kind, json.dumps(res["runs"][kind]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
