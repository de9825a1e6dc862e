"""The fp64 restatement of cvvae_frame_metrics on the CPU (torch / numpy): the 8-bit mapping of an operand in its own dtype, then
sse, psnr and the Gaussian-window SSIM in float64.  tests/test_metrics_host.py checks this module against scipy's gaussian_filter
(skimage's own construction), the closed form for flat frames and a direct 11 x 11 double loop; tests/test_gpu_metrics_edges.py
holds the HIP kernel to it."""
import math

import numpy as np
import torch

C1, C2 = 2.55 * 2.55, 7.65 * 7.65
WIN = 11
SSIM_ATOL = 1e-6      # the issue's condition on the kernel's ssim, absolute
SSE_RTOL = 1e-12      # sse on non-integer operands: fp64 accumulation in another order


def window() -> np.ndarray:
    g = np.exp(-((np.arange(WIN) - 5.0) ** 2) / 4.5)
    return g / g.sum()


def quantize_u8(x: torch.Tensor) -> torch.Tensor:
    """the byte cvvae_ncdhw_to_frames_u8 stores for each value of a float tensor, written as the kernel evaluates it: fp32 operations,
    each result rounded once to the tensor's dtype, then truncation.  (test_metrics_host.py: equal to the scripts' torch expression)"""
    dt = x.dtype
    c = torch.clamp(x.float(), -1.0, 1.0)
    a = (c + 1.0).to(dt)
    m = (a.float() * 127.5).to(dt)
    return torch.trunc(m.float()).to(torch.uint8)


def to_scale8(x: torch.Tensor, quantize: bool = True) -> np.ndarray:
    """an operand -> float64 [B,3,T,H,W] on the 8-bit scale.  uint8 frames [T,H,W,3] as they are; a float clip through the scripts'
    post-processing in ITS OWN dtype (clamp, + 1 and * 127.5 each rounded to the dtype, truncation) or, quantize=False, through
    (clamp(x,-1,1) + 1) * 127.5 in fp32, unrounded"""
    if x.dtype == torch.uint8:
        return x.permute(3, 0, 1, 2)[None].double().numpy()
    if quantize:
        return quantize_u8(x).double().numpy()
    return ((torch.clamp(x.float(), -1.0, 1.0) + 1.0) * 127.5).double().numpy()


def _valid(x: np.ndarray, g: np.ndarray) -> np.ndarray:
    """separable 'valid' correlation of the last two axes with g, float64"""
    W = x.shape[-1]
    h = sum(g[k] * x[..., k:k + W - WIN + 1] for k in range(WIN))
    H = h.shape[-2]
    return sum(g[k] * h[..., k:k + H - WIN + 1, :] for k in range(WIN))


def ssim_map(u: np.ndarray, v: np.ndarray) -> np.ndarray:
    """[..., H, W] float64 on the 8-bit scale -> the SSIM map [..., H-10, W-10]"""
    g = window()
    mx, my = _valid(u, g), _valid(v, g)
    vx, vy, cxy = _valid(u * u, g) - mx * mx, _valid(v * v, g) - my * my, _valid(u * v, g) - mx * my
    return ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def psnr_of(sse: float, n: int) -> float:
    return math.inf if sse == 0 else 10.0 * math.log10(65025.0 * n / sse)


def frame_metrics(a: torch.Tensor, b: torch.Tensor, quantize: bool = True, want_ssim: bool = True):
    """-> (sse float64 [B,T], psnr float32 [B,T], ssim float64 [B,T] or None), all torch CPU tensors.  ssim stays float64 here so that a
    test can measure the kernel's float32 against it; its float32 rounding is what the public layer returns."""
    u, v = to_scale8(a, quantize), to_scale8(b, quantize)
    assert u.shape == v.shape, (u.shape, v.shape)
    B, _, T, H, W = u.shape
    d = u - v
    sse = (d * d).sum(axis=(1, 3, 4))
    psnr = np.array([[psnr_of(float(sse[i, t]), 3 * H * W) for t in range(T)] for i in range(B)], dtype=np.float64).astype(np.float32)
    ssim = None
    if want_ssim:
        ssim = torch.from_numpy(ssim_map(u, v).mean(axis=(1, 3, 4)))
    return torch.from_numpy(sse), torch.from_numpy(psnr), ssim


def integer_valued(a: torch.Tensor, b: torch.Tensor, quantize: bool) -> bool:
    """both operands land on integer values of the 8-bit scale: sse is then exact in any order of summation"""
    return all(t.dtype == torch.uint8 or quantize for t in (a, b))


def ulp32(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))
