"""How good a reconstruction is: per-frame PSNR and SSIM of two clips on the 8-bit scale (data_range = 255), in one pass of the HIP
kernel behind ops.frame_metrics, and a meter that pools them (and LPIPS) over many clips -- the paper's PSNR / SSIM / LPIPS triple.

An operand is uint8 frames [T,H,W,3] (decord's layout, what decode_to_frames_u8 returns; B = 1) or a float clip [B,3,T,H,W] in
[-1,1] (fp16 / bf16 / fp32); the two are chosen independently.  quantize=True (the default) puts a float value on the byte the
scripts' post-processing would store for it, so a float reconstruction scores exactly as its written frames would;
quantize=False keeps (clamp(x,-1,1)+1)*127.5 unrounded.  SSIM is the Gaussian-window definition of Wang et al. (11 taps, sigma
1.5, valid positions, C1 = 2.55^2, C2 = 7.65^2), i.e. skimage's structural_similarity(gaussian_weights=True, sigma=1.5,
use_sample_covariance=False) and pytorch-msssim's.  Everything returned is a device tensor [B,T]; nothing synchronises the host."""
from typing import TYPE_CHECKING, Dict, Optional

import torch

from . import ops

if TYPE_CHECKING:
    from .lpips import LPIPS


def frame_metrics(a: torch.Tensor, b: torch.Tensor, *, quantize: bool = True) -> Dict[str, torch.Tensor]:
    """-> {"sse": fp64 [B,T], "psnr": fp32 [B,T] (+inf for identical frames), "ssim": fp32 [B,T]}"""
    ops.check_metric_operands(a, b, True)
    sse, psnr_, ssim_ = ops.frame_metrics(a, b, quantize=quantize, want_ssim=True)
    return {"sse": sse, "psnr": psnr_, "ssim": ssim_}


def psnr(a: torch.Tensor, b: torch.Tensor, *, quantize: bool = True) -> torch.Tensor:
    """10 log10(255^2 * 3HW / sse) per frame, fp32 [B,T]; +inf where the two frames are identical.  Any H, W."""
    ops.check_metric_operands(a, b, False)
    return ops.frame_metrics(a, b, quantize=quantize, want_ssim=False)[1]


def ssim(a: torch.Tensor, b: torch.Tensor, *, quantize: bool = True) -> torch.Tensor:
    """Gaussian-window SSIM per frame (mean over the 3 channels and the valid positions), fp32 [B,T].  H, W >= 11."""
    ops.check_metric_operands(a, b, True)
    return ops.frame_metrics(a, b, quantize=quantize, want_ssim=True)[2]


def _unit_frames(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """an operand as LPIPS takes it: [(B T),3,H,W] in [-1,1]; uint8 frames as u8 / 127.5 - 1"""
    if x.dtype == torch.uint8:
        return (x.permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1.0).to(dtype)
    return x.permute(0, 2, 1, 3, 4).reshape(-1, 3, x.shape[3], x.shape[4]).to(dtype)


class ReconstructionMeter:
    """Pools per-frame PSNR / SSIM (/ LPIPS, when given the network) over every clip passed to update(); the sums live on the device
    and compute() is the only host synchronisation.  Identical frames (PSNR = +inf) are counted and kept out of the PSNR mean."""

    def __init__(self, lpips: Optional["LPIPS"] = None):
        self.lpips = lpips
        self._acc: Optional[torch.Tensor] = None  # fp64 [6]: psnr sum, finite-psnr frames, identical frames, ssim sum, lpips sum, frames

    def reset(self) -> None:
        self._acc = None

    @torch.no_grad()
    def update(self, a: torch.Tensor, b: torch.Tensor, *, quantize: bool = True) -> Dict[str, torch.Tensor]:
        """score one pair of clips and add it to the sums -> the per-frame tensors (frame_metrics', plus "lpips" with the network)"""
        m = frame_metrics(a, b, quantize=quantize)
        p = m["psnr"]
        finite = torch.isfinite(p)
        lp = p.new_zeros((), dtype=torch.float64)
        if self.lpips is not None:
            cd = self.lpips.compute_dtype
            m["lpips"] = self.lpips(_unit_frames(a, cd), _unit_frames(b, cd)).float().view(p.shape)
            lp = m["lpips"].double().sum()
        add = torch.stack([torch.where(finite, p, torch.zeros_like(p)).double().sum(), finite.sum().double(),
                           (m["sse"] == 0).sum().double(), m["ssim"].double().sum(), lp,
                           torch.full((), float(p.numel()), dtype=torch.float64, device=p.device)])
        self._acc = add if self._acc is None else self._acc + add
        return m

    def compute(self, group=None) -> Dict[str, float]:
        """-> {"psnr": mean over the non-identical frames (nan if there is none), "ssim", "lpips" (None without the network), "frames",
        "identical_frames"} as plain Python numbers; one device-to-host copy.  group (a torch.distributed process group): the six
        sums are all-reduced over it first, so every rank returns the figures pooled over all ranks' clips; the meter's own sums stay"""
        if self._acc is None:
            raise RuntimeError("ReconstructionMeter.compute() before any update()")
        acc = self._acc
        if group is not None:
            from .ddp import all_reduce_sum
            acc = all_reduce_sum(acc.clone(), group)
        s_psnr, n_finite, n_same, s_ssim, s_lpips, n = acc.tolist()
        return {"psnr": s_psnr / n_finite if n_finite else float("nan"), "ssim": s_ssim / n,
                "lpips": s_lpips / n if self.lpips is not None else None, "frames": int(n), "identical_frames": int(n_same)}
