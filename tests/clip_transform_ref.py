"""References for the training clip transform, on the CPU, shared and never changed by the tests that use them:
  (a) `reference(...)`: torch's own F.interpolate(u.double(), size, mode="bilinear", antialias=..., align_corners=False), crop,
      (x / 255 - 0.5) * 2 in fp64, channels first -- what the kernel is held to;
  (b) `reference(..., dtype=torch.float32)`: the same in fp32, only to report torch's own fp32 error beside the kernel's (it is up
      to 5e-5 from (a), far outside the kernel's bound, so the kernel is never compared against it);
  `image_reference`: the image datapipe, F.interpolate on the uint8 tensor (antialias=True), crop, / 255, (x - 0.5) * 2 in fp32.
`tol32(kh, kw)`: each of the kh + kw multiply-adds, the weight rounding, the division, the subtraction and the doubling contributes
at most 2^-24 relative to a value <= 255, which on the [-1, 1] scale is (kh + kw + 4) * 2^-23."""
import functools

import torch
import torch.nn.functional as F

import clip_transform_cases as CC


def tol32(kh: int, kw: int) -> float:
    return (kh + kw + 4) * 2.0 ** -23


def reference(frames_u8, resized, origin, crop, antialias, frame_index=None, dtype=torch.float64):
    """[T,H,W,3] uint8 -> [3,T',h,w] in `dtype` arithmetic"""
    u = frames_u8 if frame_index is None else frames_u8[torch.tensor(frame_index)]
    x = u.permute(0, 3, 1, 2).to(dtype)
    if tuple(resized) != tuple(x.shape[-2:]):
        x = F.interpolate(x, size=tuple(resized), mode="bilinear", antialias=antialias, align_corners=False)
    (top, left), (th, tw) = origin, crop
    x = x[:, :, top:top + th, left:left + tw]
    return ((x / 255 - 0.5) * 2).permute(1, 0, 2, 3).contiguous()


@functools.lru_cache(maxsize=None)
def case_reference(name, antialias, dtype=torch.float64):
    """reference (a) (or (b) with dtype=torch.float32) of a case of clip_transform_cases.py, computed once"""
    c = CC.BY_NAME[name]
    return reference(CC.frames_of(c), c.resized, CC.origin_of(c), c.crop, antialias, c.frame_index, dtype)


def image_reference(image_u8, resized, crop):
    """[T,H,W,3] uint8 -> [3,T,h,w] fp32: the uint8 antialiased resize, centre crop, ToTensor, (x - 0.5) * 2"""
    x = image_u8.permute(0, 3, 1, 2)
    if tuple(resized) != tuple(x.shape[-2:]):
        x = F.interpolate(x, size=tuple(resized), mode="bilinear", antialias=True, align_corners=False)
    (rh, rw), (th, tw) = resized, crop
    top, left = int(round((rh - th) / 2.0)), int(round((rw - tw) / 2.0))
    x = x[:, :, top:top + th, left:left + tw].float().div(255)
    return ((x - 0.5) * 2).permute(1, 0, 2, 3).contiguous()


def case_taps(case, antialias):
    """(kh, kw): the most taps any output position of the case's crop window has, per axis"""
    from cvvae_amd.data import resample_tables
    (top, left), (th, tw) = CC.origin_of(case), case.crop
    _, H, W = case.frames
    kh = int(resample_tables(H, case.resized[0], antialias, top, top + th)[1].max())
    kw = int(resample_tables(W, case.resized[1], antialias, left, left + tw)[1].max())
    return kh, kw
