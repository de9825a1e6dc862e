"""The data side of CV-VAE training on the MI355X: decoded uint8 frames -> the `[B,3,T,H,W]` batch in [-1,1] that
`engine.training_step(batch, i)` takes.

The reference does this on the host, per sample (`lvdm/data/decoder.py:71-109,122`, `lvdm/data/transform.py:66-121`): the uint8
frames become a float `[T,C,H,W]` tensor, `transforms.Resize` resizes every whole frame, `RandomCrop` / `CenterCrop` keeps a window,
`(x / 255 - 0.5) * 2`, `permute`, and the float tensor is uploaded.  Here the uint8 frames go to the device as uint8 and ONE HIP pass
(`ops.clip_from_frames_u8`, csrc/clip_kernels.hip) does frame selection, the float bilinear resize of ONLY the crop window, the
normalisation and the layout move straight into the batch slot.  torchvision, PIL and decord are not needed: their arithmetic is
restated below and cited; the host tests pin it to `F.interpolate` in fp64 (tests/test_clip_transform_host.py).

ONE DEVIATION from the reference's objects: its spatial transform maps a float `[T,C,H,W]` tensor to a resized and cropped float
tensor and the decoder normalises and permutes afterwards; `ClipTransform` takes the uint8 frames `[T,H,W,3]` and returns the
finished clip `[3,T,h,w]`.  Reading files (decord, webdataset, `CustomDataModuleFromConfig`) stays the user's: any reader that yields
uint8 `[T,H,W,3]` feeds this."""
import math
import random
from typing import List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

from . import ops

__all__ = ["resized_size", "resample_tables", "center_crop_origin", "draw_random_crop", "sample_clip_indices", "ClipTransform",
           "ImageTransform", "collate_clips"]

Size = Union[int, Sequence[int]]


def _pair(v: Size) -> Tuple[int, int]:
    if isinstance(v, int):
        return v, v
    if len(v) == 1:
        return int(v[0]), int(v[0])
    h, w = v
    return int(h), int(w)


def resized_size(h: int, w: int, size: Size, cover: bool = False) -> Tuple[int, int]:
    """the frame size after the resize.  `Resize(int)` (torchvision's `_compute_resized_output_size`): the short side becomes `size`,
    the long side `int(size * long / short)`.  `Resize((h, w))`: exactly that.  cover=True is the reference's `CoverResize`
    (`lvdm/data/transform.py:49-55`): the larger of the two scale factors, each side `round(side * factor)`."""
    if cover:
        th, tw = _pair(size)
        f = max(th / h, tw / w)
        return round(h * f), round(w * f)
    if isinstance(size, int) or len(size) == 1:
        s = size if isinstance(size, int) else int(size[0])
        short, long = (h, w) if h <= w else (w, h)
        new_long = int(s * long / short)
        return (s, new_long) if h <= w else (new_long, s)
    return _pair(size)


def _taps(n_in: int, n_out: int, antialias: bool, lo: int, hi: int):
    """-> (first input position, tap count, fp64 weights) per output position in [lo, hi), and the table width k"""
    if not 0 <= lo < hi <= n_out:
        raise ValueError(f"resample_tables: output positions [{lo},{hi}) of {n_out}")
    if n_in == n_out:
        return [(i, 1, [1.0]) for i in range(lo, hi)], 1
    scale = n_in / n_out
    rows = []
    if antialias:
        # torch's separable antialias filter (aten UpSampleKernel.cpp `_compute_indices_min_size_weights_aa`, triangle filter): what
        # ops.resize_tables computes before it quantises the weights to integers
        support = scale if scale >= 1.0 else 1.0
        invscale = 1.0 / scale if scale >= 1.0 else 1.0
        for i in range(lo, hi):
            center = scale * (i + 0.5)
            a = max(0, int(center - support + 0.5))
            b = min(n_in, int(center + support + 0.5))
            ws = [max(0.0, 1.0 - abs((j + a - center + 0.5) * invscale)) for j in range(b - a)]
            tot = sum(ws)
            ws = [v / tot for v in ws]
            while len(ws) > 1 and ws[-1] == 0.0:      # a tap of weight zero at the end reads nothing
                ws.pop()
            rows.append((a, len(ws), ws))
        return rows, max(r[1] for r in rows)      # (never more than ceil(support) * 2 + 1)
    # torch's plain bilinear with align_corners=False (aten UpSample.h `area_pixel_compute_source_index`, `guard_index_and_lambda`)
    for i in range(lo, hi):
        src = max(0.0, scale * (i + 0.5) - 0.5)
        a = min(int(src), n_in - 1)
        lam = min(max(src - a, 0.0), 1.0)
        if a < n_in - 1:
            rows.append((a, 2, [1.0 - lam, lam]))
        else:
            rows.append((a, 1, [1.0]))
    return rows, max(r[1] for r in rows)


def resample_tables(n_in: int, n_out: int, antialias: bool, lo: int = 0, hi: Optional[int] = None, dtype: torch.dtype = torch.float32):
    """Tap tables of ONE axis of torch's bilinear interpolation of float tensors (`F.interpolate(mode="bilinear",
    align_corners=False, antialias=...)`, which is what `transforms.Resize` runs on the decoder's float clip) for the output positions
    [lo, hi) of n_out -> (xmin int32 [hi-lo], xsize int32 [hi-lo], weights [hi-lo, k], k): output position lo + i is
    sum_j weights[i, j] * src[xmin[i] + j] over j < xsize[i]; weights beyond xsize are 0.  Computed in Python floats (fp64) and
    rounded ONCE to `dtype` (fp32 is what the kernel reads; float64 keeps them as computed, for checks against fp64 torch).
    antialias=True: the triangle filter of `ops.resize_tables` before its integer quantisation.  antialias=False: source position
    max(0, n_in / n_out * (i + 0.5) - 0.5), taps (1 - lambda, lambda), one tap at the last input position.  n_in == n_out: identity
    tables, one tap of weight 1.0."""
    hi = n_out if hi is None else hi
    rows, k = _taps(int(n_in), int(n_out), bool(antialias), int(lo), int(hi))
    xmin = torch.tensor([r[0] for r in rows], dtype=torch.int32)
    xsize = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    w = torch.tensor([r[2] + [0.0] * (k - r[1]) for r in rows], dtype=torch.float64).to(dtype)
    return xmin, xsize, w, k


def center_crop_origin(h: int, w: int, th: int, tw: int) -> Tuple[int, int]:
    """(top, left) of torchvision's `center_crop` (transforms/functional.py): `int(round((h - th) / 2.0))` per axis.  A crop larger
    than the frame raises: torchvision pads there, which is not built."""
    if th > h or tw > w:
        raise ValueError(f"crop {th}x{tw} is larger than the resized frame {h}x{w} (padding is not built)")
    return int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))


def draw_random_crop(h: int, w: int, th: int, tw: int, generator: Optional[torch.Generator] = None) -> Tuple[int, int]:
    """(top, left) of torchvision's `RandomCrop.get_params`: `torch.randint(0, h - th + 1, (1,))`, then `torch.randint(0, w - tw + 1,
    (1,))`, in that order; no draw at all when the sizes are equal.  generator=None draws from torch's global generator, as
    torchvision does."""
    if th > h or tw > w:
        raise ValueError(f"crop {th}x{tw} is larger than the resized frame {h}x{w} (padding is not built)")
    if (h, w) == (th, tw):
        return 0, 0
    top = int(torch.randint(0, h - th + 1, size=(1,), generator=generator).item())
    left = int(torch.randint(0, w - tw + 1, size=(1,), generator=generator).item())
    return top, left


def sample_clip_indices(frame_num: int, video_length: int, frame_stride_range: Sequence[int] = (1, 8), rng=random,
                        random_start_frame: bool = True) -> Optional[Tuple[List[int], int]]:
    """The frame choice of the reference's video decoders (`lvdm/data/decoder.py:71-91`) -> (indices, frame_stride), or None when
    the video has fewer than `video_length` frames (no draw is made then).  One stride draw `rng.randint(lo, hi)`; a video too short
    for that stride falls back to `frame_num // video_length`; one start draw `rng.randint(0, slack)` when there is slack and
    random_start_frame, else start 0.  rng: the `random` module or a `random.Random`."""
    if frame_num < video_length:
        return None
    stride = rng.randint(frame_stride_range[0], frame_stride_range[1])
    need = stride * (video_length - 1) + 1
    if frame_num < need:
        stride = frame_num // video_length
        need = stride * (video_length - 1) + 1
    slack = frame_num - need
    start = rng.randint(0, slack) if (random_start_frame and slack > 0) else 0
    return [start + stride * i for i in range(video_length)], stride


class _AxisCache:
    """whole-axis tables per (n_in, n_out, antialias, device): the host lists and ONE device copy.  A crop window [lo, hi) is a slice
    of the device tensors (rows of a contiguous table are contiguous), so a new random origin uploads nothing."""

    MAX = 64

    def __init__(self):
        self._d = {}

    def window(self, n_in: int, n_out: int, lo: int, hi: int, antialias: bool, device) -> "ops.ClipAxisTable":
        key = (n_in, n_out, bool(antialias), str(device))
        e = self._d.get(key)
        if e is None:
            if len(self._d) >= self.MAX:
                self._d.clear()
            xmin, xsize, w, k = resample_tables(n_in, n_out, antialias)
            ends = (xmin + xsize).tolist()
            e = (xmin.tolist(), ends, xmin.to(device), xsize.to(device), w.to(device), k)
            self._d[key] = e
        mins, ends, dmin, dsize, dw, k = e
        return ops.ClipAxisTable(dmin[lo:hi], dsize[lo:hi], dw[lo:hi], k, min(mins[lo:hi]), max(ends[lo:hi]))


def _as_clip(frames_u8: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8:
        raise ValueError(f"{what}: uint8 frames [T,H,W,3] (or one image [H,W,3]); got "
                         f"{getattr(frames_u8, 'dtype', type(frames_u8).__name__)}")
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8[None]          # the YAML's add_time_dim: an image is a one-frame clip
    if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3 or frames_u8.numel() == 0:
        raise ValueError(f"{what}: uint8 frames [T,H,W,3] (or one image [H,W,3]); got {tuple(frames_u8.shape)}")
    return frames_u8


def _upload(frames_u8: torch.Tensor, device) -> torch.Tensor:
    """a CPU tensor goes to the device AS uint8 (a quarter of the float bytes); asynchronously when it is pinned"""
    if frames_u8.is_cuda or device is None:
        return frames_u8
    return frames_u8.to(device, non_blocking=frames_u8.is_pinned())


def _index_list(frame_indices, T_in: int) -> Optional[List[int]]:
    if frame_indices is None or isinstance(frame_indices, torch.Tensor) and frame_indices.is_cuda:
        return None
    idx = [int(i) for i in (frame_indices.tolist() if isinstance(frame_indices, torch.Tensor) else frame_indices)]
    if not idx or min(idx) < 0 or max(idx) >= T_in:
        raise ValueError(f"frame_indices {idx} outside the {T_in} decoded frames")
    return idx


class ClipTransform:
    """uint8 frames `[T,H,W,3]` -> the training clip `[3,T',h,w]` in [-1,1]: resize (short side / exact size / cover), random or
    centre crop to `resolution`, `(x / 255 - 0.5) * 2`, channels first -- the reference's `transforms.Resize` + `RandomCrop` /
    `CenterCrop` (`lvdm/data/transform.py:66-109`) and the decoder's normalisation and permute (`lvdm/data/decoder.py:99-109,122`) in
    one object (the module docstring states the deviation).

    resolution: int or (h, w), the crop.  resize_resolution: None (no resize), int (short side) or (h, w); with cover=True the
    (h, w) is covered (`CoverResize`).  antialias=True is what current torchvision does for tensors (and the project's uint8
    resize); False is what older torchvision did for tensors -- the reference pins no version, so both are built.

    __call__(frames_u8, frame_indices=None, generator=None, out=None, origin=None):
      a device tensor runs the HIP pass; a CPU tensor with `device=` set is uploaded as uint8 (non_blocking when pinned) and runs
      it; a CPU tensor with no device takes the eager torch expression, the reference's arithmetic (as the discriminator does for
      CPU tensors).  frame_indices picks T' frames out of a longer decoded buffer in place (a list, or an int32 device tensor that is
      trusted).  generator feeds the random crop's draw.  out: a `[3,T',h,w]` view such as `batch[b]`, written in place.
      origin=(top, left) fixes the crop and makes no draw."""

    def __init__(self, resolution: Size, resize_resolution: Optional[Size] = None, random_crop: bool = False, cover: bool = False,
                 antialias: bool = True, dtype: torch.dtype = torch.float32, device=None):
        self.resolution = _pair(resolution)
        self.resize_resolution = resize_resolution if resize_resolution is None or isinstance(resize_resolution, int) \
            else tuple(int(v) for v in resize_resolution)
        if cover and (self.resize_resolution is None or isinstance(self.resize_resolution, int) or len(self.resize_resolution) != 2):
            raise ValueError("size must be (h, w)")      # CoverResize's own condition
        self.random_crop, self.cover, self.antialias = bool(random_crop), bool(cover), bool(antialias)
        if dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise ValueError(f"ClipTransform: the clip is fp16 / bf16 / fp32; got {dtype}")
        self.dtype = dtype
        self.device = None if device is None else torch.device(device)
        self._tables = _AxisCache()

    def __repr__(self):
        return (f"{type(self).__name__}(resolution={self.resolution}, resize_resolution={self.resize_resolution}, "
                f"random_crop={self.random_crop}, cover={self.cover}, antialias={self.antialias}, dtype={self.dtype}, device={self.device})")

    def plan(self, H: int, W: int, generator: Optional[torch.Generator] = None, origin: Optional[Tuple[int, int]] = None):
        """-> (resized height, resized width, top, left) for a raw frame H x W; makes the random crop's draw"""
        rh, rw = (H, W) if self.resize_resolution is None else resized_size(H, W, self.resize_resolution, self.cover)
        th, tw = self.resolution
        if origin is not None:
            top, left = int(origin[0]), int(origin[1])
            if top < 0 or left < 0 or top + th > rh or left + tw > rw:
                raise ValueError(f"crop {th}x{tw} at {(top, left)} leaves the resized frame {rh}x{rw}")
        elif self.random_crop:
            top, left = draw_random_crop(rh, rw, th, tw, generator)
        else:
            top, left = center_crop_origin(rh, rw, th, tw)
        return rh, rw, top, left

    def eager(self, frames_u8: torch.Tensor, rh: int, rw: int, top: int, left: int) -> torch.Tensor:
        """the reference's arithmetic in eager torch, fp32: float [T,C,H,W], F.interpolate, crop, normalise, permute"""
        th, tw = self.resolution
        x = frames_u8.permute(0, 3, 1, 2).float()
        if (rh, rw) != tuple(x.shape[-2:]):
            x = F.interpolate(x, size=(rh, rw), mode="bilinear", align_corners=False, antialias=self.antialias)
        x = x[:, :, top:top + th, left:left + tw]
        x = (x / 255 - 0.5) * 2
        return x.permute(1, 0, 2, 3).to(self.dtype)

    def __call__(self, frames_u8: torch.Tensor, frame_indices=None, generator: Optional[torch.Generator] = None,
                 out: Optional[torch.Tensor] = None, origin: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        frames_u8 = _as_clip(frames_u8, type(self).__name__)
        T_in, H, W, _ = frames_u8.shape
        idx = _index_list(frame_indices, T_in)
        T_out = T_in if frame_indices is None else (len(idx) if idx is not None else int(frame_indices.numel()))
        rh, rw, top, left = self.plan(H, W, generator, origin)
        th, tw = self.resolution
        if out is not None and tuple(out.shape) != (3, T_out, th, tw):
            raise ValueError(f"out is [3,{T_out},{th},{tw}]; got {tuple(out.shape)}")
        if not frames_u8.is_cuda and self.device is None:
            if frame_indices is not None:
                frames_u8 = frames_u8[torch.as_tensor(idx) if idx is not None else frame_indices.cpu().long()]
            clip = self.eager(frames_u8, rh, rw, top, left)
            return clip if out is None else out.copy_(clip)
        frames_u8 = _upload(frames_u8, self.device)
        dev = frames_u8.device
        with torch.cuda.device(dev):
            if idx is not None:
                frame_indices = torch.tensor(idx, dtype=torch.int32).to(dev)
            ytab = self._tables.window(H, rh, top, top + th, self.antialias, dev)
            xtab = self._tables.window(W, rw, left, left + tw, self.antialias, dev)
            if out is None:
                out = torch.empty((3, T_out, th, tw), dtype=self.dtype, device=dev)
            return ops.clip_from_frames_u8(frames_u8, frame_indices, ytab, xtab, out)


class ImageTransform:
    """The YAML's image datapipe (`get_image_transform`: `Resize(min(resolution))`, `CenterCrop(resolution)`, `ToTensor`, then the
    decoder's `(x - 0.5) * 2`, `lvdm/data/transform.py:112-121`, `lvdm/data/decoder.py:161-166`) on uint8 images `[H,W,3]` or frames
    `[T,H,W,3]` -> `[3,T,h,w]`.  An image is resized AS uint8 (antialiased bilinear, what torchvision does for a PIL image and for a
    uint8 tensor): `ops.resize_frames_u8`, then the clip pass with identity tables over the centre-crop window.  For a uint8 value u,
    `(u / 255 - 0.5) * 2` in fp32 is the same expression, so the device path equals eager torch bit for bit.  A CPU tensor with no
    device takes the eager expression."""

    def __init__(self, resolution: Size, dtype: torch.dtype = torch.float32, device=None):
        self.resolution = _pair(resolution)
        self._crop = ClipTransform(self.resolution, None, random_crop=False, dtype=dtype, device=device)
        self.dtype, self.device = self._crop.dtype, self._crop.device

    def __repr__(self):
        return f"{type(self).__name__}(resolution={self.resolution}, dtype={self.dtype}, device={self.device})"

    def __call__(self, image_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        frames = _as_clip(image_u8, type(self).__name__)
        _, H, W, _ = frames.shape
        rh, rw = resized_size(H, W, min(self.resolution))
        if not frames.is_cuda and self.device is None:
            x = frames.permute(0, 3, 1, 2)
            if (rh, rw) != (H, W):
                x = F.interpolate(x, size=(rh, rw), mode="bilinear", align_corners=False, antialias=True)
            top, left = center_crop_origin(rh, rw, *self.resolution)
            x = x[:, :, top:top + self.resolution[0], left:left + self.resolution[1]]
            x = (x.float().div(255) - 0.5) * 2
            clip = x.permute(1, 0, 2, 3).to(self.dtype)
            return clip if out is None else out.copy_(clip)
        frames = _upload(frames, self.device)
        with torch.cuda.device(frames.device):
            if (rh, rw) != (H, W):
                frames = ops.resize_frames_u8(frames.contiguous(), (rh, rw))
            return self._crop(frames, out=out)


def collate_clips(clips: Sequence[torch.Tensor], transform: ClipTransform, frame_indices=None,
                  generator: Optional[torch.Generator] = None) -> dict:
    """a list of uint8 clips `[T_b,H_b,W_b,3]` (raw resolutions may differ) -> `{"frames": [B,3,T,h,w]}`: one launch per sample,
    straight into its slot of the batch.  frame_indices: None or one entry per sample (each picks the same number of frames)."""
    if len(clips) == 0:
        raise ValueError("collate_clips: no clips")
    if frame_indices is not None and len(frame_indices) != len(clips):
        raise ValueError(f"collate_clips: {len(frame_indices)} frame_indices for {len(clips)} clips")
    fi = [None] * len(clips) if frame_indices is None else list(frame_indices)
    first = _as_clip(clips[0], "collate_clips")
    T = first.shape[0] if fi[0] is None else len(fi[0])
    device = first.device if first.is_cuda else (transform.device or first.device)
    batch = torch.empty((len(clips), 3, T) + tuple(transform.resolution), dtype=transform.dtype, device=device)
    for b, clip in enumerate(clips):
        transform(clip, fi[b], generator, out=batch[b])
    return {"frames": batch}
