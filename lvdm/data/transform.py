"""`lvdm.data.transform` as the training YAML names it (`spatial_transform_config.target:
lvdm.data.transform.get_webvid_spatial_transform`): the three factories with the reference's parameter names and defaults
(`lvdm/data/transform.py:66-121`), returning the device-side objects of cvvae_amd/data.py.

The returned object takes the decoded uint8 frames `[T,H,W,3]` and returns the finished clip `[3,T,h,w]` in [-1,1] -- resize,
crop, `(x / 255 - 0.5) * 2` and the permute in one HIP pass -- where the reference's `transforms.Compose` maps a float `[T,C,H,W]`
tensor to a resized and cropped one and leaves normalisation and permute to the decoder.  `antialias`, `dtype` and `device` are
additions (keyword only)."""
import torch

from cvvae_amd.data import ClipTransform, ImageTransform

__all__ = ["get_webvid_spatial_transform", "get_video_spatial_transform", "get_image_transform"]


def _res(resolution):
    return [resolution, resolution] if isinstance(resolution, int) else list(resolution)


def get_webvid_spatial_transform(resolution=[256, 512], resize_resolution=None, random_crop=False, *, antialias=True,
                                 dtype=torch.float32, device=None):
    """`Resize(resize_resolution)` (default: the short side to `min(resolution)`), then `RandomCrop` / `CenterCrop(resolution)`"""
    resolution = _res(resolution)
    if resize_resolution is None:
        resize_resolution = min(resolution)
    return ClipTransform(resolution, resize_resolution, random_crop=random_crop, antialias=antialias, dtype=dtype, device=device)


def get_video_spatial_transform(resolution=[256, 512], resize_resolution=None, random_crop=False, *, antialias=True,
                                dtype=torch.float32, device=None):
    """`CoverResize(resize_resolution)` (default: `resolution`), then `RandomCrop` / `CenterCrop(resolution)`"""
    resolution = _res(resolution)
    if resize_resolution is None:
        resize_resolution = resolution
    return ClipTransform(resolution, resize_resolution, random_crop=random_crop, cover=True, antialias=antialias, dtype=dtype,
                         device=device)


def get_image_transform(resolution=[256, 512], to_tensor=True, *, dtype=torch.float32, device=None):
    """`Resize(min(resolution))`, `CenterCrop(resolution)`, `ToTensor` and the image decoders' `(x - 0.5) * 2`.  to_tensor=False
    (a PIL image out) has no counterpart here."""
    if not to_tensor:
        raise ValueError("get_image_transform(to_tensor=False) returns a PIL image in the reference; only the tensor path is built")
    return ImageTransform(_res(resolution), dtype=dtype, device=device)
