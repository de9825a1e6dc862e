"""Drop-in import path of the reference (`lvdm.data...`): the spatial transforms the training YAML names (`lvdm/data/transform.py`),
as objects that run on the MI355X (cvvae_amd/data.py).  Reading files -- the decoders, webdataset, `CustomDataModuleFromConfig` --
is not part of this package: any reader that yields uint8 frames `[T,H,W,3]` feeds the transforms."""
from .transform import get_image_transform, get_video_spatial_transform, get_webvid_spatial_transform  # noqa: F401

__all__ = ["get_webvid_spatial_transform", "get_video_spatial_transform", "get_image_transform"]
