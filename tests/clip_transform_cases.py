"""One case list for the training clip transform (cvvae_clip_from_frames_u8, cvvae_amd/data.py), shared by
tests/test_clip_transform_host.py (CPU: the tap tables against torch in fp64) and tests/test_gpu_clip_transform.py (the kernel).

The shapes are the smallest at which the pass can still go wrong: non-integer downscales (4-tap tables, odd crop origins), an
upscale, a heavy downscale (11-12 taps, many staged rows, few output rows per workgroup), a crop wider than two 64-column tiles with
a ragged last tile, the reference's CoverResize with a centre crop, no resize at all (identity tables, rows that start on no
boundary), a frame table that picks and repeats frames out of a longer buffer, and the image datapipe.

Inputs: seeded `torch.randint` bytes.  Each case runs with antialias True and False and each output dtype."""
import collections

import torch

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# half an ulp below 1 of the output dtype, added to the fp32 chain's bound
DTYPE_TERM = {torch.float32: 0.0, torch.float16: 2.0 ** -12, torch.bfloat16: 2.0 ** -9}

# resize: None | ("short", n) | ("cover", (h, w));  origin: (top, left) | "centre";  frame_index: None | list
Case = collections.namedtuple("Case", "name frames resize resized origin crop frame_index")
CASES = [
    Case("down_nonint", (3, 45, 70), ("short", 24), (24, 37), (3, 9), (16, 16), None),
    Case("up", (3, 20, 33), ("short", 32), (32, 52), (0, 12), (32, 40), None),
    Case("heavy_down", (2, 64, 85), ("short", 12), (12, 15), (0, 2), (12, 12), None),
    Case("wide", (2, 24, 200), ("short", 18), (18, 150), (1, 21), (17, 129), None),
    Case("cover", (2, 40, 90), ("cover", (32, 48)), (32, 72), "centre", (32, 48), None),
    Case("identity", (3, 33, 47), None, (33, 47), (5, 6), (20, 31), None),
    Case("gather", (9, 20, 33), ("short", 16), (16, 26), "centre", (16, 16), [8, 0, 4, 4]),
]
BY_NAME = {c.name: c for c in CASES}
IMAGE = Case("image", (1, 50, 75), ("short", 32), (32, 48), "centre", (32, 32), None)   # ImageTransform(32)
ANTIALIAS = [True, False]


def frames_of(case, seed=0) -> torch.Tensor:
    """the case's uint8 frames [T,H,W,3] on the CPU"""
    g = torch.Generator().manual_seed(4000 + seed + sum(case.frames))
    return torch.randint(0, 256, tuple(case.frames) + (3,), generator=g, dtype=torch.uint8)


def origin_of(case):
    if case.origin != "centre":
        return case.origin
    (rh, rw), (th, tw) = case.resized, case.crop
    return int(round((rh - th) / 2.0)), int(round((rw - tw) / 2.0))


def transform_of(case, antialias, dtype=torch.float32, device=None):
    """the case's ClipTransform (the origin goes to its call)"""
    from cvvae_amd.data import ClipTransform
    if case.resize is None:
        return ClipTransform(case.crop, None, antialias=antialias, dtype=dtype, device=device)
    kind, size = case.resize
    return ClipTransform(case.crop, size, cover=kind == "cover", antialias=antialias, dtype=dtype, device=device)
