"""Time the training clip transform on an MI355X at the training YAML's shape: 17 decoded frames of 336x596 uint8, short side to 512
(-> 512x908), a random 256x256 crop, fp32 and bf16 output --
  (a) `kernel`: the uint8 frames uploaded as uint8, then ONE launch of cvvae_clip_from_frames_u8 (cvvae_amd.data.ClipTransform with
      device="cuda" on a pinned CPU tensor) straight into a [3,17,256,256] slot;
  (b) `eager`:  the reference's composition on the same GPU: the same frames as a float [T,C,H,W] tensor uploaded (4x the bytes),
      F.interpolate of every whole frame, crop, (x / 255 - 0.5) * 2, permute().contiguous(), cast;
the two taking turns sample by sample in ONE process, the same crop origin in both.  Each is also timed without its upload
(`*_device_only`: inputs already resident).

    timeout -k 10 300 python tools/clip_transform.py             # writes profiles/clip_transform.json

Per path: the median / min / max over `--iters` samples of the time between two device events around the call (the upload and
host time the device does not hide are in it) and the host's own time in the call.  Recorded with the figures: the ratio of the
medians, the bytes each path moves over the host link and through HBM (computed from the shapes), and the kernel's largest
difference from the eager result.  The condition is only that the kernel is not slower than the eager composition at this shape.
There is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvvae_amd import _lib  # noqa: E402
from cvvae_amd.data import ClipTransform, resized_size  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
T, H, W = 17, 336, 596
RESIZE, CROP = 512, 256


def sample(fn):
    """-> (device ms, host ms) of one call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), host


def stats(rows):
    ms, host = zip(*rows)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "host_median_ms": statistics.median(host),
            "iters": len(ms)}


def measure(dtype, antialias, warmup, iters):
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).pin_memory()
    floats = frames.permute(0, 3, 1, 2).float().contiguous().pin_memory()        # what the reference's decoder hands its transform
    rh, rw = resized_size(H, W, RESIZE)
    tr = ClipTransform(CROP, RESIZE, random_crop=True, antialias=antialias, dtype=dtype, device="cuda")
    top, left = tr.plan(H, W, torch.Generator().manual_seed(1))[2:]
    slot = torch.empty((3, T, CROP, CROP), dtype=dtype, device="cuda")
    frames_dev, floats_dev = frames.cuda(), floats.cuda()

    def eager_from(x):
        x = F.interpolate(x, size=(rh, rw), mode="bilinear", align_corners=False, antialias=antialias)
        x = x[:, :, top:top + CROP, left:left + CROP]
        x = (x / 255 - 0.5) * 2
        return x.permute(1, 0, 2, 3).contiguous().to(dtype)

    paths = {
        "kernel": lambda: tr(frames, origin=(top, left), out=slot),
        "eager": lambda: eager_from(floats.to("cuda", non_blocking=True)),
        "kernel_device_only": lambda: tr(frames_dev, origin=(top, left), out=slot),
        "eager_device_only": lambda: eager_from(floats_dev),
    }
    for _ in range(warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    diff = float((tr(frames_dev, origin=(top, left)).float() - eager_from(floats_dev).float()).abs().max())
    rows = {p: [] for p in paths}
    for _ in range(iters):
        for p, fn in paths.items():                # sample by sample, the paths taking turns
            rows[p].append(sample(fn))
    out = {p: stats(r) for p, r in rows.items()}
    esz = slot.element_size()
    # the input rows and columns the crop window's tables touch (about a seventh of the frame), every channel, once per row tile
    window_in = int((CROP * H / rh + 3) * (CROP * W / rw + 3)) * 3 * T
    out["bytes"] = {
        "kernel_upload": frames.numel(), "eager_upload": floats.numel() * 4,
        "kernel_hbm": {"read_window_u8": window_in, "write_slot": slot.numel() * esz},
        "eager_hbm_at_least": {"read_float_frames": floats.numel() * 4, "write_resized": T * 3 * rh * rw * 4,
                               "crop_normalise_permute_cast": slot.numel() * (4 * 2 + 4 + esz)},
    }
    k, e = out["kernel"]["median_ms"], out["eager"]["median_ms"]
    kd, ed = out["kernel_device_only"]["median_ms"], out["eager_device_only"]["median_ms"]
    out.update(dtype=str(dtype)[6:], antialias=antialias, crop_origin=[top, left], resized=[rh, rw],
               eager_over_kernel=e / k, eager_over_kernel_device_only=ed / kd, kernel_not_slower=k <= e and kd <= ed,
               kernel_slot_bytes_per_s=slot.numel() * esz / (kd * 1e-3), max_abs_diff_kernel_vs_eager=diff)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_transform.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_transform.py measures on an MI355X; no GPU found (there is no CPU path)")
    torch.cuda.set_device(0)
    res = {"what": "the training clip transform, one sample: uint8 upload + one HIP pass against the eager composition (float upload, "
                   "F.interpolate, crop, normalise, permute) on the same GPU",
           "shape": {"frames_u8": [T, H, W, 3], "resize_short_side": RESIZE, "crop": [CROP, CROP], "slot": [3, T, CROP, CROP]},
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernel_sources": _lib.source_fingerprint(),
           "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "timing": "device events around each call, paths interleaved sample by sample in one process; pinned host memory", "runs": {}}
    for dtype in (torch.float32, torch.bfloat16):
        for antialias in (True, False):
            name = f"{str(dtype)[6:]}_{'antialias' if antialias else 'plain'}"
            res["runs"][name] = measure(dtype, antialias, a.warmup, a.iters)
            print(name, json.dumps(res["runs"][name])[:1500], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
