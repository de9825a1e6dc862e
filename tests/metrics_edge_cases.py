"""One case list for cvvae_frame_metrics, shared by tests/test_metrics_host.py (CPU: the list itself, the restatement) and
tests/test_gpu_metrics_edges.py (the HIP kernel).  Every case is a few thousand samples.

The kernel's output tile is TILE_H x TILE_W map positions; the shapes put H - 10 and W - 10 on one, two and three valid positions, on
either side of one tile, just past two tiles, and on a 3 x 3 grid of tiles.  11 x 13 uint8 frames have an odd number of bytes, so the
frame slice `frames[1:]` starts on an odd byte."""
from dataclasses import dataclass
from typing import Tuple

import torch

TILE_H, TILE_W = 16, 32       # csrc/metrics_kernels.hip MT_H, MT_W
DTYPE = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8}

SMALL = [(11, 11), (12, 13), (13, 12), (11, 13)]
AROUND_TILE = [(TILE_H - 1 + 10, TILE_W - 1 + 10), (TILE_H + 10, TILE_W + 10), (TILE_H + 1 + 10, TILE_W + 1 + 10),
               (TILE_H + 10, 2 * TILE_W + 1 + 10), (2 * TILE_H + 1 + 10, TILE_W + 10)]
GRID_3X3 = (2 * TILE_H + 1 + 10, 2 * TILE_W + 1 + 10)
CONTENTS = ["random", "same", "flat_255_254", "flat_0_1", "inverse", "ramp", "bright"]
VIEWS = ["none", "frame_slice", "window", "cat_half", "row_crop"]


@dataclass(frozen=True)
class Case:
    name: str
    ka: str           # operand kinds: "u8" | "f16" | "bf16" | "f32"
    kb: str
    B: int
    T: int
    H: int
    W: int
    content: str
    quantize: bool = True
    view: str = "none"
    seed: int = 0


def _bytes(case: Case, T: int, H: int, W: int, B: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """the two clips as byte values, int64 [B,3,T,H,W]"""
    g = torch.Generator().manual_seed(1000 + case.seed)
    shape = (B, 3, T, H, W)
    c = case.content
    if c == "random":
        return torch.randint(0, 256, shape, generator=g), torch.randint(0, 256, shape, generator=g)
    if c == "same":
        x = torch.randint(0, 256, shape, generator=g)
        return x, x.clone()
    if c == "flat_255_254":
        return torch.full(shape, 255), torch.full(shape, 254)
    if c == "flat_0_1":
        return torch.zeros(shape, dtype=torch.int64), torch.ones(shape, dtype=torch.int64)
    if c == "inverse":
        x = torch.randint(0, 256, shape, generator=g)
        return x, 255 - x
    if c == "ramp":
        x = ((torch.arange(W) * 255) // max(W - 1, 1)).expand(shape).clone()
        return x, torch.clamp(x + torch.randint(-3, 4, shape, generator=g), 0, 255)
    if c == "bright":
        return torch.randint(250, 256, shape, generator=g), torch.randint(250, 256, shape, generator=g)
    raise AssertionError(c)


def _operand(kind: str, by: torch.Tensor, case: Case, salt: int) -> torch.Tensor:
    """byte values [B,3,T,H,W] -> the operand's base tensor: uint8 frames [T,H,W,3] or a float clip around byte/127.5 - 1"""
    if kind == "u8":
        assert by.shape[0] == 1
        return by[0].permute(1, 2, 3, 0).contiguous().to(torch.uint8)
    x = by.double() / 127.5 - 1.0
    if case.content == "random":  # off the byte grid and past the clamp on both sides
        g = torch.Generator().manual_seed(2000 + case.seed + salt)
        x = x * 1.1 + (torch.rand(by.shape, generator=g, dtype=torch.float64) - 0.5) / 100.0
    return x.to(DTYPE[kind])


def bases(case: Case) -> Tuple[torch.Tensor, torch.Tensor]:
    """the two tensors the operands are views of (CPU).  apply() cuts the case's view out of them, on whatever device they are."""
    B, T, H, W = case.B, case.T, case.H, case.W
    if case.view in ("frame_slice", "window"):
        T += 1
    elif case.view == "cat_half":
        B *= 2
    elif case.view == "row_crop":
        H += 3
    a, b = _bytes(case, T, H, W, B)
    if case.content == "same" and case.ka == case.kb:
        x = _operand(case.ka, a, case, 0)
        return x, x.clone()
    return _operand(case.ka, a, case, 0), _operand(case.kb, b, case, 1)


def _cut(x: torch.Tensor, case: Case) -> torch.Tensor:
    u8 = x.dtype == torch.uint8
    if case.view == "none":
        return x
    if case.view in ("frame_slice", "window"):
        return x[1:] if u8 else x[:, :, 1:]
    if case.view == "cat_half":
        return x if u8 else x[case.B:]
    if case.view == "row_crop":
        return x[:, 2:2 + case.H] if u8 else x[:, :, :, 2:2 + case.H]
    raise AssertionError(case.view)


def apply(case: Case, a: torch.Tensor, b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return _cut(a, case), _cut(b, case)


def cases():
    out = []
    k = 0

    def add(tag, ka, kb, B, T, hw, content, quantize=True, view="none"):
        nonlocal k
        k += 1
        q = "" if "u8" == ka == kb else ("-q" if quantize else "-raw")
        out.append(Case(f"{tag}-{ka}_{kb}-B{B}T{T}-{hw[0]}x{hw[1]}-{content}{q}" + ("" if view == "none" else f"-{view}"),
                        ka, kb, B, T, hw[0], hw[1], content, quantize, view, seed=k))

    # shapes: uint8 against uint8, random bytes
    for hw in SMALL + AROUND_TILE + [GRID_3X3]:
        add("shape", "u8", "u8", 1, 1, hw, "random")
    add("shape", "u8", "u8", 1, 3, GRID_3X3, "random")
    add("shape", "f32", "f32", 2, 3, AROUND_TILE[2], "random", quantize=False)
    add("shape", "bf16", "bf16", 2, 1, GRID_3X3, "random")
    # contents
    for c in CONTENTS[1:]:
        add("content", "u8", "u8", 1, 3, AROUND_TILE[2], c)
        add("content", "f32", "f32", 2, 1, SMALL[1], c, quantize=False)
    add("content", "f16", "f16", 1, 1, AROUND_TILE[0], "same")
    add("content", "bf16", "bf16", 1, 1, AROUND_TILE[0], "same", quantize=False)
    # operand kinds
    for dt in ("f16", "bf16", "f32"):
        for q in (True, False):
            add("kind", dt, dt, 2, 3, AROUND_TILE[1], "random", quantize=q)
            add("kind", dt, dt, 1, 1, SMALL[3], "bright", quantize=q)
    for q in (True, False):
        add("kind", "u8", "bf16", 1, 3, SMALL[1], "random", quantize=q)
        add("kind", "bf16", "u8", 1, 1, GRID_3X3, "inverse", quantize=q)
        add("kind", "f16", "f32", 2, 1, AROUND_TILE[3], "random", quantize=q)
        add("kind", "f32", "f16", 1, 3, SMALL[0], "ramp", quantize=q)
    # views, read in place
    add("view", "u8", "u8", 1, 3, SMALL[3], "random", view="frame_slice")          # 11 x 13 x 3 bytes per frame: an odd start
    add("view", "u8", "u8", 1, 2, AROUND_TILE[2], "random", view="frame_slice")
    add("view", "u8", "u8", 1, 2, AROUND_TILE[1], "random", view="row_crop")
    add("view", "u8", "f16", 1, 2, SMALL[3], "random", view="frame_slice")
    for dt in ("f16", "bf16", "f32"):
        add("view", dt, dt, 2, 3, AROUND_TILE[2], "random", view="window")
        add("view", dt, dt, 2, 2, SMALL[2], "random", quantize=False, view="cat_half")
    add("view", "f32", "bf16", 1, 2, AROUND_TILE[0], "random", view="row_crop")
    return out


CASES = cases()
