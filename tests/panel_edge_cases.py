"""One case list for cvvae_recon_panels, shared by tests/test_train_engine_contract.py (CPU: the list itself and the kernel's
arithmetic plan against eager torch) and tests/test_gpu_panel_edges.py (the kernel).

A case is dtype x shape x view.  Shapes: one element per row, rows of 5 and 9 (every output row starts at another offset from a
16-byte boundary, so the scalar head and tail both run), W = 8 and 16 (whole groups for the 16-bit types and for float), and the GPU
tests' clip.  Views of x: contiguous, every second frame of a longer clip, a crop of rows and columns out of a larger picture (rows
start one element off), and the second half of a cat (the base pointer is off a 16-byte boundary for the odd shapes).

Values: uniform in [-1.5, 1.5] in both operands (so both clamps act), with these (x, xrec) pairs planted from element 0 on, one
every 5 elements, cyclically: the difference that hits the upper clamp (x = -3, xrec = 1), exactly +-1 against each other and
against themselves, +0 against -0 both ways, values beyond +-1 in either operand, and a small difference that `f` boosts."""
import collections

import torch

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
SHAPES = [(1, 3, 1, 1, 1), (1, 3, 2, 3, 5), (2, 3, 3, 7, 9), (1, 3, 2, 4, 8), (1, 3, 2, 3, 16), (1, 3, 5, 32, 32)]
VIEWS = ["none", "frames", "crop", "cat"]
BOOSTS = [0.0, 1.0, 2.5, 3.0]
PLANTED = [(-3.0, 1.0), (0.0, -0.0), (2.0, 0.5), (-0.0, 0.0), (1.0, -1.0), (-1.0, 1.0), (1.0, 1.0), (-1.0, -1.0), (0.5, -2.0),
           (0.25, 0.375), (-1.25, -1.5), (0.0, 1.0)]

Case = collections.namedtuple("Case", "name dtype shape view")
CASES = [Case(f"{d}-{'x'.join(map(str, s))}-{v}", DTYPES[d], s, v) for d in DTYPES for s in SHAPES for v in VIEWS]


def bases(case, seed=0):
    """(x, xrec) on the CPU, contiguous, in the case's dtype"""
    g = torch.Generator().manual_seed(1000 + seed + sum(case.shape))
    x = torch.rand(case.shape, generator=g) * 3.0 - 1.5
    r = (x + (torch.rand(case.shape, generator=g) - 0.5)).clamp(-1.5, 1.5)
    fx, fr = x.view(-1), r.view(-1)
    for k, i in enumerate(range(0, fx.numel(), 5)):
        fx[i], fr[i] = PLANTED[k % len(PLANTED)]
    return x.to(case.dtype), r.to(case.dtype)


def view_of(case, x: torch.Tensor) -> torch.Tensor:
    """x (any device) as the case's view: equal values, another layout"""
    b, c, t, h, w = x.shape
    if case.view == "none":
        return x
    if case.view == "frames":
        big = torch.full((b, c, 2 * t, h, w), 7.0, dtype=x.dtype, device=x.device)
        big[:, :, ::2] = x
        return big[:, :, ::2]
    if case.view == "crop":
        big = torch.full((b, c, t, h + 2, w + 3), 7.0, dtype=x.dtype, device=x.device)
        big[:, :, :, 1:-1, 1:1 + w] = x
        return big[:, :, :, 1:-1, 1:1 + w]
    if case.view == "cat":
        return torch.cat([torch.full_like(x, 7.0), x], dim=0)[b:]
    raise AssertionError(case.view)
