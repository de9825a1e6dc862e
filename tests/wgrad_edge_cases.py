"""Case tables of the weight-gradient edge tests (a plain module, imported by tests/test_wgrad_edges_host.py and
tests/test_gpu_wgrad_edges.py): cvvae_conv_wgrad / cvvae_conv_wgrad_bias on all three of its kernels, the per-channel sums
(ops.bias_grad, ops.gn_bwd_params) and the padding adjoint (ops.pad_fold) -- everything in cvvae_amd/csrc/wgrad_kernel.hip, and of
cvvae_amd/csrc/bwd_kernels.hip what tests/pass_edge_cases.py and tests/boundary_edge_cases.py do not cover.

A case is data only.  A conv case names the edge it reaches and DECLARES the facts of the launch plan it depends on: the kernel,
the slab count, the fewest and most K panels a slab multiplies, how many slabs start in the middle of an output row, which
boundary a mid-row slab crosses, and whether the launch is eligible for the scalar-base wave-loads (FAST).  The host test reads
the slab count from the library and fails when a declared fact no longer holds, so a change of wgrad_workspace (the slab split) cannot quietly turn
the deep-pipeline cases back into one-panel launches."""
from dataclasses import dataclass
from typing import List, Tuple

F32, F16, BF16 = "f32", "f16", "bf16"
HALF = (F16, BF16)
REP, ZERO = 1, 0
CAUSAL = ((2, 0), (1, 1), (1, 1))
SYM = ((1, 1), (1, 1), (1, 1))
FRAME = ((0, 0), (1, 1), (1, 1))
DOWN = ((0, 0), (0, 1), (0, 1))       # Downsample3D of the SD2.1 family: back pads only
NOPAD = ((0, 0), (0, 0), (0, 0))
DMA, REG = "dma", "reg"                # wgrad_dma_kernel / wgrad_kernel


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _seed(name: str) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


@dataclass(frozen=True)
class Conv:
    name: str
    edge: str                          # the edge of the kernel this shape reaches
    cin: int                           # real channels ...
    cs: int                            # ... and stored width of a
    cout: int
    cg: int                            # stored width of gy
    k: Tuple[int, int, int]
    stride: Tuple[int, int, int]
    pad: Tuple[Tuple[int, int], ...]
    mode_t: int
    mode_hw: int
    dims: Tuple[int, int, int, int]    # the INPUT's B, Ti, Hi, Wi
    dtypes: Tuple[str, ...]
    # ---- declared plan facts
    kernel: str
    nslab: int
    pmin: int                          # fewest / most K panels of a slab
    pmax: int
    midrow: int                        # slabs whose first panel is not the first of an output row
    crosses: str = ""                  # "frame" / "batch": a slab that starts mid-row runs across that boundary
    fast: bool = False                 # eligible for the scalar-base wave-loads
    nan_gap: bool = False              # channels between round_up(c, 8) and the stored width hold NaN, in a and in gy

    @property
    def seed(self) -> int:
        return _seed(self.name)

    @property
    def out_grid(self) -> Tuple[int, int, int]:
        _, Ti, Hi, Wi = self.dims
        return tuple((n + p[0] + p[1] - kk) // s + 1 for n, p, kk, s in zip((Ti, Hi, Wi), self.pad, self.k, self.stride))

    @property
    def pixels(self) -> int:
        To, Ho, Wo = self.out_grid
        return self.dims[0] * To * Ho * Wo

    @property
    def ntaps(self) -> int:
        return self.k[0] * self.k[1] * self.k[2]

    @property
    def xp(self) -> bool:
        return self.dtypes[0] == F32

    @property
    def kp(self) -> int:
        """output pixels of a K panel (wgrad_kernel's KP; wgrad_dma_kernel's is the same 64)"""
        return (64 if self.xp else 128) if self.k[1] == 1 else (32 if self.xp else 64)


def _conv(name, edge, ch, k, stride, pad, modes, dims, dtypes, kernel, nslab, pmin, pmax, midrow, **kw) -> Conv:
    cin, cs, cout, cg = ch if len(ch) == 4 else (ch[0], ch[0], ch[1], ch[1])
    assert all(d in (F16, BF16) for d in dtypes) or dtypes == (F32,), "one plan per case: 16-bit or fp32"
    return Conv(name, edge, cin, cs, cout, cg, k, stride, pad, modes[0], modes[1], dims, tuple(dtypes), kernel, nslab, pmin, pmax, midrow, **kw)


K333, K133, K111, K311 = (3, 3, 3), (1, 3, 3), (1, 1, 1), (3, 1, 1)
S1, S122, S222 = (1, 1, 1), (1, 2, 2), (2, 2, 2)
GAP = (72, 80, 136, 144)   # 72 -> 136 channels stored as 80 -> 144: the second channel block holds ONE 16-byte piece


def conv_cases() -> List[Conv]:
    c = []
    # ---------------------------------------------------------------- wgrad_dma_kernel, deep pipeline (>= 24 workgroups per slab)
    c.append(_conv("dma-deep-causal333-512", "ring wraps; vmcnt steady state; 2-pixel third panel per row; slabs cross the frame boundary",
                   (512, 512), K333, S1, CAUSAL, (REP, REP), (1, 3, 5, 130), HALF, DMA, 8, 5, 6, 5, crosses="frame"))
    c.append(_conv("dma-deep-frame133-zero-512", "the same rows through the zero page, 32 members per slab",
                   (512, 512), K133, S1, FRAME, (ZERO, ZERO), (1, 3, 5, 130), (F16,), DMA, 8, 5, 6, 5, crosses="frame"))
    c.append(_conv("dma-deep-stride122-512", "the two-buffer ring of SW = 2, 6-7 panels per slab",
                   (512, 512), K133, S122, DOWN, (ZERO, ZERO), (1, 3, 12, 258), (BF16,), DMA, 8, 6, 7, 4, crosses="frame"))
    c.append(_conv("dma-deep-sym333-256", "position counters across the batch boundary",
                   (256, 256), K333, S1, SYM, (REP, REP), (3, 2, 9, 70), (F16,), DMA, 32, 3, 4, 16, crosses="batch"))
    c.append(_conv("dma-deep-fast-512", "scalar-base wave-loads, exactly four panels per slab, no zero page",
                   (512, 512), K333, S1, CAUSAL, (REP, REP), (2, 2, 4, 128), (BF16,), DMA, 8, 4, 4, 0, fast=True))
    # ---------------------------------------------------------------- scalar-base wave-loads through the zero page and at stride 2
    c.append(_conv("dma-fast-frame133-zero-128", "scalar-base form with the zero page; nslab = 8 + 2",
                   (128, 128), K133, S1, FRAME, (ZERO, ZERO), (1, 2, 5, 64), HALF, DMA, 10, 1, 1, 0, fast=True))
    c.append(_conv("dma-fast-stride222-128", "scalar-base form at stride 2 (replicate in time, zero in the plane)",
                   (128, 128), K333, S222, ((2, 0), (0, 1), (0, 1)), (REP, ZERO), (1, 3, 6, 128), HALF, DMA, 6, 1, 1, 0, fast=True))
    c.append(_conv("dma-fast-nan-gap-64to128", "scalar-base form over pixel strides of 72 and 136 channels, NaN in the gap",
                   (64, 72, 128, 136), K333, S1, SYM, (REP, ZERO), (1, 2, 3, 64), HALF, DMA, 6, 1, 1, 0, fast=True, nan_gap=True))
    # ---------------------------------------------------------------- wgrad_dma_kernel, ragged tiles
    for W, modes, pad in ((1, (REP, REP), CAUSAL), (63, (ZERO, ZERO), SYM), (64, (REP, REP), CAUSAL), (65, (REP, REP), CAUSAL)):
        n = 6 * ((W + 63) // 64)
        c.append(_conv(f"dma-w{W}", f"row of {W} pixels against the 64-pixel panel", (64, 128), K333, S1, pad, modes, (1, 2, 3, W), HALF,
                       DMA, n, 1, 1, n // 2 if W > 64 else 0, fast=W == 64))
    for W in (1, 2):
        for mode, tag in ((REP, "rep"), (ZERO, "zero")):
            c.append(_conv(f"dma-wi{W}-{tag}", f"Wi = {W}: every tap along W clamps or vanishes", (64, 128), K333, S1, SYM, (mode, mode),
                           (1, 2, 3, W), HALF, DMA, 6, 1, 1, 0))
    c.append(_conv("dma-t1h1", "Ti = Hi = 1: every tap along T and H clamps", (64, 128), K333, S1, CAUSAL, (REP, REP), (1, 1, 1, 20), HALF,
                   DMA, 1, 1, 1, 0))
    c.append(_conv("dma-nan-gap-72to136", "one 16-byte piece in the second channel block; NaN in the gap channels", GAP, K333, S1, SYM,
                   (REP, ZERO), (1, 2, 3, 37), HALF, DMA, 6, 1, 1, 0, nan_gap=True))
    c.append(_conv("dma-conv-in-3of16", "3 of 16 stored channels (conv_in)", (3, 16, 128, 128), K333, S1, CAUSAL, (REP, REP), (1, 3, 5, 40), HALF,
                   DMA, 15, 1, 1, 0))
    c.append(_conv("dma-conv-out-512to32", "32 output channels of the 128-row tile (conv_out)", (512, 32), K333, S1, CAUSAL, (REP, REP),
                   (1, 2, 4, 12), HALF, DMA, 8, 1, 1, 0))
    c.append(_conv("dma-8to8-1px", "one pixel, one slab: the reduce kernel's tail loop alone", (8, 8), K333, S1, SYM, (REP, REP), (1, 1, 1, 1), HALF,
                   DMA, 1, 1, 1, 0))
    c.append(_conv("dma-stride222-odd", "stride 2 on every axis with odd Ti, Hi, Wi", (64, 128), K333, S222, CAUSAL, (REP, REP), (1, 5, 7, 9), HALF,
                   DMA, 12, 1, 1, 0))
    # ---------------------------------------------------------------- wgrad_kernel, fp32 models (three bf16 MFMAs per product)
    c.append(_conv("reg32-deep-causal333-512", "4-5 panels of 32 pixels per slab, slabs start mid-row and cross the frame boundary",
                   (512, 512), K333, S1, CAUSAL, (REP, REP), (1, 3, 4, 70), (F32,), REG, 8, 4, 5, 4, crosses="frame"))
    for W, modes in ((1, (REP, REP)), (31, (ZERO, ZERO)), (32, (REP, REP)), (33, (REP, REP))):
        n = 6 * ((W + 31) // 32)
        c.append(_conv(f"reg32-w{W}", f"row of {W} pixels against the 32-pixel panel", (64, 128), K333, S1, SYM, modes, (1, 2, 3, W), (F32,),
                       REG, n, 1, 1, n // 2 if W > 32 else 0))
    c.append(_conv("reg32-linear-512-row10000", "one long row, several 64-pixel panels per slab", (512, 512), K111, S1, NOPAD, (ZERO, ZERO),
                   (1, 1, 1, 10000), (F32,), REG, 24, 6, 7, 23))
    c.append(_conv("reg32-k311", "(3, 1, 1) taps: admitted by the ABI", (64, 128), K311, S1, ((2, 0), (0, 0), (0, 0)), (REP, ZERO), (1, 4, 3, 50),
                   (F32,), REG, 12, 1, 1, 0))
    c.append(_conv("reg32-nan-gap-72to136", "NaN in the gap channels", GAP, K333, S1, SYM, (REP, ZERO), (1, 2, 3, 37), (F32,), REG, 12, 1, 1, 6,
                   nan_gap=True))
    c.append(_conv("reg32-stride222", "stride 2 on every axis, zero padding", (64, 128), K333, S222, SYM, (ZERO, ZERO), (1, 5, 7, 9), (F32,), REG,
                   12, 1, 1, 0))
    # ---------------------------------------------------------------- wgrad_kernel, 16-bit single-tap (KP = 128)
    c.append(_conv("reg16-linear-512-row15400", "about five 128-pixel panels per slab, ragged last panel", (512, 512), K111, S1, NOPAD, (ZERO, ZERO),
                   (1, 1, 1, 15400), HALF, REG, 24, 5, 6, 23))
    for W in (127, 128, 129):
        n = 6 * ((W + 127) // 128)
        c.append(_conv(f"reg16-w{W}", f"row of {W} pixels against the 128-pixel panel", (64, 128), K111, S1, NOPAD, (ZERO, ZERO), (1, 2, 3, W), HALF,
                       REG, n, 1, 1, n // 2 if W > 128 else 0))
    c.append(_conv("reg16-8to8-w1", "8 -> 8 channels, one pixel per row", (8, 8), K111, S1, NOPAD, (ZERO, ZERO), (1, 2, 3, 1), HALF, REG, 6, 1, 1, 0))
    return c


# the 16-bit kH = 3 register-staged kernel (CVVAE_WGRAD_DMA=0, read once per process): run in ONE child process, bf16
REG16_K3_CHILD = ("dma-w65", "dma-wi1-zero", "dma-nan-gap-72to136", "dma-stride222-odd")


# ------------------------------------------------------------------------------------------------------------ per-channel sums
@dataclass(frozen=True)
class Chan:
    """ops.bias_grad (op "bias": gy [rows * S pixels, ps], NaN in the channels C .. ps) or ops.gn_bwd_params (op "gn": rows x S)"""
    name: str
    op: str
    C: int
    rows: int
    S: int
    ps: int = 0
    silu: int = 0
    dtypes: Tuple[str, ...] = (F32, F16, BF16)

    @property
    def seed(self) -> int:
        return _seed(self.name)

    @property
    def ppp(self) -> int:      # pixels a workgroup takes per pass (chan_sums_kernel)
        return max(256 // ((self.C + 7) // 8), 1)

    @property
    def nparts(self) -> int:   # cvvae_channel_sums: rows x chan_sums_splits
        rows = 1 if self.op == "bias" else self.rows
        S = self.rows * self.S if self.op == "bias" else self.S
        per = max(32 * self.ppp, 128)
        return rows * max(min((S + per - 1) // per, (2048 + rows - 1) // rows), 1)


def split_len(C: int) -> int:
    return max(32 * max(256 // ((C + 7) // 8), 1), 128)


def chan_cases() -> List[Chan]:
    c = []
    for C in (8, 24, 512, 2048):   # cv = 1, 3 (one idle thread), 64, 256 (one pixel per pass)
        ppp = max(256 // (C // 8), 1)
        for S in (4 * ppp - 1, 4 * ppp, 4 * ppp + 1, split_len(C)):   # around one 4-deep trip; exactly one split
            c.append(Chan(f"bias-C{C}-S{S}", "bias", C, 1, S, ps=C + 8))
        c.append(Chan(f"gn-C{C}-S{4 * ppp + 1}-r2", "gn", C, 2, 4 * ppp + 1, silu=C % 16 == 8))
    # chan_sums_final_kernel: nparts below / at one 8-lane trip, in its 4-deep loop (i + 24 < nparts), at and past 32, with tails
    for n in (8, 25, 32, 33, 57):
        c.append(Chan(f"bias-C512-parts{n}", "bias", 512, 1, 128 * n - 3, ps=520, dtypes=(F32, BF16)))
    c.append(Chan("gn-C512-r5-parts25", "gn", 512, 5, 128 * 5 - 1, silu=1, dtypes=(F32, F16)))
    c.append(Chan("gn-C2048-r8-parts8", "gn", 2048, 8, 5, dtypes=(F32, BF16)))
    c.append(Chan("gn-C24-r3-parts33", "gn", 24, 3, split_len(24) * 11 - 7, silu=1, dtypes=(F32, F16)))
    return c


# ------------------------------------------------------------------------------------------------------------ padding adjoint
@dataclass(frozen=True)
class Fold:
    """ops.pad_fold: dims = the UNPADDED B, T, H, W; one pad pixel on each side of H and W"""
    name: str
    dims: Tuple[int, int, int, int]
    C: int
    pad_t: Tuple[int, int]
    mode_t: int
    mode_hw: int
    add: bool
    dtypes: Tuple[str, ...] = (F32, F16, BF16)

    @property
    def seed(self) -> int:
        return _seed(self.name)

    @property
    def vectors(self) -> int:
        B, T, H, W = self.dims
        return B * T * H * W * (self.C // 8)


def fold_cases() -> List[Fold]:
    return [
        Fold("fold-1x1x1-causal-rep-C8", (2, 1, 1, 1), 8, (2, 0), REP, REP, True),      # one element collects the whole 3 x 3 x 3 region
        Fold("fold-T1-sym-rep-C520", (1, 1, 3, 4), 520, (1, 1), REP, REP, False),
        Fold("fold-H1-causal-rep-C8", (1, 3, 1, 5), 8, (2, 0), REP, REP, False),
        Fold("fold-W1-sym-rep-C520", (2, 2, 3, 1), 520, (1, 1), REP, REP, True),
        Fold("fold-sym-zero-C8", (2, 3, 4, 5), 8, (1, 1), ZERO, ZERO, True),
        Fold("fold-1x1x1-zero-C520", (1, 1, 1, 1), 520, (1, 1), ZERO, ZERO, False),
        Fold("fold-causal-rep-zero-hw-C520", (1, 2, 3, 3), 520, (2, 0), REP, ZERO, False),
        # more than 8192 x 256 vectors: the grid-stride loop takes a second trip (and a partial third)
        Fold("fold-second-trip-C8", (1, 8, 515, 512), 8, (1, 1), REP, REP, True, dtypes=(BF16,)),
    ]
