"""Case tables of the LPIPS / discriminator pass edge tests (a plain module, imported by tests/test_lossnet_edges_host.py and
tests/test_gpu_lossnet_edges.py): the passes of cvvae_amd/csrc/lpips_kernels.hip (ScalingLayer, ReLU, 2x2 max pooling, the fused
ReLU / pooling backward, the lin heads) and of cvvae_amd/csrc/disc_kernels.hip (the 3-D average pool, GroupNorm-apply + LeakyReLU,
their adjoints, their statistics forms and the small-Cin stride-2 input gradient).

A case is data only (pass_edge_cases.Case): a name, the op, the shape parameters, the dtypes it runs in and the name of its input
recipe; tests/lossnet_ref.py builds the tensors.  Shapes are [N,H,W,C] or [B,T,H,W,C]; "255 / 256 / 257" are work-item counts one
below, at and one above a 256-thread block.  The comment next to each group names the edge it reaches."""
from typing import Dict, List

from pass_edge_cases import ALL, BF16, F16, F32, HALF, Case, _case

# ------------------------------------------------------------------------------------------------------------ lpips_scale_in(_bwd)
def scale_in_cases() -> List[Case]:
    out = []
    # all nine src -> dst pairs on 255 vectors
    for src in ALL:
        for dst in ALL:
            out.append(_case(f"scale_in-1x15x17-c8-{src}-{dst}", "scale_in", dtypes=(dst,), N=1, H=15, W=17, cpad=8, src=src, sliced=0))
    # 256 and 257 vectors, the single vector; cpad 16 / 32: the pad vectors are whole zero vectors
    out.append(_case("scale_in-1x16x16-c8", "scale_in", dtypes=(BF16,), N=1, H=16, W=16, cpad=8, src=F32, sliced=0))
    out.append(_case("scale_in-1x1x257-c8", "scale_in", dtypes=(F16,), N=1, H=1, W=257, cpad=8, src=BF16, sliced=0))
    out.append(_case("scale_in-1x1x1-c8", "scale_in", dtypes=(F32,), N=1, H=1, W=1, cpad=8, src=F16, sliced=0))
    out.append(_case("scale_in-2x3x5-c16", "scale_in", dtypes=(BF16,), N=2, H=3, W=5, cpad=16, src=F32, sliced=0))
    out.append(_case("scale_in-2x3x5-c32", "scale_in", dtypes=(F16,), N=2, H=3, W=5, cpad=32, src=F32, sliced=0))
    # out = the second half of a [1, 2N, H, W, cpad] buffer with a canary before and behind
    out.append(_case("scale_in-2x3x5-c16-slice", "scale_in", dtypes=(BF16,), N=2, H=3, W=5, cpad=16, src=F32, sliced=1))
    out.append(_case("scale_in-3x7x9-c32-slice", "scale_in", dtypes=(F32,), N=3, H=7, W=9, cpad=32, src=BF16, sliced=1))
    return out


def scale_in_bwd_cases() -> List[Case]:
    out = []
    # pixel counts 255 / 256 / 257 x pixel strides 8 and 32; g is samples N .. 2N-1 of a 2N tensor, channels 3 .. ps-1 hold NaN
    pairs = ((BF16, F32), (F16, BF16), (F32, F16), (BF16, BF16), (F16, F32), (F32, F32))
    i = 0
    for H, W in ((15, 17), (16, 16), (1, 257)):
        for ps in (8, 32):
            g, dst = pairs[i]
            i += 1
            out.append(_case(f"scale_in_bwd-1x{H}x{W}-ps{ps}-{g}-{dst}", "scale_in_bwd", dtypes=(dst,), N=1, H=H, W=W, ps=ps, g=g))
    out.append(_case("scale_in_bwd-3x2x3-ps16", "scale_in_bwd", dtypes=(BF16,), N=3, H=2, W=3, ps=16, g=BF16))
    return out


# ------------------------------------------------------------------------------------------------------------ relu_
def relu_cases() -> List[Case]:
    out = [_case(f"relu-v{v}", "relu", v=v) for v in (1, 255, 256, 257)]
    out.append(_case("relu-v1-special", "relu", recipe="special", v=1))   # +-inf, -0.0, a subnormal, the largest finite value
    out.append(_case("relu-v3-nan", "relu", recipe="nan", v=3))           # torch.relu(NaN) is NaN
    return out


# ------------------------------------------------------------------------------------------------------------ maxpool2x2
POOL2_COUNT_SHAPES = ((1, 2, 510, 8), (1, 2, 512, 8), (1, 2, 514, 8))  # 255 / 256 / 257 output vectors


def maxpool_cases() -> List[Case]:
    out = []
    # one window; the odd row and column dropped; an odd width with two vectors; odd extents, eight vectors, several samples
    for N, H, W, C in ((1, 2, 2, 8), (2, 3, 3, 8), (1, 2, 5, 16), (3, 7, 9, 64)) + POOL2_COUNT_SHAPES:
        out.append(_case(f"maxpool-{N}x{H}x{W}x{C}", "maxpool", N=N, H=H, W=W, C=C))
    out.append(_case("maxpool-3x7x9x64-neg", "maxpool", recipe="neg", N=3, H=7, W=9, C=64))   # every value negative
    out.append(_case("maxpool-3x7x9x64-tie", "maxpool", recipe="tie", N=3, H=7, W=9, C=64))   # the coarse grid: equal maxima
    for pos in range(4):  # +inf and -inf, and a NaN, in each position of the window
        out.append(_case(f"maxpool-1x4x4x8-inf{pos}", "maxpool", recipe="inf", N=1, H=4, W=4, C=8, pos=pos))
        out.append(_case(f"maxpool-1x4x4x8-nan{pos}", "maxpool", recipe="nan", N=1, H=4, W=4, C=8, pos=pos))
    return out


# ------------------------------------------------------------------------------------------------------------ relu_pool_bwd
MODES = ("both", "pool", "tap")


def relu_pool_bwd_cases() -> List[Case]:
    out = []
    # one cell; partial cells on both axes; cell-vector counts 255 / 256 / 257 (the last with a partial column)
    for N, H, W, C in ((1, 2, 2, 8), (1, 3, 3, 8), (1, 2, 510, 8), (1, 2, 512, 8), (1, 2, 513, 8), (3, 7, 9, 64)):
        for mode in MODES:
            out.append(_case(f"relu_pool_bwd-{N}x{H}x{W}x{C}-{mode}", "relu_pool_bwd", N=N, H=H, W=W, C=C, mode=mode))
    # an extent of 1: no whole window -- tap only; with g_pool the call must raise
    for N, H, W, C in ((2, 1, 5, 16), (2, 5, 1, 16)):
        out.append(_case(f"relu_pool_bwd-{N}x{H}x{W}x{C}-tap", "relu_pool_bwd", N=N, H=H, W=W, C=C, mode="tap"))
        out.append(_case(f"relu_pool_bwd-{N}x{H}x{W}x{C}-pool-raises", "relu_pool_bwd", raises=True, N=N, H=H, W=W, C=C, mode="pool"))
    for recipe in ("tie", "zero", "negy"):  # equal maxima; an all-zero y (gradient 0 whichever position wins); negative y (strict mask)
        for mode in MODES:
            out.append(_case(f"relu_pool_bwd-3x7x9x64-{recipe}-{mode}", "relu_pool_bwd", recipe=recipe, N=3, H=7, W=9, C=64, mode=mode))
    return out


# ------------------------------------------------------------------------------------------------------------ lpips_head(_bwd)
HEAD_C = (64, 128, 256, 512)


def head_cases() -> List[Case]:
    out = []
    for C in HEAD_C:
        pb = 2048 // C  # pixels per block
        for HW in sorted({1, pb - 1, pb, pb + 1}):
            out.append(_case(f"head-C{C}-HW{HW}-N3", "head", C=C, HW=HW, N=3))
    # forward pixel loop (above 256 blocks): one extra trip for block 0 only; two trips with a ragged tail
    out.append(_case("head-C512-HW1025-N2", "head", dtypes=(BF16, F32), C=512, HW=1025, N=2))
    out.append(_case("head-C64-HW16417-N2", "head", dtypes=(BF16,), C=64, HW=2 * 8192 + 32 + 1, N=2))
    # backward pixel loop (above 2048 blocks)
    out.append(_case("head-C512-HW8193-N1", "head", dtypes=(BF16,), C=512, HW=8193, N=1))
    out.append(_case("head-C64-HW65537-N1", "head", dtypes=(BF16,), C=64, HW=65537, N=1))
    # the final kernel's 64 samples per block: one block, its edge, a second block
    for N in (1, 64, 65):
        out.append(_case(f"head-C64-HW3-N{N}", "head", C=64, HW=3, N=N))
    for recipe in ("zero0", "zero01", "tiny", "same"):
        out.append(_case(f"head-C128-HW17-N3-{recipe}", "head", recipe=recipe, C=128, HW=17, N=3))
    out.append(_case("head-C256-HW9-N3-big", "head", dtypes=(F16,), recipe="big", C=256, HW=9, N=3))   # fp16 features at 6e4
    for C in (192, 1024):
        out.append(_case(f"head-C{C}-HW3-N1-raises", "head", dtypes=(BF16,), raises=True, C=C, HW=3, N=1))
    return out


# ------------------------------------------------------------------------------------------------------------ avgpool3d_down(_bwd)
def pool3d_cases() -> List[Case]:
    out = []
    for T in (1, 2, 3, 4, 5):
        for H, W in ((2, 2), (3, 2), (2, 3), (3, 3)):
            out.append(_case(f"pool3d-2x{T}x{H}x{W}x8", "pool3d", B=2, T=T, H=H, W=W, C=8))
    out.append(_case("pool3d-1x5x7x6x40", "pool3d", B=1, T=5, H=7, W=6, C=40))      # five vectors per pixel
    # group counts 255 / 256 / 257 of the OUTPUT (the forward's work items) ...
    for W in (510, 512, 514):
        out.append(_case(f"pool3d-1x2x2x{W}x8", "pool3d", B=1, T=2, H=2, W=W, C=8))
    # ... and of the INPUT (the backward's): 255, 256 and 514 = 2 * 257 (H >= 2: 257 is no product)
    out.append(_case("pool3d-1x1x3x85x8", "pool3d", B=1, T=1, H=3, W=85, C=8))      # 255 input groups
    out.append(_case("pool3d-1x1x2x128x8", "pool3d", B=1, T=1, H=2, W=128, C=8))    # 256 input groups
    out.append(_case("pool3d-1x1x257x2x8", "pool3d", B=1, T=1, H=257, W=2, C=8))    # 514 input groups, 128 output groups
    out.append(_case("pool3d-1x3x2x2x8-nan", "pool3d", recipe="nan", B=1, T=3, H=2, W=2, C=8))  # NaN propagates by arithmetic
    return out


# ------------------------------------------------------------------------------------------------------------ gn_leaky_apply, leaky_bwd
def leaky_apply_cases() -> List[Case]:
    out = []
    # (rows, per_row, C): per_row * C / 8 is no multiple of 256, so a block crosses the table row
    for rows, per, C in ((2, 37, 8), (3, 13, 64), (2, 7, 520), (2, 105, 32)):
        for affine in (1, 0):
            for slope in (0.2, 0.01):
                out.append(_case(f"leaky_apply-r{rows}-p{per}-C{C}-{'affine' if affine else 'bare'}-s{slope}", "leaky_apply",
                                 rows=rows, per_row=per, C=C, affine=affine, slope=slope))
    out.append(_case("leaky_apply-r2-p37-C8-affine-inf", "leaky_apply", recipe="inf", rows=2, per_row=37, C=8, affine=1, slope=0.2))
    out.append(_case("leaky_apply-r2-p37-C8-bare-inf", "leaky_apply", recipe="inf", rows=2, per_row=37, C=8, affine=0, slope=0.2))
    out.append(_case("leaky_apply-r2-p37-C8-bare-nan", "leaky_apply", recipe="nan", rows=2, per_row=37, C=8, affine=0, slope=0.2))
    return out


LEAKY_BWD_N = (1, 7, 8, 9, 2047, 2048, 2049, 2055)  # the element-wise tail at n % 8 of 1 and 7; one block and its edges


def leaky_bwd_cases() -> List[Case]:
    return [_case(f"leaky_bwd-n{n}-s{slope}", "leaky_bwd", n=n, slope=slope) for i, n in enumerate(LEAKY_BWD_N)
            for slope in ((0.2, 0.01)[i % 2],)]


# ------------------------------------------------------------------------------------------------------------ the statistics forms
STATS_CG = ((64, 32), (128, 32), (192, 32), (256, 32), (512, 32), (192, 8), (40, 4), (96, 8), (8, 4), (2048, 32))


def per_rows(C: int):
    ppp = 256 // (C // 8)
    return sorted({1, max(ppp - 1, 1), ppp, ppp + 1, 16 * ppp, 16 * ppp + 1, 3 * 16 * ppp + 5})


def stats_leaky_cases() -> List[Case]:
    out = []
    i = 0
    for C, G in STATS_CG:
        for per in per_rows(C):
            dt = ALL[i % 3]
            out.append(_case(f"stats_leaky-C{C}g{G}-p{per}-r2-{'affine' if i % 2 else 'bare'}", "stats_leaky", dtypes=(dt,),
                             C=C, G=G, per_row=per, rows=2, affine=i % 2))
            i += 1
    # the slab count capped by MAX_BLOCKS / rows: to 2, and to 1
    for rows in (1024, 1025):
        out.append(_case(f"stats_leaky-C8g4-p12288-r{rows}-bare", "stats_leaky", dtypes=(BF16,), recipe="device", C=8, G=4,
                         per_row=16 * 256 * 3, rows=rows, affine=0))
    # an EMPTY last slab: 18 slabs (MAX_BLOCKS / 108) of 17 pixels, 17 * 17 = 289 -- slab 17 starts at per_row and writes records
    # with n = 0.  63.9 M elements: the smallest tensor with an empty slab for any C
    out.append(_case("stats_leaky-C2048g32-p289-r108-bare-emptyslab", "stats_leaky", dtypes=(BF16,), recipe="device", C=2048, G=32,
                     per_row=289, rows=108, affine=0))
    for C, G in ((24, 8), (2056, 8), (2048, 257)):  # odd channels per group; C above 256 vectors; more groups than threads
        out.append(_case(f"stats_leaky-C{C}g{G}-raises", "stats_leaky", dtypes=(BF16,), raises=True, C=C, G=G, per_row=4, rows=1, affine=0))
    return out


def stats_pool_cases() -> List[Case]:
    """the pooled tensor is [B, To, Ho, Wo, C] with per_row = To * Ho * Wo; the input is (T, 2 Ho + 1, 2 Wo, C)"""
    out = []
    i = 0
    for C, G in STATS_CG:
        ppp = 256 // (C // 8)
        # one pixel; the step to a second pixel lane trip; several slabs: T odd and even, runs that cross a frame boundary
        for T, Ho, Wo in ((1, 1, 1), (2, 1, ppp + 1), (3, 1, 16 * ppp + 1), (4, 3, 8 * ppp + 1)):
            dt = ALL[i % 3]
            i += 1
            out.append(_case(f"stats_pool-C{C}g{G}-T{T}-Ho{Ho}-Wo{Wo}", "stats_pool", dtypes=(dt,), C=C, G=G, B=2, T=T, Ho=Ho, Wo=Wo))
    return out


# ------------------------------------------------------------------------------------------------------------ conv333_s2_dgrad_small
def dgrad_cases() -> List[Case]:
    out = []
    for T in (1, 2, 3):      # extents of 1: every live tap is k = 1; 2 and 3: both parities
        for H in (1, 2, 3):
            for W in (1, 2, 3):
                out.append(_case(f"dgrad-2x{T}x{H}x{W}-ci3-co8", "dgrad", dtypes=(BF16,), B=2, T=T, H=H, W=W, Cin=3, Cout=8))
    for W in (127, 128, 129):  # 64, 64 and 65 column pairs: one chunk, one chunk, two chunks
        out.append(_case(f"dgrad-1x2x3x{W}-ci3-co8", "dgrad", dtypes=(BF16,), B=1, T=2, H=3, W=W, Cin=3, Cout=8))
    for Cin in (1, 3, 4, 5, 8):  # the CI = 4 and CI = 8 tables
        out.append(_case(f"dgrad-1x3x4x5-ci{Cin}-co16", "dgrad", dtypes=HALF, B=1, T=3, H=4, W=5, Cin=Cin, Cout=16))
    for Cin, Cout in ((3, 144), (8, 72)):  # 62 208 B of LDS
        out.append(_case(f"dgrad-1x3x4x5-ci{Cin}-co{Cout}", "dgrad", dtypes=(BF16,), B=1, T=3, H=4, W=5, Cin=Cin, Cout=Cout))
    for Cin, Cout in ((3, 152), (8, 80)):  # 65 664 / 69 120 B: must raise
        out.append(_case(f"dgrad-1x3x4x5-ci{Cin}-co{Cout}-raises", "dgrad", dtypes=(BF16,), raises=True, B=1, T=3, H=4, W=5, Cin=Cin, Cout=Cout))
    out.append(_case("dgrad-2x3x4x5-ci3-co16-ps40", "dgrad", dtypes=(BF16,), B=2, T=3, H=4, W=5, Cin=3, Cout=16, ps=40))  # NaN in the gap
    return out


# ------------------------------------------------------------------------------------------------------------ capped grids
# bf16 cases whose work-item count is above the grid cap and no multiple of 256; the batch axis splits into halves at or below the
# cap.  `shape` is the tensor the kernel's work items are counted on ("items": how), `cap` the kernel's cap in work items.
DISC_CAP = 2048 * 256     # disc::blocks_for
LPIPS_CAP = 16384 * 256   # grid_for


def split_cases() -> List[Case]:
    return [
        # the disc kernels: just above 524 288 groups; two halves of 262 149 / 262 276 ...
        _case("split-avgpool3d_down", "split", dtypes=(BF16,), kernel="avgpool3d_down", shape=(2, 2, 2, 2 * 131077, 16), cap=DISC_CAP),
        _case("split-avgpool3d_down_bwd", "split", dtypes=(BF16,), kernel="avgpool3d_down_bwd", shape=(2, 1, 2, 131077, 8), cap=DISC_CAP),
        _case("split-gn_leaky_apply", "split", dtypes=(BF16,), kernel="gn_leaky_apply", shape=(2, 1, 1, 131077, 16), cap=DISC_CAP),
        _case("split-leaky_bwd", "split", dtypes=(BF16,), kernel="leaky_bwd", shape=(2, 1, 1, 131077, 16), cap=DISC_CAP),
        # the LPIPS kernels: above 4 194 304 vectors
        _case("split-relu", "split", dtypes=(BF16,), kernel="relu", shape=(2, 1, 1049, 1049, 16), cap=LPIPS_CAP),
        _case("split-maxpool2x2", "split", dtypes=(BF16,), kernel="maxpool2x2", shape=(2, 1, 2098, 2098, 16), cap=LPIPS_CAP),
        _case("split-relu_pool_bwd", "split", dtypes=(BF16,), kernel="relu_pool_bwd", shape=(2, 1, 1049, 1049, 64), cap=LPIPS_CAP),
    ]


def split_items(c: Case) -> int:
    """work items of a split case's whole launch (half of it per half of the batch)"""
    B, T, H, W, C = c["shape"]
    k = c["kernel"]
    if k == "avgpool3d_down":
        return B * ((T + 1) // 2) * (H // 2) * (W // 2) * (C // 8)
    if k in ("maxpool2x2",):
        return B * T * (H // 2) * (W // 2) * (C // 8)
    if k == "relu_pool_bwd":
        return B * T * ((H + 1) // 2) * ((W + 1) // 2) * (C // 8)
    return B * T * H * W * C // 8


def all_cases() -> List[Case]:
    return (scale_in_cases() + scale_in_bwd_cases() + relu_cases() + maxpool_cases() + relu_pool_bwd_cases() + head_cases()
            + pool3d_cases() + leaky_apply_cases() + leaky_bwd_cases() + stats_leaky_cases() + stats_pool_cases() + dgrad_cases()
            + split_cases())


def by_op() -> Dict[str, List[Case]]:
    d: Dict[str, List[Case]] = {}
    for c in all_cases():
        d.setdefault(c.op, []).append(c)
    return d
