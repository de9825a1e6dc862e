"""Case table of the network-boundary edge tests (a plain module, imported by tests/test_boundary_edges_host.py and
tests/test_gpu_boundary_edges.py): the ten passes through which every tensor enters and leaves the networks -- the two layout moves,
the two row-packers, the uint8 pixel conversions, the uint8 resize, the last layer's gather and the tile blend of
cvvae_amd/csrc/misc_kernels.hip, and the 2x2 sum of cvvae_amd/csrc/bwd_kernels.hip.

A case is data only (the Case of tests/pass_edge_cases.py): a name, the op, the shape parameters, the dtypes it runs in, the name of
its input recipe (tests/boundary_ref.py builds the tensors from it) and a seed.  A dtype of the converting moves is a pair
"src>dst".  The shapes are the smallest that reach each edge of the kernels; the comment next to each group names the edge.
No case goes past 2^31 elements: every index of these kernels is formed in 64-bit arithmetic from the block index on, and the one
32-bit quantity, the grid size, overflows only beyond 2^39 work items."""
from typing import Dict, List

from pass_edge_cases import ALL, BF16, F32, HALF, Case, _case

U8 = "u8"
PAIRS = tuple(f"{s}>{d}" for s in ALL for d in ALL)                  # the 9 instances of cvvae_ncdhw_to_ndhwc
PAIRS16 = tuple(f"{s}>{d}" for s in ALL for d in HALF)               # the 6 of cvvae_ncdhw_to_rowpack
PAIRS32 = tuple(f"{s}>{F32}" for s in ALL)                           # ... and the destination its header calls unsupported
BLOCK = 256                                                          # threads per block of every kernel here
GRID_CAP = 256 * 64                                                  # cvvae_upsample2x_sum: blocks beyond it become loop trips
PAD_ZERO, PAD_REPLICATE = 0, 1


# ------------------------------------------------------------------------------------------------------------ cvvae_ncdhw_to_ndhwc
def n2c_cases() -> List[Case]:
    shapes = [(1, 1, 1, 1, 1, 8),        # one pixel, one channel
              (2, 3, 2, 5, 13, 8),       # 260 pixels: two blocks, a tail of 4; b = pix / THW crosses inside the first block
              (1, 3, 1, 16, 16, 16),     # exactly 256 pixels, two vectors per pixel
              (1, 3, 1, 15, 17, 8),      # 255
              (1, 3, 1, 1, 257, 8),      # 257
              (2, 4, 1, 3, 5, 32),       # four vectors, three of them all padding
              (1, 8, 1, 3, 3, 8),        # C == Cpad: no pad channel
              (1, 12, 2, 3, 7, 16),      # the vector at c0 = 8 holds 4 real and 4 pad channels
              (3, 16, 1, 1, 1, 16)]      # THW = 1: every pixel another batch item
    return [_case(f"n2c-B{B}C{C}T{T}H{H}W{W}-pad{Cp}", "n2c", dtypes=PAIRS, recipe="rounding", B=B, C=C, T=T, H=H, W=W, Cpad=Cp)
            for B, C, T, H, W, Cp in shapes]


# ------------------------------------------------------------------------------------------------------------ cvvae_ndhwc_to_ncdhw
def c2n_cases() -> List[Case]:
    shapes = [(1, 1, 3, 5, 8, 8), (1, 2, 3, 5, 16, 16),                                # c == Cs
              (2, 1, 3, 5, 8, 3), (1, 1, 1, 1, 8, 1), (2, 2, 3, 7, 16, 4), (1, 1, 2, 3, 32, 16),   # c < Cs: NaN in the gap
              (1, 1, 15, 17, 8, 3), (1, 1, 16, 16, 8, 3), (1, 1, 1, 257, 8, 3),        # 255, 256, 257 pixels
              (2, 1, 10, 13, 8, 3)]                                                    # 260 pixels over two batch items
    return [_case(f"c2n-B{B}T{T}H{H}W{W}-c{c}of{Cs}", "c2n", recipe="gapnan", B=B, T=T, H=H, W=W, Cs=Cs, c=c)
            for B, T, H, W, Cs, c in shapes]


# ------------------------------------------------------------------------------------------------------------ cvvae_*_to_rowpack
def _rowpack_shapes():
    out = []
    for W in (1, 2, 5, 13, 61):          # W = 1, 2: both replicate columns read the same or neighbouring pixel; 61: W + 3 = 64
        for C in (1, 3, 4):              # one channel; the models' three; no zero channel slot
            for pad in (PAD_ZERO, PAD_REPLICATE):
                out.append((2, C, 2, 3, W, pad))
    # stored pixels B*T*H*(W+3) = 255, 256, 257: one below, at and one above a block
    out += [(1, 3, 1, 15, 14, PAD_REPLICATE), (1, 3, 1, 16, 13, PAD_REPLICATE), (1, 3, 1, 1, 254, PAD_REPLICATE),
            (1, 3, 1, 16, 13, PAD_ZERO)]
    return out


def rowpack_cases() -> List[Case]:
    out = []
    for B, C, T, H, W, pad in _rowpack_shapes():
        tag = f"B{B}C{C}T{T}H{H}W{W}-{'rep' if pad else 'zero'}"
        out.append(_case(f"rowpack_n-{tag}", "rowpack_n", dtypes=PAIRS16, B=B, C=C, T=T, H=H, W=W, pad=pad))
        out.append(_case(f"rowpack_c-{tag}-of8", "rowpack_c", dtypes=HALF, recipe="gapnan", B=B, C=C, T=T, H=H, W=W, pad=pad, Cs=8))
    # include/cvvae.h: no fp32 row-packed first layer
    out.append(_case("rowpack_n-B2C3T2H3W5-rep-f32dst-raises", "rowpack_n", dtypes=PAIRS32, raises=True, B=2, C=3, T=2, H=3, W=5,
                     pad=PAD_REPLICATE))
    out.append(_case("rowpack_c-B2C3T2H3W5-rep-of8-f32-raises", "rowpack_c", dtypes=(F32,), recipe="gapnan", raises=True, B=2, C=3, T=2,
                     H=3, W=5, pad=PAD_REPLICATE, Cs=8))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_frames_u8_to_ndhwc
def u8_in_cases() -> List[Case]:
    # every byte value in each channel position from 256 pixels on (recipe "allbytes"); one pixel; 255 / 256 / 257; every Cpad
    rows = [(n, cp) for n in (1, 255, 256, 257) for cp in (8, 16, 32)]
    return [_case(f"u8_in-npix{n}-pad{cp}", "u8_in", recipe="allbytes", npix=n, Cpad=cp) for n, cp in rows]


# ------------------------------------------------------------------------------------------------------------ cvvae_ncdhw_to_frames_u8
def u8_out_cases() -> List[Case]:
    out = [_case("u8_out-allbits", "u8_out", dtypes=HALF, recipe="allbits"),           # every non-NaN 16-bit pattern
           _case("u8_out-f32-steps", "u8_out", dtypes=(F32,), recipe="steps")]         # k / 127.5 - 1 and its neighbours, the ends
    for thw in (1, 255, 256, 257):
        out.append(_case(f"u8_out-thw{thw}", "u8_out", recipe="pixels", thw=thw))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_resize_u8_axis
def resize_cases() -> List[Case]:
    shapes = [(1, 1, 1, 5, 7),           # upscale from a single pixel
              (2, 5, 7, 1, 7),           # an output axis of 1 (H); W is the identity and is skipped
              (2, 5, 7, 5, 1),           # an output axis of 1 (W)
              (2, 2, 3, 7, 11),          # upscale on both axes
              (1, 64, 64, 63, 65),       # down by one, up by one
              (1, 300, 5, 7, 5),         # support of 43 input pixels
              (3, 17, 31, 40, 33),
              (2, 7, 9, 7, 20)]          # the identity axis is skipped
    out = []
    for T, H, W, oh, ow in shapes:
        for recipe in ("bytes", "binary"):   # random bytes; a random 0 / 255 pattern (the clamp and the rounding constant)
            out.append(_case(f"resize-T{T}H{H}W{W}-to{oh}x{ow}-{recipe}", "resize", dtypes=(U8,), recipe=recipe, T=T, H=H, W=W, oh=oh, ow=ow))
    # through the C ABI: inner = 1; 255, 256 and 257 output elements
    for outer, n_in, n_out in ((15, 9, 17), (16, 23, 16), (1, 300, 257)):
        out.append(_case(f"resize_axis-o{outer}-{n_in}to{n_out}-inner1", "resize_axis", dtypes=(U8,), recipe="bytes", outer=outer,
                         n_in=n_in, n_out=n_out))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_conv_out_gather
GATHER_SHAPES = [(1, 1, 1, 1),           # a frame smaller than one patch: every halo record is outside
                 (1, 1, 8, 32),          # one full patch
                 (1, 1, 9, 33),          # 4 blocks: below 8, the XCD remap is the identity
                 (2, 2, 9, 33),          # 16 blocks: remap active, no tail
                 (1, 3, 9, 65),          # 18 blocks: a tail of 2
                 (2, 5, 7, 31),          # 10 blocks, a tail of 2, every patch partial
                 (1, 1, 17, 97)]         # 12 blocks: a tail of 4, a 3 x 4 grid of patches


def gather_cases() -> List[Case]:
    out = []
    for B, T, H, W in GATHER_SHAPES:
        for pad in (PAD_ZERO, PAD_REPLICATE):
            for ldv in (28, 32, 40):              # NaN in every column >= 27; 28: the last 16-byte load ends on the row's end
                for recipe in ("normal", "ints"):  # ints: every sum exact in all three dtypes
                    tag = f"B{B}T{T}H{H}W{W}-{'rep' if pad else 'zero'}-ldv{ldv}-{recipe}"
                    out.append(_case(f"gather-{tag}", "gather", recipe=recipe, B=B, T=T, H=H, W=W, pad=pad, ldv=ldv, u8=0))
                    if B == 1:                    # the fused uint8 store
                        out.append(_case(f"gather-{tag}-u8", "gather", recipe=recipe, B=B, T=T, H=H, W=W, pad=pad, ldv=ldv, u8=1))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_blend
def blend_cases() -> List[Case]:
    rows = [  # (B, C, T, Ha, Wa, Hb, Wb, o, axis)
        (1, 2, 1, 4, 5, 4, 5, 1, 0),         # o = 1: w = 0, b's first row becomes a's last
        (1, 2, 2, 6, 7, 6, 7, 6, 0),         # the overlap spans the whole tile
        (2, 1, 1, 8, 13, 5, 13, 3, 0),       # o below both, Ha != Hb, Wb = 13
        (1, 3, 2, 9, 13, 7, 13, 7, 0),       # 546 elements: three blocks
        (1, 1, 1, 15, 17, 16, 17, 15, 0),    # 255 elements
        (1, 2, 1, 9, 16, 8, 16, 8, 0),       # 256
        (1, 1, 1, 2, 257, 1, 257, 1, 0),     # 257
        (1, 2, 1, 4, 5, 4, 5, 1, 1),         # the mirror images on W
        (1, 2, 2, 6, 7, 6, 7, 7, 1),
        (2, 1, 1, 5, 9, 5, 6, 3, 1),         # Wa != Wb
        (1, 3, 2, 13, 9, 13, 8, 4, 1),       # Hb odd, 312 elements
        (1, 2, 1, 16, 9, 16, 8, 8, 1),       # 256, o = Wb
        (1, 1, 1, 17, 20, 17, 16, 15, 1),    # 255
    ]
    return [_case(f"blend-B{B}C{C}T{T}-a{Ha}x{Wa}-b{Hb}x{Wb}-o{o}-axis{ax}", "blend", B=B, C=C, T=T, Ha=Ha, Wa=Wa, Hb=Hb, Wb=Wb, o=o,
                  axis=ax) for B, C, T, Ha, Wa, Hb, Wb, o, ax in rows]


# ------------------------------------------------------------------------------------------------------------ cvvae_upsample2x_sum
def upsum_cases() -> List[Case]:
    shapes = [(1, 1, 1, 8), (2, 3, 5, 8),
              (1, 7, 9, 24),             # three vectors per pixel
              (3, 2, 2, 520),
              (1, 3, 5, 136), (1, 4, 4, 128), (1, 1, 1, 2056)]   # 255, 256, 257 vectors
    out = [_case(f"upsum-N{N}H{H}W{W}C{C}", "upsum", N=N, H=H, W=W, C=C) for N, H, W, C in shapes]
    out.append(_case("upsum-N2H3W5C8-ints", "upsum", recipe="ints", N=2, H=3, W=5, C=8))
    # 4,196,352 vectors against the 16384 x 256 the capped grid covers in one trip: the last 2048 take the grid-stride loop
    out.append(_case("upsum-N1H2048W2049C8-gridcap", "upsum", dtypes=(BF16,), recipe="tiled_ints", N=1, H=2048, W=2049, C=8))
    return out


def all_cases() -> List[Case]:
    return (n2c_cases() + c2n_cases() + rowpack_cases() + u8_in_cases() + u8_out_cases() + resize_cases() + gather_cases()
            + blend_cases() + upsum_cases())


def by_op() -> Dict[str, List[Case]]:
    d: Dict[str, List[Case]] = {}
    for c in all_cases():
        d.setdefault(c.op, []).append(c)
    return d
