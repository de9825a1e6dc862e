"""Case table of the conv INPUT-gradient edge tests (a plain module, imported by tests/dgrad_ref.py, tests/test_dgrad_edges_host.py and
tests/test_gpu_dgrad_edges.py).  The input gradient is not one kernel but a composition -- WeightCache.conv_dgrad (taps flipped, Cin and
Cout exchanged, packed), then one launch of the forward conv kernel, and for the 3x3x3 convs zero-stuffing in front of it and a crop /
cvvae_pad_fold behind it (grad3d.dgrad333); Upsample3D adds the time un-shuffle and cvvae_upsample2x_sum -- and the table walks that
composition over the border rules of both families:

  paths       dgrad333 | conv_dgrad_133 (backward.conv_dgrad, per-frame 3x3, zero pad) | dgrad1x1 | upsample_chain
  geometries  the triples of engine.SD3_GEO / engine.V3_GEO and the discriminator's (GEO below; the host test compares them with engine's)
  strides     (1,1,1) everywhere; (2,2,2) and (1,2,2) under sd3-causal, sd3-sym, zero and v3-down
  extents     the smallest at which a rule can fail (B <= 2, nothing above (2, 5, 9, 12) but one W = 70 row, wider than any forward tile)
  channels    forward Cout -> forward Cin as the networks launch them

A case is data only.  `dims` is the extent B, T, H, W of the conv's INPUT (= of the gradient that comes out); for upsample_chain it is
the extent of Upsample3D's input, the conv runs at (B, T, 2H, 2W).  `add` is given only where the fold sums already (a replicate axis):
there the bound's n = 1 pays for the stored full correlation (tests/dgrad_ref.py); behind a copy / crop fold the stored tensor would be
one of two summands of a result the n = 0 bound holds to ONE rounding."""
from dataclasses import dataclass
from typing import List, Optional, Tuple

F32, F16, BF16 = "f32", "f16", "bf16"
ALL = (F32, F16, BF16)
REP, ZERO = 1, 0
DGRAD333, DGRAD133, DGRAD1X1, UPCHAIN = "dgrad333", "conv_dgrad_133", "dgrad1x1", "upsample_chain"
PC = ((2, 0), (1, 1), (1, 1))
P1 = ((1, 1), (1, 1), (1, 1))
PDOWN = ((2, 0), (0, 1), (0, 1))
P2D = ((0, 0), (1, 1), (1, 1))
P0 = ((0, 0), (0, 0), (0, 0))
GEO = {                       # name -> (pad, mode_t, mode_hw)
    "sd3-causal": (PC, REP, REP),
    "sd3-sym": (P1, REP, REP),
    "v3-causal": (PC, REP, ZERO),
    "zero": (P1, ZERO, ZERO),          # vae3d non-causal convs, the discriminator
    "v3-down": (PDOWN, REP, ZERO),     # Downsample3D of the SD2.1 family: strided only
    "v3-up": (P1, REP, ZERO),          # Upsample3D of the SD2.1 family: upsample_chain only
    "frame": (P2D, ZERO, ZERO),        # the per-frame 3x3 of conv_dgrad_133
    "none": (P0, ZERO, ZERO),          # 1x1
}
S1, S122, S222 = (1, 1, 1), (1, 2, 2), (2, 2, 2)
STRIDED_GEO = ("sd3-causal", "sd3-sym", "zero", "v3-down")
KERNEL = {DGRAD333: (3, 3, 3), DGRAD133: (1, 3, 3), DGRAD1X1: (1, 1, 1), UPCHAIN: (3, 3, 3)}


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


@dataclass(frozen=True)
class Case:
    name: str
    path: str
    geo: str
    stride: Tuple[int, int, int]
    cout: int                          # the FORWARD conv's output channels = real channels of g ...
    cin: int                           # ... and its input channels = real channels of the result
    dims: Tuple[int, int, int, int]    # B, T, H, W of the forward's input
    dtypes: Tuple[str, ...] = ALL
    add: bool = False                  # dgrad333(add=)
    residual: bool = False             # dgrad1x1(residual=)
    g_store: int = 0                   # stored channels of g (0: cout); the channels cout .. g_store are zero
    cin_pad: Optional[int] = None      # conv_dgrad(cin_pad=): K of the packed input-gradient weights
    cout_pad: Optional[int] = None     # conv_dgrad(cout_pad=): stored channels of the result, cin .. cout_pad exactly zero
    ncdhw: bool = False                # conv_dgrad(out_mode=OUT_NCDHW)
    up_time: bool = False              # upsample_chain: g went through the time shuffle + frame drop
    wscale: float = 0.1                # weights ~ wscale * randn

    @property
    def seed(self) -> int:
        return sum(ord(ch) * (i + 1) for i, ch in enumerate(self.name)) % 100003

    @property
    def k(self) -> Tuple[int, int, int]:
        return KERNEL[self.path]

    @property
    def pad(self):
        return GEO[self.geo][0]

    @property
    def mode_t(self) -> int:
        return GEO[self.geo][1]

    @property
    def mode_hw(self) -> int:
        return GEO[self.geo][2]

    @property
    def conv_dims(self) -> Tuple[int, int, int, int]:
        """the extent the conv itself reads: Upsample3D's conv runs over the nearest-upsampled tensor"""
        B, T, H, W = self.dims
        return (B, T, 2 * H, 2 * W) if self.path == UPCHAIN else self.dims

    @property
    def out_grid(self) -> Tuple[int, int, int]:
        """To, Ho, Wo of the forward conv"""
        return tuple((n + p[0] + p[1] - kk) // s + 1 for n, p, kk, s in zip(self.conv_dims[1:], self.pad, self.k, self.stride))

    @property
    def g_shape(self) -> Tuple[int, ...]:
        """the stored cotangent handed to the product function"""
        To, Ho, Wo = self.out_grid
        if self.path == UPCHAIN and self.up_time:   # [B, 2T-1, 2H, 2W, Cout/2]: frames 2t+n-1, frame -1 dropped
            return (self.dims[0], 2 * To - 1, Ho, Wo, self.cout // 2)
        return (self.dims[0], To, Ho, Wo, self.g_store or self.cout)

    @property
    def out_channels(self) -> int:
        """stored channels of the result (dgrad333 pads to a multiple of 8: conv_in's 3-channel gradient)"""
        if self.cout_pad is not None:
            return self.cout_pad
        return round_up(self.cin, 8) if self.path in (DGRAD333, UPCHAIN) else self.cin

    @property
    def out_shape(self) -> Tuple[int, ...]:
        B, T, H, W = self.dims
        return (B, self.cin, T, H, W) if self.ncdhw else (B, T, H, W, self.out_channels)

    @property
    def folds(self) -> bool:
        """does cvvae_pad_fold SUM here (a replicate axis with padding), or only copy / crop?"""
        (tf, tb), (hf, hb), _ = self.pad
        return self.path in (DGRAD333, UPCHAIN) and ((self.mode_t == REP and tf + tb > 0) or (self.mode_hw == REP and hf + hb > 0))


def cases() -> List[Case]:
    c: List[Case] = []

    def d3(name, geo, ch, dims, stride=S1, **kw):
        c.append(Case(name, DGRAD333, geo, stride, ch[0], ch[1], dims, **kw))

    # ---------------------------------------------------------------- dgrad333, stride 1: every fold / crop rule at its smallest extent
    d3("s1-sd3causal-T1", "sd3-causal", (128, 128), (2, 1, 3, 4), add=True)          # all three time taps fold into frame 0
    d3("s1-sd3causal-256to128", "sd3-causal", (256, 128), (1, 3, 5, 6))
    d3("s1-sd3causal-W70", "sd3-causal", (128, 128), (1, 2, 3, 70))                   # a forward tile edge inside the row padded by 2
    d3("s1-sd3sym-H1", "sd3-sym", (128, 128), (1, 2, 1, 5))                           # three padded rows fold into one
    d3("s1-sd3sym-W1-128to256", "sd3-sym", (128, 256), (2, 3, 4, 1), add=True)        # three padded columns fold into one
    d3("s1-sd3sym-T5", "sd3-sym", (128, 128), (1, 5, 2, 3))
    d3("s1-v3causal", "v3-causal", (128, 128), (1, 3, 4, 5), add=True)                # fold in time, crop in the plane
    d3("s1-v3causal-W70", "v3-causal", (128, 128), (1, 1, 2, 70))
    d3("s1-zero", "zero", (128, 128), (2, 5, 9, 12))                                  # crop on every axis; the largest extent
    d3("s1-zero-T1", "zero", (128, 128), (1, 1, 2, 3))
    d3("s1-zero-H1W1", "zero", (256, 128), (2, 2, 1, 1))
    # the networks' first and last layers
    d3("s1-conv-in-sd3causal-128to3", "sd3-causal", (128, 3), (1, 3, 4, 5))           # result stored with 8 channels, 3 .. 8 zero
    d3("s1-conv-in-v3causal-128to3", "v3-causal", (128, 3), (2, 2, 3, 6))
    d3("s1-dec-conv-out-sd3causal-3of16", "sd3-causal", (3, 128), (1, 2, 4, 5), g_store=16, wscale=0.5)
    d3("s1-dec-conv-out-v3causal-3of16", "v3-causal", (3, 128), (1, 3, 3, 4), g_store=16, wscale=0.5)
    d3("s1-enc-conv-out-sd3causal-32to512", "sd3-causal", (32, 512), (1, 2, 3, 4))
    d3("s1-dec-in-sd3causal-512to16", "sd3-causal", (512, 16), (1, 3, 2, 5))
    # ---------------------------------------------------------------- dgrad333, strided: both parities of every strided axis
    for geo in STRIDED_GEO:
        for st, tag in ((S222, "s222"), (S122, "s122")):
            folds = GEO[geo][1] == REP
            d3(f"{tag}-{geo.replace('-', '')}-even", geo, (128, 128), (2, 2, 4, 7), stride=st)   # T even, H even, W odd
            d3(f"{tag}-{geo.replace('-', '')}-odd", geo, (128, 128), (1, 3, 5, 6), stride=st, add=folds and st == S222)
    d3("s222-sd3causal-T1", "sd3-causal", (128, 128), (1, 1, 2, 3), stride=S222)      # one stuffed frame
    d3("s222-zero-T1", "zero", (128, 128), (2, 1, 3, 2), stride=S222)
    d3("s222-v3down-T5", "v3-down", (128, 128), (1, 5, 9, 12), stride=S222)
    d3("s122-sd3sym-T5-W70", "sd3-sym", (128, 128), (1, 5, 2, 70), stride=S122)
    # ---------------------------------------------------------------- backward.conv_dgrad: the per-frame 3x3 (B = frames)
    def d2(name, ch, dims, **kw):
        c.append(Case(name, DGRAD133, "frame", S1, ch[0], ch[1], dims, **kw))

    d2("f133-128", (128, 128), (2, 3, 5, 6))                                          # conv2 of a 3-D residual block: T frames
    d2("f133-256to128-W70", (256, 128), (2, 1, 3, 70))
    d2("f133-1px", (128, 128), (2, 1, 1, 1))
    d2("f133-cinpad32-3of32", (3, 128), (2, 1, 4, 5), g_store=32, cin_pad=32, wscale=0.5)   # grad.py: the 2-D decoder's conv_out
    d2("f133-ncdhw-512to16", (512, 16), (2, 1, 5, 7), ncdhw=True)                     # grad.py: conv_in's latent gradient
    d2("f133-coutpad8-64to3", (64, 3), (2, 1, 6, 5), cout_pad=8)                      # lpips.py: the first VGG conv
    d2("f133-coutpad128-512to4", (512, 4), (1, 1, 3, 4), cout_pad=128)                # grad.py: in front of post_quant_conv
    # ---------------------------------------------------------------- backward.dgrad1x1: 1, 37, 150 pixels per batch row
    def d1(name, ch, dims, **kw):
        c.append(Case(name, DGRAD1X1, "none", S1, ch[0], ch[1], dims, **kw))

    d1("l111-128-px1", (128, 128), (2, 1, 1, 1))
    d1("l111-128-px1-res", (128, 128), (2, 1, 1, 1), residual=True)
    d1("l111-256to128-px37-res", (256, 128), (2, 1, 1, 37), residual=True)
    d1("l111-128to256-px150", (128, 256), (2, 5, 3, 10))
    d1("l111-512-px37", (512, 512), (1, 1, 1, 37))
    d1("l111-512-px150-res", (512, 512), (2, 5, 3, 10), residual=True)
    # ---------------------------------------------------------------- Upsample3D: un-shuffle, dgrad333 at (2H, 2W), 2x2 block sums
    def up(name, geo, dims, up_time):
        c.append(Case(name, UPCHAIN, geo, S1, 256, 128, dims, up_time=up_time))

    up("up-v3up-time", "v3-up", (1, 3, 2, 3), True)                                   # g has 2T-1 = 5 frames of 128 channels
    up("up-v3up-time-T1", "v3-up", (2, 1, 2, 2), True)                                # one stored frame; the zero frame makes two
    up("up-v3up-plain", "v3-up", (2, 2, 3, 2), False)
    up("up-sd3causal-time-H1", "sd3-causal", (1, 2, 1, 3), True)
    return c
