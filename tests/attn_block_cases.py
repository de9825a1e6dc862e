"""Case table of the attention-BLOCK edge tests (a plain module, imported by tests/attn_block_ref.py, tests/test_attn_block_edges_host.py
and tests/test_gpu_attn_block_edges.py): the Python compositions `engine.spatial_attention` / `grad.attention_backward` and
`engine.v3_attn_spatial_temporal` / `grad3d.temporal_attention_backward`, forward and backward with parameter gradients.

A case is data only (`Case` / `_case` of tests/pass_edge_cases.py): a name, the block (`op`), the shape parameters, the dtypes, the
name of its input recipe (tests/attn_block_ref.py builds the tensors and weights from it) and a seed.

  blocks    sd3   spatial_attention(..., eps 1e-6, residual=True), names group_norm / to_q / to_k / to_v / to_out (nn.Linear weights)
            v3s   the vae3d spelling norm / q / k / v / proj_out with ConvP(c, c, (1, 1)) weights, eps 1e-5, residual=True
            v3st  v3_attn_spatial_temporal: the spatial half WITHOUT residual, the temporal half, the outer residual (the backward
                  hands it to the spatial half as `add_extra`)
  recipes   flat     default initialisation
            sharp    to_q / to_k scaled so that the fp64 score standard deviation is 4 (asserted within [2, 8] on the CPU)
            edgekey  one key m* of every frame holds >= 0.9 of every query's probability in fp64 (asserted on the CPU); `mstar`:
                     "last" = the last valid token, "block" = the first token of the last 32-key block; odd frames take its neighbour (m* - 1,
                     `block`: m* + 1) where the row has one, so that neighbouring frames differ

Tensors left out of the banded set, by case (attn_block_ref.unbanded gives the reasons in full):
  v3st-C128-N2-b2t3-sharp, v3s-C128-N2-b1t3-edgekey    k.bias     two keys: the rows of g_s are (a, -a); the restatement's fp32 comes
  v3st-C128-T2-S3-b1-sharp, v3st-C128-T2-S50-b1-flat   k_t.bias   out exactly antisymmetric and has no noise to band another order with
  every `edgekey` case                                 q.bias, k.bias   their error is ONE random number (the softmax backward's row sums)
                                                       times a fixed vector (k[m*] = 4 r, q = c r): two draws' norms differ by any factor
Those are asserted finite and bit-reproducible; the flat and sharp cases band them at every N edge they reach and every frame count.
(`k.bias` / `k_t.bias` elsewhere have a zero yardstick and are banded in the S-relative measure alone; the q / k gradients at N = 1,
q_t / k_t at T = 1, are exactly zero: tests/attn_block_ref.py.)"""
from typing import Dict, List

from pass_edge_cases import ALL, BF16, F16, F32, HALF, Case, _case  # noqa: F401  (re-exported)

SD3, V3S, V3ST = "sd3", "v3s", "v3st"
BLOCKS = (SD3, V3S, V3ST)

# token counts N = H * W as (H, W) pairs with H != W where N allows it
HW = {
    1: (1, 1), 2: (1, 2), 15: (3, 5), 16: (2, 8), 17: (1, 17),      # the smallest counts; one 16-key half of the fused kernel: 15 / 16 / 17
    31: (1, 31), 32: (4, 8), 33: (3, 11),                           # a 32-key block, a 32 x 32 transpose tile
    63: (7, 9), 64: (4, 16), 65: (5, 13),                           # a 64-pixel conv tile
    127: (1, 127), 128: (8, 16), 129: (3, 43),                      # npad 128 -> 256, a 128-query workgroup, a 128-pixel tile
    161: (7, 23),                                                   # a ragged second block (161 = 128 + 33)
    255: (15, 17), 256: (8, 32), 257: (1, 257),                     # a softmax row of 256 threads, a 256-pixel tile
}
N_EDGES = tuple(HW)
FRAMES = ((1, 1), (2, 1), (1, 3), (2, 3))        # (B, T)
ALL_FRAMES_N = (1, 33, 129)                      # every (B, T) meets these token counts
TEMPORAL_S = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (1, 5), 50: (5, 10)}   # ops.layernorm: four pixels per block


def _attn(block, C, N, B, T, recipe, mstar="last", dtypes=ALL, tag="", **kw) -> Case:
    H, W = HW[N]
    name = f"{block}-C{C}-N{N}-b{B}t{T}-{recipe}" + (f"-{mstar}" if recipe == "edgekey" and mstar != "last" else "") + tag
    return _case(name, block, dtypes=dtypes, recipe=recipe, C=C, H=H, W=W, B=B, T=T, mstar=mstar, **kw)


def spatial_cases() -> List[Case]:
    out = []
    multi = FRAMES[1:]
    # every N edge with more than one frame, the dominant key on the LAST valid token (N = 1: nothing to dominate)
    for i, N in enumerate(N_EDGES):
        B, T = multi[i % 3]
        out.append(_attn(BLOCKS[i % 3], 128, N, B, T, "edgekey" if N > 1 else "flat"))
    # ... and, from 33 tokens on, on the first token of the last 32-key block (another block, another frame count)
    for i, N in enumerate(n for n in N_EDGES if n >= 33):
        B, T = multi[(i + 2) % 3]
        out.append(_attn(BLOCKS[(i + 1) % 3], 128, N, B, T, "edgekey", mstar="block"))
    # every (B, T) at N = 1, 33, 129
    for i, N in enumerate(ALL_FRAMES_N):
        have = multi[N_EDGES.index(N) % 3]
        for j, (B, T) in enumerate(f for f in FRAMES if f != have):
            out.append(_attn(BLOCKS[(i + j + 1) % 3], 128, N, B, T, ("flat", "sharp")[(i + j) % 2]))
    # sharp scores at the power-of-two counts
    for i, N in enumerate((2, 16, 32, 64, 128, 256)):
        B, T = multi[(i + 2) % 3]
        out.append(_attn(BLOCKS[(i + 2) % 3], 128, N, B, T, "sharp"))
    # 512 channels: the fused forward of 16-bit models (and CVVAE_FUSED_ATTENTION=0); 257 x 512 x 6 frames is the largest case
    out.append(_attn(SD3, 512, 17, 2, 1, "edgekey"))
    out.append(_attn(V3ST, 512, 33, 1, 3, "sharp"))
    out.append(_attn(V3S, 512, 129, 2, 1, "edgekey", mstar="block"))
    out.append(_attn(SD3, 512, 257, 2, 3, "edgekey"))
    out.append(_attn(V3ST, 256, 65, 1, 3, "edgekey"))   # eight channels per group
    return out


def temporal_cases() -> List[Case]:
    """the temporal half: T <= 8 frames (the one-wave kernel and its backward) over S = H * W pixels"""
    out = []
    for i, (T, S, B, C) in enumerate(((1, 1, 2, 128), (2, 3, 1, 128), (5, 4, 2, 128), (8, 5, 1, 128), (2, 50, 1, 128), (8, 1, 2, 128),
                                      (5, 50, 1, 128), (1, 4, 1, 128), (8, 3, 1, 512))):
        H, W = TEMPORAL_S[S]
        out.append(_case(f"v3st-C{C}-T{T}-S{S}-b{B}-{('flat', 'sharp')[i % 2]}", V3ST, recipe=("flat", "sharp")[i % 2], C=C, H=H, W=W, B=B,
                         T=T, mstar="last"))
    # T > 8: the general forward kernel; the taped backward raises what ops.temporal_attention_bwd documents
    out.append(_case("v3st-C128-T9-S3-b1-flat-fwd", V3ST, recipe="flat", C=128, H=1, W=3, B=1, T=9, mstar="last", fwd_only=1))
    out.append(_case("v3st-C128-T17-S4-b1-sharp-fwd", V3ST, recipe="sharp", C=128, H=2, W=2, B=1, T=17, mstar="last", fwd_only=1))
    out.append(_case("v3st-C128-T9-S1-b1-flat-bwd-raises", V3ST, recipe="flat", raises=True, C=128, H=1, W=1, B=1, T=9, mstar="last"))
    return out


def all_cases() -> List[Case]:
    return spatial_cases() + temporal_cases()


def by_name() -> Dict[str, Case]:
    return {c.name: c for c in all_cases()}


def tokens(c: Case) -> int:
    return c["H"] * c["W"]


def frames(c: Case) -> int:
    return c["B"] * c["T"]
