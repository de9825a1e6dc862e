"""Case tables of the pass-kernel edge tests (a plain module, imported by tests/test_pass_edges_host.py and
tests/test_gpu_pass_edges.py): GroupNorm statistics / finalize / apply / backward, LayerNorm, the row softmax and its backward, both
temporal-attention kernels and their backward, the fused 512-channel attention and the transpose.

A case is data only: a name, the op, the shape parameters `p`, the dtypes it runs in, the name of its input recipe
(tests/pass_ref.py builds the tensors from it) and a seed.  The shapes are the smallest that reach each edge of the kernels in
cvvae_amd/csrc/misc_kernels.hip, attention_kernel.hip and bwd_kernels.hip; the comment next to each group names the edge."""
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

F32, F16, BF16 = "f32", "f16", "bf16"
ALL = (F32, F16, BF16)
HALF = (F16, BF16)


@dataclass(frozen=True)
class Case:
    name: str
    op: str
    p: Tuple[Tuple[str, object], ...]   # shape parameters as sorted (key, value) pairs (hashable: the references are cached per case)
    dtypes: Tuple[str, ...] = ALL
    recipe: str = "normal"
    seed: int = 0
    raises: bool = False                # a shape the header documents as unsupported: the call must raise

    def __getitem__(self, k):
        return dict(self.p)[k]

    def get(self, k, default=None):
        return dict(self.p).get(k, default)


def _case(name, op, dtypes=ALL, recipe="normal", raises=False, **p) -> Case:
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003
    return Case(name, op, tuple(sorted(p.items())), tuple(dtypes), recipe, seed, raises)


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------ cvvae_gn_stats
def gn_stats_cases() -> List[Case]:
    shapes = []
    # (C, groups, S, rows)
    for S in (1, 7, 8, 63, 64, 65, 100):    # ppp = 8: below one pass; below, at and above one 8-deep trip (64 pixels); tail
        shapes.append((256, 32, S, 2))
    for S in (31, 256, 257, 300):           # pairs path (SUB = 2), ppp = 32: one 8-deep trip is 256 pixels
        shapes.append((64, 32, S, 2))
    shapes.append((192, 32, 130, 2))        # six-channel groups, cv = 24: 16 idle threads
    shapes.append((2048, 32, 9, 2))         # ppp = 1
    shapes.append((8, 4, 300, 2))           # ppp = 256
    shapes.append((512, 1, 1, 37))          # the LayerNorm-backward view: one group, one pixel per row
    for S in (8192, 8193, 16385):           # one, two and three splits
        shapes.append((128, 32, S, 2))
    out = []
    for i, (C, G, S, rows) in enumerate(shapes):
        # every shape at offset 0 and at +40 sigma, in one row mode each (alternating, so both modes meet both offsets)
        out.append(_case(f"gn_stats-C{C}g{G}-S{S}-r{rows}-off0", "gn_stats", C=C, G=G, S=S, rows=rows, offset=0.0, per_frame=i % 2))
        out.append(_case(f"gn_stats-C{C}g{G}-S{S}-r{rows}-off40", "gn_stats", C=C, G=G, S=S, rows=rows, offset=40.0,
                         per_frame=1 - i % 2))
    out.append(_case("gn_stats-C256g32-S65-r2-zerovar", "gn_stats", recipe="zerovar", C=256, G=32, S=65, rows=2, offset=0.0, per_frame=0))
    out.append(_case("gn_stats-C64g32-S257-r2-zerovar", "gn_stats", recipe="zerovar", C=64, G=32, S=257, rows=2, offset=0.0, per_frame=1))
    out.append(_case("gn_stats-C256g32-S100-r2-affine", "gn_stats", recipe="affine", C=256, G=32, S=100, rows=2, offset=0.0, per_frame=0))
    # through the C ABI: pix_stride > C, NaN in the gap channels
    out.append(_case("gn_stats-C256g32-S65-r2-ps264", "gn_stats", C=256, G=32, S=65, rows=2, offset=0.0, per_frame=0, ps=264))
    out.append(_case("gn_stats-C256g32-S65-r2-ps512", "gn_stats", C=256, G=32, S=65, rows=2, offset=40.0, per_frame=0, ps=512))
    out.append(_case("gn_stats-C64g32-S257-r2-ps72", "gn_stats", C=64, G=32, S=257, rows=2, offset=0.0, per_frame=0, ps=72))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_gn_finalize_frames
def gn_finalize_cases() -> List[Case]:
    out = []
    # slabs per (row, group, frame): the 8-deep main loop runs above 1792 records; 255 / 256 / 257 = one strided trip and its edge
    for C in (128, 64):
        for frames in (1, 3):
            for slabs in (1, 255, 256, 257, 1792, 1793, 2049 + 7):
                out.append(_case(f"gn_finalize-C{C}-f{frames}-slabs{slabs}", "gn_finalize", dtypes=(F32,), C=C, G=32, rows=2,
                                 frames=frames, slabs=slabs))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_gn_silu_apply
def gn_apply_cases() -> List[Case]:
    out = []
    # (C, S, rows): vector counts 111, 208 and 910 -- none a multiple of 256, the last one four blocks
    for i, (C, S, rows) in enumerate(((8, 37, 3), (64, 13, 2), (520, 7, 2))):
        for silu in (0, 1):
            out.append(_case(f"gn_apply-C{C}-S{S}-r{rows}-silu{silu}", "gn_apply", C=C, S=S, rows=rows, silu=silu,
                             per_frame=(i + silu) % 2))
    out.append(_case("gn_apply-C64-S13-r2-silu1-ps72", "gn_apply", C=64, S=13, rows=2, silu=1, per_frame=0, ps=72))
    out.append(_case("gn_apply-C8-S37-r3-silu0-ps16", "gn_apply", C=8, S=37, rows=3, silu=0, per_frame=0, ps=16))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_gn_bwd_input(_params)
def gn_bwd_cases() -> List[Case]:
    shapes = [(64, 32, 33, 2),       # pairs
              (512, 1, 1, 37),       # the LayerNorm backward's view
              (2048, 32, 5, 1)]      # ppp = 1
    # 1, 1, 1, 1, 2, 5 and 10 splits of 512 pixels; 10 is more than the apply pass's 8 split lanes (256 / 32 groups)
    shapes += [(128, 32, S, 2 if S < 4609 else 1) for S in (1, 3, 511, 512, 513, 2049, 4609)]
    out = []
    for i, (C, G, S, rows) in enumerate(shapes):
        silu, add = i % 2, (i // 2) % 2
        out.append(_case(f"gn_bwd_input-C{C}g{G}-S{S}-r{rows}-silu{silu}-add{add}", "gn_bwd", C=C, G=G, S=S, rows=rows, silu=silu,
                         add=add, params=0, per_frame=i % 2))
        out.append(_case(f"gn_bwd_input_params-C{C}g{G}-S{S}-r{rows}-silu{1 - silu}-add{1 - add}", "gn_bwd", C=C, G=G, S=S, rows=rows,
                         silu=1 - silu, add=1 - add, params=1, per_frame=1 - i % 2))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_layernorm
def layernorm_cases() -> List[Case]:
    out = []
    for i, C in enumerate((8, 504, 512, 520, 2048)):   # 63, 64, 65 vectors: below, at and above one trip of the lane loop; 2048: four
        for j, P in enumerate((1, 3, 4, 5, 50)):       # four pixels per block: P % 4 of 1, 3, 0, 1, 2
            out.append(_case(f"layernorm-C{C}-P{P}-off{30 if (i + j) % 2 else 0}", "layernorm", C=C, P=P,
                             offset=30.0 if (i + j) % 2 else 0.0, const_row=(P - 1) if P >= 3 else -1))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_softmax_rows / _bwd_rows
SOFTMAX_N = (1, 2, 63, 64, 65, 255, 256, 257, 1000)


def softmax_cases() -> List[Case]:
    out = []
    for n in SOFTMAX_N:
        ld_s = round_up(n, 128)
        out.append(_case(f"softmax-n{n}-ldp{ld_s}", "softmax", recipe="softmax_rows", n=n, ld_s=ld_s, ld_p=ld_s))
        small = round_up(n, 8)
        if small < ld_s:  # (n = 256: ld_s = n, nothing smaller holds the row)
            out.append(_case(f"softmax-n{n}-ldp{small}", "softmax", recipe="softmax_rows", n=n, ld_s=ld_s, ld_p=small))
    return out


def softmax_bwd_cases() -> List[Case]:
    out = []
    for i, n in enumerate(SOFTMAX_N):
        for alpha in (1.0, 0.25):
            out.append(_case(f"softmax_bwd-n{n}-alpha{alpha}", "softmax_bwd", n=n, ld_p=round_up(n, 128), ld_g=round_up(n, 128),
                             ld_o=round_up(n + 1, 8), alpha=alpha, rows=5))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_temporal_attention(_bwd)
def temporal_cases() -> List[Case]:
    rows = [
        # T <= 8: temporal_attn_kernel (one wave per pixel)
        (1, 8, 1, 1, "span"), (2, 64, 3, 1, "span"), (3, 512, 2, 3, "span"), (7, 520, 1, 5, "span"), (8, 2048, 1, 1, "span"),
        (8, 512, 2, 3, "span"),
        # T > 8: temporal_attn_general_kernel (one wave per (pixel, query frame), online softmax over the key frames)
        (9, 8, 1, 1, "span"), (17, 64, 3, 1, "span"), (40, 512, 2, 3, "span"), (9, 520, 1, 5, "rise"), (17, 2048, 1, 1, "fall"),
        (40, 64, 1, 5, "rise"), (9, 512, 2, 3, "fall"), (17, 520, 2, 3, "rise"),
    ]
    out = [_case(f"temporal-T{T}-C{C}-B{B}-S{S}-{r}", "temporal", recipe=r, T=T, C=C, B=B, S=S, span=40.0) for T, C, B, S, r in rows]
    # the header: C <= 2048 when T > 8 (a lane of the general kernel owns at most 4 x 8 channels)
    out.append(_case("temporal-T9-C2056-B1-S1-raises", "temporal", recipe="span", raises=True, T=9, C=2056, B=1, S=1, span=40.0))
    return out


def temporal_bwd_cases() -> List[Case]:
    rows = [(1, 8, 1, 1), (2, 512, 2, 3), (5, 520, 3, 1), (8, 512, 1, 5), (8, 8, 2, 3), (5, 8, 1, 5), (2, 520, 2, 3), (8, 520, 1, 1)]
    out = [_case(f"temporal_bwd-T{T}-C{C}-B{B}-S{S}", "temporal_bwd", recipe="span", T=T, C=C, B=B, S=S, span=20.0) for T, C, B, S in rows]
    out.append(_case("temporal_bwd-T9-C8-B1-S1-raises", "temporal_bwd", recipe="span", raises=True, T=9, C=8, B=1, S=1, span=20.0))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_attention_d512
ATTN_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 161)


def attention_cases() -> List[Case]:
    out = []
    for i, N in enumerate(ATTN_N):  # 32-key blocks, 16-key halves, 128-query workgroups: one below, at and one above each
        batch, extra = (1, 3)[i % 2], (0, 8, 40)[i % 3]
        out.append(_case(f"attention-N{N}-b{batch}-ldvt+{extra}", "attention", dtypes=HALF, recipe="span", N=N, batch=batch,
                         ldvt=round_up(N, 32) + extra, span=30.0))
    out.append(_case("attention-N65-b3-ldvt+8-dominant", "attention", dtypes=HALF, recipe="dominant", N=65, batch=3,
                     ldvt=round_up(65, 32) + 8, span=30.0))
    out.append(_case("attention-N33-b1-ldvt+0-qzero", "attention", dtypes=HALF, recipe="qzero", N=33, batch=1, ldvt=64, span=30.0))
    return out


# ------------------------------------------------------------------------------------------------------------ cvvae_transpose
def transpose_cases() -> List[Case]:
    out = []
    for R, C in ((1, 1), (31, 33), (32, 32), (33, 31), (70, 45)):
        out.append(_case(f"transpose-R{R}-C{C}-ld{C + 3}-ldo{R + 5}", "transpose", R=R, C=C, ld=C + 3, ld_out=R + 5, batch=3))
    out.append(_case("transpose-R32-C32-ld32-ldo32", "transpose", R=32, C=32, ld=32, ld_out=32, batch=3))
    return out


def all_cases() -> List[Case]:
    return (gn_stats_cases() + gn_finalize_cases() + gn_apply_cases() + gn_bwd_cases() + layernorm_cases() + softmax_cases()
            + softmax_bwd_cases() + temporal_cases() + temporal_bwd_cases() + attention_cases() + transpose_cases())


def by_op() -> Dict[str, List[Case]]:
    d: Dict[str, List[Case]] = {}
    for c in all_cases():
        d.setdefault(c.op, []).append(c)
    return d
