"""The conv instance sweep's case table (a plain module, imported by tests/test_conv_instance_coverage.py and
tests/test_gpu_conv_instances.py).

Every (instance, dtype) that the default build registers in cvvae_api.hip's instance table is parsed from
cvvae_amd/csrc/conv_table.h and gets one case: a CVVAE_CONV_FORCE string that selects it, the environment of the
selection (CVVAE_CONV_DMA, the descriptor's four_wave bit), the op variant it runs and the shapes, each with the kernel
name(s) the launch must report.  The shapes follow the instance's tile: one full and one partial tile on every spatial axis
(of the output grid, or of the phase grid of the folded upsample), front and back padding in both pad modes, one full and one
partial N tile (Cout = BN + 32), three K chunks, and for two-frame tiles an even frame count, To = 1 (a half-empty last time
tile) and an odd To >= 3 (split onto the one-frame sibling: two launches).

Nothing here needs a GPU: `conv_desc` builds the descriptor ops.conv would build, so the CPU test can resolve every case's kernel
name through the library's own selection."""
import os
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_H = os.path.join(ROOT, "cvvae_amd", "csrc", "conv_table.h")
API_HIP = os.path.join(ROOT, "cvvae_amd", "csrc", "cvvae_api.hip")

FIELDS = ("kt", "kh", "kw", "st", "sh", "sw", "tt", "th", "tw", "wm", "wn", "kg", "ksub", "pro", "ups")

# dtype keys of a case: the storage dtype of the tensors and the dtype code of the launch
F16, BF16, F32, F32Q, F32Q6 = "f16", "bf16", "f32", "f32q", "f32q6"
DT_CODE = {F16: 0, BF16: 1, F32: 2, F32Q: 3, F32Q6: 4}

# the row macros of cvvae_api.hip's g_table: (family, dtypes served, name suffix, N-blocks per wave, DMA-staged)
ROW_MACROS = {
    "CVVAE_ROW": ("G", (F16, BF16), "", 1, 0),
    "CVVAE_ROW_LD": ("LD", (F16, BF16), "_dma", 1, 1),
    "CVVAE_ROW_NB2": ("NB2", (F16, BF16), "_nb2", 2, 0),
    "CVVAE_ROW_XP": ("XP", (F32,), "_xp", 1, 0),
    "CVVAE_ROW_XQ": ("XQ", (F32Q,), "_xq", 1, 0),
    "CVVAE_ROW_XQ6": ("XQ6", (F32Q6,), "_xq6", 1, 0),
    "CVVAE_ROW_XQ6_NB2": ("XQ6_NB2", (F32Q6,), "_xq6nb2", 2, 0),
}


# ------------------------------------------------------------------------------------------------------------ table parsing
def _default_build(text: str) -> str:
    """drop the `#ifdef CVVAE_BUILD_*` branches (off in the default build), keep their `#else` branches"""
    out, stack = [], []  # stack of "is this branch live"
    for line in text.splitlines():
        s = line.strip()
        if s.startswith("#ifdef CVVAE_BUILD_") or s.startswith("#if defined(CVVAE_BUILD_"):
            stack.append(False)
            continue
        if s.startswith("#ifndef CVVAE_BUILD_"):
            stack.append(True)
            continue
        if stack and s.startswith("#else"):
            stack[-1] = not stack[-1]
            continue
        if stack and s.startswith("#endif"):
            stack.pop()
            continue
        if all(stack):
            out.append(line)
    return "\n".join(out)


def parse_macros(text: str) -> Dict[str, List[Tuple[int, ...]]]:
    """conv_table.h (default build) -> {macro name: [row tuples in order]}, with macros that list other macros expanded"""
    text = re.sub(r"//[^\n]*", "", _default_build(text))
    text = text.replace("\\\n", " ")
    bodies = {}
    for m in re.finditer(r"^\s*#define\s+(CVVAE_CONV_\w+)\(X\)(.*)$", text, flags=re.M):
        bodies[m.group(1)] = m.group(2)

    def expand(name, seen=()):
        assert name not in seen, f"recursive macro {name}"
        rows = []
        for tok in re.finditer(r"\bX\(([^)]*)\)|\b(CVVAE_CONV_\w+)\(X\)", bodies[name]):
            if tok.group(1) is not None:
                v = tuple(int(s) for s in tok.group(1).replace(" ", "").split(","))
                assert len(v) == len(FIELDS), (name, v)
                rows.append(v)
            else:
                rows += expand(tok.group(2), seen + (name,))
        return rows

    return {n: expand(n) for n in bodies}


def parse_registration(api_text: str) -> List[Tuple[str, str]]:
    """cvvae_api.hip's `static Instance g_table[] = {...}` -> [(table macro, row macro)] in table order"""
    m = re.search(r"static\s+Instance\s+g_table\[\]\s*=\s*\{(.*?)\};", api_text, flags=re.S)
    assert m, "g_table not found in cvvae_api.hip"
    return re.findall(r"(CVVAE_CONV_\w+)\((CVVAE_ROW\w*)\)", m.group(1))


@dataclass(frozen=True)
class Instance:
    family: str
    row: Tuple[int, ...]
    dtypes: Tuple[str, ...]
    suffix: str
    nbw: int
    ld: int

    def __getattr__(self, k):
        if k in FIELDS:
            return self.row[FIELDS.index(k)]
        raise AttributeError(k)

    @property
    def name(self) -> str:  # cvvae_api.hip instance_name()
        r = dict(zip(FIELDS, self.row))
        return ("conv_k{kt}{kh}{kw}_s{st}{sh}{sw}_t{tt}x{th}x{tw}_w{wm}x{wn}x{kg}_c%d_pro{pro}_ups{ups}" % (16 * r["ksub"])).format(**r) + self.suffix

    @property
    def force(self) -> str:  # CVVAE_CONV_FORCE, always with the explicit N-block suffix
        return "%dx%dx%d:%dx%dx%d:%d:%d" % (self.tt, self.th, self.tw, self.wm, self.wn, self.kg, self.ksub, self.nbw)

    @property
    def bn(self) -> int:
        return 32 * self.wn * self.nbw


def instances(table_text: Optional[str] = None, api_text: Optional[str] = None) -> List[Instance]:
    """every registered instance of the default build, in table order"""
    table_text = open(TABLE_H).read() if table_text is None else table_text
    api_text = open(API_HIP).read() if api_text is None else api_text
    macros = parse_macros(table_text)
    out = []
    for tab, rowm in parse_registration(api_text):
        assert rowm in ROW_MACROS, f"unknown row macro {rowm}: teach tests/conv_instance_cases.py its dtypes and name suffix"
        fam, dts, suf, nbw, ld = ROW_MACROS[rowm]
        for r in macros[tab]:
            out.append(Instance(fam, r, dts, suf, nbw, ld))
    return out


def expected_kernels(insts: List[Instance]) -> set:
    """{(kernel name, dtype)}: the (instance, dtype) kernels the build registers"""
    return {(e.name, dt) for e in insts for dt in e.dtypes}


def odd_frame_sibling(insts: List[Instance], e: Instance, dt: str, To: int, ups: int, sT: int) -> Optional[Instance]:
    """cvvae_api.hip odd_frame_sibling(): the one-frame twin that runs the last frame of an odd frame count"""
    if e.tt != 2 or not (To & 1) or To < 3 or ups == 2 or sT != 1:
        return None
    for s in insts:
        if dt not in s.dtypes:
            continue
        if s.tt == 1 and all(getattr(s, f) == getattr(e, f) for f in FIELDS if f != "tt") and s.nbw == e.nbw and s.ld == e.ld:
            return s
    return None


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Shape:
    """one launch of a case.  Input [B, Ti, Hi, Wi, Cs] (NDHWC); k = the DESCRIPTOR's taps (the reference op's)."""
    B: int
    Ti: int
    Hi: int
    Wi: int
    Cin: int
    Cout: int
    k: Tuple[int, int, int]
    stride: Tuple[int, int, int] = (1, 1, 1)
    pad: Tuple[Tuple[int, int], ...] = ((0, 0), (0, 0), (0, 0))
    mode_t: int = 0
    mode_hw: int = 0
    prologue: int = 0
    ups: int = 0
    tfold: int = 0            # ups == 2 on one frame: 1 = replicate time padding (taps summed), 2 = zero (centre tap)
    time_folds: bool = False  # weights packed with the time-fold slots (replicate time padding at the clip ends)
    out_mode: int = 0         # 0 NDHWC, 1 NCDHW, 2 TIME_SHUFFLE
    out_f32: bool = False
    residual: bool = False
    sc_cin: int = 0           # fused 1x1 shortcut over a second input with this many channels
    batched: bool = False     # per-item weights (w_batch_stride): the attention blocks' QK^T / PV products
    gn_out: int = 0           # fused statistics of the stored output for a gn_out-group GroupNorm
    rowpack: bool = False     # the row-packed first layer: x = [B, 3, T, H, W], Wi = W + 3 stored columns, Cin = 16 virtual
    gather: bool = False      # taps-in-N last layer: pack_weight_tapsn + conv_out_gather (3 output channels)
    act_bound: str = ""       # F32Q6: "host" (cvvae_conv_desc.act_bound) or "dev" (act_bound_dev)
    names: Tuple[str, ...] = ()

    @property
    def out_grid(self) -> Tuple[int, int, int]:
        """(To, Ho, Wo) as ops.conv computes them"""
        kT, kH, kW = self.k
        if self.ups == 2:
            return self.Ti + self.pad[0][0] + self.pad[0][1] - kT + 1, 2 * self.Hi, 2 * self.Wi
        Hl, Wl = (2 * self.Hi, 2 * self.Wi) if self.ups else (self.Hi, self.Wi)
        To = (self.Ti + sum(self.pad[0]) - kT) // self.stride[0] + 1
        Ho = (Hl + sum(self.pad[1]) - kH) // self.stride[1] + 1
        Wo = (Wl + sum(self.pad[2]) - kW) // self.stride[2] + 1
        if self.rowpack:
            Wo = self.Wi - 3
        return To, Ho, Wo

    @property
    def pixels(self) -> int:
        To, Ho, Wo = self.out_grid
        return self.B * To * Ho * Wo


@dataclass
class Case:
    inst: Instance
    dtype: str
    dma: int
    four_wave: int
    variant: str
    shapes: List[Shape] = field(default_factory=list)

    @property
    def id(self) -> str:
        return f"{self.inst.name}-{self.dtype}"

    @property
    def force(self) -> str:
        return self.inst.force

    def env(self) -> Dict[str, str]:
        return {"CVVAE_CONV_FORCE": self.force, "CVVAE_CONV_DMA": str(self.dma), "CVVAE_FOUR_WAVE": str(self.four_wave)}


def _kchunk(k):
    return {(3, 3, 3): 16, (1, 3, 3): 32, (1, 1, 1): 128, (3, 3, 1): 16, (3, 1, 1): 32}[tuple(k)]


def _ru(x, m):
    return (x + m - 1) // m * m


def _gn_cout(bn: int) -> int:
    """an output width whose 32 groups carry fused statistics (4, 8 or 16 channels per group); a partial N tile where BN allows"""
    return 128 if bn >= 256 else 256


def _variant(e: Instance) -> str:
    k = (e.kt, e.kh, e.kw)
    if k == (3, 3, 1):
        return "rowpack"
    if k == (3, 1, 1):
        return "tapsn"
    if e.ups == 2:
        return "ups2_t1" if e.kt == 1 else "ups2"
    if e.ups == 1:
        return "ups1"
    if e.sh > 1:
        return "strided"
    if k == (1, 1, 1):
        return "c111_gn" if e.pro == 2 else "c111"
    if k == (1, 3, 3):
        return "c133"
    return "c333"


def _spatial(e: Instance, stride_hw: int = 1, fold: bool = False):
    """(Hi, Wi, Ho, Wo): a full and a partial tile on each axis of the output (per-phase) grid"""
    Ho = e.th + 3 if e.th > 1 else 3
    Wo = e.tw + 8
    if fold:
        return Ho, Wo, 2 * Ho, 2 * Wo
    if stride_hw == 2:
        return 2 * Ho - 1, 2 * Wo - 1, Ho, Wo  # pad (1, 1): the last output reads the back pad
    return Ho, Wo, Ho, Wo


def _frames(e: Instance) -> List[int]:
    """output frame counts: first and last frames in every case; two-frame tiles also take To = 1 and an odd count"""
    if e.tt == 2:
        return [4, 1, 3]
    if e.tt == 4:
        return [6]
    return [3]


def make_case(insts: List[Instance], e: Instance, dt: str) -> Case:
    v = _variant(e)
    fast = dt in (F32Q, F32Q6)
    c = Case(e, dt, dma=1 if e.ld else 0, four_wave=1, variant=v)
    fourw = e.wm * e.wn * e.kg == 4
    # three K chunks, rounded up to the family's channel granularity; the folded upsample packer pads Cin to 32 (96: six chunks of
    # 16 or three of 32)
    cin = 96 if e.ups == 2 else _ru(3 * 16 * e.ksub, _kchunk((e.kt, e.kh, e.kw)))
    cout_edge = e.bn + (64 if e.nbw == 2 else 32)
    if fourw:
        cout_edge = 128  # eligible only with Cout <= 128 = BN: no partial N tile exists for it
    ab = ("dev" if e.ups == 2 else "host") if dt == F32Q6 else ""
    out16 = dt in (F16, BF16)
    shapes = []
    REP, ZERO = 1, 0
    for i, mode in enumerate((REP, ZERO)):
        gn = 0 if i == 0 else 32
        cout = cout_edge if (i == 0 or fourw) else _gn_cout(e.bn)
        if e.nbw == 2 and cout % 64:
            cout = _ru(cout, 64)
        kw = dict(mode_t=mode, mode_hw=mode, prologue=e.pro, act_bound=ab)
        if v in ("c333", "ups1", "strided"):
            Hi, Wi, Ho, Wo = _spatial(e, e.sh)
            if v == "strided":
                To = 3
                if e.kt == 1:  # image mode: the per-frame strided conv
                    tpad = (0, 0)
                else:
                    tpad = (1, 1) if e.st == 2 else ((2, 0) if mode == REP else (1, 1))
                Ti = (To - 1) * e.st + e.kt - sum(tpad)
                shapes.append(Shape(1 + i, Ti, Hi, Wi, cin, cout, (e.kt, 3, 3), (e.st, e.sh, e.sw), (tpad, (1, 1), (1, 1)),
                                    gn_out=gn if out16 else 0, **kw))
                continue
            if v == "ups1":
                Hi, Wi = (e.th + 4) // 2, (e.tw + 8) // 2
            frames = _frames(e)
            for To in (frames if i == 0 or e.tt != 2 else [1]):
                tpad = (2, 0) if mode == REP else (1, 1)
                # causal replicate time padding through the fold slots: the record layout is walked by KG = 1 kernels only
                tf = mode == REP and e.kg == 1 and v == "c333"
                om, g = 0, (gn if out16 else 0)
                if v == "ups1":
                    tpad, om = (1, 1), (2 if i == 0 else 0)
                elif e.wn * e.nbw == 1 and i == 1 and not e.pro:
                    om, g = 1, 0  # conv_out (BN = 32): NCDHW output
                shapes.append(Shape(1, To + 2 - sum(tpad), Hi, Wi, cin, cout, (3, 3, 3), (1, 1, 1), (tpad, (1, 1), (1, 1)),
                                    time_folds=tf, out_mode=om, residual=i == 0 and e.kg == 2, gn_out=g, ups=e.ups, **kw))
            continue
        if v == "c133":
            Hi, Wi, Ho, Wo = _spatial(e)
            B, Ti = 1 + i, 3
            if fourw:  # eligible only with B * To * Ho * Wo >= 2^19: one long frame
                B, Ti, Hi = 1, 1, e.th + 3
                Wi = _ru(((1 << 19) + Hi - 1) // Hi - 8, e.tw) + 8
            sc = 128 if (i == 0 and e.kg == 1 and not fast) else 0
            res = i == 0 and not sc
            shapes.append(Shape(B, Ti, Hi, Wi, cin, cout, (1, 3, 3), (1, 1, 1), ((0, 0), (1, 1), (1, 1)), sc_cin=sc, residual=res,
                                gn_out=gn if out16 else 0, **kw))
            continue
        if v in ("c111", "c111_gn"):
            Ho, Wo = (e.th + 3 if e.th > 1 else 3), e.tw + 8
            if i == 0 and v == "c111":
                shapes.append(Shape(2, 1, Ho, Wo, cin, cout, (1, 1, 1), batched=True, out_f32=True, **kw))
            else:
                shapes.append(Shape(1 + i, 2, Ho, Wo, cin, cout, (1, 1, 1), residual=i == 0, gn_out=gn if out16 else 0, **kw))
            continue
        if v == "ups2":
            Hi, Wi, Ho, Wo = _spatial(e, fold=True)
            To = 3
            om = 2 if i == 0 else 0
            g = gn if out16 else 0
            shapes.append(Shape(1, To, Hi, Wi, cin, cout, (3, 3, 3), (1, 1, 1),
                                ((1, 1), (1, 1), (1, 1)), ups=2, time_folds=mode == REP, out_mode=om, gn_out=g, **kw))
            continue
        if v == "ups2_t1":
            Hi, Wi, Ho, Wo = _spatial(e, fold=True)
            shapes.append(Shape(1 + i, 1, Hi, Wi, cin, cout, (1, 3, 3), (1, 1, 1), ((0, 0), (1, 1), (1, 1)), ups=2,
                                tfold=1 if mode == REP else 2, gn_out=gn if out16 else 0, **kw))
            continue
        if v == "rowpack":
            Ho, Wo = e.th + 3, e.tw + 8
            for To in (_frames(e) if i == 0 else [1]):
                tpad = (2, 0) if mode == REP else (1, 1)
                shapes.append(Shape(1, To + 2 - sum(tpad), Ho, Wo + 3, 16, cout, (3, 3, 1), (1, 1, 1), (tpad, (1, 1), (0, 0)),
                                    rowpack=True, time_folds=mode == REP, gn_out=gn, **kw))
            continue
        if v == "tapsn":
            Ho, Wo = e.th + 3, e.tw + 8
            To = _frames(e)[0]
            if i == 0:  # the raw (3,1,1) conv: fp32 columns, two N tiles, causal replicate time padding with the fold slots
                shapes.append(Shape(1, To, Ho, Wo, cin, cout_edge, (3, 1, 1), (1, 1, 1), ((2, 0), (0, 0), (0, 0)), out_f32=True,
                                    time_folds=True, **kw))
            else:  # as the last layer: taps in N + conv_out_gather, 3 channels
                shapes.append(Shape(1, To, Ho, Wo, cin, 32, (3, 1, 1), (1, 1, 1), ((1, 1), (0, 0), (0, 0)), out_f32=True,
                                    gather=True, **kw))
            continue
        raise AssertionError(v)
    for s in shapes:
        To = s.out_grid[0]
        sib = odd_frame_sibling(insts, e, dt, To, s.ups, s.stride[0])
        s.names = (e.name,) + ((sib.name,) if sib else ())
    c.shapes = shapes
    return c


def cases(insts: Optional[List[Instance]] = None) -> List[Case]:
    insts = instances() if insts is None else insts
    return [make_case(insts, e, dt) for e in insts for dt in e.dtypes]


# ------------------------------------------------------------------------------------------------------------ descriptor
def conv_desc(L, case: Case, s: Shape, lib=None, act_bound_dev: int = 0x1000):
    """the cvvae_conv_desc ops.conv builds for this launch (no GPU: CPU-side name resolution).  act_bound_dev: the device
    address of the bound for "dev" cases (any non-null value resolves the name)."""
    d = L.ConvDesc()
    d.dtype = DT_CODE[case.dtype]
    kT, kH, kW = s.k
    if s.rowpack:
        kW = 1
    d.B, d.Ti, d.Hi, d.Wi, d.Cin = s.B, s.Ti, s.Hi, s.Wi, s.Cin
    d.in_pix_stride = 4 if s.rowpack else s.Cin
    d.in_overlap = 1 if s.rowpack else 0
    if case.dtype == F32Q6:
        if s.act_bound == "dev":
            d.act_bound_dev = act_bound_dev
        else:
            d.act_bound = 8.0
    d.upsample2x = s.ups
    d.kT, d.kH, d.kW = kT, kH, kW
    d.sT, d.sH, d.sW = s.stride
    d.pad_t, d.pad_h, d.pad_w = s.pad[0][0], s.pad[1][0], s.pad[2][0]
    d.pad_mode_t, d.pad_mode_hw = s.mode_t, s.mode_hw
    d.prologue = s.prologue
    d.gn_rows_per_batch = 1
    To, Ho, Wo = s.out_grid
    d.To, d.Ho, d.Wo, d.Cout = To, Ho, Wo, s.Cout
    d.out_mode = s.out_mode
    d.out_f32 = 1 if s.out_f32 else 0
    d.out_pix_stride = 0 if s.out_mode == 1 else (s.Cout // 2 if s.out_mode == 2 else s.Cout)
    d.alpha = 1.0
    if s.batched:
        lib = L.load() if lib is None else lib
        d.w_batch_stride = _ru(lib.cvvae_packed_weight_bytes(s.Cout, s.Cin, 3 if case.dtype == F32 else 1), 16)
    d.w_time_folds = 1 if s.time_folds else 0
    d.four_wave = case.four_wave
    if s.sc_cin:
        d.sc_Cin, d.sc_in_pix_stride = s.sc_cin, s.sc_cin
    return d


# ------------------------------------------------------------------------------------------------------------ fp64 reference
# Per-element bound:  |y - ref| <= a * S + b * |ref| + TINY,  S = (|W| * |A|) + |bias| + |residual| (+ the shortcut's |W2| * |X2|):
# the same convolution over absolute values, so an element's allowance follows ITS OWN terms, not the largest output.
A_ACC = 2.0 ** -16  # fp32 accumulation of <= 1728 products (K of these shapes), summation order free
ULP16 = {F16: 2.0 ** -11, BF16: 2.0 ** -8}  # one round-to-nearest of a 16-bit value, relative
XP_ULP = 4e-6       # split precision (tests/test_gpu_ops.py ULP[float32]): the dropped lo x lo products and the hi / lo split
FAST_ULP = 1.2e-4   # fast fp32 (tests/test_gpu_ops.py FAST_ULP): each product right to ~2^-14 (bf8 / e3m2 correction terms)
TINY = 1e-6
STATS_TOL = 2e-5    # fused statistics: |d mean| <= STATS_TOL * std, |d rstd| <= STATS_TOL * rstd (fp32 record merges)


def tolerance(case: Case, s: Shape) -> Tuple[float, float]:
    """(a, b) of the per-element bound for this launch"""
    dt = case.dtype
    if dt in (F16, BF16):
        # one rounding of a staged operand: the prologue's output, or a weight folded from several taps (folded upsample,
        # time-fold slots, summed time taps of one frame) -- each term's error is at most one 16-bit rounding of that term
        rounded = s.prologue or s.ups == 2 or s.time_folds or s.tfold
        a = A_ACC + (ULP16[dt] if rounded else 0.0)
        b = 2.0 ** -24 if s.out_f32 else ULP16[dt]
        return a, b
    return A_ACC + (XP_ULP if dt == F32 else FAST_ULP), 2.0 ** -24


def torch_dtype(dt: str):
    import torch
    return {F16: torch.float16, BF16: torch.bfloat16}.get(dt, torch.float32)


def make_tensors(case: Case, s: Shape, seed: int):
    """CPU operands in the storage dtype (the same rounded values the kernel consumes), NCDHW"""
    import torch
    g = torch.Generator().manual_seed(seed)
    dt = torch_dtype(case.dtype)

    def rn(*shape, scale=1.0, off=0.0):
        return torch.randn(shape, generator=g, dtype=torch.float64) * scale + off

    t = {}
    To, Ho, Wo = s.out_grid
    if s.rowpack:
        t["x"] = rn(s.B, 3, s.Ti, s.Hi, s.Wi - 3, off=0.25).to(dt)
        t["w"] = rn(s.Cout, 3, 3, 3, 3, scale=1 / 9.0).to(dt)
    elif s.gather:
        t["x"] = rn(s.B, s.Cin, s.Ti, s.Hi, s.Wi, off=0.25).to(dt)
        t["w"] = rn(3, s.Cin, 3, 3, 3, scale=(s.Cin * 27) ** -0.5).to(dt)
    else:
        t["x"] = rn(s.B, s.Cin, s.Ti, s.Hi, s.Wi, off=0.25).to(dt)
        kT = 3 if (s.ups == 2 or s.tfold) else s.k[0]
        kk = (kT, s.k[1], s.k[2])
        taps = kk[0] * kk[1] * kk[2]
        if s.batched:
            t["w"] = rn(s.B, s.Cout, s.Cin, scale=s.Cin ** -0.5).to(dt)
        else:
            t["w"] = rn(s.Cout, s.Cin, *kk, scale=(s.Cin * taps) ** -0.5).to(dt)
    t["bias"] = (torch.zeros(s.Cout if not s.gather else 3) if s.batched else rn(3 if s.gather else s.Cout, scale=0.5)).float()
    if s.prologue:
        t["scale"] = rn(s.B, s.Cin, scale=0.25, off=1.0).float()
        t["shift"] = rn(s.B, s.Cin, scale=0.25).float()
    if s.residual:
        t["res"] = rn(s.B, s.Cout, To, Ho, Wo).to(dt)
    if s.sc_cin:
        t["x2"] = rn(s.B, s.sc_cin, s.Ti, s.Hi, s.Wi, off=0.25).to(dt)
        t["w2"] = rn(s.Cout, s.sc_cin, scale=s.sc_cin ** -0.5).to(dt)
        t["bias2"] = rn(s.Cout, scale=0.5).float()
    return t


def operand(s: Shape, t) -> "torch.Tensor":
    """the conv's operand in fp64 (after the prologue), NCDHW, as stored (before upsample / padding)"""
    import torch
    x = t["x"].double()
    if s.prologue:
        x = x * t["scale"].double()[:, :, None, None, None] + t["shift"].double()[:, :, None, None, None]
        if s.prologue == 1:
            x = x * torch.sigmoid(x)
    return x


def _pad_input(s: Shape, x, mode_w_left: Optional[int] = None):
    """upsample + pad as the op sees it.  mode_w_left: override the mode of the front W pad (checker self-tests)"""
    import torch.nn.functional as F
    if s.ups:
        x = F.interpolate(x, scale_factor=(1.0, 2.0, 2.0), mode="nearest")
    (tf, tb), (hf, hb), (wf, wb) = s.pad
    if s.rowpack or s.gather:
        hf = hb = wf = wb = 1
    if s.tfold:
        tf, tb = 1, 1
    mode_t = s.mode_t if not s.tfold else (1 if s.tfold == 1 else 0)
    hw = "replicate" if s.mode_hw else "constant"
    if mode_w_left is not None and wf:
        x = F.pad(x, (wf, 0, 0, 0, 0, 0), mode="replicate" if mode_w_left else "constant")
        wf = 0
    if hf or hb or wf or wb:
        x = F.pad(x, (wf, wb, hf, hb, 0, 0), mode=hw)
    if tf or tb:
        x = F.pad(x, (0, 0, 0, 0, tf, tb), mode="replicate" if mode_t else "constant")
    return x


def _conv(xp, w, stride, pts):
    """fp64 convolution of the padded input: all outputs [B, Co, To, Ho, Wo] (pts None) or [P, Co] at pts = (b, t, y, x)"""
    import torch
    import torch.nn.functional as F
    if pts is None:
        return F.conv3d(xp, w, stride=stride)
    b, t, y, x = pts
    kT, kH, kW = w.shape[2:]
    wm = w.reshape(w.shape[0], -1).t()
    out = []
    for i in range(0, b.numel(), 4096):
        sl = slice(i, i + 4096)
        cols = []
        for dt_ in range(kT):
            for dy in range(kH):
                for dx in range(kW):
                    cols.append(xp[b[sl], :, t[sl] * stride[0] + dt_, y[sl] * stride[1] + dy, x[sl] * stride[2] + dx])
        patch = torch.stack(cols, -1).reshape(cols[0].shape[0], -1)  # [P, C * taps] in w's (C, kT, kH, kW) order
        out.append(patch @ wm)
    return torch.cat(out)


def reference(case: Case, s: Shape, t, pts=None, defect: Optional[Dict] = None):
    """(ref, S) in fp64: NCDHW [B, C, T, H, W] of the STORED layout's logical tensor (time shuffle applied), or [P, Cout] at pts.
    defect (checker self-tests only): {"w": weight override, "mode_w_left": pad mode of the front W border}"""
    import torch
    defect = defect or {}
    x = operand(s, t)
    w = defect.get("w", t["w"]).double()
    xp = _pad_input(s, x, defect.get("mode_w_left"))
    xa = _pad_input(s, x.abs(), defect.get("mode_w_left"))
    stride = s.stride
    if s.batched:
        ys, ss = [], []
        for i in range(s.B):
            wi = w[i].reshape(s.Cout, s.Cin, 1, 1, 1)
            ys.append(_conv(xp[i:i + 1], wi, stride, None))
            ss.append(_conv(xa[i:i + 1], wi.abs(), stride, None))
        y, S = torch.cat(ys), torch.cat(ss)
        assert pts is None
    else:
        y, S = _conv(xp, w, stride, pts), _conv(xa, w.abs(), stride, pts)
    bias = t["bias"].double()
    bshape = (1, -1) if pts is not None else (1, -1, 1, 1, 1)
    y = y + bias.reshape(bshape)
    S = S + bias.abs().reshape(bshape)
    if s.sc_cin:
        x2, w2 = t["x2"].double(), t["w2"].double().reshape(s.Cout, s.sc_cin, 1, 1, 1)
        y = y + _conv(x2, w2, (1, 1, 1), pts) + t["bias2"].double().reshape(bshape)
        S = S + _conv(x2.abs(), w2.abs(), (1, 1, 1), pts) + t["bias2"].double().abs().reshape(bshape)
    if s.residual:
        r = t["res"].double()
        if pts is not None:
            b, tt, yy, xx = pts
            r = r[b, :, tt, yy, xx]
        y, S = y + r, S + r.abs()
    if s.out_mode == 2:  # 'b (n c) t h w -> b c (t n) h w', frame -1 dropped
        def shuf(v):
            b_, nc, t_, h_, w_ = v.shape
            return v.reshape(b_, 2, nc // 2, t_, h_, w_).permute(0, 2, 3, 1, 4, 5).reshape(b_, nc // 2, 2 * t_, h_, w_)[:, :, 1:]
        y, S = shuf(y), shuf(S)
    return y, S


def compare(got, ref, S, a: float, b: float):
    """per-element check; returns (worst err / bound, index of the worst element, number of violations)"""
    import torch
    got = got.double()
    err = (got - ref).abs()
    bound = a * S + b * ref.abs() + TINY
    ratio = err / bound
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    worst = ratio.max().item()
    idx = tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0]) if ratio.numel() else ()
    return worst, idx, int((ratio > 1.0).sum())


def group_stats(y, groups: int, eps: float = 1e-6):
    """fp64 GroupNorm moments of a stored tensor [B, C, ...]: (mean, rstd) [B, groups]"""
    yy = y.double().reshape(y.shape[0], groups, -1)
    mean = yy.mean(-1)
    var = yy.var(-1, unbiased=False)
    return mean, (var + eps).rsqrt()


def compare_stats(mean, rstd, mean_ref, rstd_ref):
    """worst ratio of the fused statistics' error to STATS_TOL (mean error in units of the group's std)"""
    std = 1.0 / rstd_ref
    e1 = ((mean.double() - mean_ref).abs() / (STATS_TOL * std)).max().item()
    e2 = ((rstd.double() / rstd_ref - 1.0).abs() / STATS_TOL).max().item()
    return max(e1, e2)


def sample_points(case: Case, s: Shape, seed: int, n_random: int = 4096):
    """the output pixels a sampled reference evaluates: every pixel in the first or last row / column of a tile (the
    partial tile included) of the first and last frames and of every frame on a time-tile boundary, plus a seeded random set"""
    import torch
    assert s.out_mode == 0 and s.ups != 2, "sampled references: NDHWC, unfolded grids"
    e = case.inst
    To, Ho, Wo = s.out_grid

    def edges(n, tile):
        v = set()
        for s0 in range(0, n, tile):
            v.update((s0, min(s0 + tile, n) - 1))
        return v

    ts, ys, xs = edges(To, e.tt) | {0, To - 1}, edges(Ho, e.th), edges(Wo, e.tw)
    pts = set()
    for b in range(s.B):
        for t_ in ts:
            for y in range(Ho):
                for x in (range(Wo) if y in ys else sorted(xs)):
                    pts.add((b, t_, y, x))
    g = torch.Generator().manual_seed(seed)
    r = torch.stack([torch.randint(0, n, (n_random,), generator=g) for n in (s.B, To, Ho, Wo)], 1)
    pts.update(tuple(int(v) for v in row) for row in r)
    p = torch.tensor(sorted(pts), dtype=torch.long)
    return tuple(p[:, i] for i in range(4))
