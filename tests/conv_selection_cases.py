"""The corpus behind tests/test_conv_selection_parity.py and tests/test_knobs.py (a plain module, not a test).

The host side of the convolution decides, from a descriptor and the environment knobs, which kernel runs, how many GroupNorm records
the launch writes and how large the weight gradient's workspace is.  None of that needs a GPU: `cvvae_conv_kernel_name`,
`cvvae_conv_gn_slabs`, `cvvae_conv_wgrad_workspace_bytes` and `cvvae_conv_wgrad_fuses_bias` answer from the library alone.  This
module sweeps descriptors of every layer kind the networks launch over the channel pairs and frame sizes of the configurations,
writes one text row per descriptor and hashes the rows per (variant, family); tests/golden/conv_selection.json holds the hashes a
library must reproduce.  A refactor of the launch path records nothing new: the golden was written by the library BEFORE it.

  python -m tests.conv_selection_cases fwd|wgrad            {family: sha256, ..., "#pairs": [...]} of this process's environment
  python -m tests.conv_selection_cases fwd|wgrad --rows     the rows themselves (diff two libraries' outputs to find a mismatch)
  python -m tests.conv_selection_cases --record             rewrite the golden (only for a change that MEANS to alter the selection)

A variant is an environment: the read-once knobs are parsed when the library first needs them, so each of their variants runs in a
child process of its own; CVVAE_CONV_DMA is read per call and is flipped inside this one."""
import functools
import hashlib
import json
import os
import subprocess
import sys
from typing import Dict, Iterator, List, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_selection.json")

CHANNELS = ((128, 128), (128, 256), (256, 256), (256, 512), (512, 512))
FRAMES = ((1, 32, 32), (5, 32, 32), (5, 64, 64), (9, 128, 128), (17, 256, 256), (17, 512, 512))
F16, BF16, F32, F32Q, F32Q6 = range(5)
DT_NAME = ("f16", "bf16", "f32", "f32q", "f32q6")

# (variant name, environment, corpus).  "default" and "conv_dma0" run in the calling process, the others in children.
VARIANTS = (
    ("default", {}, "fwd"),
    ("conv_dma0", {"CVVAE_CONV_DMA": "0"}, "fwd"),
    ("conv_small0", {"CVVAE_CONV_SMALL": "0"}, "fwd"),
    ("conv_small_kg0", {"CVVAE_CONV_SMALL_KG": "0"}, "fwd"),
    ("conv_quant0", {"CVVAE_CONV_QUANT": "0"}, "fwd"),
    ("conv_quant_w0.5", {"CVVAE_CONV_QUANT_W": "0.5"}, "fwd"),
    ("conv_nw4_0.5", {"CVVAE_CONV_NW4": "0.5"}, "fwd"),
    ("conv_nb2_0.5", {"CVVAE_CONV_NB2": "0.5"}, "fwd"),
    ("default", {}, "wgrad"),
    ("wgrad_dma0", {"CVVAE_WGRAD_DMA": "0"}, "wgrad"),
    ("wgrad_wgs256", {"CVVAE_WGRAD_WGS": "256"}, "wgrad"),
)
IN_PROCESS = ("default", "conv_dma0")


# ------------------------------------------------------------------------------------------------------------ forward corpus
# A family is one layer kind: (name, dtypes it exists for, function (Cin, Cout, T, H, W) -> descriptor fields or None).
# Output grids follow the networks: "same" padding at stride 1, the downsamplers' one-sided padding at stride 2.
def _base(cin, cout, T, H, W, k, stride=(1, 1, 1), pro=0, **kw):
    sT, sH, sW = stride
    To = T if sT == 1 else (T + 1) // 2
    d = dict(Ti=T, Hi=H, Wi=W, Cin=cin, in_pix_stride=cin, kT=k[0], kH=k[1], kW=k[2], sT=sT, sH=sH, sW=sW,
             pad_t=k[0] - 1, pad_h=(k[1] // 2 if sH == 1 else 0), pad_w=(k[2] // 2 if sW == 1 else 0), pad_mode_t=1, pad_mode_hw=0,
             prologue=pro, To=To, Ho=H // sH, Wo=W // sW, Cout=cout, out_pix_stride=cout)
    d.update(kw)
    return d


def _conv(k, stride=(1, 1, 1), pro=0, **kw):
    return lambda ci, co, T, H, W: _base(ci, co, T, H, W, k, stride, pro, **kw)


def _upsample(kT, mode, pro=0, **kw):
    def f(ci, co, T, H, W):
        if H > 256:  # (the decoders upsample TO 512^2 at most)
            return None
        d = _base(ci, co, T, H, W, (kT, 3, 3), pro=pro, upsample2x=mode, **kw)
        d.update(Ho=2 * H, Wo=2 * W, pad_h=1, pad_w=1)
        return d
    return f


def _time_shuffle(f):
    def g(ci, co, T, H, W):
        d = f(ci, co, T, H, W)
        if d is not None:
            d.update(out_mode=2, out_pix_stride=co // 2)
        return d
    return g


def _rowpack(ci, co, T, H, W):  # the first layer: 16 virtual channels = 4 stored pixels of 4 channels, kW folded into them
    if ci != 128:  # (Cin is fixed: one row per Cout)
        return None
    d = _base(16, co, T, H, W + 4, (3, 3, 1), in_overlap=1)
    d.update(in_pix_stride=4, Wo=W, pad_w=0)
    return d


def _taps_in_n(ci, co, T, H, W):  # the last layer: (3,1,1) over 3x3 taps x 3 channels held in N, fp32 out
    if ci != co:  # (Cout is fixed: one row per Cin)
        return None
    return _base(ci, 32, T, H, W, (3, 1, 1), pro=1, out_f32=1, out_pix_stride=32)


def _shortcut(ci, co, T, H, W):  # ResnetBlock conv2 (co -> co, behind GroupNorm + SiLU) + its 1x1 shortcut (ci -> co)
    if ci == co:
        return None
    return _base(co, co, T, H, W, (1, 3, 3), pro=1, sc_Cin=ci, sc_in_pix_stride=ci)


def _batched(ci, co, T, H, W):  # per-item weights (the attention products): w_batch_stride is filled in by desc()
    d = _base(ci, co, T, H, W, (1, 1, 1))
    d["w_batch_stride"] = -1
    return d


ALL, HALF, NOFAST = (F16, BF16, F32, F32Q, F32Q6), (F16, BF16), (F16, BF16, F32)
FWD_FAMILIES = (
    ("k333_s111_pro0", ALL, _conv((3, 3, 3))),
    ("k333_s111_pro1", ALL, _conv((3, 3, 3), pro=1)),
    ("k333_s111_pro1_zero_t", ALL, _conv((3, 3, 3), pro=1, pad_mode_t=0, pad_t=1)),
    ("k333_s222_pro0", ALL, _conv((3, 3, 3), (2, 2, 2))),
    ("k333_s122_pro0", ALL, _conv((3, 3, 3), (1, 2, 2))),
    ("k133_s111_pro0", ALL, _conv((1, 3, 3))),
    ("k133_s111_pro1", ALL, _conv((1, 3, 3), pro=1)),
    ("k133_s122_pro0", ALL, _conv((1, 3, 3), (1, 2, 2))),
    ("k111_pro0", NOFAST, _conv((1, 1, 1))),
    ("k111_pro2", NOFAST, _conv((1, 1, 1), pro=2)),
    ("k111_batched", NOFAST, _batched),
    ("upfold_k333", ALL, _upsample(3, 2)),
    ("upfold_k133", ALL, _upsample(1, 2)),
    ("upfold_k333_tfolds", ALL, _upsample(3, 2, w_time_folds=1)),
    ("upfold_k333_time_shuffle", ALL, _time_shuffle(_upsample(3, 2))),
    ("upgather_k333", ALL, _upsample(3, 1)),
    ("rowpack_k331", HALF, _rowpack),
    ("tapsn_k311_out_f32", ALL, _taps_in_n),
    ("shortcut_k133", NOFAST, _shortcut),
    ("k333_s111_pro1_tfolds", ALL, _conv((3, 3, 3), pro=1, w_time_folds=1)),
    ("k333_s111_pro0_time_shuffle", ALL, _time_shuffle(_conv((3, 3, 3)))),
)


def fwd_cases() -> Iterator[Tuple[str, str, dict]]:
    """(family, row key, descriptor fields) of every forward descriptor, in a fixed order"""
    for fam, dtypes, f in FWD_FAMILIES:
        for dt in dtypes:
            for ci, co in CHANNELS:
                for T, H, W in FRAMES:
                    fields = f(ci, co, T, H, W)
                    if fields is None:
                        continue
                    for B in (1, 2):
                        for fw in (0, 1):
                            d = dict(fields, dtype=dt, B=B, four_wave=fw, alpha=1.0, gn_rows_per_batch=1)
                            if dt == F32Q6:
                                d["act_bound"] = 8.0
                            yield fam, f"{DT_NAME[dt]} {ci}->{co} {T}x{H}x{W} B{B} fw{fw}", d


# ------------------------------------------------------------------------------------------------------------ weight-gradient corpus
WGRAD_FAMILIES = tuple((f"k{k[0]}{k[1]}{k[2]}_s{s[0]}{s[1]}{s[2]}", k, s)
                       for k in ((3, 3, 3), (1, 3, 3)) for s in ((1, 1, 1), (2, 2, 2), (1, 2, 2))) + (("k111_s111", (1, 1, 1), (1, 1, 1)),)


def wgrad_cases() -> Iterator[Tuple[str, str, dict]]:
    for fam, k, s in WGRAD_FAMILIES:
        for dt in (BF16, F32):
            for ci, co in CHANNELS:
                for T, H, W in FRAMES:
                    for B in (1, 2):
                        d = _base(ci, co, T, H, W, k, s)
                        d.update(dtype=dt, B=B)
                        yield fam, f"{DT_NAME[dt]} {ci}->{co} {T}x{H}x{W} B{B}", d


def desc(L, lib, fields: dict):
    d = L.ConvDesc()
    for k, v in fields.items():
        setattr(d, k, v)
    if fields.get("w_batch_stride") == -1:
        nb = lib.cvvae_packed_weight_bytes(d.Cout, d.Cin, 3 if d.dtype == F32 else 1)
        d.w_batch_stride = (nb + 15) // 16 * 16
    return d


# ------------------------------------------------------------------------------------------------------------ rows and hashes
def rows(corpus: str) -> Dict[str, List[str]]:
    """{family: [row, ...]} under THIS process's environment"""
    from cvvae_amd import _lib as L
    lib = L.load()
    out: Dict[str, List[str]] = {}
    if corpus == "fwd":
        for fam, key, fields in fwd_cases():
            d = desc(L, lib, fields)
            n = lib.cvvae_conv_kernel_name(d)
            out.setdefault(fam, []).append(f"{key} | {n.decode() if n else 'null'} | {lib.cvvae_conv_gn_slabs(d, 32)}")
    else:
        for fam, key, fields in wgrad_cases():
            d = desc(L, lib, fields)
            out.setdefault(fam, []).append(f"{key} | {lib.cvvae_conv_wgrad_workspace_bytes(d)} | {lib.cvvae_conv_wgrad_fuses_bias(d)}")
    return out


def pairs(fwd_rows: Dict[str, List[str]]) -> List[str]:
    """the distinct "dtype kernel" pairs a forward record reaches"""
    seen = set()
    for rs in fwd_rows.values():
        for r in rs:
            key, name, _ = r.split(" | ")
            if name != "null":
                seen.add(key.split(" ")[0] + " " + name)
    return sorted(seen)


def digest(r: Dict[str, List[str]]) -> Dict[str, str]:
    return {fam: hashlib.sha256("\n".join(rs).encode()).hexdigest() for fam, rs in r.items()}


def _here(corpus: str, env: Dict[str, str]) -> Dict[str, List[str]]:
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return rows(corpus)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _child(corpus: str, env: Dict[str, str]) -> subprocess.Popen:
    return subprocess.Popen([sys.executable, "-m", "tests.conv_selection_cases", corpus, "--json-rows"], cwd=ROOT,
                            stdout=subprocess.PIPE, text=True, env=dict(os.environ, **env))


@functools.lru_cache(maxsize=None)
def recorded() -> Dict[str, Dict[str, Dict[str, List[str]]]]:
    """{corpus: {variant: {family: rows}}} of the library in the tree, every variant (computed once per process)"""
    out: Dict[str, Dict[str, Dict[str, List[str]]]] = {"fwd": {}, "wgrad": {}}
    children = [(name, corpus, _child(corpus, env)) for name, env, corpus in VARIANTS if name not in IN_PROCESS]  # side by side
    for name, env, corpus in VARIANTS:
        if name in IN_PROCESS:
            out[corpus][name] = _here(corpus, env)
    for name, corpus, proc in children:
        text = proc.communicate()[0]
        assert proc.returncode == 0, f"variant {name}: the child process failed"
        out[corpus][name] = json.loads(text)
    return out


def summary(rec) -> dict:
    """what the golden stores: one sha256 per (corpus, variant, family) and the distinct (dtype, kernel) pairs of the default"""
    return {"hashes": {c: {v: digest(r) for v, r in vs.items()} for c, vs in rec.items()},
            "pairs": pairs(rec["fwd"]["default"]),
            "rows": {c: sum(len(x) for x in vs["default"].values()) for c, vs in rec.items()}}


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        with open(GOLDEN, "w") as fh:
            json.dump(summary(recorded()), fh, indent=1, sort_keys=True)
            fh.write("\n")
        s = json.load(open(GOLDEN))
        print(f"{GOLDEN}: {s['rows']} rows, {len(s['pairs'])} (dtype, kernel) pairs")
    else:
        r = rows(sys.argv[1])
        if "--json-rows" in sys.argv:
            json.dump(r, sys.stdout)
        elif "--rows" in sys.argv:
            for fam, rs in r.items():
                for x in rs:
                    print(fam, "|", x)
        else:
            print(json.dumps(dict(digest(r), **({"#pairs": pairs(r)} if sys.argv[1] == "fwd" else {})), indent=1))
