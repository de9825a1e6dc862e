"""Case list and input generator of the packed-weight byte pin (a plain module, imported by tests/test_pack_cases_host.py,
tests/test_gpu_pack_bytes.py and tools/record_pack_hashes.py).

Every case calls ONE public packer of cvvae_amd.ops and is summarised as the sha256 of the packed buffer (whole, read-ahead tail
included), the sha256 of the padded bias and the scalar fields of the returned PackedConv.  The packed format is private to the
library (cvvae_pack_weights* write it, conv_fwd_kernel reads it), so the reference is the bytes the library wrote when
tests/golden/packed_weight_hashes.json was recorded; the fixture names that commit.

Inputs are the same on every machine: a multiplicative hash of the flat index, reduced to an odd multiple of 2^-24 in (-1, 1)
(exact in fp32, and wide enough that fp32 sums of a few of them round, which pins the summation order of the folds), cast to the
case's dtype on the CPU and only then moved to the device.  Into every weight (logical layout [.., co, ci, taps..]) go the values
at which a packer can differ from another one that is "almost" the same:

  -0.0       (co 0, ci 1), every tap.  The unfolded 16-bit path copies the element (the bytes keep the sign); every summing path --
             folds, upsample folds, and every fp32 form -- starts from +0.0 and writes +0.0.
  zero row   co 1 is all +0.0: the e3m2 block scale of a lane whose 32 values are all zero.
  spread     co 2, ci < 16: channel 5 is 0.75, odd channels are scaled by 2^-10 and even ones by 2^-6, so that one e3m2 lane holds
             a code at the top of the range next to subnormal and zero codes.
  fold ties  (3x3x3 weights) co 0, ci 0: time taps (1, u/2, u/1024) at every (ky, kx); co 0, ci 2: the same along kx at every
             (kt, ky); u = the ulp of 1.0 in the 16-bit type the sum is rounded to (fp16 for fp32 weights, whose hi part is fp16).
             1 + u/2 is a tie (to even: 1), 1 + u/2 + u/1024 rounds up only when summed in fp32 and rounded once.
The 9-tap runs of the (1,3,3) and (3,3,3) cases end on an unpaired tap (the fast-fp32 forms pair taps inside a run)."""
import hashlib
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

FORMS = ("f16", "bf16", "f32", "f32q", "f32q6")   # f32q: fast=True, f32q6: fast="fp6"
PLAIN = FORMS[:3]
HALF = FORMS[:2]
_TORCH = {"f16": torch.float16, "bf16": torch.bfloat16}
FIELDS = ("cout", "cin", "k", "cin_real", "folded", "batch_stride", "alg_taps", "time_folds", "wscale", "dt")


def torch_dtype(form: str) -> torch.dtype:
    return _TORCH.get(form, torch.float32)


def fast_arg(form: str):
    return {"f32q": True, "f32q6": "fp6"}.get(form, False)


@dataclass(frozen=True)
class Case:
    name: str
    packer: str                   # the function of cvvae_amd.ops
    shape: Tuple[int, ...]        # LOGICAL weight [co, ci, *k] ([batch, co, ci] for pack_weight_batched)
    forms: Tuple[str, ...]
    kw: Tuple[Tuple[str, object], ...] = ()
    variant: str = ""             # "wscale" | "out" | "strided" (pack_weight), "K" | "VT" (pack_weight_batched)


def _c(name, packer, shape, forms, variant="", **kw) -> Case:
    return Case(name, packer, tuple(shape), tuple(forms), tuple(sorted(kw.items())), variant)


CASES: List[Case] = [
    # Cout 40: two 32-row blocks, the second partial; Cin 20 -> cin_pad 128: eight k16 chunks, channels 20.. are padding
    _c("pack_weight-k111-40x20", "pack_weight", (40, 20, 1, 1, 1), FORMS, k=(1, 1, 1)),
    # Cout 33: one row in the second block; Cin 17 -> cin_pad 32: the second chunk holds one channel; 9 taps: an odd run
    _c("pack_weight-k133-33x17", "pack_weight", (33, 17, 1, 3, 3), FORMS, k=(1, 3, 3)),
    _c("pack_weight-k333-8x16", "pack_weight", (8, 16, 3, 3, 3), FORMS, k=(3, 3, 3)),      # three 9-tap runs; Cout < 32
    _c("pack_weight-k133-33x17-wscale", "pack_weight", (33, 17, 1, 3, 3), FORMS, "wscale", k=(1, 3, 3)),
    _c("pack_weight-k333-8x16-out", "pack_weight", (8, 16, 3, 3, 3), FORMS, "out", k=(3, 3, 3)),
    # the transposed view of a stored [33, 17, 9] weight, as the input-gradient convs read their weights: s_co < s_ci
    _c("pack_weight-k133-17x33-strided", "pack_weight", (17, 33, 1, 3, 3), FORMS, "strided", k=(1, 3, 3)),
    _c("pack_weight_t1-sum", "pack_weight_t1", (24, 20, 3, 3, 3), FORMS, mode="sum"),
    _c("pack_weight_t1-center", "pack_weight_t1", (24, 20, 3, 3, 3), FORMS, mode="center"),
    _c("pack_weight_tfolds", "pack_weight_tfolds", (33, 17, 3, 3, 3), FORMS),
    _c("pack_weight_tapsn", "pack_weight_tapsn", (3, 16, 3, 3, 3), PLAIN, time_folds=False),
    _c("pack_weight_tapsn-tfolds", "pack_weight_tapsn", (3, 16, 3, 3, 3), PLAIN, time_folds=True),
    _c("pack_weight_rowpack", "pack_weight_rowpack", (40, 3, 3, 3, 3), HALF, time_folds=False),
    _c("pack_weight_rowpack-tfolds", "pack_weight_rowpack", (40, 3, 3, 3, 3), HALF, time_folds=True),
    _c("pack_weight_upfold-t0", "pack_weight_upfold", (33, 17, 3, 3, 3), FORMS, tfold=0),
    _c("pack_weight_upfold-t1", "pack_weight_upfold", (33, 17, 3, 3, 3), FORMS, tfold=1),
    _c("pack_weight_upfold-t2", "pack_weight_upfold", (33, 17, 3, 3, 3), FORMS, tfold=2),
    _c("pack_weight_upfold-tfolds", "pack_weight_upfold", (33, 17, 3, 3, 3), FORMS, time_folds=True),
    # the attention blocks' per-frame matrices: K [N 40, C 128] and V^T [C 128, N 40 in rows of npad 48 -> cin_pad 128]
    _c("pack_weight_batched-K", "pack_weight_batched", (3, 40, 128), PLAIN, "K"),
    _c("pack_weight_batched-VT", "pack_weight_batched", (3, 128, 48), PLAIN, "VT"),
]
FORCED_WSCALE = 4.0


def case_ids() -> List[str]:
    return [f"{c.name}-{f}" for c in CASES for f in c.forms]


def params() -> List[Tuple[Case, str]]:
    return [(c, f) for c in CASES for f in c.forms]


def _seed(name: str) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


def dyadic(shape, seed: int) -> torch.Tensor:
    """fp32 tensor of odd multiples of 2^-24 in (-1, 1), a function of (flat index, seed) in integer arithmetic only"""
    n = 1
    for s in shape:
        n *= s
    h = ((torch.arange(n, dtype=torch.int64) + seed + 1) * 2654435761) & 0xFFFFFFFF
    num = 2 * (h >> 8) - (2 ** 24 - 1)                      # odd, |num| < 2^24
    return (num.to(torch.float64) / 2.0 ** 24).to(torch.float32).reshape(shape)


def tie_ulp(form: str) -> float:
    return 2.0 ** -7 if form == "bf16" else 2.0 ** -10


def has_ties(case: Case) -> bool:
    return len(case.shape) == 5 and case.shape[2:] == (3, 3, 3)


def make_weight(case: Case, form: str) -> torch.Tensor:
    """the LOGICAL weight of a case, CPU, in the case's dtype, planted values in place"""
    w = dyadic(case.shape, _seed(case.name))
    v = w if case.packer != "pack_weight_batched" else w.movedim(0, -1)   # [co, ci, ...]: a view, the plants go to every item
    g = min(16, v.shape[1])
    scale = torch.tensor([2.0 ** -10 if j % 2 else 2.0 ** -6 for j in range(g)])
    v[2, :g] = v[2, :g] * scale.reshape((g,) + (1,) * (v.dim() - 2))
    if g > 5:
        v[2, 5] = 0.75
    if has_ties(case):
        u = tie_ulp(form)
        roles = torch.tensor([1.0, u / 2, u / 1024])
        v[0, 0] = roles.reshape(3, 1, 1).expand(3, 3, 3)
        v[0, 2] = roles.reshape(1, 1, 3).expand(3, 3, 3)
    v[0, 1] = -0.0
    v[1] = 0.0
    return w.to(torch_dtype(form))


def make_bias(case: Case, form: str) -> torch.Tensor:
    co = case.shape[0]
    return dyadic((co,), _seed(case.name) + 7).to(torch_dtype(form))


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(ops, case: Case, form: str, device="cuda"):
    """call the case's packer of `ops` on the generated input; returns (PackedConv, sha256 of the input weight)"""
    w = make_weight(case, form)
    win = sha(w)
    kw: Dict[str, object] = dict(case.kw)
    fast = fast_arg(form)
    p = case.packer
    if p == "pack_weight_batched":
        wd = w.to(device)
        if case.variant == "K":       # K [batch, N, C]: rows are output channels
            return ops.pack_weight_batched(wd, (1, 1, 1), cin_pad=128, strides=(128, 1, 0), cout=40, cin=128), win
        return ops.pack_weight_batched(wd, (1, 1, 1), cin_pad=128, strides=(48, 1, 0), cout=128, cin=40), win   # row longer than cin
    if p == "pack_weight_tapsn":
        return ops.pack_weight_tapsn(w.to(device), **kw), win
    b = make_bias(case, form).to(device)
    if p == "pack_weight_rowpack":
        return ops.pack_weight_rowpack(w.to(device), b, **kw), win
    if p == "pack_weight":
        co, ci = case.shape[:2]
        k = kw.pop("k")
        taps = k[0] * k[1] * k[2]
        if case.variant == "strided":
            stored = w.reshape(co, ci, taps).permute(1, 0, 2).contiguous().to(device)      # [ci, co, taps]
            return ops.pack_weight(stored, b, k, strides=(taps, co * taps, 1), cout=co, cin=ci, fast=fast), win
        wd = w.reshape(co, ci, taps).to(device)
        if case.variant == "wscale":
            return ops.pack_weight(wd, b, k, wscale=FORCED_WSCALE, fast=fast), win
        if case.variant == "out":     # a caller's buffer, 64 bytes longer than needed: what the packer does not write stays
            from cvvae_amd import _lib as L
            nbytes = L.load().cvvae_packed_weight_bytes(co, ops.round_up(ci, ops.kchunk(k)), taps * (3 if form[:3] == "f32" else 1))
            out = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=device)
            return ops.pack_weight(wd, b, k, out=out, fast=fast), win
        return ops.pack_weight(wd, b, k, fast=fast), win
    return getattr(ops, p)(w.to(device), b, fast=fast, **kw), win        # pack_weight_t1 / _tfolds / _upfold


def summarise(pw, win: str) -> dict:
    fields = {f: getattr(pw, f) for f in FIELDS}
    fields["k"] = list(fields["k"])
    return dict(input_sha256=win, w_sha256=sha(pw.w), bias_sha256=sha(pw.bias), fields=fields)
