"""Yardstick, per-element bound, product call, emulation and seeded defects of the conv input-gradient edge tests (plain torch on the
CPU; nothing here needs a GPU).  tests/dgrad_edge_cases.py holds the cases; tests/test_dgrad_edges_host.py checks this module,
tests/test_gpu_dgrad_edges.py uses it against the HIP kernels.

The yardstick is fp64 torch.autograd of the FORWARD op over the dtype-rounded operands: F.conv3d(pad3(x), w, stride) with the
padding applied H / W first, then T (emu_ops._pad3's order, the reference's); for upsample_chain nearest interpolate, the conv, then
the time shuffle "b (n c) t h w -> b c (t n) h w" with frame 0 dropped, as Upsample3D does.  `add` / `residual` are added in fp64.
S is the same gradient over |g|, |w| (+ |add|, |residual|): the element's OWN summands.

The bound of every element has the conv tests' form, with the constants of tests/conv_instance_cases.py:

    |got - ref| <= a * S + b * |ref| + TINY

  16-bit   a = A_ACC + n * ULP16[dt],  b = ULP16[dt]
  fp32     a = A_ACC + XP_ULP,         b = 2^-24

A_ACC pays the fp32 accumulation (K <= 512 * 27 here sums in MFMA order; 2^-16 of S is 256 roundings), XP_ULP the split-precision
products of fp32 models, b the ONE rounding of the result to its storage dtype.  n counts the INTERMEDIATE tensors that are stored in
the storage dtype and of which several elements are then summed into one result element: each stored partial is off by at most one
rounding, ULP16 of ITS value, and the partials' magnitudes sum to at most the element's share of S, so every such tensor costs at
most ULP16 * S.

  n = 0    one launch writes the result: backward.conv_dgrad, backward.dgrad1x1 (the residual joins the fp32 accumulator inside the
           launch), and dgrad333 where the padding's adjoint is a crop / copy of the stored full correlation (zero modes)
  n = 1    dgrad333 with a replicate axis: cvvae_pad_fold sums stored elements of the full correlation (and `add`) in fp32
  n = 2    upsample_chain: cvvae_upsample2x_sum sums four stored elements of dgrad333's result, itself n = 1

These follow from the number formats and the composition alone; nothing is fitted to a kernel's or the emulation's output.  Operands
are of order 1 (weights ~ 0.1, or 0.5 where only three cotangent channels are real), so that TINY stays below 1 % of the median
bound of every case (asserted on the CPU) and is never what lets an element pass.

`emulate` restates the composition over tests/emu_ops.py -- independently of cvvae_amd/grad3d.py and backward.py, whose real
functions the host test runs under emu_ops.patched() and compares with it bit for bit -- and takes one seeded defect of `DEFECTS`,
which the host test must see beyond the bound."""
import functools
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

import dgrad_edge_cases as DC
from conv_instance_cases import A_ACC, TINY, ULP16, XP_ULP
from dgrad_edge_cases import BF16, DGRAD1X1, DGRAD133, DGRAD333, F16, F32, REP, UPCHAIN, ZERO, Case

DTYPE = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
FULL = ((2, 2), (2, 2), (2, 2))
DEFECTS = ("no_flip_w", "no_flip_t", "swap_fold_t", "swap_crop", "stuff_phase", "drop_last_row", "no_add", "swap_unshuffle",
           "frame_at_end", "rep_as_zero_hw")


def n_stored(case: Case) -> int:
    """the n of the bound: see the module docstring"""
    if case.path == UPCHAIN:
        return 2 if case.folds else 1
    return 1 if case.folds else 0


def coefficients(case: Case, dt: str) -> Tuple[float, float]:
    if dt == F32:
        return A_ACC + XP_ULP, 2.0 ** -24
    return A_ACC + n_stored(case) * ULP16[dt], ULP16[dt]


# =============================================================================================================== inputs
@functools.lru_cache(maxsize=4)
def inputs(case: Case, dt: str) -> Dict[str, torch.Tensor]:
    """w [cout, cin, *k], the stored cotangent g, `add` / `residual` where the case has them: randn of order 1, rounded to dt"""
    gen = torch.Generator().manual_seed(case.seed * 3 + DC.ALL.index(dt))
    rn = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)  # noqa: E731
    t = {"w": (rn(case.cout, case.cin, *case.k) * case.wscale).to(DTYPE[dt])}
    gs = case.g_shape
    real = gs[-1] if (case.path == UPCHAIN and case.up_time) else case.cout
    g = torch.zeros(gs, dtype=torch.float64)
    g[..., :real] = rn(*gs[:-1], real)
    t["g"] = g.to(DTYPE[dt])
    if case.add or case.residual:
        extra = torch.zeros(*case.dims, case.out_channels, dtype=torch.float64)
        extra[..., :case.cin] = rn(*case.dims, case.cin)
        t["add" if case.add else "residual"] = extra.to(DTYPE[dt])
    return t


# =============================================================================================================== fp64 yardstick
def pad3(f: torch.Tensor, pad, mode_t: int, mode_hw: int) -> torch.Tensor:
    """f [B,C,T,H,W]: H and W first, then T (emu_ops._pad3)"""
    (tf, tb), (hf, hb), (wf, wb) = pad
    if hf or hb or wf or wb:
        f = F.pad(f, (wf, wb, hf, hb, 0, 0), mode="replicate") if mode_hw == REP else F.pad(f, (wf, wb, hf, hb))
    if tf or tb:
        f = F.pad(f, (0, 0, 0, 0, tf, tb), mode="replicate") if mode_t == REP else F.pad(f, (0, 0, 0, 0, tf, tb))
    return f


def _forward(case: Case, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """the forward op of the case, x [B,Cin,T,H,W] fp64 -> what the stored cotangent pairs with, [B,*,*,*,C] channels last"""
    if case.path == UPCHAIN:
        x = F.interpolate(x, scale_factor=(1.0, 2.0, 2.0), mode="nearest")
    y = F.conv3d(pad3(x, case.pad, case.mode_t, case.mode_hw), w, None, stride=case.stride)
    if case.path == UPCHAIN and case.up_time:
        B, C2, T, H, W = y.shape
        y = y.reshape(B, 2, C2 // 2, T, H, W).permute(0, 2, 3, 1, 4, 5).reshape(B, C2 // 2, 2 * T, H, W)[:, :, 1:]
    return y.permute(0, 2, 3, 4, 1)


def _grad(case: Case, g: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    B, T, H, W = case.dims
    x = torch.zeros(B, case.cin, T, H, W, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        y = _forward(case, x, w)
        assert tuple(y.shape) == tuple(g.shape), (case.name, tuple(y.shape), tuple(g.shape))
        (gx,) = torch.autograd.grad((y * g).sum(), x)
    return gx.permute(0, 2, 3, 4, 1).contiguous()


def reference(case: Case, t: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ref, S) [B,T,H,W,cin] fp64 over the REAL channels"""
    real = t["g"].shape[-1] if (case.path == UPCHAIN and case.up_time) else case.cout
    g, w = t["g"][..., :real].double(), t["w"].double()
    ref, S = _grad(case, g, w), _grad(case, g.abs(), w.abs())
    extra = t.get("add", t.get("residual"))
    if extra is not None:
        e = extra[..., :case.cin].double()
        ref, S = ref + e, S + e.abs()
    return ref, S


@functools.lru_cache(maxsize=4)
def reference_of(case: Case, dt: str):
    """(ref, S, bound) of the case's own inputs in dtype dt"""
    ref, S = reference(case, inputs(case, dt))
    a, b = coefficients(case, dt)
    return ref, S, a * S + b * ref.abs() + TINY


def real_channels(case: Case, got: torch.Tensor) -> torch.Tensor:
    """the product's result -> [B,T,H,W,cin] (channels last, pad channels cut)"""
    if case.ncdhw:
        return got.permute(0, 2, 3, 4, 1)
    return got[..., :case.cin]


def worst(case: Case, dt: str, got: torch.Tensor):
    """(worst err / bound, its index (b, t, y, x, c), elements beyond their bound); a non-finite element counts as inf"""
    ref, _, bound = reference_of(case, dt)
    v = real_channels(case, got).double()
    ratio = (v - ref).abs() / bound
    ratio = torch.where(torch.isfinite(v), ratio, torch.full_like(ratio, float("inf")))
    top = ratio.max()
    return float(top), tuple(int(i) for i in torch.nonzero(ratio == top)[0]), int((ratio > 1.0).sum())


def check_result(case: Case, dt: str, got: torch.Tensor) -> int:
    """what holds for every result, emulated or from the GPU, besides the bound: shape, dtype, zero pad channels, exact zeros"""
    assert tuple(got.shape) == case.out_shape and got.dtype == DTYPE[dt], (case.name, dt, tuple(got.shape), got.dtype)
    if not case.ncdhw:
        pad_ch = got[..., case.cin:]
        assert torch.equal(pad_ch, torch.zeros_like(pad_ch)), (case.name, dt, "pad channels are not exactly zero")
    _, S, _ = reference_of(case, dt)
    dead = S == 0                      # no window reaches the position (no summand at all): the gradient is exactly 0
    assert bool((real_channels(case, got)[dead] == 0).all()), (case.name, dt, "an unreached position is not exactly zero")
    return int(dead.sum())


def rel_l2(case: Case, dt: str, got: torch.Tensor) -> float:
    """the network tests' measure: relative L2 error over the whole tensor"""
    ref = reference_of(case, dt)[0]
    return float((real_channels(case, got).double() - ref).norm() / ref.norm())


# =============================================================================================================== the product functions
def holder(w: torch.Tensor) -> torch.nn.Module:
    """a module tree with the one layer `c` for WeightCache"""
    m = torch.nn.Module()
    m.c = torch.nn.Module()
    m.c.weight = torch.nn.Parameter(w.clone(), requires_grad=False)
    return m


def call(case: Case, t: Dict[str, torch.Tensor], wc) -> torch.Tensor:
    """ONE call of the case through the product's own functions; t on the device the ops run on, wc = WeightCache(holder(t['w']))"""
    from cvvae_amd import _lib as L
    from cvvae_amd import backward, grad3d
    if case.path == DGRAD333:
        return grad3d.dgrad333(wc, t["g"], "c", case.pad, case.mode_t, case.mode_hw, case.dims, stride=case.stride, add=t.get("add"))
    if case.path == DGRAD133:
        kw = {}
        if case.cout_pad is not None:
            kw["cout_pad"] = case.cout_pad
        if case.ncdhw:
            kw["out_mode"] = L.OUT_NCDHW
        return backward.conv_dgrad(wc, t["g"], "c", case.k, case.pad, cin_pad=case.cin_pad, **kw)
    if case.path == DGRAD1X1:
        return backward.dgrad1x1(wc, t["g"], "c", residual=t.get("residual"))
    assert case.path == UPCHAIN
    x = t["g"].new_empty((*case.dims, case.cin))       # the tape's operand: read for its shape only when grads is None
    e = dict(x=x, pre="c", pad=case.pad, mode_t=case.mode_t, mode_hw=case.mode_hw, up_time=case.up_time)
    return grad3d.sd3_upsample_backward(wc, t["g"], e, None)


# =============================================================================================================== emulation + defects
def _dgrad_weights(emu, case: Case, w: torch.Tensor, defect: Optional[str]):
    """taps flipped on every axis, Cin / Cout exchanged, packed with K = cin_pad"""
    kt, kh, kw = case.k
    w5 = w.reshape(case.cout, case.cin, kt, kh, kw)
    axes = [a for a, skip in ((2, "no_flip_t"), (3, None), (4, "no_flip_w")) if defect != skip or skip is None]
    wt = w5.flip(axes).transpose(0, 1).contiguous().reshape(case.cin, case.cout, kt * kh * kw)
    return emu.pack_weight(wt, None, case.k, cin_pad=case.cin_pad)


def _emu_dgrad333(emu, case: Case, g: torch.Tensor, w: torch.Tensor, in_shape, add, defect: Optional[str]) -> torch.Tensor:
    B, T, H, W = in_shape
    (tf, tb), (hf, hb), (wf, wb) = case.pad
    Tz, Hz, Wz = T + tf + tb - 2, H + hf + hb - 2, W + wf + wb - 2
    st, sh, sw = case.stride
    if case.stride != (1, 1, 1):
        if defect == "drop_last_row":
            g = g.clone()
            g[:, :, -1] = 0
        gz = g.new_zeros((B, Tz, Hz, Wz, g.shape[-1]))
        if defect == "stuff_phase":      # the columns land one to the right of o * sw (what does not fit is lost)
            n = len(range(1, Wz, sw))
            gz[:, ::st, ::sh, 1::sw] = g[:, :, :, :n]
        else:
            gz[:, ::st, ::sh, ::sw] = g
        g = gz
    assert tuple(g.shape[1:4]) == (Tz, Hz, Wz)
    pw = _dgrad_weights(emu, case, w, defect)
    cp = DC.round_up(pw.cout, 8)
    gp = emu.conv(g, pw, pad=FULL, pad_mode_t=ZERO, pad_mode_hw=ZERO, cout_pad=cp if cp != pw.cout else None)
    mode_hw = case.mode_hw
    if defect == "rep_as_zero_hw":
        assert mode_hw == REP
        mode_hw = ZERO
    if mode_hw == ZERO:
        if defect == "swap_crop":
            hf, hb, wf, wb = hb, hf, wb, wf
        gp = gp[:, :, hf:hf + H, wf:wf + W].contiguous()
        phw = 0
    else:
        phw = hf
    pt = (tb, tf) if defect == "swap_fold_t" else (tf, tb)
    return emu.pad_fold(gp, pt, phw, case.mode_t, mode_hw, add=None if defect == "no_add" else add)


def _emu_unshuffle(g: torch.Tensor, defect: Optional[str]) -> torch.Tensor:
    """[B,2T-1,H,W,C] -> [B,T,H,W,2C]: the dropped frame back in front as zeros, frame 2t+n -> channel block n of frame t"""
    B, F2, H, W, C = g.shape
    zero = g.new_zeros((B, 1, H, W, C))
    gf = torch.cat([g, zero] if defect == "frame_at_end" else [zero, g], dim=1)
    T = (F2 + 1) // 2
    out = g.new_zeros((B, T, H, W, 2 * C))
    for n in range(2):
        m = 1 - n if defect == "swap_unshuffle" else n
        out[..., m * C:(m + 1) * C] = gf[:, n::2]
    return out


def emulate(case: Case, dt: str, defect: Optional[str] = None) -> torch.Tensor:
    """the composition over tests/emu_ops.py on the case's own inputs; defect: one seeded error of DEFECTS"""
    from tests import emu_ops as emu
    assert defect is None or defect in DEFECTS
    t = inputs(case, dt)
    g, w = t["g"], t["w"]
    if case.path == DGRAD333:
        return _emu_dgrad333(emu, case, g, w, case.dims, t.get("add"), defect)
    if case.path == UPCHAIN:
        B, T, H, W = case.dims
        gc = _emu_unshuffle(g, defect) if case.up_time else g
        gup = _emu_dgrad333(emu, case, gc, w, case.conv_dims, None, defect)
        return emu.upsample2x_sum(gup.view(B * T, 1, 2 * H, 2 * W, gup.shape[-1])).view(B, T, H, W, gup.shape[-1])
    pw = _dgrad_weights(emu, case, w, defect)
    if case.path == DGRAD133:
        from cvvae_amd import _lib as L
        return emu.conv(g, pw, pad=case.pad, pad_mode_t=ZERO, pad_mode_hw=ZERO, cout_pad=case.cout_pad,
                        out_mode=L.OUT_NCDHW if case.ncdhw else L.OUT_NDHWC)
    assert case.path == DGRAD1X1
    flat = lambda v: v.view(v.shape[0], 1, 1, -1, v.shape[-1])  # noqa: E731
    res = None if defect == "no_add" else t.get("residual")
    return emu.conv(flat(g), pw, residual=flat(res) if res is not None else None).view(*g.shape[:-1], pw.cout)


def _outer_taps_differ(L: int, pad, mode: int, stride: int) -> bool:
    """do the first and the last of three taps along one axis meet the input differently?  Per tap, the list of (output, input)
    index pairs under the forward's coordinate map; when the two lists agree, exchanging the taps' weights changes nothing"""
    n_out = (L + pad[0] + pad[1] - 3) // stride + 1
    meets = []
    for tap in (0, 2):
        pairs = []
        for o in range(n_out):
            i = o * stride + tap - pad[0]
            if mode == REP:
                i = min(max(i, 0), L - 1)
            if 0 <= i < L:
                pairs.append((o, i))
        meets.append(pairs)
    return meets[0] != meets[1]


def applies(defect: str, case: Case) -> bool:
    """can the defect change the case's result at all?  (where it cannot, the host test asserts that it does not)"""
    strided = case.stride != (1, 1, 1)
    is3 = case.path in (DGRAD333, UPCHAIN)
    (tf, tb), (hf, hb), (wf, wb) = case.pad
    W, T = case.conv_dims[3], case.conv_dims[1]
    return {
        # e.g. one column: the three W taps meet the same pixel (zero pad: only the centre tap does; replicate: their sum)
        "no_flip_w": case.k[2] == 3 and _outer_taps_differ(W, case.pad[2], case.mode_hw, case.stride[2]),
        "no_flip_t": case.k[0] == 3 and _outer_taps_differ(T, case.pad[0], case.mode_t, case.stride[0]),
        "swap_fold_t": is3 and tf != tb and T > 1,       # (one frame under replicate: every padded frame folds into it)
        "swap_crop": is3 and case.mode_hw == ZERO and (hf != hb or wf != wb),
        "stuff_phase": is3 and strided,
        "drop_last_row": is3 and strided,
        "no_add": case.add or case.residual,
        "swap_unshuffle": case.path == UPCHAIN and case.up_time,
        "frame_at_end": case.path == UPCHAIN and case.up_time,
        "rep_as_zero_hw": is3 and case.mode_hw == REP,
    }[defect]


# =============================================================================================================== launch descriptors
def conv_desc(x: torch.Tensor, pw, pad, out_mode: int, cout_pad: Optional[int]):
    """the cvvae_conv_desc ops.conv builds for a stride-1 zero-mode launch of these paths (CPU-side kernel name resolution)"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    B, Ti, Hi, Wi, Cs = x.shape
    d = L.ConvDesc()
    d.dtype = ops._dt(x.dtype)
    d.B, d.Ti, d.Hi, d.Wi, d.Cin = B, Ti, Hi, Wi, pw.cin
    d.in_pix_stride = Cs
    d.kT, d.kH, d.kW = pw.k
    d.sT, d.sH, d.sW = 1, 1, 1
    d.pad_t, d.pad_h, d.pad_w = pad[0][0], pad[1][0], pad[2][0]
    d.pad_mode_t, d.pad_mode_hw = ZERO, ZERO
    d.prologue = L.PRO_NONE
    d.gn_rows_per_batch = 1
    d.To, d.Ho, d.Wo = (n + p[0] + p[1] - k + 1 for n, p, k in zip((Ti, Hi, Wi), pad, pw.k))
    d.Cout = pw.cout
    d.out_mode = out_mode
    d.out_pix_stride = 0 if out_mode == L.OUT_NCDHW else (pw.cout if cout_pad is None else cout_pad)
    d.alpha = 1.0
    d.four_wave = 1 if ops.four_wave() else 0
    return d
