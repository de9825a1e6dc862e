"""fp64 references, per-element bounds, input recipes and an fp32 emulation for the weight-gradient edge tests (plain torch on the
CPU; nothing here needs a GPU).  tests/wgrad_edge_cases.py holds the cases; tests/test_wgrad_edges_host.py checks this module,
tests/test_gpu_wgrad_edges.py uses it against the HIP kernels.

The bound of every output element has the conv tests' form

    |got - ref| <= a * S + b * |ref| + TINY

with ref in fp64 from the dtype-rounded operands and S the same sum over absolute values (the element's OWN summands).

  a = A_ACC = 2^-16                     an element that sums K <= K_ACC = 1728 products in fp32 (the project's figure)
  a = A_ACC * sqrt(K / K_ACC)           above that
  a += XP_BF16 = 3 * 2^-16              fp32 models (dW only): the split-precision product, see below
  b = 2^-24                             fp32 outputs; one rounding of the storage dtype for ops.pad_fold's output

The sqrt(K) factor.  A chain of K fp32 additions loses at most (K - 1) * 2^-24 * S and about sqrt(K) * 2^-24 * (a typical
partial sum) when the roundings are independent; A_ACC grants 256 roundings at K = 1728, about 6 sqrt(K), and the factor keeps
that ratio for longer sums.  The fp32 emulation below (panels of KP pixels as fp32 matmuls, panels added in order inside a slab,
slabs in index order) was held against the bound on every case (tests/test_wgrad_edges_host.py, -s prints the table): for 16-bit
operands its worst err / bound is 0.013 (K = 20) and falls to 0.0003 at K = 15400, so the factor is loose for the accumulation
and is kept as it stands -- nothing here is fitted to a kernel's output.

The split-precision term.  The forward convs' XP_ULP = 4e-6 belongs to their fp16 hi / lo split (11 significant bits each).
wgrad_kernel splits into bf16 (8 bits: gradients need fp32's range): x = hi + lo + d with |lo| <= 2^-8 |x| and
|d| <= 2^-8 |lo| <= 2^-16 |x|, and the product g a - (g_hi a_hi + g_hi a_lo + g_lo a_hi) = g_lo a_lo + d_g a + g d_a is at
most 3 * 2^-16 |g a| to first order -- the kernel's own header says "~2^-16 relative".  With XP_ULP the emulation of that
arithmetic reaches 0.90 of the bound on the six-pixel case reg32-w1 (a sum too short to average the products' errors), above
the 0.5 the host test allows it; with XP_BF16 = 3 * 2^-16, the format's own figure, it is 0.29.  The GPU test prints the ratio
under XP_ULP next to each fp32 line for the record.

tests/test_wgrad_edges_host.py holds the emulation to <= 0.5 of the bound on every element and shows that each seeded defect of
`DEFECTS` exceeds it.

ops.gn_bwd_params adds the element's own evaluation error to a * S: xh = fma(x, rstd, nmean) and the affine map round once
each, silu_grad_f is rcp(1 + __expf(-a)) (pass_ref.expf_rel, RCP), every product rounds once (U32)."""
import functools
import math
from typing import Dict, Optional, Tuple

import torch

import wgrad_edge_cases as WC
from conv_instance_cases import A_ACC, TINY
from pass_ref import DTYPE, RCP, ST, U32, Check, _bits, compare, expf_rel
from wgrad_edge_cases import BF16, F16, F32, REP, ZERO, Chan, Conv, Fold, round_up

K_ACC = 1728
XP_BF16 = 3 * 2.0 ** -16   # the bf16 hi / lo product of fp32 models: see the module docstring
DEFECTS = ("drop_tail", "panel_twice", "tap_shift", "clamp", "skip_slab", "swap_tail")


def a_of(K: int, dt: str, xp: Optional[float] = None) -> float:
    """the factor a of an element that sums K products; xp: the split-precision term of fp32 models (default XP_BF16)"""
    return A_ACC * max(1.0, math.sqrt(K / K_ACC)) + ((XP_BF16 if xp is None else xp) if dt == F32 else 0.0)


def _gen(case, dt: str) -> torch.Generator:
    return torch.Generator().manual_seed(case.seed * 3 + (F32, F16, BF16).index(dt))


def _rn(g, *shape, scale=1.0, off=0.0):
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale + off


def _stored(v: torch.Tensor, c: int, width: int, nan_gap: bool, dt: str) -> torch.Tensor:
    """real channels v [..., c] -> the stored tensor [..., width]: zeros up to round_up(c, 8), then zeros or NaN"""
    out = torch.zeros(*v.shape[:-1], width, dtype=torch.float64)
    out[..., :c] = v
    if nan_gap:
        out[..., round_up(c, 8):] = float("nan")
    return out.to(DTYPE[dt])


# =============================================================================================================== conv weight gradient
@functools.lru_cache(maxsize=2)
def conv_inputs(c: Conv, dt: str) -> Dict[str, torch.Tensor]:
    g = _gen(c, dt)
    B, Ti, Hi, Wi = c.dims
    To, Ho, Wo = c.out_grid
    return {"a": _stored(_rn(g, B, Ti, Hi, Wi, c.cin, off=0.25), c.cin, c.cs, c.nan_gap, dt),
            "gy": _stored(_rn(g, B, To, Ho, Wo, c.cout), c.cout, c.cg, c.nan_gap, dt)}


def _axis(n_out: int, stride: int, off: int, pad_front: int, L: int, mode: int):
    """the forward's coordinate map along one axis: (source index, taken?) per output coordinate -- replicate = clamp, zero = skip"""
    i = torch.arange(n_out) * stride + off - pad_front
    ok = (i >= 0) & (i < L)
    return i.clamp(0, L - 1), (ok if mode == ZERO else torch.ones_like(ok))


def tap_operand(c: Conv, a: torch.Tensor, tap: Tuple[int, int, int], mode_hw: Optional[int] = None, shift_x: int = 0) -> torch.Tensor:
    """a [B, Ti, Hi, Wi, cin] -> the operand of one tap at every output pixel, [B * To * Ho * Wo, cin]"""
    _, Ti, Hi, Wi = c.dims
    To, Ho, Wo = c.out_grid
    mhw = c.mode_hw if mode_hw is None else mode_hw
    it, mt = _axis(To, c.stride[0], tap[0], c.pad[0][0], Ti, c.mode_t)
    iy, my = _axis(Ho, c.stride[1], tap[1], c.pad[1][0], Hi, mhw)
    ix, mx = _axis(Wo, c.stride[2], tap[2] + shift_x, c.pad[2][0], Wi, mhw)
    v = a[:, it][:, :, iy][:, :, :, ix]
    m = mt[:, None, None] & my[None, :, None] & mx[None, None, :]
    return (v * m[None, :, :, :, None].to(v.dtype)).reshape(-1, a.shape[-1])


def _taps(c: Conv):
    return [(t, y, x) for t in range(c.k[0]) for y in range(c.k[1]) for x in range(c.k[2])]


@functools.lru_cache(maxsize=2)
def _conv_sums(c: Conv, dt: str):
    """(dW, S, db, Sb) in fp64: one matmul per tap over the coordinate-mapped operand, and the same over absolute values"""
    t = conv_inputs(c, dt)
    a = t["a"][..., :c.cin].double()
    g = t["gy"][..., :c.cout].double().reshape(-1, c.cout)
    gt, gat = g.t().contiguous(), g.abs().t().contiguous()
    dw = torch.empty(c.cout, c.cin, c.ntaps, dtype=torch.float64)
    S = torch.empty_like(dw)
    for i, tap in enumerate(_taps(c)):
        op = tap_operand(c, a, tap)
        dw[:, :, i] = gt @ op
        S[:, :, i] = gat @ op.abs()
    return dw, S, g.sum(0), g.abs().sum(0)


def conv_reference(c: Conv, dt: str, xp: Optional[float] = None) -> Dict[str, Check]:
    """dW [cout, cin, taps] and the bias gradient [cout] with their bounds; no autograd.  xp: see a_of (the bias gradient is a
    plain fp32 sum, or an MFMA against exact ones: no split-precision term)"""
    dw, S, db, Sb = _conv_sums(c, dt)
    return {"dw": Check(dw, a_of(c.pixels, dt, xp) * S + U32 * dw.abs() + TINY, U32),
            "db": Check(db, a_of(c.pixels, dt, 0.0) * Sb + U32 * db.abs() + TINY, U32)}


def conv_post(c: Conv, raw) -> Dict[str, torch.Tensor]:
    dw, db = raw
    return {"dw": dw.reshape(c.cout, c.cin, c.ntaps), "db": db}


def _worst(ref: Dict[str, Check], out: Dict[str, torch.Tensor]):
    best = (-1.0, "", 0)
    bad = 0
    for name, chk in ref.items():
        w, idx, n = compare(out[name], chk.ref, chk.bound)
        bad += n
        if w > best[0]:
            best = (w, f"{name}{idx}", 0)
    return best[0], best[1], bad


def conv_worst(c: Conv, dt: str, raw, xp: Optional[float] = None):
    """(worst err / bound over dW and the bias gradient, "dw(co, ci, tap)" or "db(co,)", elements beyond their bound)"""
    return _worst(conv_reference(c, dt, xp), conv_post(c, raw))


# ---- the launch plan, from the slab count
def slab_bounds(c: Conv, nslab: int):
    """(panels per row, [first panel of slab s for s = 0 .. nslab]) as both kernels cut them"""
    To, Ho, Wo = c.out_grid
    npr = (Wo + c.kp - 1) // c.kp
    ptotal = c.dims[0] * To * Ho * npr
    return npr, [ptotal * s // nslab for s in range(nslab + 1)]


def plan_facts(c: Conv, nslab: int) -> Dict[str, object]:
    To, Ho, _ = c.out_grid
    npr, beg = slab_bounds(c, nslab)
    n = [beg[s + 1] - beg[s] for s in range(nslab)]
    crossed = set()
    for s in range(nslab):
        if beg[s] % npr and n[s]:
            r0, r1 = beg[s] // npr, (beg[s + 1] - 1) // npr
            if r0 // Ho != r1 // Ho:
                crossed.add("frame")
            if r0 // (Ho * To) != r1 // (Ho * To):
                crossed.add("batch")
    return {"pmin": min(n), "pmax": max(n), "midrow": sum(1 for s in range(nslab) if beg[s] % npr), "crossed": crossed}


def fast_eligible(c: Conv) -> bool:
    """the launcher's static conditions for the scalar-base wave-loads (the 4 GB window is the allocator's)"""
    Wo = c.out_grid[2]
    n_co, n_ci = (round_up(c.cout, 8) + 127) // 128, (round_up(c.cin, 8) + 63) // 64
    return c.kernel == WC.DMA and Wo % 64 == 0 and c.cs >= n_ci * 64 and c.cg >= n_co * 128 and Wo * c.cg * 2 < 2 ** 31


def conv_desc(L, c: Conv, dt: str):
    """the descriptor ops.conv_wgrad builds"""
    d = L.ConvDesc()
    d.dtype = {F16: L.F16, BF16: L.BF16, F32: L.F32}[dt]
    d.B, d.Ti, d.Hi, d.Wi = c.dims
    d.Cin, d.in_pix_stride = round_up(c.cin, 8), c.cs
    d.kT, d.kH, d.kW = c.k
    d.sT, d.sH, d.sW = c.stride
    d.pad_t, d.pad_h, d.pad_w = c.pad[0][0], c.pad[1][0], c.pad[2][0]
    d.pad_mode_t, d.pad_mode_hw = c.mode_t, c.mode_hw
    d.To, d.Ho, d.Wo = c.out_grid
    d.Cout = round_up(c.cout, 8)
    return d


def lib_nslab(lib, d) -> int:
    """the slab count of the launch, out of cvvae_conv_wgrad_workspace_bytes: partial tiles (a multiple of 256 bytes) + the
    512-byte zero page + the per-slab bias sums"""
    n_co, n_ci, taps = (d.Cout + 127) // 128, (d.Cin + 63) // 64, d.kT * d.kH * d.kW
    tile = taps * n_co * 128 * n_ci * 64 * 4
    nb = int(lib.cvvae_conv_wgrad_workspace_bytes(d))
    assert nb > 0, nb
    for n in range(1, 4097):
        if (n * tile + 255) // 256 * 256 + 512 + (n * n_co * 128 * 4 + 255) // 256 * 256 == nb:
            return n
    raise AssertionError(f"workspace of {nb} bytes is not a whole number of slabs")


# ---- fp32 emulation of the kernels' arithmetic
def _panels(v: torch.Tensor, rows: int, Wo: int, npr: int, KP: int) -> torch.Tensor:
    """[rows * Wo, C] -> [rows * npr panels, KP, C], the ragged last panel of a row filled with zeros"""
    C = v.shape[-1]
    out = torch.zeros(rows, npr * KP, C, dtype=v.dtype)
    out[:, :Wo] = v.reshape(rows, Wo, C)
    return out.reshape(rows * npr, KP, C)


def _split(v: torch.Tensor):
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def conv_emulate(c: Conv, dt: str, nslab: int, defect: Optional[str] = None):
    """dtype-rounded operands, one fp32 matmul per K panel and tap (fp32 models: the three bf16 hi / lo products), the panels of a
    slab added in order, the slabs added in index order.  defect: one seeded error of DEFECTS (the checker's self-test)."""
    assert defect is None or defect in DEFECTS
    t = conv_inputs(c, dt)
    To, Ho, Wo = c.out_grid
    rows, KP = c.dims[0] * To * Ho, c.kp
    npr, beg = slab_bounds(c, nslab)
    a = t["a"][..., :c.cin].float()
    g = t["gy"][..., :c.cout].float().reshape(-1, c.cout)
    gp = _panels(g, rows, Wo, npr, KP)
    if defect == "drop_tail":
        assert Wo % KP, "the case has no ragged panel"
        gp = gp.clone()
        gp[npr - 1, (Wo - 1) % KP] = 0.0
    gpt = gp.transpose(1, 2).contiguous()
    gparts = _split(gpt) if dt == F32 else (gpt,)
    twice = beg[nslab // 2] if defect == "panel_twice" else -1
    skip = nslab - 1 if defect == "skip_slab" else -1
    if defect == "skip_slab":
        assert nslab > 1

    def reduce(part):  # [panels, ...] -> the slabs' sums in panel order, then the slabs in index order
        total = torch.zeros_like(part[0])
        for s in range(nslab):
            if s == skip:
                continue
            acc = torch.zeros_like(part[0])
            for p in range(beg[s], beg[s + 1]):
                acc = acc + part[p]
                if p == twice:
                    acc = acc + part[p]
            total = total + acc
        return total

    taps = _taps(c)
    dw = torch.empty(c.cout, c.cin, c.ntaps)
    for i, tap in enumerate(taps):
        kw = {}
        if defect == "tap_shift" and i == 0:   # the first tap reads the column to its right
            kw["shift_x"] = 1
        if defect == "clamp":
            assert c.mode_hw == ZERO and c.pad[2][0], "clamping is a defect under zero padding only"
            kw["mode_hw"] = REP
        xp = _panels(tap_operand(c, a, tap, **kw), rows, Wo, npr, KP)
        if dt == F32:
            xh, xl = _split(xp)
            part = torch.bmm(gparts[0], xh) + torch.bmm(gparts[0], xl) + torch.bmm(gparts[1], xh)
        else:
            part = torch.bmm(gparts[0], xp)
        dw[:, :, i] = reduce(part)
    if defect == "swap_tail":  # the last two channels of the last input-channel block change places
        assert c.cin >= 2
        dw[:, [c.cin - 2, c.cin - 1]] = dw[:, [c.cin - 1, c.cin - 2]]
    db = reduce(gp.sum(1))
    return dw.reshape(c.cout, c.cin, *c.k), db


# =============================================================================================================== per-channel sums
@functools.lru_cache(maxsize=2)
def chan_inputs(c: Chan, dt: str) -> Dict[str, torch.Tensor]:
    g = _gen(c, dt)
    if c.op == "bias":
        return {"gy": _stored(_rn(g, 1, 1, 1, c.rows * c.S, c.C), c.C, c.ps, True, dt)}
    shape = (c.rows, 1, 1, c.S, c.C)
    return {"x": _rn(g, *shape, scale=1.5, off=0.5).to(DTYPE[dt]), "gy": _rn(g, *shape).to(DTYPE[dt]),
            "rs": (0.5 + 1.5 * torch.rand(c.rows, c.C, generator=g, dtype=torch.float64)).float(),
            "nm": _rn(g, c.rows, c.C, scale=0.5).float(),
            "gamma": _rn(g, c.C, scale=0.3, off=1.0).float(), "beta": _rn(g, c.C, scale=0.3).float()}


@functools.lru_cache(maxsize=2)
def chan_reference(c: Chan, dt: str) -> Dict[str, Check]:
    t = chan_inputs(c, dt)
    al = a_of(c.rows * c.S, dt, xp=0.0)   # (plain fp32 sums: no split products)
    if c.op == "bias":
        g = t["gy"][..., :c.C].double().reshape(-1, c.C)
        db = g.sum(0)
        return {"db": Check(db, al * g.abs().sum(0) + U32 * db.abs() + TINY, U32)}
    x, gy = t["x"].double().reshape(c.rows, c.S, c.C), t["gy"].double().reshape(c.rows, c.S, c.C)
    rs, nm = t["rs"].double()[:, None], t["nm"].double()[:, None]
    ga, be = t["gamma"].double(), t["beta"].double()
    xh = x * rs + nm
    a = xh * ga + be
    exh = U32 * xh.abs()                                          # one fma
    da = exh * ga.abs() + U32 * a.abs()
    if c.silu:
        sg = torch.sigmoid(a)
        d = sg * (1 + a * (1 - sg))
        ed = (expf_rel(a) + RCP + 4 * U32) * sg * (1 + a.abs()) + 0.5 * da   # as pass_ref._gn_bwd_reference: |silu''| <= 0.5
    else:
        d, ed = torch.ones_like(a), torch.zeros_like(a)
    gact = gy * d
    egact = gy.abs() * ed + U32 * gact.abs()
    dg, db = (gact * xh).sum((0, 1)), gact.sum((0, 1))
    b_dg = (egact * xh.abs() + gact.abs() * exh + U32 * (gact * xh).abs()).sum((0, 1)) + al * (gact * xh).abs().sum((0, 1)) + U32 * dg.abs() + TINY
    b_db = egact.sum((0, 1)) + al * gact.abs().sum((0, 1)) + U32 * db.abs() + TINY
    return {"dgamma": Check(dg, b_dg, U32), "dbeta": Check(db, b_db, U32)}


def chan_post(c: Chan, raw) -> Dict[str, torch.Tensor]:
    return {"db": raw[0]} if c.op == "bias" else {"dgamma": raw[0], "dbeta": raw[1]}


def chan_call(ops, c: Chan, t):
    """the op under test (cvvae_amd.ops or tests/emu_ops) on tensors t"""
    if c.op == "bias":
        return (ops.bias_grad(t["gy"], cout=c.C),)
    return ops.gn_bwd_params(t["x"], t["gy"], (t["rs"], t["nm"]), t["gamma"], t["beta"], bool(c.silu))


def chan_worst(c: Chan, dt: str, raw):
    return _worst(chan_reference(c, dt), chan_post(c, raw))


# =============================================================================================================== padding adjoint
@functools.lru_cache(maxsize=2)
def fold_inputs(c: Fold, dt: str) -> Dict[str, torch.Tensor]:
    g = _gen(c, dt)
    B, T, H, W = c.dims
    t = {"gp": _rn(g, B, T + sum(c.pad_t), H + 2, W + 2, c.C).to(DTYPE[dt])}
    if c.add:
        t["add"] = _rn(g, B, T, H, W, c.C).to(DTYPE[dt])
    return t


def _fold_axis(v: torch.Tensor, dim: int, L: int, pf: int, mode: int) -> torch.Tensor:
    """the adjoint of padding one axis: replicate -- the first / last element collects the front / back pad; zero -- the interior"""
    inner = v.narrow(dim, pf, L).clone()
    pb = v.shape[dim] - pf - L
    if mode == REP and pf:
        inner.select(dim, 0).add_(v.narrow(dim, 0, pf).sum(dim))
    if mode == REP and pb:
        inner.select(dim, L - 1).add_(v.narrow(dim, pf + L, pb).sum(dim))
    return inner


def _fold(c: Fold, v: torch.Tensor) -> torch.Tensor:
    _, T, H, W = c.dims
    v = _fold_axis(v, 1, T, c.pad_t[0], c.mode_t)
    v = _fold_axis(v, 2, H, 1, c.mode_hw)
    return _fold_axis(v, 3, W, 1, c.mode_hw)


@functools.lru_cache(maxsize=2)
def fold_reference(c: Fold, dt: str) -> Dict[str, Check]:
    t = fold_inputs(c, dt)
    gp = t["gp"].double()
    ref, S = _fold(c, gp), _fold(c, gp.abs())
    if c.add:
        ref, S = ref + t["add"].double(), S + t["add"].double().abs()
    return {"out": Check(ref, A_ACC * S + ST[dt] * ref.abs() + TINY, ST[dt])}


def fold_call(ops, c: Fold, t):
    return (ops.pad_fold(t["gp"], c.pad_t, 1, c.mode_t, c.mode_hw, add=t.get("add")),)


def fold_worst(c: Fold, dt: str, raw):
    return _worst(fold_reference(c, dt), {"out": raw[0]})
