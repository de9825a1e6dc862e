"""fp64 references, per-element bounds and input recipes of the LPIPS / discriminator pass edge tests (plain torch on the CPU; nothing
here needs a GPU).  tests/lossnet_edge_cases.py holds the cases; tests/test_lossnet_edges_host.py checks this module,
tests/test_gpu_lossnet_edges.py uses it against the HIP kernels of cvvae_amd/csrc/lpips_kernels.hip and disc_kernels.hip.

For a case and a dtype:
  inputs(case, dt)      -> the CPU operands, rounded to the storage dtype the kernel receives (a dict of tensors)
  reference(case, dt)   -> {output name: Check(ref, bound)}: ref in fp64 from those rounded operands; bound the per-element allowance,
                           or None where the output must match bit for bit (selections, exact scalings, untouched memory)
  emulate(case, dt)     -> {output name: tensor}: a plain fp32 torch evaluation BEFORE the store rounding (`round_emu` rounds it)
  torch_pairs(case, dt) -> [(name, this module's fp64 value, torch's own fp64 op / autograd)]
The statistics forms take the tensor the pass STORED: stats_reference(case, y) -> the checks on the (mean, rstd) tables.

Bounds have the form a * S + b * |ref| + TINY of tests/pass_ref.py (U32, RCP, ST, acc and STATS_TOL are those from there),
with S built from the element's own summands in absolute value.  The 3-D pool and the small-Cin input gradient keep the bounds their
first tests derived (tests/test_gpu_disc_ops.py, tests/test_gpu_disc_dgrad.py): n fp32 roundings of the summands plus half an ulp of
the storage dtype at the result.  Exact comparisons treat +0 and -0 as equal (the kernels write +0 where torch may write -0) and any
NaN as equal to any NaN; a non-finite reference element of a bounded output must be met exactly."""
import functools
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

import lpips_ref
from pass_edge_cases import BF16, F16, F32, Case
from pass_ref import DTYPE, GN_EPS, RCP, ST, TINY, U32, Check, _gen, _moments, _rn, _table_checks, acc, compare

FMT = {F16: (11, -14), BF16: (8, -126), F32: (24, -126)}   # significant bits, smallest normal exponent
LPIPS_EPS = 1e-10


def half_ulp(mag: torch.Tensor, dt: str) -> torch.Tensor:
    """half a unit in the last place of `dt` at magnitude `mag` (fp64): what one round-to-nearest store may lose"""
    p, emin = FMT[dt]
    e = torch.floor(torch.log2(mag.clamp_min(1e-300))).clamp_min(emin)
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - (p - 1))


def canon(t: torch.Tensor) -> torch.Tensor:
    """-0 -> +0, every NaN -> the one NaN torch writes: what an exact comparison must not tell apart"""
    t = t + torch.zeros((), dtype=t.dtype)
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)


def check_one(got: torch.Tensor, chk: Check, before_store: bool = False):
    """pass_ref.compare with this module's notion of exact: (worst err / bound, index, violations)"""
    if chk.bound is None:
        if chk.ref.dtype in (torch.float16, torch.bfloat16):   # (an emulation's fp32 value: the store rounding first)
            got = got.to(chk.ref.dtype)
        return compare(canon(got), canon(chk.ref.to(got.dtype)), None)
    bound = chk.before_store() if before_store else chk.bound
    odd = ~torch.isfinite(chk.ref)
    if not bool(odd.any()):
        return compare(got, chk.ref, bound)
    # the non-finite reference elements exactly, the others under their bound
    g, r = got.double(), chk.ref
    same = (torch.isnan(g) & torch.isnan(r)) | (g == r)
    ratio = torch.where(odd, torch.where(same, 0.0, float("inf")).double(), (g - r).abs() / bound)
    ratio = torch.where(torch.isfinite(g) | odd, ratio, torch.full_like(ratio, float("inf")))
    worst = ratio.max().item()
    return worst, tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0]), int((ratio > 1.0).sum())


def _slope32(c: Case) -> float:
    return float(torch.tensor(c["slope"], dtype=torch.float32))


# =============================================================================================================== lpips_scale_in
CANARY = 7.0


def _consts():
    return torch.tensor(lpips_ref.SHIFT, dtype=torch.float32), torch.tensor(lpips_ref.SCALE, dtype=torch.float32)


def _scale_in_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    shift, scale = _consts()
    return {"x": (_rn(g, c["N"], 3, c["H"], c["W"], scale=0.5).clamp(-1, 1)).to(DTYPE[c["src"]]), "shift": shift, "scale": scale}


def _scale_in_reference(c: Case, dt: str, t):
    x, sh, sc = t["x"].double(), t["shift"].double().view(1, 3, 1, 1), t["scale"].double().view(1, 3, 1, 1)
    y = ((x - sh) / sc).permute(0, 2, 3, 1)
    S_ = ((x.abs() + sh.abs()) / sc.abs()).permute(0, 2, 3, 1)        # the difference's summands, through the division
    out = {"y": Check(y, 3 * U32 * S_ + ST[dt] * y.abs() + TINY, ST[dt]),
           "pad": Check(torch.zeros(c["N"], c["H"], c["W"], c["cpad"] - 3), None)}
    if c["sliced"]:
        out["canary"] = Check(torch.full((c["N"] * c["H"] * c["W"] * c["cpad"] + 64,), CANARY), None)
    return out


def _scale_in_emulate(c: Case, dt: str, t):
    y = ((t["x"].float() - t["shift"].view(1, 3, 1, 1)) / t["scale"].view(1, 3, 1, 1)).permute(0, 2, 3, 1)
    out = {"y": y, "pad": torch.zeros(c["N"], c["H"], c["W"], c["cpad"] - 3)}
    if c["sliced"]:
        out["canary"] = torch.full((c["N"] * c["H"] * c["W"] * c["cpad"] + 64,), CANARY)
    return out


def _scale_in_pairs(c: Case, dt: str, t):
    """lpips.py's ScalingLayer on NCHW in fp64, then the layout change"""
    x = t["x"].double()
    theirs = (x - t["shift"].double()[None, :, None, None]) / t["scale"].double()[None, :, None, None]
    return [("y", _scale_in_reference(c, dt, t)["y"].ref, theirs.permute(0, 2, 3, 1))]


def _scale_in_bwd_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    gt = torch.full((c["N"], c["H"], c["W"], c["ps"]), float("nan"), dtype=torch.float64)
    gt[..., :3] = _rn(g, c["N"], c["H"], c["W"], 3)
    return {"g": gt.to(DTYPE[c["g"]]), "scale": _consts()[1]}


def _scale_in_bwd_reference(c: Case, dt: str, t):
    gx = (t["g"][..., :3].double() / t["scale"].double()).permute(0, 3, 1, 2)
    return {"gx": Check(gx, (2 * U32 + ST[dt]) * gx.abs() + TINY, ST[dt])}


def _scale_in_bwd_emulate(c: Case, dt: str, t):
    return {"gx": (t["g"][..., :3].float() / t["scale"]).permute(0, 3, 1, 2)}


def _scale_in_bwd_pairs(c: Case, dt: str, t):
    x = torch.zeros(c["N"], 3, c["H"], c["W"], dtype=torch.float64, requires_grad=True)
    shift, scale = _consts()
    with torch.enable_grad():
        y = ((x - shift.double()[None, :, None, None]) / scale.double()[None, :, None, None]).permute(0, 2, 3, 1)
        (y * t["g"][..., :3].double()).sum().backward()
    return [("gx", _scale_in_bwd_reference(c, dt, t)["gx"].ref, x.grad)]


# =============================================================================================================== relu_, maxpool2x2
def _relu_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    x = _rn(g, c["v"] * 8).to(DTYPE[dt])
    fi = torch.finfo(DTYPE[dt])
    if c.recipe == "special":
        x = torch.tensor([float("inf"), float("-inf"), -0.0, fi.tiny / 4, -fi.tiny / 4, fi.max, -fi.max, 1.0], dtype=torch.float64).to(DTYPE[dt])
    if c.recipe == "nan":
        x[0] = x[9] = x[23] = float("nan")
    return {"x": x}


def _relu_reference(c: Case, dt: str, t):
    return {"y": Check(torch.relu(t["x"].float()).to(DTYPE[dt]), None)}


def _relu_emulate(c: Case, dt: str, t):
    x = t["x"].float()
    return {"y": torch.where(x <= 0, torch.zeros_like(x), x)}


def _relu_pairs(c: Case, dt: str, t):
    return [("y", canon(_relu_emulate(c, dt, t)["y"].double()), canon(torch.relu(t["x"].double())))]


def _tie_grid(g, shape):
    """values on a coarse grid: most 2x2 windows hold equal maxima (and many zeros, as a ReLU output does)"""
    return torch.relu(torch.round(_rn(g, *shape) * 2) / 2)


def _window(H, W, wy, wx, pos):
    return 2 * wy + (pos >> 1), 2 * wx + (pos & 1)


def _maxpool_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    shape = (c["N"], c["H"], c["W"], c["C"])
    x = _rn(g, *shape)
    if c.recipe == "neg":
        x = -x.abs() - 0.1
    elif c.recipe == "tie":
        x = _tie_grid(g, shape)
    elif c.recipe in ("inf", "nan"):
        pos = c["pos"]
        y0, x0 = _window(c["H"], c["W"], 0, 0, pos)
        y1, x1 = _window(c["H"], c["W"], 1, 1, pos)
        y2, x2 = _window(c["H"], c["W"], 1, 0, (pos + 1) % 4)
        if c.recipe == "inf":
            x[0, y0, x0, :] = float("inf")
            x[0, y1, x1, :] = float("-inf")
            x[0, 2:4, 0:2, :] = float("-inf")          # a window of -inf only
        else:
            x[0, y0, x0, :4] = float("nan")            # four channels of the vector, the others finite
            x[0, y1, x1, :] = float("nan")
            x[0, y2, x2, :] = float("nan")             # two NaNs in one window
            x[0, y2, x2 ^ 1, :] = float("nan")
    return {"x": x.to(DTYPE[dt])}


def _maxpool_reference(c: Case, dt: str, t):
    return {"y": Check(F.max_pool2d(t["x"].float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).to(DTYPE[dt]), None)}


def _max4(x):
    """the maximum of the four window positions in scan order, a NaN winning: the kernel's formula"""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    m = x[:, 0:2 * Ho:2, 0:2 * Wo:2]
    for d in (1, 2, 3):
        f = x[:, (d >> 1):2 * Ho:2, (d & 1):2 * Wo:2]
        m = torch.where((f > m) | torch.isnan(f), f, m)
    return m


def _maxpool_emulate(c: Case, dt: str, t):
    return {"y": _max4(t["x"].float())}


def _maxpool_pairs(c: Case, dt: str, t):
    x = t["x"].double()
    return [("y", canon(_max4(x)), canon(F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)))]


# =============================================================================================================== relu_pool_bwd
def _relu_pool_bwd_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    shape = (c["N"], c["H"], c["W"], c["C"])
    if c.recipe == "tie":
        y = _tie_grid(g, shape)
    elif c.recipe == "zero":
        y = torch.zeros(shape, dtype=torch.float64)
    elif c.recipe == "negy":
        y = _rn(g, *shape)
    else:
        y = torch.relu(_rn(g, *shape))
    t = {"y": y.to(DTYPE[dt])}
    if c["mode"] in ("both", "tap"):
        t["g_tap"] = _rn(g, *shape).to(DTYPE[dt])
    if c["mode"] in ("both", "pool"):
        t["g_pool"] = _rn(g, c["N"], c["H"] // 2, c["W"] // 2, c["C"]).to(DTYPE[dt])
    return t


def _relu_pool_bwd_reference(c: Case, dt: str, t):
    """(g_tap + max_pool2d's backward of g_pool on the SAME stored values) * (y > 0): fp32 sum, one rounding (ATen routes ties to the
    first maximum in scan order)"""
    y = t["y"]
    g = torch.zeros(y.shape, dtype=torch.float32) if "g_tap" not in t else t["g_tap"].float()
    if "g_pool" in t:
        v = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
        with torch.enable_grad():
            F.max_pool2d(v, 2, 2).backward(t["g_pool"].permute(0, 3, 1, 2).contiguous())
        g = g + v.grad.float().permute(0, 2, 3, 1)
    return {"gx": Check((g * (y.float() > 0)).to(y.dtype), None)}


def route(y, g_tap, g_pool):
    """the kernel's formula in the operands' dtype: the first maximum in scan order by a strict >, recomputed from y; mask y > 0"""
    N, H, W, C = y.shape
    Ho, Wo = H // 2, W // 2
    g = torch.zeros_like(y) if g_tap is None else g_tap.clone()
    if g_pool is not None:
        win = [y[:, (d >> 1):2 * Ho:2, (d & 1):2 * Wo:2] for d in range(4)]
        m, best = win[0], torch.zeros_like(win[0], dtype=torch.long)
        for d in (1, 2, 3):
            up = win[d] > m
            m, best = torch.where(up, win[d], m), torch.where(up, torch.full_like(best, d), best)
        for d in range(4):
            g[:, (d >> 1):2 * Ho:2, (d & 1):2 * Wo:2] += torch.where(best == d, g_pool, torch.zeros_like(g_pool))
    return torch.where(y > 0, g, torch.zeros_like(g))


def _relu_pool_bwd_emulate(c: Case, dt: str, t):
    return {"gx": route(t["y"].float(), t["g_tap"].float() if "g_tap" in t else None, t["g_pool"].float() if "g_pool" in t else None)}


def _relu_pool_bwd_pairs(c: Case, dt: str, t):
    """fp64 autograd of the tap and of max_pool2d on relu(x), at an x whose ReLU output is y (x = y where y > 0, -1 elsewhere)"""
    if c.recipe == "negy":   # y is no ReLU output: the ATen reference on the stored values is all there is
        return []
    y = t["y"].double()
    gt, gp = (t[k].double() if k in t else None for k in ("g_tap", "g_pool"))
    x = torch.where(y > 0, y, -torch.ones_like(y)).permute(0, 3, 1, 2).clone().requires_grad_(True)
    with torch.enable_grad():
        r = torch.relu(x)
        loss = r.sum() * 0.0
        if gt is not None:
            loss = loss + (r * gt.permute(0, 3, 1, 2)).sum()
        if gp is not None:
            loss = loss + (F.max_pool2d(r, 2, 2) * gp.permute(0, 3, 1, 2)).sum()
        loss.backward()
    return [("gx", route(y, gt, gp), x.grad.permute(0, 2, 3, 1))]


# =============================================================================================================== lpips_head(_bwd)
def _head_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    N, HW, C = c["N"], c["HW"], c["C"]
    f0, f1 = torch.relu(_rn(g, N, HW, C, off=1.5)), torch.relu(_rn(g, N, HW, C, off=1.7))   # ReLU'd normals, about 6 % zeros
    gs = max(1.0, HW / 16.0)      # the gradients carry 1 / HW: the cotangent grows with HW so that they stay above TINY
    if c.recipe == "zero0":
        f0[0, 0] = 0
        f0[N - 1, HW - 1] = 0
    elif c.recipe == "zero01":
        f0[0, 0] = f1[0, 0] = 0
        f0[N - 1, HW - 1] = f1[N - 1, HW - 1] = 0
    elif c.recipe == "tiny":      # |f| about 1e-7: the sum of squares is below the 1e-10 epsilon
        f0, f1 = f0 * 1e-7, f1 * 1e-7
    elif c.recipe == "same":
        f1 = f0.clone()
    elif c.recipe == "big":       # fp16 features up to 6e4; the cotangent is scaled so that the gradients stay above TINY
        f0, f1, gs = f0 * (6.0e4 / f0.max()), f1 * (6.0e4 / f1.max()), 1.0e4
    w = _rn(g, C).abs().float()
    gout = (0.5 + _rn(g, N).abs()) * gs
    if N >= 3:
        gout[1] = -gout[1]
    if N >= 64:
        gout[5] = 0.0
    out0 = 0.25 + 0.1 * torch.arange(N, dtype=torch.float32)
    return {"f0": f0.to(DTYPE[dt]), "f1": f1.to(DTYPE[dt]), "w": w, "gout": gout.float(), "out0": out0}


def _head_math(f0, f1, w, gout, HW):
    """value [N] and both gradients from the kernel's own formulas (lpips_kernels.hip, lpips_head_bwd_kernel's header) in the
    dtype of the operands -> (value, g0, g1, the intermediates the bounds need)"""
    s0, s1 = (f0 * f0).sum(-1, keepdim=True), (f1 * f1).sum(-1, keepdim=True)
    r0, r1 = torch.sqrt(s0 + LPIPS_EPS), torch.sqrt(s1 + LPIPS_EPS)
    i0, i1 = 1.0 / (r0 + LPIPS_EPS), 1.0 / (r1 + LPIPS_EPS)
    e = f0 * i0 - f1 * i1
    we = w * e
    val = (we * e).sum((-1, -2)) / HW
    d0, d1 = (we * f0).sum(-1, keepdim=True), (we * f1).sum(-1, keepdim=True)
    q0, q1 = d0 * i0 * i0 / r0, d1 * i1 * i1 / r1
    k = (2.0 * gout / HW).view(-1, 1, 1)
    g0, g1 = k * (we * i0 - q0 * f0), k * (q1 * f1 - we * i1)
    return val, g0, g1, (i0, i1, r0, r1, e, we, d0, d1, q0, q1, k)


def _head_reference(c: Case, dt: str, t):
    N, HW, C = c["N"], c["HW"], c["C"]
    f0, f1, w, gout = t["f0"].double(), t["f1"].double(), t["w"].double(), t["gout"].double()
    val, g0, g1, (i0, i1, r0, r1, e, we, d0, d1, q0, q1, k) = _head_math(f0, f1, w, gout, HW)
    out0 = t["out0"].double()
    if c.recipe == "same":  # e is 0 - 0: the value adds exactly 0 and both gradients are exactly 0
        z = torch.zeros(N, HW, C)
        return {"out": Check(out0, None), "g0": Check(z, None), "g1": Check(z, None)}
    # 1 / (sqrt(s + eps) + eps): the sum of squares in free order (half of its relative error goes through the root), one rounding
    # each of the two additions, the root and the reciprocal
    ri = 0.5 * (acc(C) + U32) + RCP + 3 * U32
    de = (f0.abs() * i0 + f1.abs() * i1) * (ri + 2 * U32)            # e = f0 i0 - f1 i1
    dwe = w.abs() * de + U32 * we.abs()
    # --- the value, per sample: fp32 accumulation over C, then over HW, in free order
    terms = (we * e).abs()
    dterm = 2 * we.abs() * de + 3 * U32 * terms
    b_val = (dterm.sum((-1, -2)) + (acc(C) + acc(HW)) * terms.sum((-1, -2))) / HW + 2 * U32 * val.abs()
    out = out0 + val
    b_out = b_val + U32 * out.abs() + TINY                               # out += level
    # --- the gradients, per element
    checks = {"out": Check(out, b_out, U32)}
    for name, gg, f, i_, r_, d_, q_ in (("g0", g0, f0, i0, r0, d0, q0), ("g1", g1, f1, i1, r1, d1, q1)):
        dd = (dwe * f.abs()).sum(-1, keepdim=True) + acc(C) * (we * f).abs().sum(-1, keepdim=True)
        dq = (dd + d_.abs() * (3 * ri + 4 * U32)) * i_ * i_ / r_
        S_ = we.abs() * i_ + q_.abs() * f.abs()
        err = k.abs() * (dwe * i_ + we.abs() * i_ * ri + dq * f.abs() + 3 * U32 * S_)
        checks[name] = Check(gg, err + ST[dt] * gg.abs() + TINY, ST[dt])
    return checks


def _head_emulate(c: Case, dt: str, t):
    val, g0, g1, _ = _head_math(t["f0"].float(), t["f1"].float(), t["w"], t["gout"], c["HW"])
    return {"out": t["out0"] + val, "g0": g0, "g1": g1}


def _head_pairs(c: Case, dt: str, t):
    """the head of tests/lpips_ref.py (normalize_tensor on NCHW, squared difference, lin, spatial mean) and its autograd"""
    a = t["f0"].double().clone().requires_grad_(True)
    b = t["f1"].double().clone().requires_grad_(True)
    w, gout = t["w"].double(), t["gout"].double()
    with torch.enable_grad():
        n0, n1 = lpips_ref.normalize_tensor(a.permute(0, 2, 1)), lpips_ref.normalize_tensor(b.permute(0, 2, 1))   # [N, C, HW]
        val = (((n0 - n1) ** 2) * w[None, :, None]).sum(1).mean(1)
        (val * gout).sum().backward()
    mine = _head_math(t["f0"].double(), t["f1"].double(), w, gout, c["HW"])
    return [("value", mine[0], val.detach()), ("g0", mine[1], a.grad), ("g1", mine[2], b.grad)]


# =============================================================================================================== avgpool3d_down(_bwd)
def _pool_frames(T: int):
    """stored frame of every padded frame: an odd T has frame 0 in front of itself"""
    return list(range(T)) if T % 2 == 0 else [0] + list(range(T))


def pool3d_fwd(x):
    """[B,T,H,W,C] -> the downsample: the padded frames by index, odd rows / columns dropped, means of 2x2x2"""
    B, T, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    xp = x[:, _pool_frames(T), :2 * Ho, :2 * Wo]
    return xp.reshape(B, xp.shape[1] // 2, 2, Ho, 2, Wo, 2, C).mean((2, 4, 6))


def pool3d_bwd(gy, shape):
    """the adjoint as the kernel's gather: 0.125 gy; 0.25 gy for frame 0 of an odd T; 0 for the dropped row / column"""
    B, T, H, W, C = shape
    Ho, Wo = H // 2, W // 2
    odd = T & 1
    gx = torch.zeros(shape, dtype=gy.dtype)
    up = gy.repeat_interleave(2, 2).repeat_interleave(2, 3)
    for tt in range(T):
        gx[:, tt, :2 * Ho, :2 * Wo] = up[:, (tt + odd) >> 1] * (0.25 if (odd and tt == 0) else 0.125)
    return gx


def _away_from_zero(v):
    """|v| >= 2^-6, signs kept: an eighth of it is a normal number in every dtype"""
    return torch.where(v >= 0, v.clamp_min(2.0 ** -6), v.clamp_max(-2.0 ** -6))


def _pool3d_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    shape = (c["B"], c["T"], c["H"], c["W"], c["C"])
    x = _rn(g, *shape)
    if c.recipe == "nan":
        x[0, 1, 0, 0, :] = float("nan")
    gy = _away_from_zero(_rn(g, shape[0], (shape[1] + 1) // 2, shape[2] // 2, shape[3] // 2, shape[4]))
    return {"x": x.to(DTYPE[dt]), "gy": _away_from_zero(gy.to(DTYPE[dt]).double()).to(DTYPE[dt])}


def _pool3d_reference(c: Case, dt: str, t):
    x = t["x"].double()
    y, mean_abs = pool3d_fwd(x), pool3d_fwd(torch.nan_to_num(x.abs(), nan=0.0))
    arith = 8 * U32 * mean_abs + 1e-300
    store = torch.zeros_like(arith) if dt == F32 else half_ulp(torch.nan_to_num(y.abs()) + arith, dt)
    gx = pool3d_bwd(t["gy"].double(), tuple(t["x"].shape)).to(DTYPE[dt])   # exact scalings: the fp64 gradient rounded once
    return {"y": Check(y, arith + store, 0.0, store), "gx": Check(gx, None)}


def _pool3d_emulate(c: Case, dt: str, t):
    return {"y": pool3d_fwd(t["x"].float()), "gx": pool3d_bwd(t["gy"].float(), tuple(t["x"].shape))}


def _ncdhw(v):
    return v.permute(0, 4, 1, 2, 3)


def _pool3d_pairs(c: Case, dt: str, t):
    """models/discriminator.py: if T is odd, h = cat([h[:, :, :1], h], 2); h = avg_pool3d(h, 2, 2) -- and its autograd"""
    if c.recipe == "nan":
        return []
    x = _ncdhw(t["x"].double()).clone().requires_grad_(True)
    with torch.enable_grad():
        h = torch.cat([x[:, :, :1], x], 2) if x.shape[2] % 2 else x
        y = F.avg_pool3d(h, 2, 2)
        (y * _ncdhw(t["gy"].double())).sum().backward()
    return [("y", pool3d_fwd(t["x"].double()), y.detach().permute(0, 2, 3, 4, 1)),
            ("gx", pool3d_bwd(t["gy"].double(), tuple(t["x"].shape)), x.grad.permute(0, 2, 3, 4, 1))]


# =============================================================================================================== gn_leaky_apply, leaky_bwd
def _leaky_x(c: Case, dt: str, g, rows, per, C):
    x = _rn(g, rows, per, C)
    x[:, ::2, 3] = 0.0                 # with shift[:, 3] = 0: exact zeros in the pre-activation
    if c.recipe == "inf":
        x[0, 0, 0], x[0, 0, 1], x[rows - 1, per - 1, C - 1] = float("inf"), float("-inf"), float("-inf")
    if c.recipe == "nan":
        x[0, 0, 0] = x[rows - 1, per - 1, C - 1] = float("nan")
    return x.to(DTYPE[dt])


def _tables(g, rows, C):
    scale, shift = _rn(g, rows, C, scale=0.3, off=1.0).float(), _rn(g, rows, C, scale=0.5).float()
    shift[:, 3] = 0.0
    return scale, shift


def _leaky_apply_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    rows, per, C = c["rows"], c["per_row"], c["C"]
    t = {"x": _leaky_x(c, dt, g, rows, per, C)}
    if c["affine"]:
        t["scale"], t["shift"] = _tables(g, rows, C)
    return t


def _leaky_apply_reference(c: Case, dt: str, t):
    slope = _slope32(c) if "slope" in dict(c.p) else SLOPE32
    if not c["affine"]:   # one multiply rounded once: the fp32 product, then the store
        x = t["x"].float()
        return {"y": Check(torch.where(x > 0, x, slope * x).to(DTYPE[dt]), None)}
    x, sc, sh = t["x"].double(), t["scale"].double()[:, None], t["shift"].double()[:, None]
    v = x * sc + sh
    y = torch.where(v > 0, v, slope * v)
    S_ = torch.nan_to_num((x * sc).abs() + sh.abs(), posinf=0.0)
    return {"y": Check(y, 2 * U32 * S_ + (U32 + ST[dt]) * torch.nan_to_num(y.abs(), posinf=0.0) + TINY, ST[dt])}   # one fma, one multiply


def _leaky_apply_emulate(c: Case, dt: str, t):
    """ONE fused multiply-add, as the kernel's (the product and sum in fp64, rounded once to fp32), then the fp32 LeakyReLU"""
    slope = _slope32(c) if "slope" in dict(c.p) else SLOPE32
    v = t["x"].float()
    if c["affine"]:
        v = (t["x"].double() * t["scale"].double()[:, None] + t["shift"].double()[:, None]).float()
    return {"y": torch.where(v > 0, v, slope * v)}


def _leaky_apply_pairs(c: Case, dt: str, t):
    """F.leaky_relu, and for the affine form F.leaky_relu(F.group_norm(x)) with the tables' own statistics: scale = gamma rstd,
    shift = beta - mean scale"""
    s = _slope32(c)
    ref = _leaky_apply_reference(c, dt, t)["y"].ref
    if not c["affine"]:   # the reference is the fp32 evaluation itself
        return [("y", ref.double(), F.leaky_relu(t["x"].float(), s).to(DTYPE[dt]).double())]
    x = t["x"].double()
    out = [("y", ref, F.leaky_relu(x * t["scale"].double()[:, None] + t["shift"].double()[:, None], s))]
    if c.recipe == "normal":
        rows, per, C = x.shape
        G = 4
        gamma, beta = t["scale"][0].double(), t["shift"][0].double()
        mean, _, rstd = _moments(t["x"], G, GN_EPS)
        sc = gamma[None] * rstd.repeat_interleave(C // G, 1)
        sh = beta[None] - mean.repeat_interleave(C // G, 1) * sc
        v = x * sc[:, None] + sh[:, None]
        out.append(("group_norm", torch.where(v > 0, v, s * v),
                    F.leaky_relu(F.group_norm(x.transpose(1, 2), G, gamma, beta, GN_EPS), s).transpose(1, 2)))
    return out


def _leaky_bwd_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    n = c["n"]
    y = _rn(g, n)
    y[::5] = 0.0
    y[1::10] = -0.0
    return {"y": y.to(DTYPE[dt]), "gy": _rn(g, n).to(DTYPE[dt])}


def _leaky_bwd_reference(c: Case, dt: str, t):
    gy = t["gy"].float()
    return {"gv": Check(torch.where(t["y"].float() > 0, gy, _slope32(c) * gy).to(DTYPE[dt]), None)}


def _leaky_bwd_emulate(c: Case, dt: str, t):
    gy = t["gy"].float()
    return {"gv": gy * torch.where(t["y"].float() > 0, 1.0, _slope32(c))}


def _leaky_bwd_pairs(c: Case, dt: str, t):
    """autograd of F.leaky_relu at a pre-activation whose output is y (slope > 0: y / slope where y < 0)"""
    y = t["y"].double()
    s = _slope32(c)
    x = torch.where(y > 0, y, y / s).clone().requires_grad_(True)
    with torch.enable_grad():
        (F.leaky_relu(x, s) * t["gy"].double()).sum().backward()
    gy = t["gy"].double()
    return [("gv", torch.where(y > 0, gy, s * gy), x.grad)]


# =============================================================================================================== the statistics forms
SLOPE32 = float(torch.tensor(0.2, dtype=torch.float32))


def _stats_leaky_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    rows, per, C = c["rows"], c["per_row"], c["C"]
    t = {"x": (_rn(g, rows, per, C, scale=1.3, off=0.25)).to(DTYPE[dt])}
    if c["affine"]:
        t["scale"], t["shift"] = _tables(g, rows, C)
    return t


def _stats_pool_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    return {"x": _rn(g, c["B"], c["T"], 2 * c["Ho"] + 1, 2 * c["Wo"], c["C"], scale=1.3, off=0.25).to(DTYPE[dt])}


def stats_rows(c: Case) -> Tuple[int, int]:
    """(rows, per_row) of the tensor a statistics case stores"""
    if c.op == "stats_pool":
        return c["B"], ((c["T"] + 1) // 2) * c["Ho"] * c["Wo"]
    return c["rows"], c["per_row"]


def stats_reference(c: Case, y: torch.Tensor) -> Dict[str, Check]:
    """y: the STORED tensor (any shape [rows, ..., C]) -> checks on (mean, rstd) [rows, C] under STATS_TOL (compare_stats' definition)"""
    rows, C = y.shape[0], y.shape[-1]
    mean, _, rstd = _moments(y.reshape(rows, -1, C), c["G"], GN_EPS)
    return _table_checks(mean, rstd, None, None, C, False)


def stats_emulate(c: Case, y: torch.Tensor) -> Dict[str, torch.Tensor]:
    """fp32 statistics of the stored tensor over one contiguous axis per group (torch's cascade sum), as pass_ref's"""
    rows, C, G = y.shape[0], y.shape[-1], c["G"]
    xg = y.float().reshape(rows, -1, G, C // G).permute(0, 2, 1, 3).reshape(rows, G, -1).contiguous()
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    return {"mean": mean.double().repeat_interleave(C // G, 1), "rstd": (var + GN_EPS).rsqrt().double().repeat_interleave(C // G, 1)}


def _stats_y_emulate(c: Case, dt: str, t):
    if c.op == "stats_pool":
        return {"y": pool3d_fwd(t["x"].float())}
    return _leaky_apply_emulate(c, dt, t)


def _stats_pairs(c: Case, dt: str, t):
    """the (mean, rstd) the checks hold are those of F.group_norm: normalising the stored tensor with them is its output"""
    y = _stats_y_emulate(c, dt, t)["y"].to(DTYPE[dt])
    rows, C = y.shape[0], y.shape[-1]
    y3 = y.reshape(rows, -1, C).double()
    ref = stats_reference(c, y)
    mine = (y3 - ref["mean"].ref[:, None]) * ref["rstd"].ref[:, None]
    return [("normalised", mine, F.group_norm(y3.transpose(1, 2), c["G"], eps=GN_EPS).transpose(1, 2))]


# =============================================================================================================== conv333_s2_dgrad_small
def dgrad_ref(gy, w, in_shape):
    """fp64 autograd of F.conv3d(stride=2, padding=1): gy [B,To,Ho,Wo,Cout], w [Cout,Cin,3,3,3] -> [B,T,H,W,Cin]"""
    B, T, H, W = in_shape
    x = torch.zeros(B, w.shape[1], T, H, W, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        y = F.conv3d(x, w.double(), None, stride=2, padding=1)
        assert tuple(y.shape[2:]) == tuple(gy.shape[1:4])
        (y * gy.double().permute(0, 4, 1, 2, 3)).sum().backward()
    return x.grad.permute(0, 2, 3, 4, 1)


def dgrad_arith(terms, cout):
    """n 2^-24 sum|terms| for the fp32 accumulation of n <= 8 Cout products (an input pixel gathers from at most 8 output pixels)"""
    return 8 * cout * 2.0 ** -24 * terms


def dgrad_bound(ref, terms, dtype, cout):
    """dgrad_arith plus half an ulp of the storage dtype at the result (fp32 storage: none)"""
    a = dgrad_arith(terms, cout)
    if dtype == torch.float32:
        return a
    fi = torch.finfo(dtype)
    e = torch.floor(torch.log2((ref.abs() + a).clamp_min(fi.tiny)))      # binade of the result (subnormals: the smallest normal's)
    return a + 0.5 * fi.eps * torch.exp2(e)


def _dgrad_shape(c: Case):
    return (c["B"], c["T"], c["H"], c["W"])


def _dgrad_inputs(c: Case, dt: str):
    g = _gen(c, dt)
    B, T, H, W = _dgrad_shape(c)
    cout, cin = c["Cout"], c["Cin"]
    w = _rn(g, cout, cin, 3, 3, 3, scale=0.1).to(DTYPE[dt])
    gy = _rn(g, B, (T - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1, cout).to(DTYPE[dt])
    return {"gy": gy, "w": w}


def _dgrad_reference(c: Case, dt: str, t):
    shape = _dgrad_shape(c)
    ref, terms = dgrad_ref(t["gy"], t["w"], shape), dgrad_ref(t["gy"].abs(), t["w"].abs(), shape)
    bound = dgrad_bound(ref, terms, DTYPE[dt], c["Cout"])
    return {"gx": Check(ref, bound, 0.0, bound - dgrad_arith(terms, c["Cout"])),
            "pad": Check(torch.zeros(*shape, 8 - c["Cin"]), None)}


def _dgrad_emulate(c: Case, dt: str, t):
    """the gather as fp32 conv_transpose3d"""
    return {"gx": _dgrad_transposed(c, t, torch.float32), "pad": torch.zeros(*_dgrad_shape(c), 8 - c["Cin"])}


def _dgrad_transposed(c: Case, t, dtype):
    B, T, H, W = _dgrad_shape(c)
    gy = t["gy"].to(dtype).permute(0, 4, 1, 2, 3)
    op = tuple(n - 2 * o + 1 for n, o in zip((T, H, W), gy.shape[2:]))
    return F.conv_transpose3d(gy, t["w"].to(dtype), None, stride=2, padding=1, output_padding=op).permute(0, 2, 3, 4, 1)


def _dgrad_pairs(c: Case, dt: str, t):
    return [("gx", _dgrad_transposed(c, t, torch.float64), _dgrad_reference(c, dt, t)["gx"].ref)]


# =============================================================================================================== dispatch
_OPS = {
    "scale_in": (_scale_in_inputs, _scale_in_reference, _scale_in_emulate, _scale_in_pairs),
    "scale_in_bwd": (_scale_in_bwd_inputs, _scale_in_bwd_reference, _scale_in_bwd_emulate, _scale_in_bwd_pairs),
    "relu": (_relu_inputs, _relu_reference, _relu_emulate, _relu_pairs),
    "maxpool": (_maxpool_inputs, _maxpool_reference, _maxpool_emulate, _maxpool_pairs),
    "relu_pool_bwd": (_relu_pool_bwd_inputs, _relu_pool_bwd_reference, _relu_pool_bwd_emulate, _relu_pool_bwd_pairs),
    "head": (_head_inputs, _head_reference, _head_emulate, _head_pairs),
    "pool3d": (_pool3d_inputs, _pool3d_reference, _pool3d_emulate, _pool3d_pairs),
    "leaky_apply": (_leaky_apply_inputs, _leaky_apply_reference, _leaky_apply_emulate, _leaky_apply_pairs),
    "leaky_bwd": (_leaky_bwd_inputs, _leaky_bwd_reference, _leaky_bwd_emulate, _leaky_bwd_pairs),
    "stats_leaky": (_stats_leaky_inputs, None, _stats_y_emulate, _stats_pairs),
    "stats_pool": (_stats_pool_inputs, None, _stats_y_emulate, _stats_pairs),
    "dgrad": (_dgrad_inputs, _dgrad_reference, _dgrad_emulate, _dgrad_pairs),
}
STATS_OPS = ("stats_leaky", "stats_pool")
# outputs the kernels store in fp32 whatever the case's dtype
FP32_OUT = {"head": ("out",)}


@functools.lru_cache(maxsize=None)
def inputs(case: Case, dt: str) -> Dict[str, torch.Tensor]:
    """the CPU operands of a case (computed once per process and shared: treat them as read-only)"""
    return _OPS[case.op][0](case, dt)


@functools.lru_cache(maxsize=None)
def reference(case: Case, dt: str) -> Dict[str, Check]:
    """the fp64 reference and bounds of a case (computed once per process and shared: treat them as read-only)"""
    return _OPS[case.op][1](case, dt, inputs(case, dt))


def emulate(case: Case, dt: str) -> Dict[str, torch.Tensor]:
    return _OPS[case.op][2](case, dt, inputs(case, dt))


def round_emu(case: Case, dt: str, emu: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the one store rounding of the case's dtype on an emulation's fp32 outputs"""
    keep = FP32_OUT.get(case.op, ())
    return {k: (v if k in keep else v.to(DTYPE[dt])) for k, v in emu.items()}


def torch_pairs(case: Case, dt: str) -> List[Tuple[str, torch.Tensor, torch.Tensor]]:
    return _OPS[case.op][3](case, dt, inputs(case, dt))


def worst(checks: Dict[str, Check], got: Dict[str, torch.Tensor], before_store: bool = False):
    """(worst err / bound over every checked output, 'name[index]' of it, violations)"""
    w, where, bad = 0.0, "-", 0
    for name, chk in checks.items():
        r, idx, n = check_one(got[name], chk, before_store and chk.bound is not None)
        bad += n
        if r > w or where == "-":
            w, where = r, f"{name}{list(idx)}"
    return w, where, bad
