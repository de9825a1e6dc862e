"""References of the attention-BLOCK edge tests (plain torch on the CPU; tests/attn_block_cases.py is the case table).

  inputs(case, dt)      the block's input, cotangent and parameters, built by the case's recipe and rounded to the model's dtype
  yardstick(case, dt)   fp64 autograd of a functional restatement of the block over those rounded operands: y, dL/dx for the seeded
                        cotangent and every parameter gradient -- and, for every parameter gradient, S: the same contraction over the
                        absolute values of its summands (|a|^T |g| of a weight, sum |g| of a bias, sum |g xhat| / sum |g| of a norm)
  rounded(case, dt)     the same restatement, forward and a hand-written backward, in fp64 with ONE rounding to the storage dtype at
                        every tensor the product path stores (STORED below); `model=None` switches every rounding off, and that
                        run has to equal the autograd yardstick (the host test holds it to 1e-10): the hand-written adjoint is right
  noise(case, dt)       the error measure of `rounded` against `yardstick`, per tensor: what the storage roundings alone cost
  emulate(case, dt, defect)   the composition restated over tests/emu_ops.py (fp32 torch), written from the block's definition and
                        independent of grad.py / grad3d.py; takes one seeded defect of DEFECTS
  run_product(...)      the REAL engine / grad / grad3d functions on a device (the GPU test), or on the CPU under
                        emu_ops.patched() (the host test's second draw)

STORED (read off engine.spatial_attention, engine.v3_attn_spatial_temporal, grad.attention_backward and
grad3d.temporal_attention_backward): forward n (the 1x1 kernel stages GroupNorm's output in the storage dtype), q, k, v, P, o, y; the
temporal half's n, q_t, k_t, v_t, o, y.  Backward g_o, g_s, (P^T and g_s^T: copies), g_v, g_q, g_k, the running g_n after each of
the three chained launches, dx; the temporal half's g_o, g_q, g_k, g_v, the running g_n, g_h.  The scores S = q k^T / sqrt(C) and g_p
are fp32 tensors in every model: they are rounded to fp32, never to the storage dtype.  Parameter gradients are fp32.

fp32 models.  The storage roundings are fp32.  The 1x1 MFMA kernel multiplies in split precision: conv_kernel.h stages every fp32
operand as hi = fp16(x), lo = fp16(x - hi) -- an fp16 split, NOT bf16 -- and runs Whi.hi + Whi.lo + Wlo.hi into one fp32
accumulator (Wlo.lo is dropped); module weights are packed from w * 2^k (ops._wscale, so that Wlo stays normal), the per-frame
"weights" packed from activations are not scaled.  The weight-gradient kernel splits both operands into bf16 hi + lo instead
(tests/wgrad_ref.py).  `rounded` models each kernel's own split, and sums the three part products in fp32 (torch's fp32 matmul: one
more summation order), because for an fp32 model the accumulator's rounding is of the size of the storage roundings.  XP_ULP of
tests/conv_instance_cases.py is the bound of the first form; the host test ties the model to it.

Error measures.  Activations (y, dx): per token row ||got - ref|| / max(||ref||, 1e-3 median row norm), the worst row.  Parameter
gradients: ||got - ref|| / ||S|| over the tensor (the same per output channel is reported).  A product-path tensor has to satisfy
measure <= MARGIN * noise with MARGIN = 3: the product path rounds at the same places but sums in another order, so it is another
draw of the same error process; two draws differ by at most twice the noise in norm, and 3 leaves room for the worst row of a few
hundred.  Nothing measured on a GPU enters: noise comes from `rounded`, MARGIN is held on the CPU by the second draw.

Exact conditions (no band): EXACT_ZERO(case) -- the q / k gradients at N = 1 and q_t / k_t at T = 1; the key-bias gradients have a
zero yardstick for every N (softmax is shift invariant) and are measured against S alone, which is why S exists."""
import contextlib
import functools
import math
import os
from typing import Dict, List, Optional

import torch

import attn_block_cases as AC
from attn_block_cases import BF16, F16, F32, SD3, V3S, V3ST, Case

DTYPE = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
MARGIN = 3.0
G32 = 32
K1 = (1, 1, 1)
LN_EPS = 1e-5
EPS = {SD3: 1e-6, V3S: 1e-5, V3ST: 1e-5}
SPATIAL = ("norm", "q", "k", "v", "proj")
TEMPORAL = ("norm_t", "q_t", "k_t", "v_t", "proj_t")
# role -> the module's name of the layer
NAMES = {SD3: dict(norm="group_norm", q="to_q", k="to_k", v="to_v", proj="to_out"),
         V3S: dict(norm="norm", q="q", k="k", v="v", proj="proj_out"),
         V3ST: dict(norm="attn.norm", q="attn.q", k="attn.k", v="attn.v", proj="attn.proj_out", norm_t="attn.norm_t", q_t="attn.q_t",
                    k_t="attn.k_t", v_t="attn.v_t", proj_t="attn.proj_out_t")}
EDGE_MASS = 0.9          # what the edgekey recipe guarantees in the fp64 yardstick
_EDGE_TARGET = 0.93      # what it is built for (the dtype roundings of the operands move the mass a little)


def roles(case: Case):
    return SPATIAL + (TEMPORAL if case.op == V3ST else ())


def param_keys(case: Case) -> List[str]:
    return [f"{r}.{s}" for r in roles(case) for s in ("weight", "bias")]


def mstar(case: Case, f: int) -> int:
    """the dominant key of frame f: the last valid token (`block`: the first token of the last 32-key block); odd frames take its
    neighbour inside the row, so that a frame reading another frame's K is seen"""
    N = AC.tokens(case)
    if case["mstar"] == "block":
        base = 32 * ((N - 1) // 32)
        return base + (f % 2 if base + 1 <= N - 1 else 0)
    return N - 1 - (f % 2 if N >= 2 else 0)


# ----------------------------------------------------------------------------------------------------------------- the restatement
def _gn_hat(x, eps, groups):
    """x [F, N, C] -> (xhat, rstd and mean per element): statistics per frame and group over (N, C / groups)"""
    Fr, N, C = x.shape
    xg = x.reshape(Fr, N, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = (var + eps).rsqrt()
    ex = lambda a: a.expand(Fr, N, groups, C // groups).reshape(Fr, N, C)   # noqa: E731
    return ((xg - mean) * rstd).reshape(Fr, N, C), ex(rstd), ex(mean)


def _gn_bwd(gh, xh, rstd, groups):
    """input gradient of xhat given gh = dL/dxhat: rstd (gh - mean(gh) - xhat mean(gh xhat)) over each frame's group"""
    Fr, N, C = gh.shape
    sh = (Fr, N, groups, C // groups)
    c1 = gh.reshape(sh).mean((1, 3), keepdim=True).expand(sh).reshape(Fr, N, C)
    c2 = (gh * xh).reshape(sh).mean((1, 3), keepdim=True).expand(sh).reshape(Fr, N, C)
    return rstd * (gh - c1 - xh * c2)


LOG2E_F32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))


class Arith:
    """the arithmetic of one run: `st` rounds a stored tensor, `f32` rounds a tensor the product path keeps in fp32, `mm(a, w, ws)` is
    the 1x1 kernel's product a @ w (ws: the pack scale of a module weight), `mmw(gt, a)` the weight-gradient kernel's gt @ a"""

    def __init__(self, model: Optional[str]):
        self.model = model
        if model is None:
            self.st = self.f32 = self.wk = lambda t: t
        else:
            dt = DTYPE[model]
            self.st = lambda t: t.to(dt).double()
            self.f32 = lambda t: t.float().double()
            self.wk = lambda t: t.float()   # the element-wise kernels (norms, softmax, temporal attention) work in fp32

    @staticmethod
    def _split(t, part):
        hi = t.to(part).float()
        return hi, (t - hi).to(part).float()

    def rows(self, t):
        """sum of t [P, C] over its P rows as a bias / affine gradient kernel makes it: in fp32.  Sequentially -- of the orders a
        kernel can take the one with the largest expected error, so that MARGIN x this draw covers a blocked or pairwise order"""
        if self.model is None:
            return t.sum(0)
        t32 = t.float()
        acc = torch.zeros_like(t32[0])
        for i in range(t32.shape[0]):   # (torch.cumsum accumulates a float tensor in double on the CPU)
            acc += t32[i]
        return acc.double()

    def softmax(self, s):
        """the kernels' row softmax (softmax_rows_kernel, temporal_attn_kernel and its backward): __expf, i.e. exp2 of the fp32 product
        (s - max) * log2(e), summed in fp32, times the fp32 reciprocal of the sum"""
        if self.model is None:
            return torch.softmax(s, -1)
        s32 = s.float()
        e = torch.exp2(((s32 - s32.max(-1, keepdim=True).values) * LOG2E_F32).double()).float()
        return e * (1.0 / e.sum(-1, keepdim=True))

    def mm(self, a, w, ws: float = 1.0):
        if self.model is None:
            return a @ w
        if self.model != F32:   # 16-bit operands: exact products, summed in the fp32 accumulator
            return (a.float() @ w.float()).double()
        ah, al = self._split(a.float(), torch.float16)
        wh, wl = self._split((w * ws).float(), torch.float16)
        return (ah @ wh + (al @ wh + ah @ wl)).double() / ws

    def mmw(self, gt, a):
        if self.model is None:
            return gt @ a
        if self.model != F32:
            return (gt.float() @ a.float()).double()
        gh, gl = self._split(gt.float(), torch.bfloat16)
        ah, al = self._split(a.float(), torch.bfloat16)
        return (gh @ ah + (gh @ al + gl @ ah)).double()


def _ws(w) -> float:
    """the power-of-two pack scale of an fp32 module weight (ops._wscale)"""
    from cvvae_amd import ops
    return ops._wscale(w.float())


def _linear(A: Arith, a, P, r, extra=None):
    w, b = P[r + ".weight"], P[r + ".bias"]
    y = A.mm(a, w.t(), _ws(w.detach()) if A.model == F32 else 1.0) + b
    return A.st(y if extra is None else y + extra)


def _dlinear(A: Arith, g, P, r, extra=None):
    """g . W (+ extra): the input gradient of a linear layer, the running sum in the launch's residual input"""
    w = P[r + ".weight"]
    y = A.mm(g, w, _ws(w.detach()) if A.model == F32 else 1.0)
    return A.st(y if extra is None else y + extra)


def forward(A: Arith, case: Case, x, P) -> Dict[str, torch.Tensor]:
    """x [F, N, C] fp64 (frames b-major), P: role.weight / role.bias fp64 -> every tensor the pass makes (keys as in STORED)"""
    B, T, C = case["B"], case["T"], case["C"]
    Fr, N, _ = x.shape
    scale = float(C) ** -0.5
    t = {}
    wk = A.wk
    t["xh"], t["rstd"], mean = _gn_hat(x, EPS[case.op], G32)
    sc = P["norm.weight"] * t["rstd"]                                  # the kernel's fp32 (scale, shift) tables
    n = t["n"] = A.st(wk(x) * wk(sc) + wk(P["norm.bias"] - mean * sc))
    q, k, v = (_linear(A, n, P, r) for r in ("q", "k", "v"))
    t["q"], t["k"], t["v"] = q, k, v
    t["s"] = A.f32(A.mm(q, k.transpose(1, 2)) * scale)
    p = t["p"] = A.st(A.softmax(t["s"]))
    o = t["o"] = A.st(A.mm(p, v))
    h = t["h"] = _linear(A, o, P, "proj", extra=x if case.op != V3ST else None)
    if case.op != V3ST:
        t["y"] = h
        return t
    # the temporal half: LayerNorm over C per token, attention over the T frames of every pixel, one residual from outside
    mu = h.mean(-1, keepdim=True)
    t["rstd_t"] = (((h - mu) ** 2).mean(-1, keepdim=True) + LN_EPS).rsqrt()
    t["hh"] = (h - mu) * t["rstd_t"]
    sc = P["norm_t.weight"] * t["rstd_t"]
    nt = t["n_t"] = A.st(wk(h) * wk(sc) + wk(P["norm_t.bias"] - mu * sc))
    pix = lambda a: a.reshape(B, T, N, C).permute(0, 2, 1, 3)          # noqa: E731  [B, N, T, C]
    t["q_t"], t["k_t"], t["v_t"] = (_linear(A, nt, P, r) for r in ("q_t", "k_t", "v_t"))
    t["s_t"] = wk(pix(t["q_t"])) @ wk(pix(t["k_t"])).transpose(-1, -2) * scale
    t["p_t"] = A.softmax(t["s_t"])
    t["o_t"] = A.st((t["p_t"] @ wk(pix(t["v_t"]))).permute(0, 2, 1, 3).reshape(Fr, N, C))
    t["y"] = _linear(A, t["o_t"], P, "proj_t", extra=x)
    return t


def _lin_grads(A: Arith, out, S, r, a, g):
    """dW = g^T a, db = sum g of a linear layer over every pixel of every frame; S over absolute values"""
    C = a.shape[-1]
    a2, g2 = a.reshape(-1, C), g.reshape(-1, g.shape[-1])
    out[r + ".weight"], out[r + ".bias"] = A.mmw(g2.t(), a2), A.rows(g2)
    S[r + ".weight"], S[r + ".bias"] = g2.abs().t() @ a2.abs(), g2.abs().sum(0)


def backward(A: Arith, case: Case, x, P, t, gy):
    """the hand-written adjoint of `forward` with the product path's roundings -> ({dx, parameter gradients}, S)"""
    B, T, C = case["B"], case["T"], case["C"]
    Fr, N, _ = x.shape
    scale = float(C) ** -0.5
    out, S = {}, {}
    g = gy
    wk = A.wk
    if case.op == V3ST:
        pix = lambda a: wk(a.reshape(B, T, N, C).permute(0, 2, 1, 3))  # noqa: E731
        unpix = lambda a: a.permute(0, 2, 1, 3).reshape(Fr, N, C)      # noqa: E731
        _lin_grads(A, out, S, "proj_t", t["o_t"], g)
        g_o = pix(_dlinear(A, g, P, "proj_t"))
        q, k, v, p = pix(t["q_t"]), pix(t["k_t"]), pix(t["v_t"]), t["p_t"]
        g_v = A.st(unpix(p.transpose(-1, -2) @ g_o))
        g_p = g_o @ v.transpose(-1, -2)
        g_s = scale * p * (g_p - (p * g_p).sum(-1, keepdim=True))
        g_q, g_k = A.st(unpix(g_s @ k)), A.st(unpix(g_s.transpose(-1, -2) @ q))
        g_n = None
        for r, gg in (("q_t", g_q), ("k_t", g_k), ("v_t", g_v)):
            _lin_grads(A, out, S, r, t["n_t"], gg)
            g_n = _dlinear(A, gg, P, r, extra=g_n)
        hh = t["hh"]
        out["norm_t.weight"], out["norm_t.bias"] = A.rows((wk(g_n) * wk(hh)).reshape(-1, C)), A.rows(g_n.reshape(-1, C))
        S["norm_t.weight"], S["norm_t.bias"] = (g_n * hh).abs().sum((0, 1)), g_n.abs().sum((0, 1))
        gh, hw = wk(g_n) * wk(P["norm_t.weight"]), wk(hh)
        g = A.st(wk(t["rstd_t"]) * (gh - gh.mean(-1, keepdim=True) - hw * (gh * hw).mean(-1, keepdim=True)))
    add = gy  # (sd3 / v3s: the block's own residual; v3st: the outer one, `add_extra`)
    q, k, v, p = t["q"], t["k"], t["v"], t["p"]
    _lin_grads(A, out, S, "proj", t["o"], g)
    g_o = _dlinear(A, g, P, "proj")
    g_p = A.f32(A.mm(g_o, v.transpose(1, 2)))
    g_s = A.st(scale * wk(p) * (wk(g_p) - (wk(p) * wk(g_p)).sum(-1, keepdim=True)))
    g_v = A.st(A.mm(p.transpose(1, 2), g_o))
    g_q = A.st(A.mm(g_s, k))
    g_k = A.st(A.mm(g_s.transpose(1, 2), q))
    g_n = None
    for r, gg in (("q", g_q), ("k", g_k), ("v", g_v)):
        _lin_grads(A, out, S, r, t["n"], gg)
        g_n = _dlinear(A, gg, P, r, extra=g_n)
    xh = t["xh"]
    out["norm.weight"], out["norm.bias"] = A.rows((wk(g_n) * wk(xh)).reshape(-1, C)), A.rows(g_n.reshape(-1, C))
    S["norm.weight"], S["norm.bias"] = (g_n * xh).abs().sum((0, 1)), g_n.abs().sum((0, 1))
    out["dx"] = A.st(_gn_bwd(wk(g_n) * wk(P["norm.weight"]), wk(xh), wk(t["rstd"]), G32) + wk(add))
    return out, S


# ----------------------------------------------------------------------------------------------------------------- inputs
def _f64(d):
    return {k: v.double() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _base(case: Case):
    """the case's operands in fp32 before the dtype rounding: x, gy [F, N, C], parameters by role"""
    g = torch.Generator().manual_seed(case.seed)
    C, N, Fr = case["C"], AC.tokens(case), AC.frames(case)
    rnd = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
    uni = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * C ** -0.5  # noqa: E731  (torch's default linear / conv initialisation)
    x = rnd(Fr, N, C) * 1.3 + 0.2 if case.recipe != "edgekey" else rnd(Fr, N, C)
    gy = rnd(Fr, N, C)
    P = {}
    for r in roles(case):
        if r.startswith("norm"):
            P[r + ".weight"], P[r + ".bias"] = 1.0 + 0.1 * rnd(C), 0.1 * rnd(C)
        else:
            P[r + ".weight"], P[r + ".bias"] = uni(C, C), uni(C)
    A = Arith(None)
    if case.recipe == "sharp":
        # to_q / to_k (weights and biases) by one factor each so that the fp64 score standard deviation is 4; the temporal half alike
        for rq, rk, key in (("q", "k", "s"), ("q_t", "k_t", "s_t")):
            if rq + ".weight" not in P or (key == "s" and N == 1) or (key == "s_t" and case["T"] == 1):
                continue
            sd = float(forward(A, case, x.double(), _f64(P))[key].std(unbiased=False))
            f = math.sqrt(4.0 / sd)
            for r in (rq, rk):
                P[r + ".weight"], P[r + ".bias"] = P[r + ".weight"] * f, P[r + ".bias"] * f
    elif case.recipe == "edgekey":
        # token m* of every frame is 4 r (r a +-1 vector), to_k ~ the identity, to_q ~ its bias c r: every query's score at m* is about
        # 4 c sqrt(C) / sigma above the others'; c is the smallest of a geometric ladder that puts _EDGE_TARGET of every row on m*
        r = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
        for f in range(Fr):   # (+ a part of the frame's own, so that the frames' outputs differ and the temporal half has something to attend to)
            x[f, mstar(case, f)] = 4.0 * r + 1.5 * rnd(C)
        P["k.weight"], P["k.bias"] = torch.eye(C) + 0.1 * P["k.weight"], 0.1 * P["k.bias"]
        P["q.weight"] = 0.1 * P["q.weight"]
        xh = _gn_hat(x.double(), EPS[case.op], G32)[0]
        n = xh * P["norm.weight"].double() + P["norm.bias"].double()
        k = n @ P["k.weight"].double().t() + P["k.bias"].double()
        base = (n @ P["q.weight"].double().t()) @ k.transpose(1, 2) * C ** -0.5          # the scores without the bias
        per_c = (k @ r.double()) * C ** -0.5                                              # what c adds to column m
        ms = torch.tensor([mstar(case, f) for f in range(Fr)])
        c = 0.02
        while True:
            mass = torch.softmax(base + c * per_c[:, None, :], -1)[torch.arange(Fr), :, ms].min()
            if mass >= _EDGE_TARGET:
                break
            c *= 1.15
            assert c < 50.0, case.name
        P["q.bias"] = c * r
    return x, gy, P


@functools.lru_cache(maxsize=None)
def inputs(case: Case, dt: str):
    """-> dict(x, gy [B, T, H, W, C] in the model's dtype, P: role.weight / role.bias in the model's dtype (weights [C, C]))"""
    x, gy, P = _base(case)
    tdt = DTYPE[dt]
    sh = (case["B"], case["T"], case["H"], case["W"], case["C"])
    return dict(x=x.to(tdt).reshape(sh), gy=gy.to(tdt).reshape(sh), P={k: v.to(tdt) for k, v in P.items()})


def _operands(case: Case, dt: str):
    d = inputs(case, dt)
    Fr, N, C = AC.frames(case), AC.tokens(case), case["C"]
    return d["x"].double().reshape(Fr, N, C), d["gy"].double().reshape(Fr, N, C), _f64(d["P"])


# ----------------------------------------------------------------------------------------------------------------- yardstick, rounded, noise
@functools.lru_cache(maxsize=None)
def yardstick(case: Case, dt: str):
    """-> (out: y, dx, parameter gradients from fp64 AUTOGRAD of `forward`; S; the forward's tensors (scores, probabilities))"""
    x, gy, P = _operands(case, dt)
    A = Arith(None)
    xr = x.clone().requires_grad_(True)
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    with torch.enable_grad():
        t = forward(A, case, xr, Pr)
        (t["y"] * gy).sum().backward()
    out = {"y": t["y"].detach(), "dx": xr.grad}
    out.update({k: v.grad for k, v in Pr.items()})
    with torch.no_grad():
        td = {k: v.detach() for k, v in t.items()}
        _, S = backward(A, case, x, P, td, gy)
    return out, S, td


@functools.lru_cache(maxsize=None)
def rounded(case: Case, dt: str, model="same"):
    """the restatement with the product path's storage roundings of model `dt` (model=None: none at all) -> out as yardstick's"""
    x, gy, P = _operands(case, dt)
    A = Arith(dt if model == "same" else model)
    with torch.no_grad():
        t = forward(A, case, x, P)
        out, _ = backward(A, case, x, P, t, gy)
    out["y"] = t["y"]
    return out


def row_measure(got, ref) -> float:
    C = ref.shape[-1]
    g, r = got.reshape(-1, C).double(), ref.reshape(-1, C).double()
    rn = r.norm(dim=1)
    floor = max(1e-3 * float(rn.median()), 1e-300)
    return float(((g - r).norm(dim=1) / rn.clamp_min(floor)).max())


S_FLOOR = 2.0 ** -24   # every summand of a parameter gradient is rounded to fp32 at least once: the noise of an S-relative measure is
#                        never taken below one fp32 rounding of S (the restatement can come out exact where a kernel does not, e.g. the
#                        two-key softmax backward, whose rows are exactly antisymmetric in torch's fp32 but not in another order)


def s_measure(got, ref, S) -> float:
    return float((got.double().reshape(S.shape) - ref.reshape(S.shape)).norm() / S.norm().clamp_min(1e-300))


def s_measure_channels(got, ref, S) -> float:
    """the worst output channel of a weight gradient under its own ||S||"""
    d = (got.double().reshape(S.shape) - ref.reshape(S.shape)).norm(dim=1)
    return float((d / S.norm(dim=1).clamp_min(1e-300)).max())


def measure(key: str, got, ref, S=None) -> float:
    return row_measure(got, ref) if key in ("y", "dx") else s_measure(got, ref, S[key])


def tensors(case: Case) -> List[str]:
    return ["y"] if case.get("fwd_only") or case.raises else ["y", "dx"] + param_keys(case)


def exact_zero(case: Case) -> List[str]:
    """parameter gradients that are exactly zero: one token has nothing to attend to but itself, so nothing reaches q and k"""
    z = []
    if AC.tokens(case) == 1:
        z += ["q.weight", "q.bias", "k.weight", "k.bias"]
    if case.op == V3ST and case["T"] == 1:
        z += ["q_t.weight", "q_t.bias", "k_t.weight", "k_t.bias"]
    return z


def zero_yardstick(case: Case) -> List[str]:
    """the key-bias gradients: mathematically zero for every N; only the S-relative measure means anything"""
    return ["k.bias"] + (["k_t.bias"] if case.op == V3ST else [])


def unbanded(case: Case) -> List[str]:
    """the key-bias gradient of a TWO-key softmax (N = 2; T = 2 for the temporal half).  It is the sum over queries of q times the row
    sums of g_s, and with two keys a row of g_s is (a, -a): torch's fp32 evaluates both entries by the same operations and ends exactly
    antisymmetric, so `rounded` carries no rounding at all here, while a kernel that takes the row sum in another order is left with
    eps / min(p) of |g_s|.  There is no CPU estimate of that noise to band it with; the tensor is asserted finite, and the two-key
    cases' other thirteen gradients are banded as everywhere.

    And the q- and k-bias gradients of the `edgekey` recipe.  Their error is the rows' failure to sum to zero -- the rounding of the
    softmax backward's row dot product -- times ONE fixed vector: k[m*] = 4 r for the q bias, q = c r for the k bias.  So the whole
    tensor's error is a single random number times a fixed direction, and the norms of two draws of one Gaussian differ by more than 3
    one time in five (the CPU second draw did, on v3s-C128-N129-b1t3-edgekey k.bias and v3s-C128-N33-b2t3-edgekey-block q.bias).  The
    flat and sharp cases band both tensors at N = 1 .. 256 and every frame count; here they are asserted finite and reproducible"""
    z = []
    if case.recipe == "edgekey":
        z += ["q.bias", "k.bias"]
    if AC.tokens(case) == 2 and "k.bias" not in z:
        z.append("k.bias")
    if case.op == V3ST and case["T"] == 2:
        z.append("k_t.bias")
    return z


def banded(case: Case) -> List[str]:
    z = exact_zero(case) + unbanded(case)
    return [k for k in tensors(case) if k not in z]


@functools.lru_cache(maxsize=None)
def noise(case: Case, dt: str) -> Dict[str, float]:
    ref, S, _ = yardstick(case, dt)
    r = rounded(case, dt)
    return {k: measure(k, r[k], ref[k], S) if k in ("y", "dx") else max(measure(k, r[k], ref[k], S), S_FLOOR) for k in tensors(case)}


def compare(case: Case, dt: str, got: Dict[str, torch.Tensor], keys=None):
    """-> [(tensor, measure, bound = MARGIN * noise, worst-channel measure or None)] of a product-path result against the yardstick"""
    ref, S, _ = yardstick(case, dt)
    nz = noise(case, dt)
    rows = []
    for k in (banded(case) if keys is None else keys):
        g = got[k].detach().cpu()
        ch = s_measure_channels(g, ref[k], S[k]) if k.endswith(".weight") and not k.startswith("norm") else None
        rows.append((k, measure(k, g, ref[k], S), MARGIN * nz[k], ch))
    return rows


# ----------------------------------------------------------------------------------------------------------------- the real functions
def module(case: Case, dt: str):
    """the block's module tree as tests/test_gpu_round2.py::_attn_module / modeling._v3_attn build it, holding inputs(case, dt)'s
    parameters"""
    from cvvae_amd.modeling import ConvP, NormP, _holder
    C, P = case["C"], inputs(case, dt)["P"]
    ksz = () if case.op == SD3 else (1, 1)
    kids = {}
    for r in roles(case):
        leaf = NAMES[case.op][r].split(".")[-1]
        kids[leaf] = NormP(C) if r.startswith("norm") else ConvP(C, C, () if r in TEMPORAL else ksz)
    m = _holder(**kids)
    if case.op == V3ST:
        m = _holder(attn=m)
    with torch.no_grad():
        for r in roles(case):
            for s in ("weight", "bias"):
                par = m.get_parameter(f"{NAMES[case.op][r]}.{s}")
                par.copy_(P[f"{r}.{s}"].float().reshape(par.shape))
    return m.to(DTYPE[dt])


def run_product(case: Case, dt: str, device="cpu", backward_pass=True, frozen=False, before=None):
    """engine.spatial_attention / v3_attn_spatial_temporal untaped and taped, then grad.attention_backward (+
    grad3d.temporal_attention_backward) with parameter gradients -> dict(y, y_taped, p, dx, role.weight, role.bias[, dx_frozen]).
    `before()` runs in front of every product call."""
    from cvvae_amd import engine, grad, grad3d
    before = before or (lambda: None)
    d = inputs(case, dt)
    m = module(case, dt).to(device)
    wc = engine.WeightCache(m)
    x, gy = d["x"].to(device), d["gy"].to(device)
    nm = NAMES[case.op]

    def fwd(tape):
        before()
        if case.op == V3ST:
            return engine.v3_attn_spatial_temporal(wc, x, "attn", tape=tape)[0]
        return engine.spatial_attention(wc, x, nm["norm"], nm["q"], nm["k"], nm["v"], nm["proj"], EPS[case.op], True, tape=tape)

    out = {"y": fwd(None)}
    if not backward_pass:
        return out
    tape: list = []
    out["y_taped"] = fwd(tape)
    out["p"] = tape[0]["p"]
    G: dict = {}
    before()
    if case.op == V3ST:
        g_h = grad3d.temporal_attention_backward(wc, gy, tape[1], G)
        before()
        out["dx"] = grad.attention_backward(wc, g_h, tape[0], G, add_extra=gy)
    else:
        out["dx"] = grad.attention_backward(wc, gy, tape[0], G)
        if frozen:
            before()
            out["dx_frozen"] = grad.attention_backward(wc, gy, tape[0])
    for r in roles(case):
        for s in ("weight", "bias"):
            out[f"{r}.{s}"] = G[f"{nm[r]}.{s}"]
    return out


def second_draw(case: Case, dt: str, **kw):
    """the real functions on the CPU over tests/emu_ops.py: fp32 torch arithmetic, autograd-based adjoints"""
    import emu_ops
    with emu_ops.patched(), torch.no_grad():
        return run_product(case, dt, "cpu", **kw)


# ----------------------------------------------------------------------------------------------------------------- emulate + defects
DEFECTS = ("scale_twice", "no_scale_bwd", "p_not_transposed", "k_of_next_frame", "drop_last_key", "shift_edge_key", "no_add_extra",
           "residual_twice", "qk_swapped_in_dk", "bias_over_wrong_rows", "gn_stats_per_sample", "ln_eps_of_gn", "proj_grad_from_p_v",
           "temporal_outer_residual_lost")
# proj_grad_from_p_v: with probabilities rounded to the storage dtype before the second product in both forms, the recomputed P V is the
# stored o up to its summation order, so the literal slip is inside every band by construction.  It is seeded as the form that a
# recomputation in the backward would most plainly take -- the product of the taped, PADDED p with V read at p's leading dimension --
# see emulate().


def _fused(case: Case, dt: str) -> bool:
    return os.environ.get("CVVAE_FUSED_ATTENTION", "1") != "0" and case["C"] == 512 and dt in (F16, BF16)


def emulate(case: Case, dt: str, defect: Optional[str] = None, frozen=False):
    """the two blocks and their adjoints over emu_ops, launch for launch as the block's definition asks -> as run_product"""
    import emu_ops as E
    from cvvae_amd import _lib as L
    assert defect is None or defect in DEFECTS
    d = inputs(case, dt)
    x, gy, P = d["x"], d["gy"], d["P"]
    B, T, H, W, C = x.shape
    N, BT = H * W, B * T
    npad = E.ops.round_up(N, 128)
    scale = float(C) ** -0.5
    tdt = DTYPE[dt]
    is_d = lambda name: defect == name                                  # noqa: E731
    flat = lambda a: a.view(a.shape[0], 1, 1, -1, a.shape[-1])          # noqa: E731
    frames = lambda a: a.view(BT, 1, 1, N, a.shape[-1])                 # noqa: E731

    def affine(r):
        return P[r + ".weight"].float().contiguous(), P[r + ".bias"].float().contiguous()

    def lin(r):
        return E.pack_weight(P[r + ".weight"].reshape(C, C, 1), P[r + ".bias"], K1)

    def lin_t(r):  # the input-gradient form: Cin and Cout exchanged, no bias
        return E.pack_weight(P[r + ".weight"].reshape(C, C, 1).flip(2).transpose(0, 1).contiguous(), None, K1)

    def linear(a5, r, residual=None):
        return E.conv(flat(a5), lin(r), residual=flat(residual) if residual is not None else None).view(*a5.shape[:-1], C)

    def dlinear(g5, r, residual=None):
        return E.conv(flat(g5), lin_t(r), residual=flat(residual) if residual is not None else None).view(*g5.shape[:-1], C)

    def lin_grads(G, r, a5, g5, rows=None):
        a5, g5 = a5.reshape(a5.shape[0], 1, 1, -1, C).contiguous(), g5.reshape(g5.shape[0], 1, 1, -1, C).contiguous()
        G[r + ".weight"] = E.conv_wgrad(a5, g5, K1, cin=C, cout=C).reshape(C, C)
        gb = g5 if rows is None else g5[:, :, :, :rows].contiguous()
        G[r + ".bias"] = E.bias_grad(gb, cout=C)

    # ---- forward, spatial half
    gamma, beta = affine("norm")
    eps = EPS[case.op]
    if is_d("gn_stats_per_sample"):
        gn = tuple(a.repeat_interleave(T, 0).contiguous() for a in E.gn_stats(x, gamma, beta, eps, per_frame=False))
    else:
        gn = E.gn_stats(x, gamma, beta, eps, per_frame=True)
    xf = frames(x)
    qq, kk, vv = (E.conv(xf, lin(r), prologue=L.PRO_GN, gn=gn) for r in ("q", "k", "v"))
    kk_f = kk.view(BT, N, C)
    if is_d("k_of_next_frame"):
        kk_f = torch.roll(kk_f, -1, 0).contiguous()
    if is_d("shift_edge_key"):
        kk_f = torch.roll(kk_f, 1, 1).contiguous()
    fscale = scale * scale if is_d("scale_twice") else scale
    nv = N - 1 if is_d("drop_last_key") and N > 1 else N
    o = None
    if _fused(case, dt):
        vt = E.transpose(vv.view(BT, N, C), ld_out=E.ops.round_up(N, 32))
        if nv != N:
            vt = vt.clone()
            vt[:, :, nv:] = 0
        o = E.attention_d512(qq.view(BT, N, C), kk_f[:, :nv].contiguous(), vt, nv, fscale)
    kp = E.pack_weight_batched(kk_f, K1, cin_pad=C, strides=(C, 1, 0), cout=N, cin=C)
    s = E.conv(qq, kp, out_f32=True, alpha=fscale, cout_pad=npad)
    p = E.softmax_rows(s.view(BT * N, npad), nv, tdt)
    if o is None:
        vp = E.pack_weight_batched(E.transpose(vv.view(BT, N, C)), K1, cin_pad=npad, strides=(N, 1, 0), cout=C, cin=N)
        o = E.conv(p.view(BT, 1, 1, N, npad), vp)
    o5 = o.view(B, T, H, W, C)
    own = case.op != V3ST
    h = linear(o5, "proj", residual=x if own else None)
    if own and is_d("residual_twice"):
        h = (h.float() + x.float()).to(tdt)
    out = {"p": p}
    if own:
        out["y"] = out["y_taped"] = h
    else:
        # ---- forward, temporal half
        ln_eps = 1e-6 if is_d("ln_eps_of_gn") else LN_EPS
        gt, bt = affine("norm_t")
        n_t = E.layernorm(h, gt, bt, ln_eps)
        q_t, k_t, v_t = (linear(n_t, r) for r in ("q_t", "k_t", "v_t"))
        o_t = E.temporal_attention(q_t, k_t, v_t)
        out["y"] = out["y_taped"] = linear(o_t, "proj_t", residual=None if is_d("temporal_outer_residual_lost") else x)
    if case.get("fwd_only") or case.raises:
        return out
    # ---- backward
    G: dict = {}
    g = gy
    if not own:
        f1 = lambda a: a.view(B, 1, 1, -1, C)                           # noqa: E731
        lin_grads(G, "proj_t", f1(o_t), f1(g))
        g_o = dlinear(g, "proj_t")
        g_q, g_k, g_v = E.temporal_attention_bwd(q_t, k_t, v_t, g_o)
        g_n = None
        for r, gg in (("q_t", g_q), ("k_t", g_k), ("v_t", g_v)):
            lin_grads(G, r, f1(n_t), f1(gg))
            g_n = dlinear(gg, r, residual=g_n)
        g, G["norm_t.weight"], G["norm_t.bias"] = E.layernorm_bwd(h, g_n, gt, bt, ln_eps)
    g_o = frames(dlinear(g, "proj"))
    vw = E.pack_weight_batched(vv.view(BT, N, C), K1, cin_pad=C, strides=(C, 1, 0), cout=N, cin=C)
    g_p = E.conv(g_o, vw, out_f32=True, cout_pad=npad)
    g_s = E.softmax_bwd_rows(p.view(BT * N, npad), g_p.view(BT * N, npad), N, 1.0 if is_d("no_scale_bwd") else scale)
    if is_d("p_not_transposed"):
        p_t = p.view(BT, N, npad)
    else:
        p_t = E.transpose(p.view(BT, N, npad), ncols=N, ld_out=npad)
    tw = lambda a: E.pack_weight_batched(E.transpose(a.view(BT, N, C)), K1, cin_pad=npad, strides=(N, 1, 0), cout=C, cin=N)  # noqa: E731
    g_v = E.conv(p_t.view(BT, 1, 1, N, npad), tw(g_o))
    g_q = E.conv(g_s.view(BT, 1, 1, N, npad), tw(kk))
    gs_t = E.transpose(g_s.view(BT, N, npad), ncols=N, ld_out=npad)
    g_k = E.conv(gs_t.view(BT, 1, 1, N, npad), tw(kk if is_d("qk_swapped_in_dk") else qq))
    g_n = dlinear(g_q, "q")
    g_n = dlinear(g_k, "k", residual=g_n)
    g_n = dlinear(g_v, "v", residual=g_n)
    one, zero = torch.ones(C), torch.zeros(C)
    tabs = E.gn_stats(x, one, zero, eps, per_frame=True)
    n = frames(E.gn_silu_apply(x, gn, silu=False, per_frame=True))
    o_w = frames(o)
    if is_d("proj_grad_from_p_v"):
        # recomputed from the taped p at ITS leading dimension against V^T packed for N keys: the probabilities of key m meet V row
        # m only where npad == N; elsewhere every frame after the first reads p rows shifted by the padding
        pv = p.view(-1)[:BT * N * N].view(BT, N, N).float()
        o_w = frames(torch.einsum("bnm,bmc->bnc", pv, vv.view(BT, N, C).float()).to(tdt).contiguous())
    lin_grads(G, "proj", o_w, frames(g))
    lin_grads(G, "q", n, g_q)
    lin_grads(G, "k", n, g_k)
    lin_grads(G, "v", n, g_v, rows=N - 1 if is_d("bias_over_wrong_rows") and N > 1 else None)
    add = gy if own or not is_d("no_add_extra") else None
    out["dx"], G["norm.weight"], G["norm.bias"] = E.gn_bwd_input_params(x, g_n.view(B, T, H, W, C), tabs, gamma, beta, silu=False,
                                                                          add=add, per_frame=True)
    if frozen and own:
        out["dx_frozen"] = E.gn_bwd_input(x, g_n.view(B, T, H, W, C), tabs, gamma, beta, silu=False, add=add, per_frame=True)
    out.update(G)
    return out


@contextlib.contextmanager
def fused_switch(on: bool):
    """CVVAE_FUSED_ATTENTION for the host test's runs (the GPU test uses monkeypatch)"""
    old = os.environ.get("CVVAE_FUSED_ATTENTION")
    os.environ["CVVAE_FUSED_ATTENTION"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["CVVAE_FUSED_ATTENTION"]
        else:
            os.environ["CVVAE_FUSED_ATTENTION"] = old
