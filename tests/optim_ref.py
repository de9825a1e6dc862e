"""References for the update-step tests: fp32 torch emulations of the four cvvae_mt_* passes (the arithmetic include/cvvae.h documents,
for the host-logic tests), the same formulas in fp64 (the GPU tests' yardstick), fp32 ulps, and the tensor list that puts every edge
of the chunk geometry into one launch."""
import math

import torch

from cvvae_amd import _lib as L

CHUNK = L.MT_CHUNK
# configs/cvvae_sd3_constraint_training.yaml: base_learning_rate 2.0e-5 x lr_g_factor 2, optimizer_config.params
YAML_ADAMW = dict(betas=[0.9, 0.98], eps=1.0e-4, weight_decay=0.01)
YAML_LR = 4.0e-5
YAML_COSINE = dict(name="cosine", num_warmup_steps=1000, num_training_steps=60000, min_lr_ratio=0.005)


# ---- fp32 emulations (signatures of cvvae_amd.ops.mt_*) ----
def emu_mt_grad_norm(mtl, max_norm):
    total = torch.zeros((), dtype=torch.float32)
    for g in mtl.tensors["g"]:
        total = total + (g.detach().float() ** 2).sum()
    norm = total.sqrt()
    c = torch.tensor(float(max_norm), dtype=torch.float32) / (norm + 1e-6)
    return torch.stack([norm, torch.where(c > 1.0, torch.ones_like(c), c)])


def emu_mt_scale(mtl, coef):
    for g in mtl.tensors["g"]:
        g.detach().mul_(coef.reshape(()))


def emu_mt_adamw(mtl, lr, beta1, beta2, eps, weight_decay, coef=None):
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731 -- a double rounded to fp32 once
    t = mtl.tensors
    for g, p, m, v, ss, b2 in zip(t["g"], t["p"], t["m"], t["v"], mtl.step_size, mtl.bias2_sqrt):
        g, p = g.detach(), p.detach()
        G = g * coef.reshape(()) if coef is not None else g
        m.copy_(f(beta1) * m + f(1.0 - beta1) * G)
        v.copy_(f(beta2) * v + f(1.0 - beta2) * (G * G))
        denom = v.sqrt() / f(b2) + f(eps)
        p.copy_(p * f(1.0 - lr * weight_decay) - f(ss) * (m / denom))


def emu_mt_ema(mtl, one_minus_decay):
    omd = torch.tensor(one_minus_decay, dtype=torch.float32)
    for p, s in zip(mtl.tensors["p"], mtl.tensors["shadow"]):
        s.sub_(omd * (s - p.detach()))


def pretend_gpu(monkeypatch, count=None):
    """route CPU tensors to the kernel path with the four launches emulated; count: a dict that receives the launches per name"""
    from cvvae_amd import ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "_need_gpu", lambda t: None)
    for name, fn in (("mt_grad_norm", emu_mt_grad_norm), ("mt_scale", emu_mt_scale), ("mt_adamw", emu_mt_adamw), ("mt_ema", emu_mt_ema)):
        def rec(*a, _n=name, _f=fn, **k):
            if count is not None:
                count[_n] = count.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, rec)


# ---- the yardstick: the header's formulas in fp64 on the same fp32 inputs ----
def adamw64(g, p, m, v, t, lr, beta1, beta2, eps, weight_decay, coef=None):
    """-> (m', v', p', G, delta) in fp64; coef: the fp32 value the device scalar holds (or None); delta = p' - p"""
    g, p, m, v = (x.detach().double() for x in (g, p, m, v))
    G = g * float(coef) if coef is not None else g
    m2 = beta1 * m + (1.0 - beta1) * G
    v2 = beta2 * v + (1.0 - beta2) * G * G
    step_size = lr / (1.0 - beta1 ** t)
    p2 = p * (1.0 - lr * weight_decay) - step_size * m2 / (v2.sqrt() / math.sqrt(1.0 - beta2 ** t) + eps)
    return m2, v2, p2, G, p2 - p


def ema64(s, p, one_minus_decay):
    s, p = s.detach().double(), p.detach().double()
    return s - one_minus_decay * (s - p)


def ulp32(x):
    """fp32's unit in the last place at magnitude |x| (x: fp64 tensor); the subnormal spacing below 2^-126"""
    _, e = torch.frexp(x.abs().double())                     # |x| = f 2^e, f in [0.5, 1)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 24).clamp_min(-149))


def log_uniform(shape, gen, lo=1e-6, hi=1.0, signed=True):
    mag = torch.exp(torch.empty(shape, dtype=torch.float64).uniform_(math.log(lo), math.log(hi), generator=gen))
    if signed:
        mag = mag * (torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1)
    return mag.float()


EDGE_NUMELS = (0, 1, 7, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
EDGE_STEPS = (1, 2, 7, 1000)
GUARD = 64  # untouched elements after every buffer


def edge_list(seed=0):
    """the tensor list of the GPU tests, on the CPU: one dict per tensor with fp32 `g` (None for the one without a gradient), `p`, `m`,
    `v`, `s` (EMA shadow) and its step count `t`.  Every tensor is a view [off, off + n) of a buffer of off + n + GUARD elements (`*_buf`);
    off = 0 except for the view that starts 4 bytes into its buffer; the 1-element tensor is 0-dim.  Gradients are log-uniform in
    magnitude over 1e-6 ... 1 with random signs, m alike, v over the squares' range 1e-12 ... 1, p and s of unit scale."""
    gen = torch.Generator().manual_seed(seed)
    specs = [(n, 0, True) for n in EDGE_NUMELS] + [(CHUNK + 3, 1, True), (1000, 0, False)]
    out = []
    for i, (n, off, has_grad) in enumerate(specs):
        d = {"n": n, "off": off, "t": EDGE_STEPS[i % len(EDGE_STEPS)]}
        for k in ("g", "p", "m", "v", "s"):
            size = off + n + GUARD
            if k in ("g", "m"):
                buf = log_uniform((size,), gen)
            elif k == "v":
                buf = log_uniform((size,), gen, 1e-12, 1.0, signed=False)
            else:
                buf = torch.randn(size, generator=gen, dtype=torch.float64).float()
            d[k + "_buf"] = buf
        out.append(d)
        d["has_grad"] = has_grad
    return out


def views(d, bufs):
    """the tensor views of entry d over (possibly device copies of) its buffers: {g, p, m, v, s}"""
    shape = () if d["n"] == 1 else (d["n"],)
    return {k: bufs[k + "_buf"][d["off"]:d["off"] + d["n"]].view(shape) for k in ("g", "p", "m", "v", "s")}
