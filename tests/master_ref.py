"""References for the master-weight tests (16-bit parameters on fp32 master weights: cvvae_amd/optim.py AdamW(master_weights=True),
lvdm/modules/ema.py LitEma(fp32_shadows=True), engine.master_weights()): torch emulations of the three wrappers
cvvae_amd.ops.mt_adamw_master / mt_sumsq / mt_norm_finish (the arithmetic include/cvvae.h documents), `pretend_gpu` = the one of
tests/optim_ref.py (and of tests/ddp_ref.py: the pack pass) plus these three, the edge list of tests/optim_ref.py stored in 16 bits,
and the stall experiment's constants."""
import torch

from tests import ddp_ref, optim_ref

CHUNK = optim_ref.CHUNK
DTYPES16 = (torch.bfloat16, torch.float16)

# the stall: 16 bf16 elements at 1.0, a constant gradient of 0.5, the YAML's hyper-parameters, 400 steps.  fp32 torch.optim.AdamW
# ends at 0.98383522 (torch 2.10 on the CPU), whose bf16 rounding is 0.984375 (the spacing there is 2^-8: the neighbours' midpoints
# 0.982421875 and 0.986328125 are 1.4e-3 and 2.5e-3 away)
STALL = dict(n=16, start=1.0, grad=0.5, steps=400, fp32_end=0.98383522, bf16_end=0.984375)


# ---- emulations (signatures of cvvae_amd.ops.mt_adamw_master / mt_sumsq / mt_norm_finish) ----
def emu_mt_adamw_master(mtl, lr, beta1, beta2, eps, weight_decay, coef=None):
    """optim_ref.emu_mt_adamw on (float(g), master, m, v), then p <- master rounded to nearest even (copy_)"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731 -- a double rounded to fp32 once
    t = mtl.tensors
    assert mtl.dtype in DTYPES16
    for g, p, m, v, w, ss, b2 in zip(t["g"], t["p"], t["m"], t["v"], t["shadow"], mtl.step_size, mtl.bias2_sqrt):
        assert g.dtype == p.dtype == mtl.dtype and m.dtype == v.dtype == w.dtype == torch.float32
        G = g.detach().float()
        if coef is not None:
            G = G * coef.reshape(())
        m.copy_(f(beta1) * m + f(1.0 - beta1) * G)
        v.copy_(f(beta2) * v + f(1.0 - beta2) * (G * G))
        denom = v.sqrt() / f(b2) + f(eps)
        w.copy_(w * f(1.0 - lr * weight_decay) - f(ss) * (m / denom))
        p.detach().copy_(w)


def emu_mt_sumsq(mtl, partials):
    """one partial per chunk, tensors in list order, chunks in element order"""
    assert partials.dtype == torch.float32 and partials.numel() >= mtl.n_chunks
    c = 0
    for g in mtl.tensors["g"]:
        assert g.dtype == mtl.dtype
        flat = g.detach().float().reshape(-1)
        for lo in range(0, flat.numel(), CHUNK):
            partials[c] = (flat[lo:lo + CHUNK] ** 2).sum()
            c += 1
    assert c == mtl.n_chunks


def emu_mt_norm_finish(partials, max_norm):
    norm = partials.sum().sqrt() if partials.numel() else torch.zeros((), dtype=torch.float32)
    c = torch.tensor(float(max_norm), dtype=torch.float32) / (norm + 1e-6)
    return torch.stack([norm, torch.where(c > 1.0, torch.ones_like(c), c)])


def pretend_gpu(monkeypatch, count=None, calls=None):
    """ddp_ref.pretend_gpu (optim_ref's four launches and the pack pass) plus the three of this file.  count: launches per name;
    calls: a list that receives (name, args) of the three new ones"""
    from cvvae_amd import ops
    ddp_ref.pretend_gpu(monkeypatch, count)
    for name, fn in (("mt_adamw_master", emu_mt_adamw_master), ("mt_sumsq", emu_mt_sumsq), ("mt_norm_finish", emu_mt_norm_finish)):
        def rec(*a, _n=name, _f=fn, **k):
            if count is not None:
                count[_n] = count.get(_n, 0) + 1
            if calls is not None:
                calls.append((_n, a))
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, rec)


# ---- the edge list in 16 bits ----
def edge_list16(dtype, seed=0):
    """optim_ref.edge_list() with g and p stored in `dtype` (their buffers rounded once; `w_buf`, the master, is the fp32 p buffer
    itself, as unrelated to the 16-bit p as a test can make it), plus the two alignment cases of the 16-bit operands: a view that
    starts 2 bytes into its buffers (off = 1 for g and p), and one whose g is 16-byte aligned while its p starts 2 bytes in.  Every
    entry: n, t, has_grad, per-operand offsets `off[k]`, the fp32 buffers m_buf / v_buf / w_buf and the 16-bit g_buf / p_buf"""
    out = []
    base = optim_ref.edge_list(seed)
    extra = [dict(base[5], _off16=(1, 1), t=7), dict(base[5], _off16=(0, 1), t=2)]   # numel CHUNK + 1: whole groups and a tail
    gen = torch.Generator().manual_seed(seed + 100)
    for j, d in enumerate(base + extra):
        n, off32 = d["n"], d["off"]
        og, op = d.get("_off16", (off32, off32))
        e = {"n": n, "t": d["t"], "has_grad": d["has_grad"], "off": {"g": og, "p": op, "m": off32, "v": off32, "w": off32}}
        for k, src in (("m", "m"), ("v", "v"), ("w", "p")):
            e[k + "_buf"] = d[src + "_buf"].clone()
        for k, o in (("g", og), ("p", op)):
            buf = d[k + "_buf"]
            if j >= len(base):      # the extra entries get values of their own
                buf = optim_ref.log_uniform(buf.shape, gen) if k == "g" else torch.randn(buf.shape, generator=gen)
            need = o + n + optim_ref.GUARD
            if buf.numel() < need:
                buf = torch.cat([buf, buf[:need - buf.numel()]])
            e[k + "_buf"] = buf.to(dtype)
        out.append(e)
    return out


def views16(e, bufs):
    """{g, p, m, v, w}: the views of entry e over (possibly device copies of) its buffers"""
    shape = () if e["n"] == 1 else (e["n"],)
    return {k: bufs[k + "_buf"][e["off"][k]:e["off"][k] + e["n"]].view(shape) for k in ("g", "p", "m", "v", "w")}
