"""References for the wide-gradient tests (cvvae_amd/ddp.py GradientSync(wide_gradients=True), cvvae_amd/optim.py `main_grad`): torch
emulations of the two wrappers cvvae_amd.ops.mt_pack_wide / mt_adamw_master_wide (the arithmetic include/cvvae.h documents),
`pretend_gpu` = the one of tests/master_ref.py plus these two, the special values of the 16-bit formats that the GPU pack test mixes
in, and the expected synchronised gradient of 16-bit per-rank gradients, formed on the host in fp32."""
import torch

from tests import ddp_ref, master_ref, optim_ref

DTYPES16 = master_ref.DTYPES16


# ---- emulations (signatures of cvvae_amd.ops.mt_pack_wide / mt_adamw_master_wide) ----
def emu_mt_pack_wide(mtl, divisor):
    """ddp_ref.emu_mt_pack on float(g): the widening is exact, the quotient one fp32 division"""
    assert mtl.dtype in DTYPES16
    d = torch.tensor(float(divisor), dtype=torch.float32)
    for g, s in zip(mtl.tensors["g"], mtl.tensors["shadow"]):
        assert s.dtype == torch.float32
        if g is None:
            s.zero_()
        else:
            assert g.dtype == mtl.dtype
            s.copy_(torch.div(g.detach().float(), d).view(s.shape))


def emu_mt_adamw_master_wide(mtl, lr, beta1, beta2, eps, weight_decay, coef=None):
    """master_ref.emu_mt_adamw_master with g in fp32: optim_ref.emu_mt_adamw on (g, master, m, v), then p <- master rounded (copy_)"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731 -- a double rounded to fp32 once
    t = mtl.tensors
    assert mtl.dtype in DTYPES16
    for g, p, m, v, w, ss, b2 in zip(t["g"], t["p"], t["m"], t["v"], t["shadow"], mtl.step_size, mtl.bias2_sqrt):
        assert p.dtype == mtl.dtype and g.dtype == m.dtype == v.dtype == w.dtype == torch.float32
        G = g.detach()
        if coef is not None:
            G = G * coef.reshape(())
        m.copy_(f(beta1) * m + f(1.0 - beta1) * G)
        v.copy_(f(beta2) * v + f(1.0 - beta2) * (G * G))
        denom = v.sqrt() / f(b2) + f(eps)
        w.copy_(w * f(1.0 - lr * weight_decay) - f(ss) * (m / denom))
        p.detach().copy_(w)


def pretend_gpu(monkeypatch, count=None, calls=None):
    """master_ref.pretend_gpu (every launch of the update and the fp32 pack pass) plus the two of this file.  count: launches per
    name; calls: a list that receives (name, args) of master_ref's three and of these two"""
    from cvvae_amd import ops
    master_ref.pretend_gpu(monkeypatch, count, calls)
    for name, fn in (("mt_pack_wide", emu_mt_pack_wide), ("mt_adamw_master_wide", emu_mt_adamw_master_wide)):
        def rec(*a, _n=name, _f=fn, **k):
            if count is not None:
                count[_n] = count.get(_n, 0) + 1
            if calls is not None:
                calls.append((_n, a))
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, rec)


# ---- the values of the GPU pack test ----
def special_values16(n, dtype, gen):
    """n values of `dtype`: log-uniform magnitudes over the format's normal range, with every 8th element one of +-0, +-inf, NaN, the
    smallest and a larger subnormal of either sign, and the smallest and largest normals of either sign"""
    fi = torch.finfo(dtype)
    x = optim_ref.log_uniform((n,), gen, 4.0 * fi.tiny, 0.25 * fi.max).to(dtype)
    sub = fi.tiny * fi.eps       # the smallest subnormal: 2^-133 (bf16), 2^-24 (fp16) -- both exact in fp32
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), sub, -sub, 5.0 * sub, -3.0 * sub,
                            fi.tiny, -fi.tiny, fi.max, -fi.max], dtype=torch.float32).to(dtype)
    assert float(special[5]) == sub and float(special[11]) == fi.max        # representable: the conversion rounded nothing away
    idx = torch.arange(0, n, 8)
    x[idx] = special[torch.arange(idx.numel()) % special.numel()]
    return x


def mean_in_rank_order16(per_rank):
    """per_rank[r][i]: rank r's gradient of parameter i in its own dtype (or None) -> sum_r(float(g_r) / world), each quotient a
    correctly rounded fp32 division, added in rank order in fp32: ddp_ref.mean_in_rank_order on the widened gradients"""
    return ddp_ref.mean_in_rank_order([[None if g is None else g.float() for g in gs] for gs in per_rank])
