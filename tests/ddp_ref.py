"""References for the data-parallel tests (cvvae_amd/ddp.py): the torch emulation of the pack pass (signature of cvvae_amd.ops.mt_pack,
the arithmetic include/cvvae.h documents), the expected synchronised gradient formed on the host in fp32 -- no fp64 anywhere: the
exchange is compared bit for bit -- the value classes the GPU pack test mixes in, and small helpers of the process-spawning tests."""
import hashlib
import socket

import torch

from tests import optim_ref


def emu_mt_pack(mtl, divisor):
    d = torch.tensor(float(divisor), dtype=torch.float32)
    for g, s in zip(mtl.tensors["g"], mtl.tensors["shadow"]):
        if g is None:
            s.zero_()
        else:
            s.copy_(torch.div(g.detach(), d).view(s.shape))


def pretend_gpu(monkeypatch, count=None):
    """optim_ref.pretend_gpu plus the pack pass: CPU tensors take the kernel path of GradientSync and of the optimizer"""
    from cvvae_amd import ops
    optim_ref.pretend_gpu(monkeypatch, count)

    def rec(*a, **k):
        if count is not None:
            count["mt_pack"] = count.get("mt_pack", 0) + 1
        return emu_mt_pack(*a, **k)
    monkeypatch.setattr(ops, "mt_pack", rec)


def mean_in_rank_order(per_rank):
    """per_rank[r][i]: rank r's fp32 gradient of parameter i (or None) -> sum_r(g_r / world), each quotient a correctly rounded fp32
    division, the sum formed in rank order in fp32; None where no rank has a gradient"""
    world = len(per_rank)
    d = torch.tensor(float(world), dtype=torch.float32)
    out = []
    for gs in zip(*per_rank):
        if all(g is None for g in gs):
            out.append(None)
            continue
        like = next(g for g in gs if g is not None)
        acc = None
        for g in gs:
            q = torch.zeros_like(like) if g is None else torch.div(g, d.to(g.dtype))
            acc = q if acc is None else acc + q
        out.append(acc)
    return out


def magnitude(per_rank):
    """sum_r |g_r / world| per parameter: the scale at which a sum in another order may differ (by one rounding of a partial sum)"""
    world = len(per_rank)
    return [None if all(g is None for g in gs) else sum(torch.div(g, float(world)).abs() for g in gs if g is not None)
            for gs in zip(*per_rank)]


def special_values(n, gen):
    """n fp32 values: log-uniform magnitudes over 1e-30 ... 1e30 with every 16th element one of +-0, denormals, +-inf, NaN"""
    x = optim_ref.log_uniform((n,), gen, 1e-30, 1e30)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 5.9e-39, -1.1e-38, float("inf"), float("-inf"), float("nan"),
                            1.17549435e-38, 3.4028234e38, -3.4028234e38], dtype=torch.float32)
    idx = torch.arange(0, n, 16)
    x[idx] = special[torch.arange(idx.numel()) % special.numel()]
    return x


def same_bits_or_both_nan(a, b):
    """bit-equal, where a NaN matches any NaN (the bit pattern CLASS: a quotient's NaN payload is the hardware's choice)"""
    a, b = a.detach().cpu().contiguous().view(-1), b.detach().cpu().contiguous().view(-1)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = torch.isnan(a)
    if not torch.equal(nan, torch.isnan(b)):
        return False
    return torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32))


def digest(tensors):
    """one sha256 over the bytes of every tensor of {name: tensor}, in name order -> {name: hex}"""
    out = {}
    for k in sorted(tensors):
        t = tensors[k].detach().cpu().contiguous()
        out[k] = hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes() + str((t.dtype, tuple(t.shape))).encode()).hexdigest()
    return out


def engine_state(e):
    """everything a replica must share after an iteration: parameters, both optimizers' state, the EMA buffers"""
    out = {"p:" + n: p for n, p in e.named_parameters()}
    if hasattr(e, "model_ema"):
        out.update({"ema:" + n: b for n, b in e.model_ema.named_buffers()})
    for i, opt in enumerate(e.optimizers()):
        for j, p in enumerate(p for g in opt.param_groups for p in g["params"]):
            for k, v in opt.state.get(p, {}).items():
                out[f"opt{i}:{j}:{k}"] = v if torch.is_tensor(v) else torch.tensor(v)
    return out


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p
