"""`lvdm.modules.ema.LitEma`: the exponential moving average of a model's trainable parameters, with the constructor, methods, buffer
names and state_dict of the class the training loop imports under this path -- and its update as ONE multi-tensor HIP launch
(include/cvvae.h cvvae_mt_ema) instead of four small launches per parameter and a host synchronisation on `num_updates`.

Buffers: `decay` (fp32), `num_updates` (int32; -1: the decay is used as it is) and one shadow per `requires_grad` parameter, named as
the parameter with the dots removed (`m_name2s_name`); `cvvae_amd/checkpoint.py --ema` reads exactly these keys.

`copy_to` / `restore` write through `.data` (autograd leaves stay untouched) and then move the written parameters' version counters,
as every other writer of a parameter does: the weight caches of cvvae_amd (engine.WeightCache, keyed on `_version`) see the swap
without a checksum pass or `refresh_weights()`.

16-bit models: `LitEma(model, decay, use_num_upates, fp32_shadows=True, masters=None)` keeps the shadow of a bf16 / fp16 parameter in
fp32 -- a clone of `masters[p]` where that mapping (parameter -> fp32 tensor) has one, else `p.float()`; a 16-bit shadow cannot take a
step of (1 - 0.9999)(s - p).  The module's fp32 buffers, `decay` among them (0.9999 is 1.0 in bf16), then stay fp32 through
`.to(dtype)` / `.half()` / `.bfloat16()`; devices still move.  `forward(model, masters=fn)` reads `fn(p)` instead of `p` wherever the
callable returns a tensor (the optimizer's fp32 master weights: cvvae_amd.optim.AdamW.master), so the average follows the weights
the optimizer holds and not their 16-bit roundings; it is the same cvvae_mt_ema launch, on fp32 operands.  Names and keys are as
above.  Without the keyword nothing changes."""
import numpy as np
import torch
from torch import nn

from cvvae_amd import ops


def _on_kernel(p: torch.Tensor, s: torch.Tensor) -> bool:
    return (p.is_cuda and s.is_cuda and p.device == s.device and p.dtype == torch.float32 and s.dtype == torch.float32
            and p.is_contiguous() and s.is_contiguous() and p.shape == s.shape)


class LitEma(nn.Module):
    def __init__(self, model, decay=0.9999, use_num_upates=True, *, fp32_shadows=False, masters=None):
        super().__init__()
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.m_name2s_name = {}
        self.fp32_shadows = bool(fp32_shadows)
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_upates else -1, dtype=torch.int))
        for name, p in model.named_parameters():
            if p.requires_grad:
                s_name = name.replace(".", "")  # '.' is not allowed in buffer names
                self.m_name2s_name[name] = s_name
                if self.fp32_shadows and p.dtype in (torch.bfloat16, torch.float16):
                    seed = None if masters is None else masters.get(p)
                    shadow = p.detach().float() if seed is None else seed.detach().to(device=p.device, dtype=torch.float32, copy=True)
                else:
                    shadow = p.clone().detach().data
                self.register_buffer(s_name, shadow)
        self.collected_params = []
        self._host = None     # (decay as fp32, num_updates) mirrored on the host: forward() never reads the device buffers back
        self._list = None     # (parameter ids, MultiTensorList)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._forget_host())

    def _forget_host(self):
        self._host = None

    def _mirror(self):
        if self._host is None:  # first update, or after load_state_dict / reset_num_updates: ONE read-back
            self._host = [np.float32(self.decay.item()), int(self.num_updates.item())]
        return self._host

    def reset_num_updates(self):
        del self.num_updates
        self.register_buffer("num_updates", torch.tensor(0, dtype=torch.int))
        self._host = None

    def _pairs(self, model):
        shadows = dict(self.named_buffers())
        out = []
        for key, p in model.named_parameters():
            if p.requires_grad:
                out.append((p, shadows[self.m_name2s_name[key]]))
            else:
                assert key not in self.m_name2s_name
        return out

    @torch.no_grad()
    def forward(self, model, masters=None):
        host = self._mirror()
        decay = host[0]
        if host[1] >= 0:
            host[1] += 1
            self.num_updates += 1
            # fp32, as the 0-dim tensors of (1 + num_updates) / (10 + num_updates) and min() are
            decay = min(decay, np.float32(1 + host[1]) / np.float32(10 + host[1]))
        one_minus_decay = float(np.float32(1.0) - decay)
        fused, rest = [], []
        for p, s in self._pairs(model):
            src = masters(p) if masters is not None else None
            pair = (p if src is None else src, s)
            (fused if _on_kernel(*pair) else rest).append(pair)
        if fused and len({p.device for p, _ in fused}) > 1:
            rest, fused = rest + fused, []
        if fused:
            ids = tuple(id(p) for p, _ in fused)
            if self._list is None or self._list[0] != ids:
                self._list = (ids, ops.MultiTensorList([p.numel() for p, _ in fused], fused[0][0].device))
            mtl = self._list[1].set(p=[p for p, _ in fused], shadow=[s for _, s in fused])
            ops.mt_ema(mtl, one_minus_decay)
            torch.autograd.graph.increment_version([s for _, s in fused])
        for p, s in rest:
            s.sub_(one_minus_decay * (s - p.to(s.dtype)))

    def copy_to(self, model):
        written = []
        for p, s in self._pairs(model):
            p.data.copy_(s.data)
            written.append(p)
        torch.autograd.graph.increment_version(written)

    def store(self, parameters):
        """keep a copy of `parameters` (an iterable of nn.Parameter) for restore(): call before copy_to()"""
        self.collected_params = [param.detach().clone() for param in parameters]

    def restore(self, parameters):
        """write the copies store() took back into `parameters` (after validating or saving with the EMA weights)"""
        written = []
        for c_param, param in zip(self.collected_params, parameters):
            param.data.copy_(c_param.data)
            written.append(param)
        torch.autograd.graph.increment_version(written)

    def _apply(self, fn, *args, **kwargs):
        self._list = None  # .to() / .cuda() replace the shadows
        if not self.fp32_shadows:
            return super()._apply(fn, *args, **kwargs)

        def device_only(t):
            out = fn(t)
            if t.dtype == torch.float32 and out.dtype != torch.float32:
                out = t.to(out.device)
            return out
        return super()._apply(device_only, *args, **kwargs)
