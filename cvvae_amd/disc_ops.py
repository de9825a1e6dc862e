"""The non-convolution layers of the 3-D PatchGAN discriminator (the reference's models/discriminator.py:184-341) as differentiable
functions on NDHWC tensors [B, T, H, W, C] (contiguous, fp16 / bf16 / fp32, C % 8 == 0), each one torch.autograd.Function over the
kernels of csrc/disc_kernels.hip:

  avg_pool_down3d(x)                      ResnetBlockDown3D's downsample (:240-243, :250-253): an odd T gets its first frame duplicated
                                          in front, then avg_pool3d(2, 2)
  group_norm_leaky(x, weight, bias, ...)  Normalize(c) + nn.LeakyReLU(0.2, True) (:316-317, :330-331); weight = bias = None: the bare
                                          LeakyReLU behind the first conv (:302)

The block and network modules are built on these and on the existing conv launches; they are not part of this file.  There is no
CPU path."""
from typing import Optional

import torch

from . import ops


class _AvgPoolDown3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor) -> torch.Tensor:
        ctx.shape = tuple(x.shape)
        with torch.cuda.device(x.device):
            return ops.avgpool3d_down(x.detach())

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        gy = gy.detach().contiguous()
        with torch.cuda.device(gy.device):
            return ops.avgpool3d_down_bwd(gy, ctx.shape)


def avg_pool_down3d(x: torch.Tensor) -> torch.Tensor:
    """x [B, T, H, W, C] -> [B, ceil(T / 2), H // 2, W // 2, C]:  torch.cat([x[:, :1], x], 1) when T is odd, then the 2x2x2 mean.
    The duplicated frame is an index rule of the kernel, never a tensor; the backward is a gather (no atomics)."""
    ops._need_gpu(x)
    if torch.is_grad_enabled() and x.requires_grad:
        return _AvgPoolDown3dFn.apply(x)
    with torch.cuda.device(x.device):
        return ops.avgpool3d_down(x.detach())


class _GroupNormLeakyFn(torch.autograd.Function):
    """Saved for the backward, besides the inputs: the OUTPUT y (the LeakyReLU mask is its sign, as for the reference's in-place
    module) and the two unit statistics tables (rstd, -mean rstd) [B, C] -- not the pre-activation."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], num_groups: int, eps: float,
                slope: float) -> torch.Tensor:
        ctx.slope, ctx.groups = slope, num_groups
        xd = x.detach()
        with torch.cuda.device(x.device):
            if weight is None:
                y = ops.gn_leaky_apply(xd, None, slope)
                ctx.save_for_backward(y)
                return y
            C = x.shape[-1]
            ctx.param_dtypes = (weight.dtype, bias.dtype)
            w = weight.detach().to(torch.float32).contiguous()
            b = bias.detach().to(torch.float32).contiguous()
            # one statistics pass serves both directions: the unit tables are what cvvae_gn_bwd_input takes, and the module's affine is
            # folded into them on [B, C] values for the apply pass (scale = gamma rstd, shift = beta - mean gamma rstd)
            rs, nm = ops.gn_stats(xd, torch.ones(C, dtype=torch.float32, device=x.device),
                                  torch.zeros(C, dtype=torch.float32, device=x.device), eps, groups=num_groups)
            y = ops.gn_leaky_apply(xd, (rs * w, torch.addcmul(b, nm, w)), slope)
        ctx.save_for_backward(y, xd, rs, nm, w, b)
        return y

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        gy = gy.detach().contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        with torch.cuda.device(gy.device):
            if len(ctx.saved_tensors) == 1:
                (y,) = ctx.saved_tensors
                return ops.leaky_bwd(y, gy, ctx.slope), None, None, None, None, None
            y, x, rs, nm, w, b = ctx.saved_tensors
            gv = ops.leaky_bwd(y, gy, ctx.slope)
            if need_w or need_b:
                gx, dw, db = ops.gn_bwd_input_params(x, gv, (rs, nm), w, b, silu=False, groups=ctx.groups)
                wt, bt = ctx.param_dtypes
                return (gx if need_x else None, dw.to(wt) if need_w else None, db.to(bt) if need_b else None, None, None, None)
            return ops.gn_bwd_input(x, gv, (rs, nm), w, b, silu=False, groups=ctx.groups), None, None, None, None, None


def group_norm_leaky(x: torch.Tensor, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, num_groups: int = 32,
                     eps: float = 1e-6, slope: float = 0.2) -> torch.Tensor:
    """leaky_relu(group_norm(x, num_groups, weight, bias, eps), slope) on x [B, T, H, W, C] (statistics per sample over T, H, W and the
    group's channels); num_groups and eps default to the reference's Normalize.  weight = bias = None: leaky_relu(x, slope).
    Gradients for x, weight and bias (fp32 sums, returned in the parameters' dtype)."""
    ops._need_gpu(x)
    if (weight is None) != (bias is None):
        raise ValueError("group_norm_leaky: weight and bias come together (both None: the bare LeakyReLU)")
    if not slope > 0:
        raise ValueError(f"group_norm_leaky: the backward takes its mask from the output, which needs slope > 0; got {slope}")
    return _GroupNormLeakyFn.apply(x, weight, bias, num_groups, eps, slope)
