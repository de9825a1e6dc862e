"""LPIPS, the perceptual term of the training loss, on the MI355X kernels: forward and input gradient.

Every variant of the reference's loss computes `p_loss = self.perceptual_loss(inputs, reconstructions)` per frame
(lvdm/modules/autoencoding/losses/discriminator_loss.py:252-256, 459-463) with `perceptual_loss = LPIPS().eval()`
(lvdm/modules/autoencoding/lpips/loss/lpips.py): a frozen VGG16 trunk tapped after relu1_2 / 2_2 / 3_3 / 4_3 / 5_3, the taps
channel-normalised, their squared difference weighted by a 1x1 "lin" layer and averaged over the pixels, the five levels summed.

`LPIPS` here carries that module's state-dict layout and runs

  ScalingLayer + NCHW -> NHWC   cvvae_lpips_scale_in (both images into one batch of 2N frames, frames on the descriptor's Ti, kT = 1)
  13 x conv 3x3 (zero pad)      cvvae_conv_fwd, the (1,3,3) family, weights from a WeightCache over this module
  ReLU / MaxPool2d(2, 2)        cvvae_relu (in place) / cvvae_maxpool2x2
  normalise, diff, lin, mean    cvvae_lpips_head, one launch pair per level

and, as ONE autograd node, the input gradient of all of it: cvvae_lpips_head_bwd per level, cvvae_relu_pool_bwd (ReLU backward,
pooling backward and the sum of the two branches in one pass), the convolutions' input gradients on the same conv kernel with
transposed, tap-flipped weights (backward.conv_dgrad), cvvae_lpips_scale_in_bwd.  The trunk is frozen: no weight gradients.
Only the half of the batch whose argument requires a gradient is back-propagated (in the training step: `reconstructions`).

The compute dtype is the parameters' dtype: fp32 modules run as exact split-precision CVVAE_F32, `.half()` / `.bfloat16()` modules on
the 16-bit MFMA; inputs of another dtype are cast on the way in.  torch.autocast is NOT honoured (the kernels are not autocast-aware:
an fp32 module under autocast still computes in fp32).  There is no eager fallback: CPU tensors raise.  The Dropout in front of every
lin layer is the identity, as in `LPIPS().eval()`.

Nothing here reads a URL: the constructor builds the VGG16 trunk itself with default-initialised weights; weights come in through
load_state_dict or from_pretrained(<local file>).
"""
import math
import os
from typing import List, Optional

import torch
import torch.nn as nn

from . import ops
from .backward import conv_dgrad
from .engine import P2D, ZERO, WeightCache

K2D = (1, 3, 3)
CPAD_IN = ops.kchunk(K2D)  # the 3 image channels padded to the first conv's K-chunk (zero weights)
CHNS = (64, 128, 256, 512, 512)
# torchvision's vgg16().features indices, cut into the reference's five slices (lpips.py:103-118): (slice, starts with a pool, convs)
PLAN = (("slice1", False, (0, 2)), ("slice2", True, (5, 7)), ("slice3", True, (10, 12, 14)), ("slice4", True, (17, 19, 21)),
        ("slice5", True, (24, 26, 28)))


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.Tensor([-0.030, -0.088, -0.188])[None, :, None, None])
        self.register_buffer("scale", torch.Tensor([0.458, 0.448, 0.450])[None, :, None, None])


class NetLinLayer(nn.Module):
    """a 1x1 conv C -> 1 without bias behind a Dropout (index 0 of `model` when use_dropout, so the weight is `model.1.weight`)"""

    def __init__(self, chn_in: int, chn_out: int = 1, use_dropout: bool = False):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*layers)


class vgg16(nn.Module):
    """parameter holder with torchvision's VGG16 `features` numbering; the layers are never called (the launches are in _trunk)"""

    def __init__(self):
        super().__init__()
        cin = 3
        for k, (name, pool, convs) in enumerate(PLAN):
            seq = nn.Sequential()
            if pool:
                seq.add_module(str(convs[0] - 1), nn.MaxPool2d(kernel_size=2, stride=2))
            for i in convs:
                seq.add_module(str(i), nn.Conv2d(cin, CHNS[k], kernel_size=3, padding=1))
                seq.add_module(str(i + 1), nn.ReLU(inplace=True))
                cin = CHNS[k]
            setattr(self, name, seq)
        self.N_slices = 5


def _trunk_level(wc: WeightCache, h: torch.Tensor, k: int, tape: Optional[list]) -> torch.Tensor:
    """slice k of the trunk on [1, frames, H, W, C]: (pool,) then conv + ReLU per layer; tape receives every ReLU output"""
    name, pool, convs = PLAN[k]
    if pool:
        h = ops.maxpool2x2(h)
    ys = []
    for i in convs:
        h = ops.relu_(ops.conv(h, wc.conv(f"net.{name}.{i}", K2D, cin_pad=CPAD_IN if i == 0 else None), pad=P2D, pad_mode_hw=ZERO))
        ys.append(h)
    if tape is not None:
        tape.append(ys)
    return h


def _forward(m: "LPIPS", x0: torch.Tensor, x1: torch.Tensor, tape: Optional[list]) -> torch.Tensor:
    """LPIPS.forward (lpips.py:46-64) -> fp32 [N]; tape: a list that receives the ReLU outputs the backward reads again"""
    wc, cd = m._cache(), m.compute_dtype
    N, _, H, W = x0.shape
    shift, scale = m._affine()
    h = torch.empty((1, 2 * N, H, W, CPAD_IN), dtype=cd, device=x0.device)
    ops.lpips_scale_in(x0, shift, scale, CPAD_IN, cd, out=h[0, :N])
    ops.lpips_scale_in(x1, shift, scale, CPAD_IN, cd, out=h[0, N:])
    val = torch.zeros(N, dtype=torch.float32, device=x0.device)
    for k in range(len(PLAN)):
        h = _trunk_level(wc, h, k, tape)
        ops.lpips_head(h[0, :N], h[0, N:], m._lin_w(k), val)
    return val


def _backward(m: "LPIPS", tape: List[list], gout: torch.Tensor, need0: bool, need1: bool) -> torch.Tensor:
    """gout fp32 [N] -> the gradient w.r.t. the scaled NHWC input of the frames that need one: [1, F, H, W, 8] (first 3 channels),
    F = 2N (both arguments), or N (frames [0, N) = `input`, or [N, 2N) = `target`)"""
    wc = m._cache()
    N = gout.numel()
    lo, F = (0, 2 * N) if (need0 and need1) else ((0, N) if need0 else (N, N))
    g = None  # gradient w.r.t. the pooled output of the level below the one being walked
    for k in range(len(PLAN) - 1, -1, -1):
        name, _, convs = PLAN[k]
        ys = tape[k]
        y = ys[-1]
        gt = torch.empty((1, F, *y.shape[2:]), dtype=y.dtype, device=y.device)
        g0 = gt[0, :N] if need0 else None
        g1 = gt[0, F - N:] if need1 else None
        ops.lpips_head_bwd(y[0, :N], y[0, N:], m._lin_w(k), gout, g0, g1)
        for j in range(len(convs) - 1, -1, -1):
            yj = ys[j][:, lo:lo + F]
            g = ops.relu_pool_bwd(yj, gt, g) if j == len(convs) - 1 else ops.relu_pool_bwd(yj, g, None)
            first = convs[j] == 0  # 64 -> 3 channels: stored with 8 (16-byte pixels), channels 3.. zero
            g = conv_dgrad(wc, g, f"net.{name}.{convs[j]}", K2D, P2D, cout_pad=8 if first else None)
    return g


class _LPIPSFn(torch.autograd.Function):
    """(input, target) -> LPIPS value with the frozen network's input gradient as backward, both on the HIP kernels"""

    @staticmethod
    def forward(ctx, x0: torch.Tensor, x1: torch.Tensor, m: "LPIPS") -> torch.Tensor:
        tape: List[list] = []
        with torch.cuda.device(x0.device):
            val = _forward(m, x0.detach(), x1.detach(), tape)
        ctx.m, ctx.tape = m, tape
        ctx.dts = (x0.dtype, x1.dtype)
        return val.view(-1, 1, 1, 1).to(m.compute_dtype)

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        m, tape = ctx.m, ctx.tape
        need0, need1 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        N = gout.shape[0]
        # The spatial means put a factor 1 / (H W) on every gradient of the chain (1e-5 and below at training sizes): under fp16's
        # smallest normal in a 16-bit module, and under the range where the split-precision convs of an fp32 module can represent
        # the fp16 lo half of their operand.  The chain is linear in gout, so it runs on gout * 2^k (k = ceil(log2(H W)), exact)
        # and the last pass divides by scale * 2^k instead of scale.
        H, W = tape[0][0].shape[2:4]
        up = float(2 ** math.ceil(math.log2(H * W)))
        with torch.cuda.device(gout.device):
            g = _backward(m, tape, (gout.reshape(N).to(torch.float32) * up).contiguous(), need0, need1)
            scale = m._affine()[1] * up
            g0 = g1 = None
            if need0:
                g0 = ops.lpips_scale_in_bwd(g[0, :N], scale, ctx.dts[0])
            if need1:
                g1 = ops.lpips_scale_in_bwd(g[0, g.shape[1] - N:], scale, ctx.dts[1])
        return g0, g1, None


class LPIPS(nn.Module):
    """Learned perceptual metric: drop-in for lvdm.modules.autoencoding.lpips.loss.lpips.LPIPS (same state-dict layout, same
    forward(input, target) -> [N,1,1,1]) on the HIP kernels.  `use_dropout` only decides whether the lin weight is `model.1.weight`
    (True, the reference's default) or `model.0.weight`; the Dropout itself is the identity, as in eval()."""

    def __init__(self, use_dropout: bool = True):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.chns = list(CHNS)
        self.net = vgg16()
        for k, c in enumerate(CHNS):
            setattr(self, f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        for p in self.parameters():
            p.requires_grad = False
        self._lin_idx = 1 if use_dropout else 0
        self._wc: Optional[WeightCache] = None
        self._aux: dict = {}

    @classmethod
    def from_pretrained(cls, path: str, use_dropout: bool = True) -> "LPIPS":
        """weights from a LOCAL checkpoint file (the reference's vgg.pth layout); a missing file is an error -- nothing is downloaded"""
        if not isinstance(path, (str, os.PathLike)) or not os.path.isfile(path):
            raise FileNotFoundError(f"LPIPS.from_pretrained: no such file: {path!r} (weights are never downloaded; pass a local checkpoint)")
        model = cls(use_dropout=use_dropout)
        model.load_state_dict(torch.load(path, map_location=torch.device("cpu"), weights_only=True), strict=False)
        return model

    @property
    def compute_dtype(self) -> torch.dtype:
        return self.net.slice1[0].weight.dtype

    def _cache(self) -> WeightCache:
        if self._wc is None:
            self._wc = WeightCache(self)
        return self._wc

    def _f32(self, tag: str, t: torch.Tensor) -> torch.Tensor:
        """flat fp32 copy of a small tensor, remade when its source moves or changes"""
        key = (t.data_ptr(), t._version, t.dtype, t.device)
        hit = self._aux.get(tag)
        if hit is None or hit[0] != key:
            hit = self._aux[tag] = (key, t.detach().to(torch.float32).reshape(-1).contiguous())
        return hit[1]

    def _affine(self):
        return self._f32("shift", self.scaling_layer.shift), self._f32("scale", self.scaling_layer.scale)

    def _lin_w(self, k: int) -> torch.Tensor:
        return self._f32(f"lin{k}", getattr(self, f"lin{k}").model[self._lin_idx].weight)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        ops._need_gpu(input)
        ops._need_gpu(target)
        if input.dim() != 4 or input.shape != target.shape or input.shape[1] != 3:
            raise ValueError(f"LPIPS takes two [N,3,H,W] tensors of one shape; got {tuple(input.shape)} and {tuple(target.shape)}")
        if min(input.shape[2:]) < 16:
            raise ValueError("LPIPS: the VGG16 trunk pools four times; H and W must be at least 16")
        if torch.is_grad_enabled() and (input.requires_grad or target.requires_grad):
            return _LPIPSFn.apply(input, target, self)
        with torch.cuda.device(input.device):
            val = _forward(self, input.detach(), target.detach(), None)
        return val.view(-1, 1, 1, 1).to(self.compute_dtype)
