"""The 3-D PatchGAN discriminator of the training loss (the reference's models/discriminator.py:184-347) as a trainable module on the
MI355X kernels.

`NLayerDiscriminator3D` / `ResnetBlockDown3D` keep the reference's constructor signatures, defaults and module tree (real nn.Conv3d /
nn.GroupNorm(32, c, eps=1e-5) / nn.Linear / nn.LeakyReLU containers), so `state_dict()` keys and shapes are the reference's,
`.apply(weights_init)` and `load_state_dict` of a reference checkpoint work unchanged, and the unused `temb_proj` is there.

  CPU tensor   plain eager torch over those containers (so the module can be checked without a GPU; the GPU path never uses it).
  GPU tensor   [B, 3, T, H, W] -> logits [B, 1, T', H', W'] in the parameters' dtype (fp16 / bf16 / fp32), on NDHWC tensors through
               engine.WeightCache.  Every Normalize takes its tables from the GroupNorm records of its producer (ops.gn_finalize), never
               from a statistics pass of its own:
                 main.0         conv 3 -> ndf, stride 2 (no prologue), then the bare LeakyReLU pass in place with gn_out = 32 (the 64-channel
                                width the conv epilogue's 4-channel record slots cannot serve)
                 each block     conv1 with the GroupNorm + SiLU prologue; downsampling blocks: avgpool3d_down(h, gn_out = 32), the others:
                                conv1 itself with gn_out = 32; conv2 with the prologue, residual = the shortcut branch, gn_out = 32;
                                shortcut = nin_shortcut(avgpool3d_down(x)) / nin_shortcut(x) / x
                 between        gn_leaky_apply(tables, gn_out = 32), the last one without records
                 main.14        conv 512 -> 1, stored NCDHW
               A nin_shortcut whose Cin is no multiple of the 1x1x1 family's 128-channel chunk (main.2: 64) runs as a per-frame (1,3,3)
               conv whose only non-zero tap is the centre (chunk 32): 9x the MFMAs of a 1x1, on a tensor of T/4 x H/4 x W/4 pixels.

Training: ONE autograd node over the input and the parameters (`DiscFn`), a tape and a backward walker over backward.py's helpers.
It honours needs_input_grad -- a detached input (the discriminator step) skips the first layer's input gradient, frozen parameters skip
every weight-gradient / affine-sum launch --, gives `temb_proj.*` None, survives two backward calls (the loss asks
torch.autograd.grad(g_loss, last_layer, retain_graph=True) before backward()), and returns parameter gradients accumulated in fp32 in
the parameters' dtype.  The first layer's input gradient (the generator step: 64 -> 3 channels at stride 2) is the direct gather
kernel ops.conv333_s2_dgrad_small; every other conv is at stride 1 with zero padding, whose input gradient is the forward kernel
over the tap-flipped, transposed weights with the same padding.  `torch.no_grad()` and `eval()` run the forward without a tape
(an input that requires a gradient in eval() under grad mode raises instead of losing it silently).  The packed weights follow
optimizer steps, load_state_dict and .to() through the parameters' versions; unlike the codec's inference passes, no pass here runs
WeightCache.guard(), so a write through `.data` needs `net._cache().invalidate()`.
Not supported: use_actnorm / causal / half_3d / conv_shortcut (NotImplementedError at construction; the shipped config uses none),
and an fp32 module on 16-bit launches under torch.autocast (the module runs in its parameters' dtype)."""
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import backward, engine, grad3d, ops
from .backward import K1, backward_pass, begin_node, block_names, conv_dgrad, conv_param_grads, gn_backward, node_grads, taped, unit_tabs
from .engine import G32, P1, P2D, ZERO, WeightCache
from .grad3d import K133, K333
from .loss import weights_init

EPS = 1e-5      # Normalize of models/vae_models.py (the codec's own norms elsewhere in this package use 1e-6)
SLOPE = 0.2
S2 = (2, 2, 2)
GEOM = dict(pad=P1, pad_mode_t=ZERO, pad_mode_hw=ZERO)   # every conv of the network but its first: stride 1, zero padding 1

# the first layer's input gradient: the direct gather kernel (True) or grad3d.dgrad333's zero-stuffed MFMA path (False).  At the
# training clip [1,3,17,256,256] on an MI355X the gather kernel takes 82 us in bf16 and 147 us in fp32, the zero-stuffed path 384 us
# and 1130 us (tools/disc_step.py, profiles/disc_net.json)
DIRECT_FIRST_DGRAD = True


def Normalize(in_channels: int) -> nn.GroupNorm:
    return nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=EPS, affine=True)


def _pool_ref(x: torch.Tensor) -> torch.Tensor:
    """discriminator.py:240-243 on NCDHW"""
    if x.shape[2] % 2 == 1:
        x = torch.cat([x[:, :, :1], x], dim=2)
    return F.avg_pool3d(x, kernel_size=2, stride=2)


# --------------------------------------------------------------------------------------------------------
# the launch programs (NDHWC).  `pre`: a block's parameter prefix with its trailing dot ("main.2.", or "" for a block on its own)
# --------------------------------------------------------------------------------------------------------
def _nin(wc: WeightCache, x: torch.Tensor, name: str) -> torch.Tensor:
    """nin_shortcut (1x1x1).  Cin a multiple of 128: the 1x1x1 family; else (Cin = 64) the centre tap of a per-frame (1,3,3) conv"""
    w = wc.p(name + ".weight")
    if w.shape[1] % ops.kchunk(K1) == 0:
        return engine.conv1x1(wc, x, name)
    if w.shape[1] % ops.kchunk(K133):
        raise NotImplementedError(f"{name}: {w.shape[1]} input channels are no multiple of {ops.kchunk(K133)}")

    def centre133(w, b):
        w9 = torch.zeros((w.shape[0], w.shape[1], 9), dtype=w.dtype, device=w.device)
        w9[:, :, 4] = w.detach().reshape(w.shape[0], w.shape[1])
        return ops.pack_weight(w9, b.detach(), K133)
    pw = wc.cached(name + "#centre133", (name + ".weight", name + ".bias"), centre133)
    return ops.conv(x, pw, pad=P2D, pad_mode_hw=ZERO)


def block_forward(wc: WeightCache, x: torch.Tensor, xp, pre: str, down: bool, tape: Optional[list] = None, gn_out: int = G32):
    """ResnetBlockDown3D.forward (discriminator.py:231-261, temb = None, dropout 0) on x NDHWC with the GroupNorm records xp of x
    (None: a statistics pass -- a block run on its own has no producer).  Returns (y, records of y or None)."""
    n1 = wc.norm(pre + "norm1")
    g1 = ops.gn_finalize(xp, *n1, EPS) if xp is not None else ops.gn_stats(x, *n1, EPS)
    kw = dict(pad=P1, pad_mode_t=ZERO, pad_mode_hw=ZERO, prologue=L.PRO_GN_SILU)
    if down:
        h = engine.conv3(wc, x, pre + "conv1", gn=g1, act_norm=pre + "norm1", **kw)
        h_shape = tuple(h.shape)
        hq, hp = ops.avgpool3d_down(h, gn_out=G32)
        del h
        xs = ops.avgpool3d_down(x)
    else:
        hq, hp = engine.conv3(wc, x, pre + "conv1", gn=g1, act_norm=pre + "norm1", gn_out=G32, **kw)
        h_shape = tuple(hq.shape)
        xs = x
    g2 = ops.gn_finalize(hp, *wc.norm(pre + "norm2"), EPS)
    has_nin = wc.has(pre + "nin_shortcut.weight")
    sc = _nin(wc, xs, pre + "nin_shortcut") if has_nin else xs
    if tape is not None:
        tape.append(dict(op="block", pre=pre, x=x, xp=xp, g1=g1, h_shape=h_shape, hq=hq, hp=hp, g2=g2, xs=xs if has_nin else None,
                         down=down))
    y = engine.conv3(wc, hq, pre + "conv2", gn=g2, act_norm=pre + "norm2", residual=sc, gn_out=gn_out, **kw)
    return y if gn_out else (y, None)


def disc_forward(wc: WeightCache, x: torch.Tensor, layout: List[Tuple[str, int, bool]], tape: Optional[list] = None) -> torch.Tensor:
    """NLayerDiscriminator3D.forward: x NCDHW -> logits NCDHW.  layout: the Sequential's entries as (kind, index, downsample)."""
    dtype = wc.p("main.0.weight").dtype
    cin = wc.p("main.0.weight").shape[1]
    cpad = ops.round_up(cin, ops.kchunk(K333))
    xin = ops.ncdhw_to_ndhwc(x, cpad, dtype)
    h = ops.conv(xin, wc.conv("main.0", K333, cin_pad=cpad), stride=S2, pad=P1, pad_mode_t=ZERO, pad_mode_hw=ZERO)
    h, hp = ops.gn_leaky_apply(h, None, SLOPE, out=h, gn_out=G32)     # (in place: the backward's mask is the output's sign)
    if tape is not None:
        tape.append(dict(op="first", x=xin, y=h, in_shape=(x.shape[0], x.shape[2], x.shape[3], x.shape[4]), cin=cin))
    acts = [i for kind, i, _ in layout if kind == "act"]
    for kind, i, down in layout:
        if kind == "block":
            h, hp = block_forward(wc, h, hp, f"main.{i}.", down, tape)
        elif kind == "act":     # Normalize + LeakyReLU behind a block
            tabs = ops.gn_finalize(hp, *wc.norm(f"main.{i}"), EPS)
            last = i == acts[-1]
            a = ops.gn_leaky_apply(h, tabs, SLOPE, gn_out=0 if last else G32)
            a, ap = (a, None) if last else a
            if tape is not None:
                tape.append(dict(op="act", name=f"main.{i}", x=h, xp=hp, y=a))
            h, hp = a, ap
        else:                   # the 1-channel prediction map
            if tape is not None:
                tape.append(dict(op="last", name=f"main.{i}", x=h))
            return engine.conv3(wc, h, f"main.{i}", pad=P1, pad_mode_t=ZERO, pad_mode_hw=ZERO, out_mode=L.OUT_NCDHW)
    raise AssertionError("layout without a last conv")


# --------------------------------------------------------------------------------------------------------
# the backward walker
# --------------------------------------------------------------------------------------------------------
def first_layer_dgrad(wc: WeightCache, gv: torch.Tensor, in_shape, cin: int, direct: Optional[bool] = None) -> torch.Tensor:
    """dL/d(input) [B,T,H,W,8] of main.0 (stride 2) given gv = dL/d(its output): the gather kernel, or grad3d.dgrad333's
    zero-stuffed path"""
    if DIRECT_FIRST_DGRAD if direct is None else direct:
        tab = wc.cached("main.0#dgrad_small", ("main.0.weight",), ops.dgrad_small_table)
        return ops.conv333_s2_dgrad_small(gv, tab, in_shape, cin)
    return grad3d.dgrad333(wc, gv, "main.0", P1, ZERO, ZERO, tuple(in_shape), stride=S2)


def block_backward(wc: WeightCache, g: torch.Tensor, e: dict, grads: Optional[Dict[str, torch.Tensor]]) -> torch.Tensor:
    """g = dL/dy of block_forward -> dL/dx; the block's parameter gradients into `grads` (None: frozen).  Both convs are 3x3x3 at
    stride 1 with zero padding 1; a downsampling block goes back through the pool's adjoint on both branches."""
    pre = e["pre"]
    return backward.resnet_backward(
        wc, g, grads, block_names(wc, pre, "nin_shortcut"), e["x"], e["xp"], e["hq"], e["hp"], EPS, gn1=e["g1"], gn2=e["g2"],
        sc_x=e["xs"], h_shape=e["h_shape"] if e["down"] else None, conv1=(K333, GEOM), conv2=(K333, P1),
        dgrad1=lambda gh: conv_dgrad(wc, gh, pre + "conv1", K333, P1))


def disc_backward(wc: WeightCache, tape: List[dict], gy: torch.Tensor, need_input_grad: bool, need_params: bool):
    """gy = dL/d(logits) NCDHW -> (dL/d(input) NCDHW or None, {parameter name: fp32 gradient})"""
    grads: Optional[Dict[str, torch.Tensor]] = {} if need_params else None
    dtype = wc.p("main.0.weight").dtype
    gx = g = None
    for e in reversed(tape):
        if e["op"] == "last":
            g = ops.ncdhw_to_ndhwc(gy.contiguous(), ops.kchunk(K333), dtype)          # [B,T',H',W',16], channels 1.. zero
            conv_param_grads(wc, grads, e["name"], e["x"], g, K333, **GEOM)
            g = conv_dgrad(wc, g, e["name"], K333, P1)
        elif e["op"] == "act":
            gv = ops.leaky_bwd(e["y"], g, SLOPE)
            g = gn_backward(grads, e["name"], e["x"], gv, unit_tabs(e["x"], e["xp"], EPS), wc.norm(e["name"]), False)
        elif e["op"] == "block":
            g = block_backward(wc, g, e, grads)
        elif e["op"] == "first":
            if grads is None and not need_input_grad:
                continue
            gv = ops.leaky_bwd(e["y"], g, SLOPE)
            conv_param_grads(wc, grads, "main.0", e["x"], gv, K333, stride=S2, **GEOM)
            if need_input_grad:
                gx = ops.ndhwc_to_ncdhw(first_layer_dgrad(wc, gv, e["in_shape"], e["cin"]), e["cin"])
        else:
            raise AssertionError(e["op"])
    return gx, (grads if grads is not None else {})


class DiscFn(torch.autograd.Function):
    """(x, *parameters) -> logits; the tape is kept until autograd frees the node, so a second backward (retain_graph) walks the
    same tape and gives the same bits"""

    @staticmethod
    def forward(ctx, x: torch.Tensor, net, names: Tuple[str, ...], *params) -> torch.Tensor:
        y, ctx.tape = taped(x, lambda tape: disc_forward(net._cache(), x.detach(), net._layout, tape))
        begin_node(ctx, net, x, names, params)
        return y

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        with backward_pass(ctx, gy) as grads:
            gx, grads = disc_backward(ctx.net._cache(), ctx.tape, gy, ctx.need_x, grads is not None)
        return node_grads(ctx, gx, 2, grads)


# --------------------------------------------------------------------------------------------------------
# the modules
# --------------------------------------------------------------------------------------------------------
class ResnetBlockDown3D(nn.Module):
    """discriminator.py:184-261.  forward(x NCDHW): eager torch on a CPU tensor; on a GPU tensor the block's launch program on its own
    (inference only: its GroupNorm statistics come from a pass, there is no producer; training goes through the network's node)."""

    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout, temb_channels=512, half_3d=True, causal=False,
                 downsample=True):
        super().__init__()
        if half_3d or causal or conv_shortcut:
            raise NotImplementedError("ResnetBlockDown3D: half_3d=True (Conv2dWithExtraDim), causal=True (CausalConv3d) and "
                                      "conv_shortcut=True are not built; NLayerDiscriminator3D's shipped configuration uses none of them")
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = conv_shortcut
        self.norm1 = Normalize(in_channels)
        self.conv1 = nn.Conv3d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.downsample = downsample
        if temb_channels > 0:
            self.temb_proj = nn.Linear(temb_channels, out_channels)
        self.norm2 = Normalize(out_channels)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = nn.Conv3d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            self.nin_shortcut = nn.Conv3d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)
        self._wc: Optional[WeightCache] = None

    def _cache(self) -> WeightCache:
        if self._wc is None:
            self._wc = WeightCache(self)
        return self._wc

    def forward(self, x, temb=None):
        if x.is_cuda:
            if temb is not None:
                raise NotImplementedError("ResnetBlockDown3D on the GPU: temb is not used by the discriminator and not built")
            if torch.is_grad_enabled() and x.requires_grad:
                raise RuntimeError("ResnetBlockDown3D on its own runs on the GPU without a tape and would drop the input's gradient: call "
                                   "it under torch.no_grad(), or train through NLayerDiscriminator3D")
            with torch.cuda.device(x.device), torch.no_grad():
                dtype = self.conv1.weight.dtype
                xin = ops.ncdhw_to_ndhwc(x.detach(), self.in_channels, dtype)
                y, _ = block_forward(self._cache(), xin, None, "", self.downsample, gn_out=0)
                return ops.ndhwc_to_ncdhw(y, self.out_channels)
        return self.forward_eager(x, temb)

    def forward_eager(self, x, temb=None):
        """the block as plain torch ops on x NCDHW, any device (the CPU path; on a GPU: the eager baseline of tools/disc_step.py)"""
        h = self.conv1(F.silu(self.norm1(x)))
        if temb is not None:
            h = h + self.temb_proj(F.silu(temb))[:, :, None, None]
        if self.downsample:
            h = _pool_ref(h)
        h = self.conv2(self.dropout(F.silu(self.norm2(h))))
        if self.downsample:
            x = _pool_ref(x)
        if self.in_channels != self.out_channels:
            x = self.nin_shortcut(x)
        return x + h


class NLayerDiscriminator3D(nn.Module):
    """discriminator.py:264-341: conv(stride 2) + LeakyReLU, n_layers - 2 downsampling ResnetBlockDown3D, two more without
    downsampling, each followed by Normalize + LeakyReLU, then the 1-channel prediction conv."""

    def __init__(self, input_nc=3, ndf=64, n_layers=4, use_actnorm=False, half_3d=False, causal=False):
        super().__init__()
        if use_actnorm or half_3d or causal:
            raise NotImplementedError("NLayerDiscriminator3D: use_actnorm=True, half_3d=True and causal=True are not built "
                                      "(the shipped training configuration uses none of them)")
        sequence: List[nn.Module] = [nn.Conv3d(input_nc, ndf, kernel_size=3, stride=2, padding=1), nn.LeakyReLU(SLOPE, True)]
        layout: List[Tuple[str, int, bool]] = []
        nf_mult = 1
        plan = [(min(2 ** n, 8), True) for n in range(1, n_layers - 1)] + [(min(2 ** n_layers, 8), False)] * 2
        for mult, down in plan:
            nf_mult_prev, nf_mult = nf_mult, mult
            layout += [("block", len(sequence), down), ("act", len(sequence) + 1, False)]
            sequence += [ResnetBlockDown3D(in_channels=ndf * nf_mult_prev, out_channels=ndf * nf_mult, half_3d=half_3d, dropout=0.0,
                                           downsample=down),
                         Normalize(ndf * nf_mult), nn.LeakyReLU(SLOPE, True)]
        layout.append(("last", len(sequence), False))
        sequence += [nn.Conv3d(ndf * nf_mult, 1, kernel_size=3, stride=1, padding=1)]
        self.main = nn.Sequential(*sequence)
        self._layout = layout
        self._wc: Optional[WeightCache] = None

    def _cache(self) -> WeightCache:
        if self._wc is None:
            self._wc = WeightCache(self)
        return self._wc

    def forward(self, input):
        """Standard forward."""
        x = input
        if not x.is_cuda:
            return self.forward_eager(x)
        if x.dim() != 5 or x.shape[1] != self.main[0].in_channels:
            raise ValueError(f"NLayerDiscriminator3D takes [B, {self.main[0].in_channels}, T, H, W]; got {tuple(x.shape)}")
        named = list(self.named_parameters())
        if self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for _, p in named)):
            return DiscFn.apply(x, self, tuple(n for n, _ in named), *[p for _, p in named])
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("NLayerDiscriminator3D in eval() runs without a tape and would drop the gradient of an input that requires "
                               "one: call train() for a step that differentiates through it, or run under torch.no_grad()")
        with torch.cuda.device(x.device):
            return disc_forward(self._cache(), x.detach(), self._layout)

    def forward_eager(self, x):
        """the network as plain torch ops over the containers, any device"""
        for m in self.main:
            x = m.forward_eager(x) if isinstance(m, ResnetBlockDown3D) else m(x)
        return x


def get_cvvae_discriminator():
    return NLayerDiscriminator3D(input_nc=3, ndf=64, n_layers=4, use_actnorm=False, half_3d=False, causal=False)
