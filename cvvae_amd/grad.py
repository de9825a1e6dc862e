"""Input gradients through the FROZEN 2-D constraint decoders on the MI355X kernels (training-side codec use).

The reference trains the 3-D VAE with a latent-compatibility loss: the latents go through the frozen SD3 image decoder
(`self.constraint_decoder.requires_grad_(False)`, `xrec_2d = self.constraint_decoder(z)`, lvdm/models/autoencoder.py:1057-1069) and
the loss back-propagates THROUGH that decoder into z (and on into the encoder).  What the frozen module contributes to the
backward pass is autograd's input gradient of each of its ops -- no weight gradients.  This file is that pass for the per-frame 2-D
decoder program of cvvae_amd/engine.py in both spellings -- `engine.constraint_decoder2d` (SD3 image decoder) and
`engine.ldm2d_decoder` (SD2.1 image decoder, with `post_quant_conv`): one walker (`decoder2d_backward`), one autograd node:

  conv / linear   grad_input = conv(gy, W with taps flipped and Cin/Cout exchanged), same zero padding  -> the forward MFMA kernel
                  (backward.conv_dgrad / dgrad1x1; nn.Conv2d(3x3, padding=1) and nn.Linear of vae_blocks_sd3.py / diffusers Attention)
  GroupNorm+SiLU  cvvae_gn_bwd_input (two deterministic passes), the residual skip summed in the same launch
  upsample        Upsample2D = nearest x2 + conv: the conv's input gradient at the upsampled size, then cvvae_upsample2x_sum
  attention       softmax(QK^T/sqrt(C))V per frame: five more products on the 1x1 kernel with per-frame "weights" packed from
                  activations (as the forward does) + cvvae_softmax_bwd_rows

Gradients are carried in the module's dtype with fp32 accumulation inside every kernel (what autocast training does).
The decoder's own parameters must be frozen; weight gradients (training the codec itself) are not built.
"""
from typing import List, Optional

import torch

from . import _lib as L
from . import backward, engine, ops
from .backward import K1, backward_pass, begin_node, block_names, conv_dgrad, dgrad1x1, gn_backward, linear_grads, node_grads, taped, unit_tabs
from .engine import P2D, WeightCache

K2D = (1, 3, 3)


def resnet_backward(wc: WeightCache, g: torch.Tensor, e: dict, shortcut: str = "conv_shortcut") -> torch.Tensor:
    """ResnetBlock2D (vae_blocks_sd3.py:368-421; `nin_shortcut`: ResnetBlock of model.py:98-155): y = conv2(silu(norm2(h))) +
    shortcut(x), h = conv1(silu(norm1(x))).  g = dL/dy."""
    pre = e["pre"] + "."
    return backward.resnet_backward(wc, g, None, block_names(wc, pre, shortcut), e["x"], e["xp"], e["h"], e["hp"], 1e-6,
                                    conv1=(K2D, {}), conv2=(K2D, P2D), dgrad1=lambda gh: conv_dgrad(wc, gh, pre + "conv1", K2D, P2D))


def attention_backward(wc: WeightCache, g: torch.Tensor, e: dict, grads: Optional[dict] = None,
                       add_extra: Optional[torch.Tensor] = None) -> torch.Tensor:
    """engine.spatial_attention: out = x + proj(softmax(q k^T / sqrt(C)) v), q,k,v = linear(GroupNorm(x)) per frame.  g = dL/dout.
    grads: a dict that receives the block's PARAMETER gradients (training the network itself, grad3d.py); None = frozen module."""
    x, qq, kk, vv, p = e["x"], e["qq"], e["kk"], e["vv"], e["p"]
    norm, q, k, v, proj = e["names"]
    B, T, H, W, C = x.shape
    N, BT = H * W, B * T
    npad = p.shape[-1]
    scale = float(C) ** -0.5
    g_o = dgrad1x1(wc, g, proj).view(BT, 1, 1, N, C)                                            # dL/d(PV)
    # dL/dP[n,m] = sum_c g_o[n,c] V[m,c]  (fp32), then through the softmax and the score scale
    vw = ops.pack_weight_batched(vv.view(BT, N, C), K1, cin_pad=C, strides=(C, 1, 0), cout=N, cin=C)
    g_p = ops.conv(g_o, vw, out_f32=True, cout_pad=npad)                                          # [BT,1,1,N,npad]
    g_s = ops.softmax_bwd_rows(p.view(BT * N, npad), g_p.view(BT * N, npad), N, scale)            # [BT*N, npad]
    # dL/dV[m,c] = sum_n P[n,m] g_o[n,c]
    p_t = ops.transpose(p.view(BT, N, npad), ncols=N, ld_out=npad)                                # [BT, N(m), npad(n)]
    gow = ops.pack_weight_batched(ops.transpose(g_o.view(BT, N, C)), K1, cin_pad=npad, strides=(N, 1, 0), cout=C, cin=N)
    g_v = ops.conv(p_t.view(BT, 1, 1, N, npad), gow)                                              # [BT,1,1,N,C]
    # dL/dQ[n,c] = sum_m g_s[n,m] K[m,c]
    kw = ops.pack_weight_batched(ops.transpose(kk.view(BT, N, C)), K1, cin_pad=npad, strides=(N, 1, 0), cout=C, cin=N)
    g_q = ops.conv(g_s.view(BT, 1, 1, N, npad), kw)
    # dL/dK[m,c] = sum_n g_s[n,m] Q[n,c]
    gs_t = ops.transpose(g_s.view(BT, N, npad), ncols=N, ld_out=npad)
    qw = ops.pack_weight_batched(ops.transpose(qq.view(BT, N, C)), K1, cin_pad=npad, strides=(N, 1, 0), cout=C, cin=N)
    g_k = ops.conv(gs_t.view(BT, 1, 1, N, npad), qw)
    # back through to_q / to_k / to_v into the normalised input, summed in the launches' residual inputs
    g_n = dgrad1x1(wc, g_q, q)
    g_n = dgrad1x1(wc, g_k, k, residual=g_n)
    g_n = dgrad1x1(wc, g_v, v, residual=g_n)
    tabs = unit_tabs(x, None, e["eps"], per_frame=True)
    if grads is not None:
        n = ops.gn_silu_apply(x, e["gn"], silu=False, per_frame=True).view(BT, 1, 1, N, C)   # what to_q / to_k / to_v consumed
        linear_grads(wc, grads, proj, e["o"].view(BT, 1, 1, N, C), g.view(BT, 1, 1, N, C))
        linear_grads(wc, grads, q, n, g_q)
        linear_grads(wc, grads, k, n, g_k)
        linear_grads(wc, grads, v, n, g_v)
    # (add_extra: a block without its own residual -- vae3d's spatial-temporal attention -- passes the gradient of the outer one)
    return gn_backward(grads, norm, x, g_n.view(B, T, H, W, C), tabs, wc.norm(norm), False, add=g if e["residual"] else add_extra,
                       per_frame=True)


def decoder2d_backward(wc: WeightCache, tape: List[dict], gy: torch.Tensor) -> torch.Tensor:
    """gy = dL/d(output) [b,out,t,H,W] of engine.constraint_decoder2d / engine.ldm2d_decoder run with `tape` -> dL/dz [b,c,t,h,w]:
    conv_out, norm_out + SiLU, the levels (ResnetBlocks, Upsample = nearest x2 + 3x3), the mid block, conv_in and -- the legacy LDM
    checkpoints -- post_quant_conv, backwards.  The layers' names come with the tape (its last entry carries the engine.Spelling)."""
    dtype = wc.p("conv_in.weight").dtype
    last = tape[-1]
    assert last["op"] == "out"
    B, T, zin, sp = last["B"], last["T"], last["zin"], last["names"]
    out_ch = wc.p("conv_out.weight").shape[0]
    if tuple(gy.shape[:3]) != (B, out_ch, T) or out_ch > 32:
        raise NotImplementedError(f"decoder2d_backward ({sp.name} decoder): cotangent {tuple(gy.shape)} for a decoder with {out_ch} <= 32 "
                                  f"output channels over {B} x {T} frames")
    g = ops.ncdhw_to_ndhwc(gy.contiguous(), 32, dtype)                                           # [b,t,H,W,32], channels out_ch.. zero
    g = g.view(B * T, 1, g.shape[2], g.shape[3], 32)
    g = conv_dgrad(wc, g, "conv_out", K2D, P2D, cin_pad=32)                                      # dL/d silu(norm_out(h))
    x = last["x"]
    g = ops.gn_bwd_input(x, g, unit_tabs(x, last["xp"], 1e-6), *wc.norm(sp.norm_out), silu=True)
    for e in reversed(tape[:-1]):
        if e["op"] == "resnet":
            g = resnet_backward(wc, g, e, sp.shortcut[1:])
        elif e["op"] == "attn":
            g = attention_backward(wc, g, e)
        elif e["op"] == "up":  # Upsample: nearest x2, then conv 3x3
            g = ops.upsample2x_sum(conv_dgrad(wc, g, e["pre"], K2D, P2D))
        else:
            raise AssertionError(e["op"])
    if not last.get("post_quant_conv", False):
        gz = conv_dgrad(wc, g, "conv_in", K2D, P2D, out_mode=L.OUT_NCDHW)                        # [b*t, zin, 1, h, w]
    else:
        # conv_in's input gradient keeps the pixel-major layout, channel-padded to the 1x1 kernel's K chunk as the forward pads the
        # latents; post_quant_conv (zin -> zin) backwards on the flattened pixels; then the narrow gradient goes to NCDHW
        if zin > 32:
            raise NotImplementedError(f"decoder2d_backward ({sp.name} decoder): post_quant_conv with {zin} > 32 channels")
        g = conv_dgrad(wc, g, "conv_in", K2D, P2D, cout_pad=128)                                 # [b*t,1,h,w,128]
        pq = wc.conv_dgrad("post_quant_conv", K1, cin_pad=128)
        g = ops.conv(engine._flat(g), pq, cout_pad=32).view(*g.shape[:-1], 32)
        gz = ops.ndhwc_to_ncdhw(g, zin)
    return gz.view(B, T, zin, gz.shape[3], gz.shape[4]).transpose(1, 2).contiguous()


constraint_decoder2d_backward = decoder2d_backward  # (either decoder's tape through the one walker)
ldm2d_decoder_backward = decoder2d_backward


class Decoder2DInputGradFn(torch.autograd.Function):
    """z -> the frozen 2-D decoder `net` (z) with its input gradient as backward (both on the HIP kernels)"""

    @staticmethod
    def forward(ctx, z: torch.Tensor, net) -> torch.Tensor:
        y, ctx.tape = taped(z, lambda tape: type(net)._program(net._cache(), z.detach(), net._cfg, tape))
        begin_node(ctx, net, z, cd=net._cache().compute_dtype)
        return y

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        # the tape (block inputs, statistics records, attention operands) is kept until autograd frees the node, so a second
        # backward through it (retain_graph=True, two losses) walks the same tape and gives the same bits
        with backward_pass(ctx, gy):
            gz = decoder2d_backward(ctx.net._cache(), ctx.tape, gy)
        return node_grads(ctx, gz, 1, None)
