"""The backward toolkit the taped networks share: grad.py (frozen 2-D constraint decoder), grad3d.py (trainable 3-D codec),
discriminator.py (3-D PatchGAN) and lpips.py keep their tape walkers and import the pieces from here.  Each piece keeps one contract --
which operand, which padding, which launch:

  unit_tabs          the (rstd, -mean rstd) tables of a GroupNorm over x, i.e. the forward's statistics with gamma 1, beta 0: ONE
                     `gn_finalize` over the producer's records `part`, or (no records, or per-frame rows) one `gn_stats` pass over x
  conv_dgrad         input gradient of a STRIDE-1, ZERO-padded conv: ONE launch of the forward conv kernel over g with
                     WeightCache.conv_dgrad's weights (taps flipped, Cin / Cout exchanged, no bias) under the FORWARD's padding, zero mode
  dgrad1x1           the same for a 1x1 conv / nn.Linear on the flattened pixels of every batch row; `residual` is summed in the launch
  linear_grads       dW = g^T a (one `conv_wgrad`, (1,1,1)) and db (one `bias_grad`) of a 1x1 conv / nn.Linear over operand a
  conv_param_grads   dW (and db, out of the same launch) of a conv: `conv_wgrad` over the operand the FORWARD multiplied with the forward's
                     stride, padding and modes; the operand may be a callable, made only when the network is trainable
  gn_backward        input gradient of act(GroupNorm(x)) (+ add): `gn_bwd_input`; trainable: `gn_bwd_input_params` (+ affine gradients)
  resnet_backward    the adjoint of y = conv2(silu(norm2(h))) + shortcut(x), h = conv1(silu(norm1(x))) for all three networks

`grads` is the dict that receives fp32 parameter gradients by parameter name; None means a FROZEN network: every weight-gradient, bias
and affine launch (and every operand made only for one) is skipped.

The node plumbing (`taped`, `begin_node`, `backward_pass`, `node_grads` over `param_meta`, `remember_versions`, `check_unmodified`,
`grads_out`) is what every taped torch.autograd.Function does around its walker."""
import contextlib
from typing import Optional

import torch

from . import engine, ops
from .engine import ZERO, WeightCache

K1 = (1, 1, 1)


def unit_tabs(x: torch.Tensor, part, eps: float, per_frame: bool = False):
    """(rstd, -mean*rstd) tables [rows, C] of the GroupNorm over x: the forward's statistics with gamma 1, beta 0"""
    C = x.shape[-1]
    one = torch.ones(C, dtype=torch.float32, device=x.device)
    zero = torch.zeros(C, dtype=torch.float32, device=x.device)
    if part is not None and not per_frame:
        return ops.gn_finalize(part, one, zero, eps)
    return ops.gn_stats(x, one, zero, eps, per_frame=per_frame)


def conv_dgrad(wc: WeightCache, g: torch.Tensor, name: str, k, pad, cin_pad=None, **kw) -> torch.Tensor:
    """input gradient of the stride-1 conv `name` (kernel k, ZERO padding `pad`): the adjoint of (zero pad, correlate) is the correlation
    of g with the tap-flipped, transposed weights under the same zero padding -- one launch at the input's own extent"""
    return ops.conv(g, wc.conv_dgrad(name, k, cin_pad=cin_pad), pad=pad, pad_mode_t=ZERO, pad_mode_hw=ZERO, **kw)


def dgrad1x1(wc: WeightCache, g: torch.Tensor, pre: str, residual=None) -> torch.Tensor:
    """g [..., Cout] -> g . W  ([..., Cin]) on the flattened pixels of every batch row (+ residual)"""
    pw = wc.conv_dgrad(pre, K1)
    y = ops.conv(engine._flat(g), pw, residual=engine._flat(residual) if residual is not None else None)
    return y.view(*g.shape[:-1], pw.cout)


def linear_grads(wc: WeightCache, grads: dict, pre: str, a: torch.Tensor, g: torch.Tensor):
    """parameter gradients of y = linear(a) (nn.Linear / 1x1 conv `pre`) given g = dL/dy: dW = g^T a on the wgrad kernel, db = sum g"""
    w = wc.p(pre + ".weight")
    a5, g5 = a.reshape(a.shape[0], 1, 1, -1, a.shape[-1]), g.reshape(g.shape[0], 1, 1, -1, g.shape[-1])
    grads[pre + ".weight"] = ops.conv_wgrad(a5.contiguous(), g5.contiguous(), K1, cin=w.shape[1], cout=w.shape[0]).reshape(w.shape)
    if wc.has(pre + ".bias"):
        grads[pre + ".bias"] = ops.bias_grad(g5.contiguous(), cout=w.shape[0])


def conv_param_grads(wc: WeightCache, grads: Optional[dict], pre: str, a, g: torch.Tensor, k, **geom):
    """dW, db of `pre` (a conv over operand a with output gradient g); grads None = a frozen network: nothing to do.
    a: the operand, or a callable that produces it (so that a frozen pass does not re-create operands it never reads)"""
    if grads is None:
        return
    if callable(a):
        a = a()
    w = wc.p(pre + ".weight")
    if wc.has(pre + ".bias"):   # (the bias gradient comes out of the weight-gradient launch where the kernel fuses it)
        dw, grads[pre + ".bias"] = ops.conv_wgrad(a, g, k, cin=w.shape[1], cout=w.shape[0], bias=True, **geom)
    else:
        dw = ops.conv_wgrad(a, g, k, cin=w.shape[1], cout=w.shape[0], **geom)
    grads[pre + ".weight"] = dw.reshape(w.shape)


def gn_backward(grads: Optional[dict], name: str, x, g, tabs, affine, silu: bool, add=None, per_frame: bool = False):
    """input gradient of act(GroupNorm(x)) (+ add), and -- trainable network -- the norm's affine gradients into `grads`"""
    if grads is None:
        return ops.gn_bwd_input(x, g, tabs, *affine, silu=silu, add=add, per_frame=per_frame)
    gx, grads[name + ".weight"], grads[name + ".bias"] = ops.gn_bwd_input_params(x, g, tabs, *affine, silu=silu, add=add,
                                                                                  per_frame=per_frame)
    return gx


def block_names(wc: WeightCache, pre: str, shortcut: str):
    """(norm1, conv1, norm2, conv2, shortcut or None) of the residual block with parameter prefix `pre` (its trailing dot included)"""
    return pre + "norm1", pre + "conv1", pre + "norm2", pre + "conv2", pre + shortcut if wc.has(pre + shortcut + ".weight") else None


def resnet_backward(wc: WeightCache, g: torch.Tensor, grads: Optional[dict], names, x, xp, h, hp, eps: float, conv1, conv2, dgrad1,
                    gn1=None, gn2=None, sc_x=None, h_shape=None) -> torch.Tensor:
    """y = conv2(silu(norm2(h))) + shortcut(x), h = conv1(silu(norm1(x))); g = dL/dy -> dL/dx, parameter gradients into `grads`.
    names: block_names(); xp / hp: the GroupNorm records of x / h; gn1 / gn2: the forward's norm tables (the weight gradients'
    operands silu(norm(.)) are re-made from them -- trainable only); conv2 = (kernel, zero padding): stride 1, its input gradient is
    conv_dgrad; conv1 = (kernel, the forward's padding and modes), its input gradient is dgrad1(g_h) -- the network's own;
    sc_x: what the 1x1 shortcut multiplied; h_shape: the block average-pooled conv1's output of that shape (and x, in front of the
    shortcut) -- the discriminator's downsampling blocks -- so both branches go back through the pool's adjoint."""
    norm1, c1, norm2, c2, sc = names
    (k1, geom1), (k2, pad2) = conv1, conv2
    conv_param_grads(wc, grads, c2, lambda: ops.gn_silu_apply(h, gn2), g, k2, pad=pad2, pad_mode_t=ZERO, pad_mode_hw=ZERO)
    g_a2 = conv_dgrad(wc, g, c2, k2, pad2)
    g_h = gn_backward(grads, norm2, h, g_a2, unit_tabs(h, hp, eps), wc.norm(norm2), True)
    del g_a2
    if h_shape is not None:
        g_h = ops.avgpool3d_down_bwd(g_h, h_shape)
    conv_param_grads(wc, grads, c1, lambda: ops.gn_silu_apply(x, gn1), g_h, k1, **geom1)
    g_a1 = dgrad1(g_h)
    del g_h
    skip = g
    if sc is not None:
        if grads is not None:
            linear_grads(wc, grads, sc, sc_x, g)
        skip = dgrad1x1(wc, g, sc)
    if h_shape is not None:
        skip = ops.avgpool3d_down_bwd(skip, tuple(x.shape))
    return gn_backward(grads, norm1, x, g_a1, unit_tabs(x, xp, eps), wc.norm(norm1), True, add=skip)


# ---- the plumbing of a taped autograd node --------------------------------------------------------------
def param_meta(params):
    return [(p.dtype, p.requires_grad, tuple(p.shape)) for p in params]


# The backward reads the weights LIVE (packed input-gradient forms, norm affines) instead of saving them on the tape.  PyTorch's own
# conv backward would raise "one of the variables needed for gradient computation has been modified by an inplace operation" when
# a parameter changes between forward and backward (an optimizer.step() under retain_graph, a GAN's generator / discriminator
# alternation on one graph); so does this one: the parameters' (storage, version) are remembered by the forward and checked.
def remember_versions(ctx, params):
    ctx.pobj = params
    ctx.pver = [(p.data_ptr(), p._version) for p in params]


def check_unmodified(ctx):
    for name, p, was in zip(ctx.names, ctx.pobj, ctx.pver):
        if (p.data_ptr(), p._version) != was:
            raise RuntimeError(f"parameter {name} of {type(ctx.net).__name__} was modified (in place, or replaced) between the forward "
                               f"and this backward pass: the taped activations belong to the old weights (version {was[1]} -> "
                               f"{p._version}).  Run the backward before optimizer.step(), or re-run the forward.")


def grads_out(names, pmeta, grads):
    """the fp32 gradients in the parameters' order, shapes and dtypes.  The conversions of a 16-bit model are ONE multi-tensor copy
    (a `.to(dt)` per parameter was 244 five-microsecond launches per training step of the sd3 pair)."""
    out, src, dst = [], [], []
    for name, (dt, req, shape) in zip(names, pmeta):
        gq = grads.get(name)
        if not (req and gq is not None):
            out.append(None)
            continue
        gq = gq.reshape(shape)
        if gq.dtype != dt:
            src.append(gq)
            gq = torch.empty(shape, dtype=dt, device=gq.device)
            dst.append(gq)
        out.append(gq)
    if dst:
        torch._foreach_copy_(dst, src)
    return out


def taped(x: torch.Tensor, program):
    """program(tape) under x's device context -> (its result, the tape it filled)"""
    tape: list = []
    with torch.cuda.device(x.device):
        return program(tape), tape


def begin_node(ctx, net, x: torch.Tensor, names=(), params=(), cd=None):
    """what a node's forward leaves for its backward: the module, its parameters' names, meta and versions, the input's dtype and need,
    and the pass's compute dtype (torch.autocast: the backward thread runs outside the context -- same 16-bit weight copies)"""
    ctx.net, ctx.names, ctx.cd = net, names, cd
    ctx.x_dtype, ctx.need_x = x.dtype, x.requires_grad
    ctx.pmeta = param_meta(params)
    remember_versions(ctx, params)


@contextlib.contextmanager
def backward_pass(ctx, g: torch.Tensor):
    """a node's backward: the parameters are those of the forward, the device and compute-dtype contexts are entered; yields the dict
    for the parameter gradients, or None when no parameter asks for one"""
    check_unmodified(ctx)
    with torch.cuda.device(g.device), ctx.net._cache().computing_in(ctx.cd):
        yield {} if any(req for _, req, _ in ctx.pmeta) else None


def node_grads(ctx, gx, nones: int, grads):
    """backward's return value: (input gradient in the input's dtype, None for the non-tensor arguments, *parameter gradients)"""
    return (gx.to(ctx.x_dtype) if gx is not None else None, *[None] * nones, *grads_out(ctx.names, ctx.pmeta, grads or {}))
