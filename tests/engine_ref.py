"""fp64 restatement of ONE iteration of the training engines (lvdm/models/autoencoder.py:355-378, 1057-1116, 1518-1589), composed
from the restatements the repository already has: the networks of oracle/cvvae_oracle.py, the regulariser and the loss of
tests/loss_ref.py / tests/allconstraint_ref.py, the discriminator of tests/disc_ref.py, LPIPS of tests/lpips_ref.py and the update of
tests/optim_ref.py.  Two things are restated here because nothing else holds them: the frozen 2-D halves of the SD2.1-compatible
image VAE (lvdm/modules/diffusionmodules/model.py:491-887; held to the reference's own outputs, tests/golden/ldm2d_*.npz, by
tests/test_train_engine_host_logic.py) and the domain-constraint loss with a frame-mapped 2-D target.

An iteration is restated from a state dict taken at its start (the engine's own `state_dict()`), so that AdamW's near-sign update
does not compound errors from one iteration into the next."""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import cvvae_oracle as O
from tests import allconstraint_ref, disc_ref, loss_ref, lpips_ref

LOSS = dict(perceptual_weight=0.5, disc_start=1, disc_weight=0.5, rec2d_weight=1.0,
            regularization_weights={"kl_loss": 1.0})          # tests/engine_cases.py `_loss`: the training YAML's values
FROZEN = ("constraint_encoder.", "constraint_decoder.", "loss.perceptual_loss.")


# ---- the SD2.1-compatible image VAE's halves (model.py), NCHW, any float dtype ----
def _gn(x, sd, pre):
    return F.group_norm(x, 32, sd[pre + ".weight"], sd[pre + ".bias"], 1e-6)


def _swish(x):
    return x * torch.sigmoid(x)


def _conv(x, sd, pre, **kw):
    return F.conv2d(x, sd[pre + ".weight"], sd[pre + ".bias"], **kw)


def ldm_resnet(x, sd, pre):
    """ResnetBlock.forward (temb None, dropout 0)"""
    h = _conv(_swish(_gn(x, sd, pre + ".norm1")), sd, pre + ".conv1", padding=1)
    h = _conv(_swish(_gn(h, sd, pre + ".norm2")), sd, pre + ".conv2", padding=1)
    if pre + ".nin_shortcut.weight" in sd:
        x = _conv(x, sd, pre + ".nin_shortcut")
    return x + h


def ldm_attn(x, sd, pre):
    """AttnBlock.forward: softmax(q^T k / sqrt(c)) over the h w positions"""
    h = _gn(x, sd, pre + ".norm")
    q, k, v = (_conv(h, sd, f"{pre}.{n}") for n in "qkv")
    b, c, hh, ww = q.shape
    w = torch.bmm(q.reshape(b, c, -1).transpose(1, 2), k.reshape(b, c, -1)) * (int(c) ** (-0.5))
    w = F.softmax(w, dim=2)
    h = torch.bmm(v.reshape(b, c, -1), w.transpose(1, 2)).reshape(b, c, hh, ww)
    return x + _conv(h, sd, pre + ".proj_out")


def _frames(x):
    b, c, t, h, w = x.shape
    return x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w), (b, t)


def _clip(y, bt):
    return y.reshape(*bt, *y.shape[1:]).permute(0, 2, 1, 3, 4)


def ldm_encoder(x, sd, cfg, legacy=True):
    """EncoderWith3DWrapper.forward: frame by frame; Downsample = zero pad (0,1,0,1) + conv stride 2; legacy: quant_conv"""
    x, bt = _frames(x)
    mult, nrb = list(cfg["ch_mult"]), cfg["num_res_blocks"]
    h = _conv(x, sd, "conv_in", padding=1)
    for lvl in range(len(mult)):
        for j in range(nrb):
            h = ldm_resnet(h, sd, f"down.{lvl}.block.{j}")
        if lvl != len(mult) - 1:
            h = _conv(F.pad(h, (0, 1, 0, 1)), sd, f"down.{lvl}.downsample.conv", stride=2)
    h = ldm_resnet(ldm_attn(ldm_resnet(h, sd, "mid.block_1"), sd, "mid.attn_1"), sd, "mid.block_2")
    h = _conv(_swish(_gn(h, sd, "norm_out")), sd, "conv_out", padding=1)
    if legacy:
        h = _conv(h, sd, "quant_conv")
    return _clip(h, bt)


def ldm_decoder(z, sd, cfg, legacy=True):
    """DecoderWith3DWrapper.forward: legacy: post_quant_conv first; Upsample = nearest x2 + conv"""
    z, bt = _frames(z)
    mult, nrb = list(cfg["ch_mult"]), cfg["num_res_blocks"]
    if legacy:
        z = _conv(z, sd, "post_quant_conv")
    h = _conv(z, sd, "conv_in", padding=1)
    h = ldm_resnet(ldm_attn(ldm_resnet(h, sd, "mid.block_1"), sd, "mid.attn_1"), sd, "mid.block_2")
    for lvl in reversed(range(len(mult))):
        for j in range(nrb + 1):
            h = ldm_resnet(h, sd, f"up.{lvl}.block.{j}")
        if lvl != 0:
            h = _conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), sd, f"up.{lvl}.upsample.conv", padding=1)
    return _clip(_conv(_swish(_gn(h, sd, "norm_out")), sd, "conv_out", padding=1), bt)


# ---- the domain-constraint loss with a frame-mapped target (the formulas of tests/loss_ref.py, the targets of allconstraint_ref) ----
def domain_ref(inputs, recs, recs2d, *, logvar, logvar_2d, discriminator, perceptual, target_type, indices, optimizer_idx, global_step,
               last_layer, regularization_log, split="train", training=True, perceptual_weight, disc_start, disc_weight, rec2d_weight,
               time_n_compress, regularization_weights, disc_factor=1.0):
    if optimizer_idx == 1 or target_type == "slice":
        return loss_ref.loss_ref(inputs, recs, recs2d, logvar=logvar, logvar_2d=logvar_2d, discriminator=discriminator,
                                 perceptual=perceptual, perceptual_weight=perceptual_weight, disc_start=disc_start, disc_factor=disc_factor,
                                 disc_weight=disc_weight, time_n_compress=time_n_compress, rec2d_weight=rec2d_weight,
                                 regularization_weights=regularization_weights, regularization_log=regularization_log,
                                 optimizer_idx=optimizer_idx, global_step=global_step, last_layer=last_layer, split=split, training=training)
    x5, r5 = inputs.double(), recs.double()
    x, r = loss_ref.frames(x5), loss_ref.frames(r5)
    rec = torch.abs(x - r) + perceptual_weight * perceptual(x.contiguous(), r.contiguous()).double()
    nll = rec / torch.exp(logvar) + logvar
    nll = torch.sum(nll) / nll.shape[0]
    t2 = loss_ref.frames(allconstraint_ref.targets_2d(x5, target_type, time_n_compress, indices))
    rec2d = torch.abs(t2 - loss_ref.frames(recs2d.double()))
    n2 = rec2d / torch.exp(logvar_2d) + logvar_2d
    nll = nll + rec2d_weight * (torch.sum(n2) / n2.shape[0])
    if global_step >= disc_start or not training:
        g_loss = -torch.mean(discriminator(r5.contiguous()).double())
        if training:
            ng = torch.autograd.grad(nll, last_layer, retain_graph=True)[0]
            gg = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
            d_weight = torch.clamp(torch.norm(ng) / (torch.norm(gg) + 1e-4), 0.0, 1e4).detach() * disc_weight
        else:
            d_weight = torch.tensor(1.0, dtype=torch.float64)
    else:
        d_weight, g_loss = torch.tensor(0.0, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64, requires_grad=True)
    loss = nll + d_weight * disc_factor * g_loss
    log = {}
    for k, v in regularization_log.items():
        if k in regularization_weights:
            loss = loss + regularization_weights[k] * v
            log[f"{split}/{k}"] = v.detach().double().mean()
    log.update({f"{split}/loss/total": loss.detach(), f"{split}/loss/nll": nll.detach(), f"{split}/loss/rec": rec.detach().mean(),
                f"{split}/loss/rec2d": rec2d.detach().mean(), f"{split}/loss/g": g_loss.detach(), f"{split}/scalars/logvar": logvar.detach(),
                f"{split}/scalars/logvar_2d": logvar_2d.detach(), f"{split}/scalars/d_weight": d_weight.detach()})
    return loss, log


# ---- one iteration ----
def _sub(sd: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def leaves(state: Dict[str, torch.Tensor], net_dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    """the engine's state dict as fp64 leaves; what a network of `net_dtype` holds is rounded to it first (the logvars stay fp32)"""
    out = {}
    for k, v in state.items():
        if k.startswith("model_ema.") or not v.is_floating_point():
            continue
        v = v.detach().cpu()
        if not k.startswith("loss.logvar"):
            v = v.to(net_dtype)
        out[k] = v.double().clone().requires_grad_(not k.startswith(FROZEN))
    return out


def iteration(kind: str, state: Dict[str, torch.Tensor], x: torch.Tensor, net_cfg: dict, *, noise: Optional[torch.Tensor], indices,
              optimizer_idx: int, global_step: int, net_dtype=torch.float32, target_type: str = "random", split: str = "train",
              training: bool = True, want_grads: bool = True, time_n_compress: int = 4):
    """-> (loss, log, {state-dict name: d loss / d parameter} over the parameters of the optimizer that steps), all fp64"""
    sd = leaves(state, net_dtype)
    x = x.detach().cpu().double()
    dsd = _sub(sd, "loss.discriminator.")
    lp = {k: v.detach() for k, v in _sub(sd, "loss.perceptual_loss.").items()}
    if kind == "latent":
        mom = O.sd3_encoder(x, sd, net_cfg, "encoder")
        z, kl = loss_ref.gauss_reg_ref(mom, noise)
        xrec = O.sd3_decoder(z, sd, net_cfg, "decoder")
        xrec_2d = O.constraint_decoder(z, _sub(sd, "constraint_decoder."), net_cfg)
        last = sd["decoder.conv_out.weight"]
        fn = domain_ref
    else:
        c3 = dict(ch_mult=net_cfg["ch_mult"], num_res_blocks=net_cfg["num_res_blocks"])
        with torch.no_grad():
            mom_d = ldm_encoder(x[:, :, ::time_n_compress], _sub(sd, "constraint_encoder."), c3)
        mom = torch.cat([O.v3_encoder(x, sd, c3, "encoder"), mom_d], dim=0)
        z, kl = loss_ref.gauss_reg_ref(mom, noise)
        xrec = O.v3_decoder(z, sd, c3, "decoder")
        xrec_2d = ldm_decoder(z[: z.shape[0] // 2], _sub(sd, "constraint_decoder."), c3)
        last = sd["decoder.conv_out.weight"]
        fn = allconstraint_ref.all_constraint_ref
    kw = dict(LOSS, time_n_compress=time_n_compress)
    if fn is allconstraint_ref.all_constraint_ref:
        kw["dtype"] = torch.float64
    loss, log = fn(x, xrec, xrec_2d, logvar=sd["loss.logvar"], logvar_2d=sd["loss.logvar_2d"],
                   discriminator=lambda t: disc_ref.forward(dsd, t), perceptual=lambda a, b: lpips_ref.lpips_forward(a, b, lp, torch.float64),
                   target_type=target_type, indices=None if indices is None else torch.tensor(list(indices)),
                   regularization_log={"kl_loss": kl}, optimizer_idx=optimizer_idx, global_step=global_step, last_layer=last, split=split,
                   training=training, **kw)
    if optimizer_idx == 0:
        names = [k for k in sd if k.startswith(("encoder.", "decoder.", "loss.logvar"))]
    else:
        names = [k for k in sd if k.startswith("loss.discriminator.")]
    grads = {}
    if want_grads and training and loss.requires_grad:
        gs = torch.autograd.grad(loss, [sd[k] for k in names], allow_unused=True)
        grads = {k: g for k, g in zip(names, gs)}
    return loss.detach(), {k: v.detach() for k, v in log.items()}, grads


def first_iteration(kind, engine, x, indices, net_dtype, noise, net_cfg):
    """the generator step at global_step 0 of an engine in its seeded state -> (loss, log)"""
    loss, log, _ = iteration(kind, engine.state_dict(), x, net_cfg, noise=noise, indices=indices, optimizer_idx=0, global_step=0,
                             net_dtype=net_dtype, want_grads=False)
    return loss, log
