"""Plain-torch restatement of the training loss around the networks -- the yardstick of tests/test_loss_host_logic.py and
tests/test_gpu_loss.py.  Written from the description of lvdm/modules/autoencoding/regularizers/__init__.py:12-32 (with
DiagonalGaussianDistribution, lvdm/modules/distributions/distributions.py:24-52) and of GeneralLPIPSWithDiscriminator /
LPIPSWithDiscriminatorAndDomainConstraint (lvdm/modules/autoencoding/losses/discriminator_loss.py): full-size tensors, the per-frame
LPIPS value broadcast over each frame, torch.sum / torch.mean, torch.autograd for every gradient.  Everything is evaluated in
`dtype` (fp64 by default; a 16-bit dtype measures the restatement's own noise).

The reference's own loss modules import torchvision and matplotlib at module level, neither of which this project depends on, so
the restatement is not pinned against them numerically; tests/golden/loss_names.json holds the names read from that file."""
from typing import Callable, Dict, Optional

import torch
import torch.nn.functional as F


def gauss_reg_ref(moments: torch.Tensor, noise: Optional[torch.Tensor], dtype=torch.float64):
    """-> (z, kl_loss = sum kl / B); moments [B, 2C, ...]; noise None = `sample=False` (the mode)"""
    p = moments.to(dtype)
    mean, logvar = torch.chunk(p, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    std, var = torch.exp(0.5 * logvar), torch.exp(logvar)
    z = mean if noise is None else mean + std * noise.to(dtype)
    kl = 0.5 * torch.sum(mean ** 2 + var - 1.0 - logvar, dim=list(range(1, p.dim())))
    return z, torch.sum(kl) / kl.shape[0]


def frames(x: torch.Tensor) -> torch.Tensor:
    """b c t h w -> (b t) c h w"""
    if x.dim() == 4:
        return x
    b, c, t, h, w = x.shape
    return x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)


def _rec(x, xhat, kind):
    return torch.abs(x - xhat) if kind == "l1" else (x - xhat) ** 2


def loss_ref(inputs: torch.Tensor, recs: torch.Tensor, recs2d: Optional[torch.Tensor], *, logvar: torch.Tensor,
             logvar_2d: Optional[torch.Tensor] = None, discriminator: Callable, perceptual: Optional[Callable] = None,
             perceptual_weight: float = 1.0, rec_loss: str = "l1", disc_loss: str = "hinge", disc_start: int = 0,
             disc_factor: float = 1.0, disc_weight: float = 1.0, adaptive: bool = True, time_n_compress: int = 4,
             rec2d_weight: float = 1.0, regularization_weights: Optional[Dict[str, float]] = None, additional_log_keys=(),
             regularization_log: Dict[str, torch.Tensor], optimizer_idx: int, global_step: int, last_layer=None,
             split: str = "train", weights=None, training: bool = True, dtype=torch.float64):
    """-> (loss, log).  recs2d None: GeneralLPIPSWithDiscriminator; else the DomainConstraint variant (target_type "slice", adaptive
    weight always).  perceptual(frames_x, frames_xhat) -> [N,1,1,1]; discriminator(x) -> logits, both differentiable callables.
    5-D clips go to the discriminator as they are (the rule for a discriminator that is not the 2-D NLayerDiscriminator)."""
    regularization_weights = regularization_weights or {}
    log_keys = set(additional_log_keys) | set(regularization_weights)
    x5, r5 = inputs.to(dtype), recs.to(dtype)
    x, r = frames(x5), frames(r5)
    rec = _rec(x.contiguous(), r.contiguous(), rec_loss)
    if perceptual_weight > 0:
        rec = rec + perceptual_weight * perceptual(x.contiguous(), r.contiguous()).to(dtype)
    nll = rec / torch.exp(logvar) + logvar
    weighted = nll if weights is None else weights * nll
    weighted = torch.sum(weighted) / weighted.shape[0]
    nll = torch.sum(nll) / nll.shape[0]
    rec2d = None
    if recs2d is not None:
        t2 = frames(x5[:, :, ::time_n_compress])
        rec2d = _rec(t2.contiguous(), frames(recs2d.to(dtype)).contiguous(), rec_loss)
        n2 = rec2d / torch.exp(logvar_2d) + logvar_2d
        n2 = torch.sum(n2) / n2.shape[0]
        weighted = weighted + rec2d_weight * n2
        nll = nll + rec2d_weight * n2
        adaptive = True
    dev = rec.device
    if optimizer_idx == 0:
        if global_step >= disc_start or not training:
            g_loss = -torch.mean(discriminator(r5.contiguous()).to(dtype))
            if training and adaptive:
                ng = torch.autograd.grad(nll, last_layer, retain_graph=True)[0]
                gg = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
                d_weight = torch.clamp(torch.norm(ng) / (torch.norm(gg) + 1e-4), 0.0, 1e4).detach() * disc_weight
            elif training:
                d_weight = torch.tensor(disc_weight, dtype=dtype, device=dev)
            else:
                d_weight = torch.tensor(1.0, dtype=dtype, device=dev)
        else:
            d_weight = torch.tensor(0.0, dtype=dtype, device=dev)
            g_loss = torch.tensor(0.0, dtype=dtype, device=dev, requires_grad=True)
        loss = weighted + d_weight * disc_factor * g_loss
        log = {}
        for k in regularization_log:
            if k in regularization_weights:
                loss = loss + regularization_weights[k] * regularization_log[k]
            if k in log_keys:
                log[f"{split}/{k}"] = regularization_log[k].detach().to(dtype).mean()
        log.update({f"{split}/loss/total": loss.detach().mean(), f"{split}/loss/nll": nll.detach().mean(),
                    f"{split}/loss/rec": rec.detach().mean(), f"{split}/loss/g": g_loss.detach().mean(),
                    f"{split}/scalars/logvar": logvar.detach(), f"{split}/scalars/d_weight": d_weight.detach()})
        if rec2d is not None:
            log.update({f"{split}/loss/rec2d": rec2d.detach().mean(), f"{split}/scalars/logvar_2d": logvar_2d.detach()})
        return loss, log
    if optimizer_idx == 1:
        real = discriminator(x5.contiguous().detach()).to(dtype)
        fake = discriminator(r5.contiguous().detach()).to(dtype)
        if global_step >= disc_start or not training:
            if disc_loss == "hinge":
                d = 0.5 * (torch.mean(F.relu(1.0 - real)) + torch.mean(F.relu(1.0 + fake)))
            else:
                d = 0.5 * (torch.mean(F.softplus(-real)) + torch.mean(F.softplus(fake)))
            d_loss = disc_factor * d
        else:
            d_loss = torch.tensor(0.0, dtype=dtype, device=dev, requires_grad=True)
        return d_loss, {f"{split}/loss/disc": d_loss.detach().mean(), f"{split}/logits/real": real.detach().mean(),
                        f"{split}/logits/fake": fake.detach().mean()}
    raise NotImplementedError(f"Unknown optimizer_idx {optimizer_idx}")
