"""Plain-torch restatement of LPIPSWithDiscriminatorAndAllConstraint -- the yardstick of tests/test_loss_allconstraint_host_logic.py
and tests/test_gpu_train_constraint.py.  Written from the description of lvdm/modules/autoencoding/losses/discriminator_loss.py:
821-1013 (forward and get_nll_loss): the 2-D target built as a full tensor by one of the three `target_type` rules, the inputs
doubled with torch.cat, full-size tensors, the per-frame LPIPS value broadcast over each frame, torch.sum / torch.mean,
torch.autograd for every gradient.  Everything is evaluated in `dtype` (fp64 by default; a 16-bit dtype measures the restatement's
own noise).

The reference's own loss module imports torchvision at module level, which this project does not depend on, so the restatement is
not pinned against it numerically; tests/golden/loss_names_allconstraint.json holds the names read from that file."""
from typing import Callable, Dict, Optional

import torch
import torch.nn.functional as F


def frames(x: torch.Tensor) -> torch.Tensor:
    """b c t h w -> (b t) c h w"""
    b, c, t, h, w = x.shape
    return x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)


def random_indices(t: int, n: int) -> torch.Tensor:
    """the draw of target_type "random" (from the global CPU generator)"""
    d = (t - 1) // n
    return torch.cat([torch.tensor([0]), torch.randint(1, n + 1, (d,)) + torch.arange(d) * n])


def targets_2d(inputs: torch.Tensor, target_type: str, n: int, indices: Optional[torch.Tensor] = None) -> torch.Tensor:
    b, c, t, h, w = inputs.shape
    if target_type == "mean":
        rest = inputs[:, :, 1:]
        assert rest.shape[2] % n == 0  # (einops' "b c (t n) h w -> b c t n h w" raises otherwise)
        return torch.cat([inputs[:, :, :1], rest.reshape(b, c, rest.shape[2] // n, n, h, w).mean(dim=3)], dim=2)
    if target_type == "slice":
        return inputs[:, :, ::n]
    assert target_type == "random"
    if indices is None:
        indices = random_indices(t, n)
    return inputs[:, :, indices]


def _rec(x, xhat, kind):
    return torch.abs(x - xhat) if kind == "l1" else F.mse_loss(x, xhat, reduction="none")


def all_constraint_ref(inputs: torch.Tensor, recs: torch.Tensor, recs2d: torch.Tensor, *, logvar: torch.Tensor, logvar_2d: torch.Tensor,
                       discriminator: Callable, perceptual: Optional[Callable] = None, perceptual_weight: float = 1.0,
                       rec_loss: str = "l1", disc_loss: str = "hinge", disc_start: int = 0, disc_factor: float = 1.0,
                       disc_weight: float = 1.0, time_n_compress: int = 4, rec2d_weight: float = 1.0, target_type: str = "slice",
                       indices: Optional[torch.Tensor] = None, regularization_weights: Optional[Dict[str, float]] = None,
                       additional_log_keys=(), regularization_log: Dict[str, torch.Tensor], optimizer_idx: int, global_step: int,
                       last_layer=None, split: str = "train", weights=None, training: bool = True, dtype=torch.float64):
    """-> (loss, log).  inputs [B,3,T,H,W], recs [2B,3,T,H,W], recs2d [B,3,T',H,W].  perceptual(frames_x, frames_xhat) -> [N,1,1,1];
    discriminator(x) -> logits (a 3-D discriminator: it sees the 5-D clips), both differentiable callables."""
    regularization_weights = regularization_weights or {}
    log_keys = set(additional_log_keys) | set(regularization_weights)
    x5 = inputs.to(dtype)
    t2 = frames(targets_2d(x5, target_type, time_n_compress, indices))
    x5 = torch.cat([x5, x5], dim=0)
    r5 = recs.to(dtype)
    x, r = frames(x5), frames(r5)
    rec2d = _rec(t2.contiguous(), frames(recs2d.to(dtype)).contiguous(), rec_loss)
    rec = _rec(x.contiguous(), r.contiguous(), rec_loss)
    if perceptual_weight > 0:
        rec = rec + perceptual_weight * perceptual(x.contiguous(), r.contiguous()).to(dtype)
    # get_nll_loss
    nll = rec / torch.exp(logvar) + logvar
    n2 = rec2d / torch.exp(logvar_2d) + logvar_2d
    n2 = torch.sum(n2) / n2.shape[0]
    weighted = nll if weights is None else weights * nll
    weighted = torch.sum(weighted) / weighted.shape[0]
    nll = torch.sum(nll) / nll.shape[0]
    weighted = weighted + rec2d_weight * n2
    nll = nll + rec2d_weight * n2
    dev = rec.device
    if optimizer_idx == 0:
        if global_step >= disc_start or not training:
            g_loss = -torch.mean(discriminator(r5.contiguous()).to(dtype))
            if training:
                ng = torch.autograd.grad(nll, last_layer, retain_graph=True)[0]
                gg = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
                d_weight = torch.clamp(torch.norm(ng) / (torch.norm(gg) + 1e-4), 0.0, 1e4).detach() * disc_weight
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
                    f"{split}/loss/rec": rec.detach().mean(), f"{split}/loss/rec2d": rec2d.detach().mean(),
                    f"{split}/loss/g": g_loss.detach().mean(), f"{split}/scalars/logvar": logvar.detach(),
                    f"{split}/scalars/logvar_2d": logvar_2d.detach(), f"{split}/scalars/d_weight": d_weight.detach()})
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
