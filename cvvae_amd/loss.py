"""The training loss around the networks, on the MI355X kernels: the posterior regulariser and the pixel / NLL, KL and GAN terms.

`DiagonalGaussianRegularizer` is lvdm/modules/autoencoding/regularizers/__init__.py:12-32 (DiagonalGaussianDistribution's sample
and kl) as ONE autograd node over cvvae_gauss_reg / cvvae_gauss_reg_bwd.  `GeneralLPIPSWithDiscriminator` and
`LPIPSWithDiscriminatorAndDomainConstraint` are the classes of lvdm/modules/autoencoding/losses/discriminator_loss.py:18-336 and
339-585 with the same constructor arguments, parameters, state-dict layout, forward signature, `(loss, log)` return and log keys.

Every pass that reads a tensor of more than one element is a launch of csrc/loss_kernels.hip through `reduce`, an autograd node
over cvvae_reduce_sum / cvvae_reduce_sum_bwd (a deterministic map-reduce to one fp32 scalar and its adjoint):

  sum |x - xhat| or (x - xhat)^2     ABS_DIFF / SQ_DIFF, the 5-D clips (and the `[:, :, ::n]` frame slice of the 2-D target) in place
  sum p_loss, sum logits             IDENT
  hinge / vanilla discriminator      HINGE_NEG + HINGE_POS / SOFTPLUS_NEG + SOFTPLUS_POS
  gradient norms (adaptive weight)   SQ

The reference's `rec_loss = |x - xhat| + perceptual_weight * p_loss` broadcasts the per-frame LPIPS value [N,1,1,1] over the
3 H W values of a frame and sums `rec_loss / exp(logvar) + logvar`; here the sums are taken first,
  sum rec = sum |x - xhat| + perceptual_weight * 3 H W * sum p_loss,     nll = (sum rec / exp(logvar) + logvar * count) / N,
so no full-size temporary exists.  What combines 0-dim tensors (these formulas, exp of the logvar, the clamp of the adaptive
weight) stays in torch and its autograd: the cotangent a `reduce` node receives IS gout / (exp(logvar) N), read by the adjoint
kernel from device memory, and the gradients of the logvars and of p_loss are torch's scalar expressions of the saved sums.
torch also keeps: the random numbers of the posterior sample, the discriminator (an arbitrary nn.Module; the training config's 3-D PatchGAN is
cvvae_amd/discriminator.py, one autograd node on the same library), and the `b c t h w -> (b t) c h w` copy that hands LPIPS its per-frame tensors.

Sums are fp32 whatever the operands' dtypes (fp16 / bf16 / fp32, mixed freely), so the loss, the logs and `kl_loss` are fp32
0-dim tensors.  There is no eager fallback: CPU tensors raise.

`LPIPSWithDiscriminatorAndAllConstraint` (discriminator_loss.py:768-1013) is the loss of the engine with a frozen 2-D encoder and a
frozen 2-D decoder.  It takes all three `target_type`s: "mean" and "random" targets are never materialised -- `reduce_frames`, an
autograd node over cvvae_reduce_sum_frames / _bwd, reads "frame index[t']" or "the mean of frames 1+n(t'-1) .. n t'" from the clip
in place, in the summation order of `reduce` over the materialised target (the same bits).

`LPIPSWithDiscriminatorAndDomainConstraint(..., frame_maps=True)` takes "mean" / "random" through the same frame maps (one shared
mixin, `_FrameMapTargets`); without the keyword the class keeps refusing them at construction, as it always did.

Not built: `log_images`, `scale_input_to_tgt_size=True`, per-element `weights`, the AndEncoderConstraint variant.
"""
import importlib
from typing import Dict, Iterator, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .lpips import LPIPS


class _ReduceFn(torch.autograd.Function):
    """sum f_op(a[, b]) -> 0-dim fp32; backward: coef * f_op' into a (and its negative into b), coef = the incoming cotangent"""

    @staticmethod
    def forward(ctx, op: int, a: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
        ctx.op = op
        ctx.save_for_backward(a, b)
        with torch.cuda.device(a.device):
            return ops.reduce_sum(op, a.detach(), b.detach() if b is not None else None)

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        coef = gout.detach().to(torch.float32).reshape(()).contiguous()
        with torch.cuda.device(a.device):
            ga, gb = ops.reduce_sum_bwd(ctx.op, a, b, coef, need_a, need_b)
        return None, ga, gb


def reduce(op: int, a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the differentiable form of ops.reduce_sum"""
    ops._need_gpu(a)
    if torch.is_grad_enabled() and (a.requires_grad or (b is not None and b.requires_grad)):
        return _ReduceFn.apply(op, a, b)
    with torch.cuda.device(a.device):
        return ops.reduce_sum(op, a.detach(), b.detach() if b is not None else None)


class _ReduceFramesFn(torch.autograd.Function):
    """sum f_op(a, frame-mapped target of the clip) -> 0-dim fp32; backward: coef * f_op' into a.  The clip (the inputs) gets none."""

    @staticmethod
    def forward(ctx, op: int, a: torch.Tensor, clip: torch.Tensor, mode: int, index, group) -> torch.Tensor:
        ctx.op, ctx.mode, ctx.index, ctx.group = op, mode, index, group
        ctx.save_for_backward(a, clip)
        with torch.cuda.device(a.device):
            return ops.reduce_sum_frames(op, a.detach(), clip.detach(), mode, index=index, group=group)

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        a, clip = ctx.saved_tensors
        coef = gout.detach().to(torch.float32).reshape(()).contiguous()
        with torch.cuda.device(a.device):
            ga = ops.reduce_sum_frames_bwd(ctx.op, a, clip, coef, ctx.mode, index=ctx.index, group=ctx.group)
        return None, ga, None, None, None, None


def reduce_frames(op: int, a: torch.Tensor, clip: torch.Tensor, mode: int, *, index=None, group=None) -> torch.Tensor:
    """the differentiable form of ops.reduce_sum_frames: a [B,C,T',H,W] against frames of clip [B,C,T,H,W] picked by `index`
    (L.FMAP_GATHER, host ints) or averaged in groups (L.FMAP_GROUP_MEAN), read in place.  Differentiates a only."""
    ops._need_gpu(a)
    ops._need_gpu(clip)
    if clip.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("reduce_frames has no gradient into the clip: the inputs of a loss never require grad")
    if index is not None:
        index = [int(i) for i in (index.tolist() if isinstance(index, torch.Tensor) else index)]
    a = a.contiguous()
    if torch.is_grad_enabled() and a.requires_grad:
        return _ReduceFramesFn.apply(op, a, clip, mode, index, group)
    with torch.cuda.device(a.device):
        return ops.reduce_sum_frames(op, a.detach(), clip.detach(), mode, index=index, group=group)


def _mean(t: torch.Tensor) -> torch.Tensor:
    """detached fp32 mean of a log value"""
    t = t.detach()
    return t.float().reshape(()) if t.numel() == 1 else reduce(L.RED_IDENT, t) / t.numel()


class _GaussRegFn(torch.autograd.Function):
    """moments (, noise) -> (z, kl_sum); backward: cvvae_gauss_reg_bwd on the cotangents of both"""

    @staticmethod
    def forward(ctx, moments: torch.Tensor, noise: Optional[torch.Tensor]):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(moments, noise)
        with torch.cuda.device(moments.device):
            z, kl = ops.gauss_reg(moments.detach(), noise)
        return z, kl

    @staticmethod
    def backward(ctx, g_z: Optional[torch.Tensor], g_kl: Optional[torch.Tensor]):
        moments, noise = ctx.saved_tensors
        if g_z is None and g_kl is None:
            return None, None
        coef = (torch.zeros((), dtype=torch.float32, device=moments.device) if g_kl is None
                else g_kl.detach().to(torch.float32).reshape(()).contiguous())
        if g_z is not None:
            g_z = g_z.detach().to(moments.dtype).contiguous()
        with torch.cuda.device(moments.device):
            return ops.gauss_reg_bwd(moments, noise, g_z, coef), None


class DiagonalGaussianRegularizer(nn.Module):
    """drop-in for lvdm.modules.autoencoding.regularizers.DiagonalGaussianRegularizer: forward(moments [B, 2C, ...]) ->
    (z [B, C, ...], {"kl_loss": sum kl / B}).  The noise is torch.randn on the tensor's device in its dtype (`generator=` seeds it,
    `noise=` replaces it: both for reproducible tests); everything else is one kernel pass forward and one backward."""

    def __init__(self, sample: bool = True):
        super().__init__()
        self.sample = sample

    def get_trainable_parameters(self) -> Iterator[nn.Parameter]:
        yield from ()

    def forward(self, z: torch.Tensor, *, generator: Optional[torch.Generator] = None,
                noise: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, dict]:
        ops._need_gpu(z)
        if z.dim() not in (4, 5) or z.shape[1] % 2:
            raise ValueError(f"DiagonalGaussianRegularizer takes moments [B, 2C, (T,) H, W]; got {tuple(z.shape)}")
        if self.sample:
            shape = (z.shape[0], z.shape[1] // 2, *z.shape[2:])
            if noise is None:
                noise = torch.randn(shape, generator=generator, device=z.device, dtype=z.dtype)
            elif tuple(noise.shape) != shape or noise.dtype != z.dtype or noise.device != z.device:
                raise ValueError(f"noise must be {shape} {z.dtype} on {z.device}")
            noise = noise.detach().contiguous()
        else:
            noise = None
        out, kl_sum = _GaussRegFn.apply(z, noise)
        return out, {"kl_loss": kl_sum / z.shape[0]}


def _instantiate(config: Dict) -> nn.Module:
    module, cls = config["target"].rsplit(".", 1)
    return getattr(importlib.import_module(module), cls)(**config.get("params", dict()))


def weights_init(m: nn.Module) -> None:
    """lvdm/modules/autoencoding/lpips/model/model.py:17-23"""
    name = m.__class__.__name__
    if name.find("Conv") != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif name.find("BatchNorm") != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class GeneralLPIPSWithDiscriminator(nn.Module):
    def __init__(
        self,
        disc_start: int,
        logvar_init: float = 0.0,
        disc_num_layers: int = 3,
        disc_in_channels: int = 3,
        disc_factor: float = 1.0,
        disc_weight: float = 1.0,
        perceptual_weight: float = 1.0,
        disc_loss: str = "hinge",
        rec_loss: str = "l1",
        scale_input_to_tgt_size: bool = False,
        dims: int = 2,
        learn_logvar: bool = False,
        regularization_weights: Union[None, Dict[str, float]] = None,
        additional_log_keys: Optional[List[str]] = None,
        discriminator_config: Optional[Dict] = None,
        adaptive_disc_weight: bool = True,
        *,
        discriminator: Optional[nn.Module] = None,
    ):
        super().__init__()
        self.dims = dims
        if scale_input_to_tgt_size:
            raise NotImplementedError("scale_input_to_tgt_size=True (bicubic antialiased resize of the inputs) has no kernel here")
        self.scale_input_to_tgt_size = scale_input_to_tgt_size
        assert disc_loss in ["hinge", "vanilla"]
        assert rec_loss in ["l1", "l2"]
        self.rec_loss = rec_loss
        self.perceptual_loss = LPIPS().eval()
        self.perceptual_weight = perceptual_weight
        self.logvar = nn.Parameter(torch.full((), logvar_init), requires_grad=learn_logvar)
        self.learn_logvar = learn_logvar
        self.adaptive_disc_weight = adaptive_disc_weight

        if discriminator is not None:
            if discriminator_config is not None:
                raise ValueError("pass discriminator_config or discriminator=, not both")
            self.discriminator = discriminator
        elif discriminator_config is not None:
            self.discriminator = _instantiate(discriminator_config).apply(weights_init)
        else:
            raise NotImplementedError(
                "no discriminator network ships yet: the reference's default (the 2-D NLayerDiscriminator with "
                f"input_nc={disc_in_channels}, n_layers={disc_num_layers}) is not part of this package; pass discriminator_config="
                '{"target": "dotted.path.Class", "params": {...}} or discriminator=<nn.Module>')
        self.discriminator_iter_start = disc_start
        self.disc_loss = disc_loss
        self.disc_factor = disc_factor
        self.discriminator_weight = disc_weight
        self.regularization_weights = regularization_weights if regularization_weights is not None else {}

        self.forward_keys = ["optimizer_idx", "global_step", "last_layer", "split", "regularization_log"]

        self.additional_log_keys = set(additional_log_keys if additional_log_keys is not None else [])
        self.additional_log_keys.update(set(self.regularization_weights.keys()))

    def train(self, mode: bool = True):
        super().train(mode)
        self.perceptual_loss.eval()  # LPIPS().eval(): frozen, its Dropout the identity
        return self

    def get_trainable_parameters(self) -> Iterator[nn.Parameter]:
        return self.discriminator.parameters()

    def get_trainable_autoencoder_parameters(self) -> Iterator[nn.Parameter]:
        if self.learn_logvar:
            yield self.logvar
        yield from ()

    # ---- the pieces of forward ----
    def _frames(self, x: torch.Tensor) -> torch.Tensor:
        """[B,3,T,H,W] -> [(B T),3,H,W] (a copy when T > 1); 4-D tensors as they are"""
        if x.dim() == 4:
            return x
        b, c, t, h, w = x.shape
        return x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)

    def _check_clips(self, inputs: torch.Tensor, recs: torch.Tensor, what: str = "reconstructions") -> None:
        ops._need_gpu(inputs)
        ops._need_gpu(recs)
        want = 5 if self.dims > 2 else 4
        if inputs.dim() != want or inputs.shape != recs.shape:
            raise ValueError(f"dims={self.dims}: inputs and {what} must be {want}-D tensors of one shape; got "
                             f"{tuple(inputs.shape)} and {tuple(recs.shape)}")

    def _rec_sum(self, x: torch.Tensor, xhat: torch.Tensor, perceptual: bool) -> Tuple[torch.Tensor, int, int]:
        """-> (sum over all elements of rec_loss, number of frames N, number of elements)"""
        n = x.shape[0] * (x.shape[2] if x.dim() == 5 else 1)
        count = x.numel()
        total = reduce(L.RED_ABS_DIFF if self.rec_loss == "l1" else L.RED_SQ_DIFF, xhat, x)
        if perceptual and self.perceptual_weight > 0:
            p_loss = self.perceptual_loss(self._frames(x).contiguous(), self._frames(xhat).contiguous())  # [N,1,1,1]
            total = total + (self.perceptual_weight * (count // n)) * reduce(L.RED_IDENT, p_loss)
        return total, n, count

    @staticmethod
    def _nll(rec_sum: torch.Tensor, logvar: torch.Tensor, n: int, count: int) -> torch.Tensor:
        """sum(rec / exp(logvar) + logvar) / N from the sum of rec"""
        return (rec_sum / torch.exp(logvar) + logvar * float(count)) / n

    @staticmethod
    def _weighted(nll: torch.Tensor, weights) -> torch.Tensor:
        if weights is None:
            return nll
        if isinstance(weights, torch.Tensor):
            if weights.numel() != 1:
                raise NotImplementedError("per-element `weights` (a full tensor) are not supported: None, a number or a 0-dim tensor")
            weights = weights.reshape(()).to(nll.device)
        return weights * nll

    def _disc_input(self, x: torch.Tensor) -> torch.Tensor:
        """the reference's rule: a discriminator that is not the 2-D NLayerDiscriminator sees the 5-D clip, that one sees frames"""
        if self.dims > 2 and type(self.discriminator).__name__ == "NLayerDiscriminator":
            x = self._frames(x)
        return x.contiguous()

    def calculate_adaptive_weight(self, nll_loss: torch.Tensor, g_loss: torch.Tensor, last_layer: torch.Tensor) -> torch.Tensor:
        nll_grads = torch.autograd.grad(nll_loss, last_layer, retain_graph=True)[0]
        g_grads = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
        d_weight = torch.sqrt(reduce(L.RED_SQ, nll_grads.detach())) / (torch.sqrt(reduce(L.RED_SQ, g_grads.detach())) + 1e-4)
        d_weight = torch.clamp(d_weight, 0.0, 1e4).detach()
        return d_weight * self.discriminator_weight

    def _generator_terms(self, recs: torch.Tensor, nll_loss: torch.Tensor, global_step: int, last_layer, adaptive: bool):
        dev = recs.device
        if global_step >= self.discriminator_iter_start or not self.training:
            logits_fake = self.discriminator(self._disc_input(recs))
            g_loss = -(reduce(L.RED_IDENT, logits_fake) / logits_fake.numel())
            if self.training and adaptive:
                d_weight = self.calculate_adaptive_weight(nll_loss, g_loss, last_layer=last_layer)
            elif self.training:
                d_weight = torch.tensor(float(self.discriminator_weight)).to(dev)
            else:
                d_weight = torch.tensor(1.0).to(dev)
        else:
            d_weight = torch.tensor(0.0).to(dev)
            g_loss = torch.tensor(0.0, requires_grad=True).to(dev)
        return g_loss, d_weight

    def _regularized(self, loss: torch.Tensor, regularization_log: Dict[str, torch.Tensor], split: str) -> Tuple[torch.Tensor, dict]:
        log = dict()
        for k in regularization_log:
            if k in self.regularization_weights:
                loss = loss + self.regularization_weights[k] * regularization_log[k]
            if k in self.additional_log_keys:
                log[f"{split}/{k}"] = _mean(regularization_log[k])
        return loss, log

    def _discriminator_step(self, inputs: torch.Tensor, recs: torch.Tensor, global_step: int, split: str):
        logits_real = self.discriminator(self._disc_input(inputs).detach())
        logits_fake = self.discriminator(self._disc_input(recs).detach())
        if global_step >= self.discriminator_iter_start or not self.training:
            neg, pos = ((L.RED_HINGE_NEG, L.RED_HINGE_POS) if self.disc_loss == "hinge" else (L.RED_SOFTPLUS_NEG, L.RED_SOFTPLUS_POS))
            d_loss = self.disc_factor * (0.5 * (reduce(neg, logits_real) / logits_real.numel()
                                                + reduce(pos, logits_fake) / logits_fake.numel()))
        else:
            d_loss = torch.tensor(0.0, requires_grad=True).to(recs.device)
        log = {
            f"{split}/loss/disc": d_loss.detach().clone(),
            f"{split}/logits/real": _mean(logits_real),
            f"{split}/logits/fake": _mean(logits_fake),
        }
        return d_loss, log

    def forward(
        self,
        inputs: torch.Tensor,
        reconstructions: torch.Tensor,
        *,
        regularization_log: Dict[str, torch.Tensor],
        optimizer_idx: int,
        global_step: int,
        last_layer: torch.Tensor,
        split: str = "train",
        weights: Union[None, float, torch.Tensor] = None,
    ) -> Tuple[torch.Tensor, dict]:
        self._check_clips(inputs, reconstructions)
        if optimizer_idx == 0:
            rec_sum, n, count = self._rec_sum(inputs, reconstructions, perceptual=True)
            nll_loss = self._nll(rec_sum, self.logvar, n, count)
            weighted_nll_loss = self._weighted(nll_loss, weights)
            g_loss, d_weight = self._generator_terms(reconstructions, nll_loss, global_step, last_layer, self.adaptive_disc_weight)
            loss = weighted_nll_loss + d_weight * self.disc_factor * g_loss
            loss, log = self._regularized(loss, regularization_log, split)
            log.update({
                f"{split}/loss/total": loss.detach().clone(),
                f"{split}/loss/nll": nll_loss.detach(),
                f"{split}/loss/rec": rec_sum.detach() / count,
                f"{split}/loss/g": g_loss.detach(),
                f"{split}/scalars/logvar": self.logvar.detach(),
                f"{split}/scalars/d_weight": d_weight.detach(),
            })
            return loss, log
        elif optimizer_idx == 1:
            return self._discriminator_step(inputs, reconstructions, global_step, split)
        raise NotImplementedError(f"Unknown optimizer_idx {optimizer_idx}")


class _FrameMapTargets:
    """the 2-D term's targets of the two constraint losses: "slice" is the strided view read in place, "mean" and "random" are frame
    maps of cvvae_reduce_sum_frames (no materialised target).  The random frames are drawn on the CPU with the reference's own
    expression, so a seeded global generator reproduces its draw; `generator=` seeds the draw, `frame_indices=` replaces it."""

    def draw_frame_indices(self, t: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """target_type "random": frame 0, then one frame of every group of time_n_compress (discriminator_loss.py:855-862)"""
        d = (t - 1) // self.time_n_compress
        indices = torch.cat(
            [
                torch.tensor([0]),
                torch.randint(1, self.time_n_compress + 1, (d,), generator=generator)
                + torch.arange(d) * self.time_n_compress,
            ]
        )
        return indices

    def _rec2d_sum(self, inputs: torch.Tensor, recs2d: torch.Tensor, generator, frame_indices) -> Tuple[torch.Tensor, int, int]:
        """-> (sum of the 2-D term's rec_loss against the target frames of `inputs`, frames N2, elements), nothing materialised"""
        b, c, t, h, w = inputs.shape
        n = self.time_n_compress
        op = L.RED_ABS_DIFF if self.rec_loss == "l1" else L.RED_SQ_DIFF
        if self.target_type == "mean" and (t - 1) % n:
            raise ValueError(f'target_type="mean": the {t - 1} frames behind the first do not split into groups of {n}')
        if self.target_type == "random":
            if frame_indices is None:
                frame_indices = self.draw_frame_indices(t, generator)
            index = [int(i) for i in (frame_indices.tolist() if isinstance(frame_indices, torch.Tensor) else frame_indices)]
            if len(index) != 1 + (t - 1) // n or any(i < 0 or i >= t for i in index):
                raise ValueError(f"frame_indices: {1 + (t - 1) // n} frame numbers in [0, {t}); got {index}")
            frames2d = len(index)
        else:
            frames2d = 1 + (t - 1) // n if self.target_type == "mean" else len(range(0, t, n))
        want = (b, c, frames2d, h, w)
        if tuple(recs2d.shape) != want:
            raise ValueError(f'dims={self.dims}: reconstructions_2d must be {want} (target_type="{self.target_type}", time_n_compress='
                             f"{n}, inputs {tuple(inputs.shape)}); got {tuple(recs2d.shape)}")
        if self.target_type == "slice":
            total = reduce(op, recs2d, inputs[:, :, ::n, :, :])
        elif self.target_type == "mean":
            total = reduce_frames(op, recs2d, inputs, L.FMAP_GROUP_MEAN, group=n)
        else:
            total = reduce_frames(op, recs2d, inputs, L.FMAP_GATHER, index=index)
        return total, b * frames2d, recs2d.numel()


class LPIPSWithDiscriminatorAndDomainConstraint(_FrameMapTargets, GeneralLPIPSWithDiscriminator):
    def __init__(
        self,
        disc_start: int,
        logvar_init: float = 0.0,
        disc_num_layers: int = 3,
        disc_in_channels: int = 3,
        disc_factor: float = 1.0,
        disc_weight: float = 1.0,
        perceptual_weight: float = 1.0,
        disc_loss: str = "hinge",
        rec_loss: str = "l1",
        scale_input_to_tgt_size: bool = False,
        dims: int = 2,
        learn_logvar: bool = False,
        regularization_weights: Union[None, Dict[str, float]] = None,
        additional_log_keys: Optional[List[str]] = None,
        discriminator_config: Optional[Dict] = None,
        time_n_compress: int = 4,
        rec2d_weight: float = 1.0,
        target_type: str = "slice",
        *,
        discriminator: Optional[nn.Module] = None,
        frame_maps: bool = False,
    ):
        super().__init__(disc_start, logvar_init, disc_num_layers, disc_in_channels, disc_factor, disc_weight, perceptual_weight,
                         disc_loss, rec_loss, scale_input_to_tgt_size, dims, learn_logvar, regularization_weights,
                         additional_log_keys, discriminator_config, discriminator=discriminator)
        self.time_n_compress = time_n_compress
        self.logvar_2d = nn.Parameter(torch.full((), logvar_init), requires_grad=learn_logvar)
        self.rec2d_weight = rec2d_weight
        assert target_type in ["random", "slice", "mean"]
        if target_type != "slice" and not frame_maps:
            raise NotImplementedError(f'target_type="{target_type}" is not supported without frame_maps=True: by default only "slice" '
                                      "(every time_n_compress-th frame, read in place as a strided view); frame_maps=True reads the "
                                      '"mean" and "random" targets through cvvae_reduce_sum_frames')
        self.target_type = target_type
        self.frame_maps = bool(frame_maps)

    def get_trainable_autoencoder_parameters(self) -> Iterator[nn.Parameter]:
        if self.learn_logvar:
            for param in [self.logvar, self.logvar_2d]:
                yield param
        yield from ()

    def forward(
        self,
        inputs: torch.Tensor,
        reconstructions: torch.Tensor,
        reconstructions_2d: torch.Tensor,
        *,
        regularization_log: Dict[str, torch.Tensor],
        optimizer_idx: int,
        global_step: int,
        last_layer: torch.Tensor,
        split: str = "train",
        weights: Union[None, float, torch.Tensor] = None,
        generator: Optional[torch.Generator] = None,
        frame_indices=None,
    ) -> Tuple[torch.Tensor, dict]:
        assert self.dims > 2
        self._check_clips(inputs, reconstructions)
        if self.frame_maps:
            ops._need_gpu(reconstructions_2d)
            if reconstructions_2d.dim() != 5:
                raise ValueError(f"dims={self.dims}: reconstructions_2d must be a 5-D tensor; got {tuple(reconstructions_2d.shape)}")
        else:
            if generator is not None or frame_indices is not None:
                raise ValueError("generator= / frame_indices= seed the frame maps: construct the loss with frame_maps=True")
            targets_2d = inputs[:, :, :: self.time_n_compress, :, :]
            self._check_clips(targets_2d, reconstructions_2d, "reconstructions_2d (against inputs[:, :, ::time_n_compress])")
        if optimizer_idx == 0:
            rec_sum, n, count = self._rec_sum(inputs, reconstructions, perceptual=True)
            if self.frame_maps:
                rec2d_sum, n2, count2 = self._rec2d_sum(inputs, reconstructions_2d, generator, frame_indices)
            else:
                rec2d_sum, n2, count2 = self._rec_sum(targets_2d, reconstructions_2d, perceptual=False)
            rec2d_loss = self._nll(rec2d_sum, self.logvar_2d, n2, count2)
            nll_loss = self._nll(rec_sum, self.logvar, n, count)
            weighted_nll_loss = self._weighted(nll_loss, weights) + self.rec2d_weight * rec2d_loss
            nll_loss = nll_loss + self.rec2d_weight * rec2d_loss
            g_loss, d_weight = self._generator_terms(reconstructions, nll_loss, global_step, last_layer, True)
            loss = weighted_nll_loss + d_weight * self.disc_factor * g_loss
            loss, log = self._regularized(loss, regularization_log, split)
            log.update({
                f"{split}/loss/total": loss.detach().clone(),
                f"{split}/loss/nll": nll_loss.detach(),
                f"{split}/loss/rec": rec_sum.detach() / count,
                f"{split}/loss/rec2d": rec2d_sum.detach() / count2,
                f"{split}/loss/g": g_loss.detach(),
                f"{split}/scalars/logvar": self.logvar.detach(),
                f"{split}/scalars/logvar_2d": self.logvar_2d.detach(),
                f"{split}/scalars/d_weight": d_weight.detach(),
            })
            return loss, log
        elif optimizer_idx == 1:
            return self._discriminator_step(inputs, reconstructions, global_step, split)
        raise NotImplementedError(f"Unknown optimizer_idx {optimizer_idx}")


class LPIPSWithDiscriminatorAndAllConstraint(_FrameMapTargets, GeneralLPIPSWithDiscriminator):
    """discriminator_loss.py:768-1013, the loss of AutoencodingEngineWithAllConstraint (a frozen 2-D encoder AND a frozen 2-D decoder):
    `reconstructions` [2B,3,T,H,W] holds the decodings of the 3-D encoder's latents and then of the frozen 2-D encoder's, `inputs`
    [B,3,T,H,W] stands for cat([inputs, inputs]) -- the pixel sum reads it through a stride-0 outer dimension, LPIPS and the
    discriminator's "real" pass get the doubled tensor as in the reference.  All three `target_type`s of the 2-D term: "slice" is the
    strided view read in place, "mean" and "random" are frame maps of cvvae_reduce_sum_frames (no materialised target).  The random
    frames are drawn on the CPU with the reference's own expression, so a seeded global generator reproduces its draw;
    `generator=` seeds the draw, `frame_indices=` replaces it (both for reproducible tests)."""

    def __init__(
        self,
        disc_start: int,
        logvar_init: float = 0.0,
        disc_num_layers: int = 3,
        disc_in_channels: int = 3,
        disc_factor: float = 1.0,
        disc_weight: float = 1.0,
        perceptual_weight: float = 1.0,
        disc_loss: str = "hinge",
        rec_loss: str = "l1",
        scale_input_to_tgt_size: bool = False,
        dims: int = 2,
        learn_logvar: bool = False,
        regularization_weights: Union[None, Dict[str, float]] = None,
        additional_log_keys: Optional[List[str]] = None,
        discriminator_config: Optional[Dict] = None,
        time_n_compress: int = 4,
        rec2d_weight: float = 1.0,
        target_type: str = "slice",
        *,
        discriminator: Optional[nn.Module] = None,
    ):
        super().__init__(disc_start, logvar_init, disc_num_layers, disc_in_channels, disc_factor, disc_weight, perceptual_weight,
                         disc_loss, rec_loss, scale_input_to_tgt_size, dims, learn_logvar, regularization_weights,
                         additional_log_keys, discriminator_config, discriminator=discriminator)
        self.time_n_compress = time_n_compress
        self.logvar_2d = nn.Parameter(torch.full((), logvar_init), requires_grad=learn_logvar)
        self.rec2d_weight = rec2d_weight
        assert target_type in ["random", "slice", "mean"]
        self.target_type = target_type

    def get_trainable_autoencoder_parameters(self) -> Iterator[nn.Parameter]:
        if self.learn_logvar:
            for param in [self.logvar, self.logvar_2d]:
                yield param
        yield from ()

    def forward(
        self,
        inputs: torch.Tensor,
        reconstructions: torch.Tensor,
        reconstructions_2d: torch.Tensor,
        *,
        regularization_log: Dict[str, torch.Tensor],
        optimizer_idx: int,
        global_step: int,
        last_layer: torch.Tensor,
        split: str = "train",
        weights: Union[None, float, torch.Tensor] = None,
        generator: Optional[torch.Generator] = None,
        frame_indices=None,
    ) -> Tuple[torch.Tensor, dict]:
        assert self.dims > 2
        for x in (inputs, reconstructions, reconstructions_2d):
            ops._need_gpu(x)
        if inputs.dim() != 5 or reconstructions.dim() != 5 or reconstructions_2d.dim() != 5 or \
                tuple(reconstructions.shape) != (2 * inputs.shape[0], *inputs.shape[1:]):
            raise ValueError(f"dims={self.dims}: inputs [B,3,T,H,W] and reconstructions [2B,3,T,H,W] (the 3-D encoder's half, then the "
                             f"2-D encoder's); got {tuple(inputs.shape)} and {tuple(reconstructions.shape)}")
        b, c, t, h, w = inputs.shape
        if optimizer_idx == 0:
            rec2d_sum, n2, count2 = self._rec2d_sum(inputs, reconstructions_2d, generator, frame_indices)
            # cat([inputs, inputs]) as a stride-0 outer dimension: [2,B,3,T,H,W] against the reconstructions' two halves
            op = L.RED_ABS_DIFF if self.rec_loss == "l1" else L.RED_SQ_DIFF
            rec_sum = reduce(op, reconstructions.unflatten(0, (2, b)), inputs.unsqueeze(0).expand(2, *inputs.shape))
            n, count = 2 * b * t, 2 * inputs.numel()
            if self.perceptual_weight > 0:
                doubled = torch.cat([inputs, inputs], dim=0)
                p_loss = self.perceptual_loss(self._frames(doubled).contiguous(), self._frames(reconstructions).contiguous())
                rec_sum = rec_sum + (self.perceptual_weight * (count // n)) * reduce(L.RED_IDENT, p_loss)
            rec2d_loss = self._nll(rec2d_sum, self.logvar_2d, n2, count2)
            nll_loss = self._nll(rec_sum, self.logvar, n, count)
            weighted_nll_loss = self._weighted(nll_loss, weights) + self.rec2d_weight * rec2d_loss
            nll_loss = nll_loss + self.rec2d_weight * rec2d_loss
            g_loss, d_weight = self._generator_terms(reconstructions, nll_loss, global_step, last_layer, True)
            loss = weighted_nll_loss + d_weight * self.disc_factor * g_loss
            loss, log = self._regularized(loss, regularization_log, split)
            log.update({
                f"{split}/loss/total": loss.detach().clone(),
                f"{split}/loss/nll": nll_loss.detach(),
                f"{split}/loss/rec": rec_sum.detach() / count,
                f"{split}/loss/rec2d": rec2d_sum.detach() / count2,
                f"{split}/loss/g": g_loss.detach(),
                f"{split}/scalars/logvar": self.logvar.detach(),
                f"{split}/scalars/logvar_2d": self.logvar_2d.detach(),
                f"{split}/scalars/d_weight": d_weight.detach(),
            })
            return loss, log
        elif optimizer_idx == 1:
            return self._discriminator_step(torch.cat([inputs, inputs], dim=0), reconstructions, global_step, split)
        raise NotImplementedError(f"Unknown optimizer_idx {optimizer_idx}")
