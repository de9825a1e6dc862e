"""The small engines the training-engine tests build (tests/test_train_engine_contract.py, test_train_engine_host_logic.py,
test_gpu_train_engine.py): the training YAML's entries (configs/cvvae_sd3_constraint_training.yaml, verbatim keys) with the widths
and depths cut, every network loaded with a seeded state dict, and the hand-assembled sequence of the same public calls that one
iteration of an engine must equal.

"latent": AutoencodingEngineWithLatentConstraint over the vae3d_sd3 family and the frozen SD3 2-D decoder (the shipped YAML).
"all":    AutoencodingEngineWithAllConstraint over the SD2.1-compatible family and its frozen 2-D halves (SMALL3D / SMALL2D of
          tests/test_gpu_train_constraint.py)."""
import contextlib
import copy
import warnings

import torch

from oracle.seeded import seeded_state_dict

# the GPU tests' widths: the sd3 widths with layers_per_block = 1; the CPU tests cut a level as tests/test_training_config_path.py does,
# which leaves one temporal halving: their networks compress time by 2, the loss's and the engine's time_n_compress follow
SD3_GPU = dict(block_out_channels=[128, 256, 512, 512], layers_per_block=1)
SD3_CPU = dict(block_out_channels=[128, 256, 256], layers_per_block=1)
SMALL3D = dict(ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=1)
SMALL2D = dict(ch=128, out_ch=3, ch_mult=[1, 2, 4, 4], num_res_blocks=1, attn_resolutions=[], dropout=0.0, in_channels=3, resolution=32,
               z_channels=4, double_z=True)
SMALL3D_CPU = dict(ch=128, ch_mult=[1, 2, 2], num_res_blocks=1)
SMALL2D_CPU = dict(SMALL2D, ch_mult=[1, 2, 2])

YAML_DISC = dict(target="lvdm.modules.autoencoding.lpips.model.model.NLayerDiscriminator3D",
                 params=dict(input_nc=3, ndf=64, n_layers=4, use_actnorm=False, causal=False, half_3d=False))
YAML_OPT = dict(target="cvvae_amd.optim.AdamW", params=dict(betas=[0.9, 0.98], eps=1.0e-4, weight_decay=0.01, max_grad_norm=1.0))
YAML_COSINE = dict(target="lvdm.lr_scheduler.get_scheduler",
                   params=dict(name="cosine", num_warmup_steps=1000, num_training_steps=60000, min_lr_ratio=0.005))
BASE_LR = 2.0e-5


def _loss(target_type, frame_maps, cls, n):
    params = dict(perceptual_weight=0.5, disc_start=1, disc_weight=0.5, learn_logvar=True, rec_loss="l1", dims=3, time_n_compress=n,
                  rec2d_weight=1.0, target_type=target_type, regularization_weights=dict(kl_loss=1.0),
                  discriminator_config=copy.deepcopy(YAML_DISC))
    if frame_maps:
        params["frame_maps"] = True
    return dict(target="lvdm.modules.autoencoding.losses." + cls, params=params)


def time_n_compress(gpu):
    return 4 if gpu else 2


def latent_config(widths, target_type="random", tn=4, **engine):
    n = len(widths["block_out_channels"])
    common = dict(norm_num_groups=32, act_fn="silu", mid_block_add_attention=True, **widths)
    params = dict(
        input_key="frames", monitor="train/loss/rec", disc_start_iter=0,
        encoder_config=dict(target="lvdm.modules.diffusionmodules.vae_models3d_sd3.Encoder3D", params=dict(
            in_channels=3, out_channels=16, down_block_types=["DownEncoderBlock3D"] * n, double_z=True, causal=True, half_3d=True, **common)),
        decoder_config=dict(target="lvdm.modules.diffusionmodules.vae_models3d_sd3.Decoder3D", params=dict(
            in_channels=16, out_channels=3, up_block_types=["UpDecoderBlock3D"] * n, causal=False, half_3d=True, **common)),
        constraint_decoder_config=dict(target="lvdm.modules.diffusionmodules.vae_models_sd3.DecoderWith3DWrapper", params=dict(
            in_channels=16, out_channels=3, up_block_types=["UpDecoderBlock2D"] * n, **common)),
        regularizer_config=dict(target="lvdm.modules.autoencoding.regularizers.DiagonalGaussianRegularizer"),
        loss_config=_loss(target_type, target_type != "slice", "LPIPSWithDiscriminatorAndDomainConstraint", tn),
        optimizer_config=copy.deepcopy(YAML_OPT), lr_g_factor=2, lr_g_scheduler_config=copy.deepcopy(YAML_COSINE))
    params.update(engine)
    return dict(model=dict(base_learning_rate=BASE_LR, target="lvdm.models.autoencoder.AutoencodingEngineWithLatentConstraint",
                           params=params))


def all_config(small3d, small2d, target_type="random", tn=4, **engine):
    c3 = dict(out_ch=3, attn_resolutions=[], dropout=0.0, in_channels=3, z_channels=4, double_z=True, use_3d_conv=True, half_3d=True,
              resolution=32, **small3d)
    params = dict(
        input_key="frames", disc_start_iter=0, time_n_compress=tn,
        encoder_config=dict(target="lvdm.modules.diffusionmodules.model_3d.Encoder", params=dict(c3, attn_type="vanilla-xformers", causal=True)),
        decoder_config=dict(target="lvdm.modules.diffusionmodules.model_3d.Decoder",
                            params=dict(c3, attn_type="spatial-temporal-xformer", causal=False)),
        constraint_encoder_config=dict(target="lvdm.modules.diffusionmodules.model.EncoderWith3DWrapper", params=dict(small2d)),
        constraint_decoder_config=dict(target="lvdm.modules.diffusionmodules.model.DecoderWith3DWrapper", params=dict(small2d)),
        regularizer_config=dict(target="lvdm.modules.autoencoding.regularizers.DiagonalGaussianRegularizer"),
        loss_config=_loss(target_type, False, "LPIPSWithDiscriminatorAndAllConstraint", tn),
        optimizer_config=copy.deepcopy(YAML_OPT), lr_g_factor=2, lr_g_scheduler_config=copy.deepcopy(YAML_COSINE))
    params.update(engine)
    return dict(model=dict(base_learning_rate=BASE_LR, target="lvdm.models.autoencoder.AutoencodingEngineWithAllConstraint", params=params))


def config(kind, gpu, **engine):
    if kind == "latent":
        return latent_config(SD3_GPU if gpu else SD3_CPU, tn=time_n_compress(gpu), **engine)
    return all_config(SMALL3D if gpu else SMALL3D_CPU, SMALL2D if gpu else SMALL2D_CPU, tn=time_n_compress(gpu), **engine)


SEEDS = dict(encoder=7, decoder=8, constraint_encoder=3, constraint_decoder=4)


def seed_engine(engine):
    """every network gets a seeded state dict (the discriminator: tests/disc_ref.py's, LPIPS: tests/lpips_ref.py's); the EMA shadows,
    copies taken at construction, are taken again"""
    from tests import disc_ref, lpips_ref
    for name, seed in SEEDS.items():
        net = getattr(engine, name, None)
        if net is not None:
            net.load_state_dict(seeded_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed), strict=True)
    engine.loss.discriminator.load_state_dict(disc_ref.seeded_state())
    engine.loss.perceptual_loss.load_state_dict(lpips_ref.lpips_state_dict(3), strict=True)
    engine._build_ema()
    return engine


def net_cfg(kind, gpu):
    """the widths as oracle/cvvae_oracle.py takes them"""
    if kind == "latent":
        return dict(SD3_GPU if gpu else SD3_CPU)
    return dict(SMALL3D if gpu else SMALL3D_CPU)


NETWORKS = ("encoder", "decoder", "constraint_encoder", "constraint_decoder")


def to_device(engine, dtype, device="cuda"):
    """the networks, LPIPS and the discriminator in `dtype` (the logvars stay fp32), the EMA shadows taken again in that dtype"""
    for n in NETWORKS:
        if hasattr(engine, n):
            getattr(engine, n).to(dtype)
    engine.loss.perceptual_loss.to(dtype)
    engine.loss.discriminator.to(dtype)
    engine._build_ema()
    return engine.to(device)


def build(kind, gpu, **engine):
    from lvdm.models.autoencoder import build_from_config
    return seed_engine(build_from_config(config(kind, gpu, **engine))).train()


# ---- the hand-assembled sequence: the same public calls, written out ----
class ByHand:
    """what one iteration of the engine is made of, from the networks, the loss, the regulariser, two optimizers, two schedulers and
    a LitEma handed to it (an engine's own submodules, or another copy of them): lvdm/models/autoencoder.py:355-378, 1057-1116,
    1518-1589 with Lightning's toggle_model and clip_gradients written out"""

    def __init__(self, kind, mods, lr=BASE_LR, lr_g_factor=2, ema=None, disc_start_iter=0, tn=4, optimizer_config=None,
                 lr_g_scheduler_config=None):
        from lvdm.util import get_obj_from_str
        self.kind, self.m, self.ema, self.disc_start_iter, self.tn = kind, mods, ema, disc_start_iter, tn
        loss = mods["loss"]
        self.ae_params = list(loss.get_trainable_autoencoder_parameters()) + list(mods["encoder"].parameters()) + list(mods["decoder"].parameters())
        self.disc_params = list(loss.get_trainable_parameters())
        oc = optimizer_config or YAML_OPT
        sc = lr_g_scheduler_config or YAML_COSINE
        make = get_obj_from_str(oc["target"])
        self.opts = [make(self.ae_params, lr=lr_g_factor * lr, **oc.get("params", {})), make(self.disc_params, lr=lr, **oc.get("params", {}))]
        self.sches = [get_obj_from_str(sc["target"])(optimizer=self.opts[0], **sc.get("params", {})),
                      get_obj_from_str(YAML_COSINE["target"])(optimizer=self.opts[1], name="constant")]
        self.global_step = 0
        self.generator = None
        self.frame_indices = None
        self.seen_requires_grad = None

    def networks(self, x):
        m = self.m
        if self.kind == "latent":
            z, rlog = m["regularization"](m["encoder"](x), generator=self.generator)
            return m["decoder"](z), m["constraint_decoder"](z), rlog
        with torch.no_grad():
            z_d = m["constraint_encoder"](x[:, :, :: self.tn, :, :])
        z, rlog = m["regularization"](torch.cat([m["encoder"](x), z_d], dim=0), generator=self.generator)
        return m["decoder"](z), m["constraint_decoder"](z[: z.shape[0] // 2]), rlog

    @contextlib.contextmanager
    def toggled(self, idx):
        other = self.disc_params if idx == 0 else self.ae_params
        mine = {id(p) for p in (self.ae_params if idx == 0 else self.disc_params)}
        state = [(p, p.requires_grad) for p in other if id(p) not in mine]
        for p, _ in state:
            p.requires_grad = False
        try:
            yield
        finally:
            for p, flag in state:
                p.requires_grad = flag

    def step(self, x, batch_idx):
        """-> (loss, log, optimizer_idx)"""
        idx = batch_idx % 2
        if self.global_step < self.disc_start_iter:
            idx = 0
        opt = self.opts[idx]
        opt.zero_grad()
        with self.toggled(idx):
            self.seen_requires_grad = [p.requires_grad for p in self.ae_params + self.disc_params]
            xrec, xrec_2d, rlog = self.networks(x)
            kw = dict(frame_indices=self.frame_indices) if self.frame_indices is not None else {}
            loss, log = self.m["loss"](x, xrec, xrec_2d, regularization_log=rlog, optimizer_idx=idx, global_step=self.global_step,
                                       last_layer=self.m["decoder"].get_last_layer(), split="train", **kw)
            loss.backward()
            if getattr(opt, "max_grad_norm", None) is None:     # (max_grad_norm=1.0: the clip is inside the step)
                from cvvae_amd.optim import clip_grad_norm_
                clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], 1.0)
        opt.step()
        self.global_step += 1
        with warnings.catch_warnings():   # (the scheduler of the optimizer that did not step this iteration steps too)
            warnings.filterwarnings("ignore", message=r"Detected call of `lr_scheduler.step\(\)` before `optimizer.step\(\)`")
            for s in self.sches:
                s.step()
        if self.ema is not None:
            self.ema(self.ema_model)
        return loss.detach(), log, idx


def modules_of(engine):
    return {n: getattr(engine, n) for n in ("encoder", "decoder", "loss", "regularization", "constraint_encoder", "constraint_decoder")
            if hasattr(engine, n)}
