"""`lvdm.modules.autoencoding.lpips.model.model` as the reference's training config names it
(`discriminator_config.target: lvdm.modules.autoencoding.lpips.model.model.NLayerDiscriminator3D`,
configs/cvvae_sd3_constraint_training.yaml): the 3-D PatchGAN discriminator as a trainable module on the MI355X kernels
(cvvae_amd/discriminator.py).  The 2-D NLayerDiscriminator / ActNorm of that file are not part of this package."""
from cvvae_amd.discriminator import NLayerDiscriminator3D, ResnetBlockDown3D, weights_init  # noqa: F401
