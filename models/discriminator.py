"""`models.discriminator` of the reference: the 3-D PatchGAN discriminator as a trainable module on the MI355X kernels
(cvvae_amd/discriminator.py)."""
from cvvae_amd.discriminator import NLayerDiscriminator3D, ResnetBlockDown3D, get_cvvae_discriminator, weights_init  # noqa: F401
