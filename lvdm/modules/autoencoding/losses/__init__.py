"""`lvdm.modules.autoencoding.losses` as the training YAML names it (`loss_config.target:
lvdm.modules.autoencoding.losses.LPIPSWithDiscriminatorAndDomainConstraint`): the pixel / NLL, KL and GAN terms of the training loss
on the MI355X kernels (cvvae_amd/loss.py).  No discriminator network ships yet: pass `discriminator_config` or `discriminator=`."""
from cvvae_amd.loss import (GeneralLPIPSWithDiscriminator, LPIPSWithDiscriminatorAndAllConstraint,  # noqa: F401
                            LPIPSWithDiscriminatorAndDomainConstraint)

__all__ = ["GeneralLPIPSWithDiscriminator", "LPIPSWithDiscriminatorAndDomainConstraint", "LPIPSWithDiscriminatorAndAllConstraint"]
