"""Drop-in import path of the reference (`lvdm...`): the discriminator of the training loss (cvvae_amd/discriminator.py)."""
