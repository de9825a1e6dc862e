"""`lvdm.models.autoencoder` as the training YAML names it (`model.target:
lvdm.models.autoencoder.AutoencodingEngineWithLatentConstraint`, configs/cvvae_sd3_constraint_training.yaml:3): the training
engines as plain `nn.Module`s on the MI355X kernels (cvvae_amd/autoencoder.py).  AutoencodingEngineWithEncoderConstraint, the
legacy / VQ engines and the Lightning hooks of that file are not part of this package."""
from cvvae_amd.autoencoder import (AbstractAutoencoder, AutoencodingEngine, AutoencodingEngineWithAllConstraint,  # noqa: F401
                                   AutoencodingEngineWithLatentConstraint, build_from_config)

__all__ = ["AbstractAutoencoder", "AutoencodingEngine", "AutoencodingEngineWithLatentConstraint",
           "AutoencodingEngineWithAllConstraint", "build_from_config"]
