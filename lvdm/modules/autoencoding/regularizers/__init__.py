"""`lvdm.modules.autoencoding.regularizers` as the training YAML names it (`regularizer_config.target:
lvdm.modules.autoencoding.regularizers.DiagonalGaussianRegularizer`): the posterior sample and its KL term on the MI355X kernels,
forward and backward (cvvae_amd/loss.py)."""
from cvvae_amd.loss import DiagonalGaussianRegularizer  # noqa: F401
