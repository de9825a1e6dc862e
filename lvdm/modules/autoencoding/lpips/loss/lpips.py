"""`lvdm.modules.autoencoding.lpips.loss.lpips` as the reference's losses import it (`from ..lpips.loss.lpips import LPIPS`,
lvdm/modules/autoencoding/losses/discriminator_loss.py; `self.perceptual_loss = LPIPS().eval()`): the frozen VGG16 perceptual metric on
the MI355X kernels, forward and input gradient (cvvae_amd/lpips.py).  The constructor never downloads: weights come through
load_state_dict or LPIPS.from_pretrained(<local file>)."""
from cvvae_amd.lpips import LPIPS, NetLinLayer, ScalingLayer, vgg16  # noqa: F401
