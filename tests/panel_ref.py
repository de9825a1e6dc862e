"""cvvae_recon_panels restated twice, on whatever device the operands live:

`panels`        the eager torch expression of the engines' log_images (lvdm/models/autoencoder.py:499-511), in the operands' dtype.
                This is the yardstick: the kernel must give its bits.
`kernel_model`  the kernel's plan -- fp32 arithmetic with one rounding to the dtype wherever eager torch stores a tensor, the scalar
                f multiplied in fp32.  tests/test_train_engine_contract.py holds it to `panels` bit for bit on the CPU, so the plan
                is checked without a device; the GPU test then holds the kernel to `panels`."""
import torch


def frames(x: torch.Tensor) -> torch.Tensor:
    """b c t h w -> (b t) c h w"""
    b, c, t, h, w = x.shape
    return x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)


def panels(x: torch.Tensor, xrec: torch.Tensor, f: float):
    """-> (inputs, reconstructions, diff, diff_boost), each [(B T),3,H,W]"""
    x, xrec = frames(x), frames(xrec)
    diff = 0.5 * torch.abs(torch.clamp(xrec, -1.0, 1.0) - x)
    diff.clamp_(0, 1.0)
    return x, xrec, 2.0 * diff - 1.0, 2.0 * torch.clamp(f * diff, 0.0, 1.0) - 1


def kernel_model(x: torch.Tensor, xrec: torch.Tensor, f: float):
    dt = x.dtype
    rnd = lambda v: v.to(dt).float()  # noqa: E731
    xf, rf = frames(x).float(), frames(xrec).float()
    f32 = torch.tensor(f, dtype=torch.float32)      # the scalar as opmath holds it
    d = rnd(rf.clamp(-1.0, 1.0) - xf).abs()
    h = rnd(0.5 * d).clamp(0.0, 1.0)
    diff = rnd(rnd(2.0 * h) - 1.0)
    g = rnd(f32 * h).clamp(0.0, 1.0)
    boost = rnd(rnd(2.0 * g) - 1.0)
    return frames(x), frames(xrec), diff.to(dt), boost.to(dt)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))
