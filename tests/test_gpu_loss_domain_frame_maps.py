"""LPIPSWithDiscriminatorAndDomainConstraint(frame_maps=True) on a real MI355X: the "random" (given frame indices) and "mean"
targets of the 2-D term read through cvvae_reduce_sum_frames must give, BIT FOR BIT, the loss, the logs and every gradient of a
test subclass that materialises the target and sums it with the plain reduction -- the equality
tests/test_gpu_train_constraint.py::test_one_step_of_the_family asserts for the all-constraint class, whose code this class shares.
"mean" with (T-1) % n != 0 raises ValueError; without the keyword the class refuses both at construction."""
import pytest
import torch

from oracle.seeded import seeded_input
from tests import lpips_ref
from tests.test_gpu_loss import Disc
from tests.test_gpu_train_constraint import _mean_target

pytestmark = pytest.mark.gpu
INDICES = [0, 3]


def _run(dtype, target_type, materialised):
    from cvvae_amd import _lib as L
    from cvvae_amd import loss as loss_mod
    from cvvae_amd.loss import DiagonalGaussianRegularizer, LPIPSWithDiscriminatorAndDomainConstraint

    class Materialised(LPIPSWithDiscriminatorAndDomainConstraint):
        def _rec2d_sum(self, inputs, recs2d, generator, frame_indices):
            tgt = inputs[:, :, list(frame_indices)].contiguous() if self.target_type == "random" else _mean_target(inputs, self.time_n_compress)
            op = L.RED_ABS_DIFF if self.rec_loss == "l1" else L.RED_SQ_DIFF
            return loss_mod.reduce(op, recs2d.contiguous(), tgt), tgt.shape[0] * tgt.shape[2], tgt.numel()

    cls = Materialised if materialised else LPIPSWithDiscriminatorAndDomainConstraint
    m = cls(disc_start=10, dims=3, learn_logvar=True, logvar_init=1.0, perceptual_weight=0.7, disc_factor=0.8, disc_weight=0.6,
            rec2d_weight=0.5, regularization_weights={"kl_loss": 1e-3}, discriminator=Disc(), target_type=target_type, frame_maps=True)
    m.perceptual_loss.load_state_dict(lpips_ref.lpips_state_dict(3), strict=True)
    m.perceptual_loss.to(dtype)
    m = m.cuda().train()
    x = seeded_input((1, 3, 5, 32, 32), 40).to(dtype).cuda()
    feat = seeded_input((1, 3, 5, 32, 32), 45).cuda()
    lv = {"base": (x.float() + 0.3 * seeded_input((1, 3, 5, 32, 32), 41).cuda()).clamp(-1, 1).requires_grad_(True),
          "xhat2d": (x.float()[:, :, ::4] + 0.2 * seeded_input((1, 3, 2, 32, 32), 42).cuda()).clamp(-1, 1).requires_grad_(True),
          "moments": (1.5 * seeded_input((1, 32, 2, 4, 4), 43)).to(dtype).cuda().requires_grad_(True),
          "last": torch.tensor([0.05, -0.04, 0.03], device="cuda", requires_grad=True)}
    z, rlog = DiagonalGaussianRegularizer()(lv["moments"], noise=seeded_input((1, 16, 2, 4, 4), 44).to(dtype).cuda())
    xhat = (lv["base"] + lv["last"].view(1, 3, 1, 1, 1) * feat + 0.01 * z.float()[:, :3, :1, :1, :1]).to(dtype)
    kw = dict(frame_indices=INDICES) if target_type == "random" else {}
    loss, log = m(x, xhat, lv["xhat2d"].to(dtype), regularization_log=rlog, optimizer_idx=0, global_step=20, last_layer=lv["last"], **kw)
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach(), **{"log:" + k: v.detach() for k, v in log.items()}}
    for n, t in {**lv, "logvar": m.logvar, "logvar_2d": m.logvar_2d, "disc.gain": m.discriminator.gain}.items():
        if t.grad is not None:
            out["grad:" + n] = t.grad
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("target_type", ["random", "mean"])
def test_frame_mapped_target_equals_the_materialised_one_bit_for_bit(target_type, dtype):
    got, want = _run(dtype, target_type, False), _run(dtype, target_type, True)
    assert sorted(got) == sorted(want)
    assert {"grad:base", "grad:xhat2d", "grad:moments", "grad:last", "grad:logvar", "grad:logvar_2d", "log:train/loss/rec2d"} <= set(got)
    bad = [k for k in got if not torch.equal(got[k], want[k])]
    assert not bad, {k: float((got[k].double() - want[k].double()).abs().max()) for k in bad}
    assert float(got["log:train/loss/rec2d"]) > 0.0 and float(got["grad:xhat2d"].abs().sum()) > 0.0 and bool(torch.isfinite(got["loss"]))
    if target_type == "random":   # another draw is another loss: the indices reach the kernel
        from cvvae_amd.loss import LPIPSWithDiscriminatorAndDomainConstraint as D
        m = D(disc_start=10, dims=3, perceptual_weight=0.0, discriminator=Disc(), target_type="random", frame_maps=True).cuda()
        x = seeded_input((1, 3, 5, 32, 32), 40).to(dtype).cuda()
        r2 = torch.zeros(1, 3, 2, 32, 32, dtype=dtype, device="cuda")
        sums = [m._rec2d_sum(x, r2, None, idx)[0] for idx in ([0, 3], [0, 4], [0, 3])]
        assert torch.equal(sums[0], sums[2]) and not torch.equal(sums[0], sums[1])


def test_mean_refuses_frames_that_do_not_split_into_groups_and_the_default_stays():
    from cvvae_amd.loss import LPIPSWithDiscriminatorAndDomainConstraint as D
    m = D(disc_start=10, dims=3, perceptual_weight=0.0, discriminator=Disc(), target_type="mean", frame_maps=True).cuda().train()
    x = seeded_input((1, 3, 7, 16, 16), 1).cuda()             # (7 - 1) % 4 != 0
    last = torch.zeros(3, device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match='target_type="mean"'):
        m(x, x.clone(), x[:, :, :2].clone(), regularization_log={}, optimizer_idx=0, global_step=0, last_layer=last)
    with pytest.raises(NotImplementedError, match="frame_maps=True"):
        D(disc_start=10, dims=3, discriminator=Disc(), target_type="mean")
    plain = D(disc_start=10, dims=3, perceptual_weight=0.0, discriminator=Disc()).cuda().train()
    with pytest.raises(ValueError, match="frame_maps=True"):
        plain(x, x.clone(), x[:, :, ::4].clone(), regularization_log={}, optimizer_idx=0, global_step=0, last_layer=last, frame_indices=[0, 1])
