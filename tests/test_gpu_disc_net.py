"""The whole 3-D PatchGAN discriminator (cvvae_amd/discriminator.py) on the MI355X with the seeded weights of tests/disc_ref.py,
forward and the backward walker, against fp64 disc_ref on the CPU (same inputs, same -- dtype-rounded -- weights).

Errors are relative L2; parameter tensors use the floor of tests/test_gpu_grad3d.py (denominator at least 1e-3 of the largest
parameter gradient's norm).  fp16 / bf16 modules: the logits, dL/dx and the worst parameter gradient are each held to 2x the same
figure of disc_ref(round_to=dtype) against fp64 -- the ideal 16-bit execution of the same graph, computed here on the CPU at the
same inputs; the factor 2 covers the other summation order and the fused rounding points (the margin tests/test_gpu_disc_stats.py
uses over its yardstick).  fp32 modules run on the split-precision MFMA path, for which fp32 CPU noise is no yardstick: they are held
to NET_IN_TOL / NET_W_TOL[float32] of tests/test_gpu_grad3d.py, the project's figures for deeper networks on the same kernels.
Shapes: [1,3,5,32,32] (T odd then even at the two pools; the last blocks run at T = 1) and [2,3,9,36,44] (T odd at both pools, an odd
row and column dropped at the second).  Every measured figure goes, with its yardstick, to $CVVAE_TEST_LOG_DIR/disc_net_step_bands.json when that directory is given (the
recorded copy: tests/golden/disc_net_step_bands.json); the asserts use the yardstick computed in the run.
CPU-side yardstick figures at the first shape (logits / dL/dx / worst parameter): bf16 4.3e-3 / 7.6e-2 / 9.0e-2, fp16 4.9e-4 / 1.0e-2 /
1.1e-2; at the second: bf16 7.1e-3 / 6.4e-2 / 7.6e-2, fp16 7.9e-4 / 1.4e-2 / 2.2e-2."""
import json
import os

import pytest
import torch

from oracle.seeded import seeded_input, seeded_tensor
from tests import disc_ref
from tests.test_gpu_grad3d import NET_IN_TOL, NET_W_TOL, rel

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16, torch.float32]
SHAPES = [(1, 3, 5, 32, 32), (2, 3, 9, 36, 44)]
LOGITS = {SHAPES[0]: (1, 1, 1, 4, 4), SHAPES[1]: (2, 1, 2, 4, 5)}
YAML_DISC = {"target": "lvdm.modules.autoencoding.lpips.model.model.NLayerDiscriminator3D",
             "params": {"input_nc": 3, "ndf": 64, "n_layers": 4, "use_actnorm": False, "causal": False, "half_3d": False}}

_REF = {}


def _record(key, figures):
    print(f"\n[disc net {key}] " + "; ".join(f"{k} {v:.3e}" for k, v in figures.items()))
    d = os.environ.get("CVVAE_TEST_LOG_DIR", "")          # a directory that receives the figures of a run; unset: printed only
    if not (d and os.path.isdir(d)):
        return
    path = os.path.join(d, "disc_net_step_bands.json")
    blob = {}
    if os.path.isfile(path):
        with open(path) as f:
            blob = json.load(f)
    blob[key] = {k: float(f"{v:.6e}") for k, v in figures.items()}
    with open(path, "w") as f:
        json.dump(blob, f, indent=1, sort_keys=True)
        f.write("\n")


def _case(shape, dtype):
    """operands and CPU references of one (shape, dtype), computed once: the dtype-rounded weights, input and cotangent, fp64
    disc_ref, and for 16-bit dtypes the round_to yardstick's figures against it"""
    key = (shape, dtype)
    if key not in _REF:
        state = {k: v.to(dtype).float() for k, v in disc_ref.seeded_state().items()}
        x = seeded_input(shape, 3).to(dtype)
        c = torch.randn(LOGITS[shape], generator=torch.Generator().manual_seed(5)).to(dtype).float()
        y, dx, gp = disc_ref.run(state, x.float(), c)
        scale = max(float(g.norm()) for g in gp.values() if g is not None)
        yard = None
        if dtype != torch.float32:
            y2, dx2, gp2 = disc_ref.run(state, x.float(), c, round_to=dtype)
            yard = (rel(y2, y), rel(dx2, dx), max(rel(gp2[k], gp[k], 1e-3 * scale) for k in gp if gp[k] is not None))
        _REF[key] = dict(state=state, x=x, c=c, y=y, dx=dx, gp=gp, scale=scale, yard=yard)
    return _REF[key]


def _module(state, dtype):
    from cvvae_amd.discriminator import get_cvvae_discriminator
    net = get_cvvae_discriminator()
    net.load_state_dict(state, strict=True)
    return net.to(dtype).cuda().train()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", SHAPES)
def test_whole_network_forward_and_backward_vs_fp64(shape, dtype):
    r = _case(shape, dtype)
    net = _module(r["state"], dtype)
    xa = r["x"].cuda().requires_grad_(True)
    y = net(xa)
    assert tuple(y.shape) == LOGITS[shape] and y.dtype == dtype and y.requires_grad
    (y.float() * r["c"].cuda()).sum().backward()
    named = list(net.named_parameters())
    e_y, e_x = rel(y, r["y"]), rel(xa.grad, r["dx"])
    errs = sorted(((rel(p.grad, r["gp"][n], 1e-3 * r["scale"]), n) for n, p in named if ".temb_proj." not in n), reverse=True)
    fig = {"logits": e_y, "dx": e_x, "worst_param": errs[0][0]}
    if r["yard"] is not None:
        fig.update(yard_logits=r["yard"][0], yard_dx=r["yard"][1], yard_worst_param=r["yard"][2])
    else:
        fig.update(bound_logits=NET_IN_TOL[dtype], bound_dx=NET_IN_TOL[dtype], bound_worst_param=NET_W_TOL[dtype])
    _record(f"{'x'.join(map(str, shape))}_{str(dtype)[6:]}", fig)
    print(f"worst parameters: {errs[:3]}")
    # structure of the result
    for n, p in named:
        if ".temb_proj." in n:
            assert p.grad is None, n
        else:
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape, n
    assert xa.grad.dtype == dtype
    # two forward runs: the same bits; a detached input (the discriminator step): the same parameter gradients, bit for bit
    want = {n: p.grad.clone() for n, p in named if p.grad is not None}
    net.zero_grad(set_to_none=True)
    xd = r["x"].cuda()
    y2 = net(xd)
    assert torch.equal(y2, y)
    (y2.float() * r["c"].cuda()).sum().backward()
    assert all(torch.equal(p.grad, want[n]) for n, p in named if n in want)
    with torch.no_grad():
        assert torch.equal(net(xd), y.detach())
    if r["yard"] is not None:
        assert e_y <= 2 * r["yard"][0], (e_y, r["yard"][0])
        assert e_x <= 2 * r["yard"][1], (e_x, r["yard"][1])
        assert errs[0][0] <= 2 * r["yard"][2], (errs[:5], r["yard"][2])
    else:
        assert e_y <= NET_IN_TOL[dtype] and e_x <= NET_IN_TOL[dtype], (e_y, e_x)
        assert errs[0][0] <= NET_W_TOL[dtype], errs[:5]


def test_block_with_small_variance_input_pins_eps():
    """ResnetBlockDown3D(64 -> 128), fp32, T = 3 (the duplicated first frame), on an input of standard deviation 1e-2: at that variance
    eps = 1e-5 moves rstd by about 5 % (the module default elsewhere in this package, 1e-6, by 0.5 %), so a wrong eps cannot pass the
    fp32 bound -- and cannot fail the whole-network test, whose activations have unit scale."""
    from cvvae_amd.discriminator import ResnetBlockDown3D
    blk = ResnetBlockDown3D(in_channels=64, out_channels=128, dropout=0.0, half_3d=False)
    state = {k: seeded_tensor("main.2." + k, tuple(v.shape), 1) for k, v in blk.state_dict().items()}
    blk.load_state_dict(state, strict=True)
    x = 1e-2 * torch.randn(1, 3, 8, 8, 64, generator=torch.Generator().manual_seed(2))          # NDHWC
    xc = x.permute(0, 4, 1, 2, 3).contiguous()
    sd = {k: v.double() for k, v in state.items()}
    ref = disc_ref.block(sd, "", xc.double(), down=True)
    wrong = disc_ref.block(sd, "", xc.double(), down=True, eps=1e-6)
    got = blk.cuda()(xc.cuda())
    assert tuple(got.shape) == (1, 128, 2, 4, 4) and got.dtype == torch.float32
    e, sens = rel(got, ref), rel(wrong, ref)
    _record("block_64_128_eps", {"forward": e, "bound": NET_IN_TOL[torch.float32], "wrong_eps_would_give": sens})
    assert sens > 5 * NET_IN_TOL[torch.float32]
    assert e <= NET_IN_TOL[torch.float32], e


def test_whole_loss_runs_both_optimizer_indices_with_the_configured_discriminator(golden_dir):
    from cvvae_amd.discriminator import NLayerDiscriminator3D
    from cvvae_amd.loss import GeneralLPIPSWithDiscriminator
    with open(os.path.join(golden_dir, "loss_names.json")) as f:
        names = json.load(f)["GeneralLPIPSWithDiscriminator"]
    torch.manual_seed(0)
    m = GeneralLPIPSWithDiscriminator(disc_start=0, dims=3, perceptual_weight=0.0, discriminator_config=YAML_DISC).cuda().train()
    assert type(m.discriminator) is NLayerDiscriminator3D
    x = seeded_input(SHAPES[0], 1).cuda()
    last = torch.nn.Parameter(torch.ones(1, device="cuda"))                     # stands in for the decoder's last layer
    recs = (x + 0.1 * seeded_input(SHAPES[0], 2).cuda()) * last
    loss, log = m(x, recs, regularization_log={}, optimizer_idx=0, global_step=1, last_layer=last)
    assert list(log) == names["log_keys_generator"]
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in log.values())
    loss.backward()
    assert last.grad is not None and bool(torch.isfinite(last.grad).all())
    dloss, dlog = m(x, recs.detach(), regularization_log={}, optimizer_idx=1, global_step=1, last_layer=last)
    assert list(dlog) == names["log_keys_discriminator"]
    assert bool(torch.isfinite(dloss)) and all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in dlog.values())
    m.discriminator.zero_grad(set_to_none=True)
    dloss.backward()
    got = [n for n, p in m.discriminator.named_parameters() if p.grad is not None and bool(torch.isfinite(p.grad).all())]
    assert len(got) == 50 and not any(".temb_proj." in n for n in got)
