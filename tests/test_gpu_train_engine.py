"""The training engines on a real MI355X (cvvae_amd/autoencoder.py): four iterations -- generator, discriminator, generator,
discriminator -- of each engine, in fp32 and with bf16 networks, against the hand-assembled sequence of the same public calls
(tests/engine_cases.py ByHand: the networks, the regulariser, the loss, two AdamW with max_grad_norm, two LambdaLR, LitEma; toggle_model
written out) on a second copy of the same seeded modules, with seeded device generators and given frame indices.

The kernels are deterministic, so the comparison is a condition, not a band: every loss, every log entry, every parameter, both
optimizers' moments and the EMA shadows must be equal BIT FOR BIT after every iteration.  A mismatch means the engine reordered,
dropped or added work.

Two more assertions per case: `log_images` returns the reference's keys and shapes, bit for bit the eager expression on the
reconstructions it shows, and leaves the training weights in place; the first iteration's loss and logs agree with the fp64
restatement of the iteration (tests/engine_ref.py) within NET_IN_TOL / NET_W_TOL[dtype] of tests/test_gpu_grad3d.py, the project's own
figures for whole networks on these kernels.  The measured figures go to $CVVAE_TEST_LOG_DIR/engine_step_bands.json when that
directory is set; tests/golden/engine_step_bands.json keeps the copy of one run."""
import copy
import json
import os

import pytest
import torch

from oracle.seeded import seeded_input
from tests import engine_cases as EC
from tests import engine_ref
from tests import panel_ref
from tests.test_gpu_grad3d import NET_IN_TOL, NET_W_TOL  # noqa: F401

pytestmark = pytest.mark.gpu
SHAPE = (1, 3, 5, 32, 32)
INDICES = [0, 2]
NOISE = {"latent": (1, 16, 2, 4, 4), "all": (2, 4, 2, 4, 4)}     # the posterior samples: what the regulariser draws from the generator
TAG = {torch.float32: "fp32", torch.bfloat16: "bf16"}
_BUILT = {}
_FIGURES = {}


def _pair(kind, dtype):
    """two engines over equal seeded modules (built once per kind on the CPU, copied per case)"""
    if kind not in _BUILT:
        _BUILT[kind] = EC.build(kind, True, ema_decay=0.999)
    out = []
    for _ in range(2):
        e = copy.deepcopy(_BUILT[kind])
        out.append(EC.to_device(e, dtype))
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _state_mismatches(a, hand, b):
    bad = [n for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()) if not _same(p, q)]
    bad += ["ema:" + n for (n, p), (_, q) in zip(a.model_ema.named_buffers(), b.model_ema.named_buffers()) if not _same(p, q)]
    for i, (oa, ob) in enumerate(zip(a.optimizers(), hand.opts)):
        pa = [p for g in oa.param_groups for p in g["params"]]
        pb = [p for g in ob.param_groups for p in g["params"]]
        assert len(pa) == len(pb) and [g["lr"] for g in oa.param_groups] == [g["lr"] for g in ob.param_groups]
        for j, (p, q) in enumerate(zip(pa, pb)):
            sa, sb = oa.state.get(p, {}), ob.state.get(q, {})
            if set(sa) != set(sb) or any(not _same(sa[k], sb[k]) for k in sa):
                bad.append(f"opt{i}:{j}")
    return bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["latent", "all"])
def test_four_iterations_equal_the_hand_assembled_sequence_bit_for_bit(kind, dtype):
    a, b = _pair(kind, dtype)
    x = seeded_input(SHAPE, 12).to(dtype).cuda()
    a.sample_generator = torch.Generator("cuda").manual_seed(5)
    a.frame_indices = INDICES
    hand = EC.ByHand(kind, EC.modules_of(b), ema=b.model_ema)
    hand.ema_model, hand.generator, hand.frame_indices = b, torch.Generator("cuda").manual_seed(5), INDICES
    assert not _state_mismatches(a, hand, b)
    first = None
    for it in range(4):
        loss_a = a.training_step({"frames": x}, it)
        a.on_train_batch_end()
        logs_a = dict(a.last_logs)
        loss_b, logs_b, idx = hand.step(x, it)
        assert idx == it % 2 and a.global_step == hand.global_step == it + 1
        assert _same(loss_a, loss_b), (it, float(loss_a), float(loss_b))
        if idx == 0:
            assert _same(logs_a.pop("loss"), loss_b)
        assert sorted(logs_a) == sorted(logs_b), (it, sorted(logs_a), sorted(logs_b))
        assert all(v.is_cuda and v.dim() == 0 for v in logs_a.values())
        diff = [k for k in logs_a if not _same(logs_a[k], logs_b[k])]
        assert not diff, (it, {k: (float(logs_a[k]), float(logs_b[k])) for k in diff})
        bad = _state_mismatches(a, hand, b)
        assert not bad, (it, len(bad), bad[:8])
        assert bool(torch.isfinite(loss_a))
        if it == 0:
            first = (loss_a.clone(), {k: v.clone() for k, v in logs_a.items()})   # (the logvars in the logs are the live parameters)
        if it == 2:   # the second generator step runs with the discriminator on
            assert float(logs_a["train/loss/g"]) != 0.0 and float(logs_a["train/scalars/d_weight"]) > 0.0
    assert [s.last_epoch for s in a.lr_schedulers()] == [4, 4]
    assert all(p.requires_grad for p in a.get_autoencoder_params() + a.get_discriminator_params())

    # the first iteration against the fp64 restatement, from the seeded state every engine of this kind starts with
    noise = torch.randn(NOISE[kind], generator=torch.Generator("cuda").manual_seed(5), device="cuda", dtype=dtype).cpu()
    ref_loss, ref_logs = engine_ref.first_iteration(kind, _BUILT[kind], seeded_input(SHAPE, 12).to(dtype), INDICES, dtype, noise,
                                                    EC.net_cfg(kind, True))
    tol = NET_IN_TOL[dtype]   # (the tighter of the two figures: losses and logs are outputs of the networks, not parameter gradients)
    figures = {}
    for k, got, want in [("loss", first[0], ref_loss)] + [(k, first[1][k], ref_logs[k]) for k in sorted(ref_logs)]:
        err = abs(float(got) - float(want)) / max(abs(float(want)), 1e-6)
        figures[k] = err
        print(f"\n[engine step band] {kind} {TAG[dtype]} {k}: got {float(got):.6e} fp64 {float(want):.6e} rel {err:.3e} (tolerance {tol:.1e})")
    assert sorted(ref_logs) == sorted(first[1])
    _FIGURES[f"{kind}_{TAG[dtype]}"] = figures
    out = os.environ.get("CVVAE_TEST_LOG_DIR")
    if out:
        with open(os.path.join(out, "engine_step_bands.json"), "w") as f:
            json.dump(_FIGURES, f, indent=1, sort_keys=True)
    worst = max(figures, key=figures.get)
    assert figures[worst] <= tol, (worst, figures[worst], tol)


@pytest.mark.parametrize("kind", ["latent", "all"])
def test_log_images_keys_shapes_values_and_the_training_weights_stay(kind):
    dtype = torch.bfloat16
    (e, _) = _pair(kind, dtype)
    x = seeded_input(SHAPE, 12).to(dtype).cuda()
    e.sample_generator = torch.Generator("cuda").manual_seed(5)
    e.frame_indices = INDICES
    e.training_step({"frames": x}, 0)
    e.on_train_batch_end()                     # the shadows now differ from the weights
    before = [p.detach().clone() for p in e.parameters()]
    shadows = [s.detach().clone() for s in e.model_ema.buffers()]
    log = e.log_images({"frames": x})
    want = ["inputs", "reconstructions", "reconstructions_2d" if kind == "latent" else "rec_d", "diff", "diff_boost",
            "reconstructions_ema", "diff_ema", "diff_boost_ema"]
    assert list(log) == want
    for k, v in log.items():
        frames = 2 if k == "reconstructions_2d" else 5
        assert tuple(v.shape) == (frames, 3, 32, 32) and v.dtype == dtype and v.is_contiguous() and not v.requires_grad, k
    assert all(torch.equal(p, q) for p, q in zip(before, e.parameters())), "log_images moved the training weights"
    assert all(torch.equal(p, q) for p, q in zip(shadows, e.model_ema.buffers()))
    assert torch.equal(log["inputs"], panel_ref.frames(x))
    back = lambda t: t.view(1, 5, 3, 32, 32).permute(0, 2, 1, 3, 4)  # noqa: E731
    for post in ("", "_ema"):
        _, _, d, db = panel_ref.panels(x, back(log["reconstructions" + post]), e.diff_boost_factor)
        assert panel_ref.same_bits(log["diff" + post].cpu(), d.cpu()) and panel_ref.same_bits(log["diff_boost" + post].cpu(), db.cpu())
    assert not torch.equal(log["reconstructions"], log["reconstructions_ema"])


@pytest.mark.parametrize("kind", ["latent", "all"])
def test_training_step_does_not_synchronise_the_host(kind):
    """bf16 networks, after one generator and one discriminator iteration (library load, the train() transition's checksum, the
    optimizers' lazy state): the next two iterations and their EMA updates run with torch's synchronisation check on "error".  (An
    fp32 network repacks its changed weights in split precision, and that packing reads max|w| back: cvvae_amd/ops.py _wscale.)"""
    (e, _) = _pair(kind, torch.bfloat16)
    x = seeded_input(SHAPE, 12).to(torch.bfloat16).cuda()
    e.sample_generator = torch.Generator("cuda").manual_seed(5)
    e.frame_indices = INDICES
    for it in range(2):
        e.training_step({"frames": x}, it)
        e.on_train_batch_end()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for it in range(2, 4):
            loss = e.training_step({"frames": x}, it)
            e.on_train_batch_end()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert e.global_step == 4 and bool(torch.isfinite(loss))
