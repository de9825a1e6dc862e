"""CPU check of the HOST logic of the training engines (cvvae_amd/autoencoder.py) on the emulated kernels: tests/emu_ops.patched(
whole_model=True) plus the discriminator's, LPIPS', the loss's, the frame maps' and the optimizer's emulations of the existing
host-logic tests, and `recon_panels` emulated as the eager expression (tests/panel_ref.py).

Four iterations of each engine -- with and without `ema_decay`, with `disc_start_iter` 0 and 2 -- are held to tests/engine_ref.py,
the fp64 restatement of the reference's iteration, restated from the engine's own state dict at the start of every iteration (so
that AdamW's near-sign update does not compound errors): the optimizer_idx sequence and global_step, which parameters had
requires_grad during the backward and that all are restored, the loss and every log key and value, the gradients, the update
(from the engine's own gradients through tests/optim_ref.py adamw64 with the clip coefficient), both schedulers, the EMA shadows.
Then: validation_step and its `_ema` pass, log_images, apply_ckpt through a .ckpt and a .safetensors and on through
checkpoint.convert_training_checkpoint, and the launch-trace condition: an engine's generator and discriminator iterations issue
exactly the `cvvae_amd.ops` calls of the hand-assembled sequence (tests/engine_cases.py ByHand), same order, same arguments.

Tolerances.  Loss and logs: 1e-4 relative, tests/test_loss_host_logic.py's RTOL for the same emulated reductions.  Gradients: the
rule of tests/test_training_config_path.py for the same emulated networks -- relative L2 below 5e-4 with the norm floored at 1e-3 of
the largest gradient norm of the group; `d_weight`, the quotient of two such gradients' norms (the last layer's, through LPIPS and
through the discriminator), is held to twice that, 1e-3.  Update, moments and shadows: 1e-5 relative L2 (fp32 emulation of a few operations)."""
import contextlib
import copy
import math
import os

import pytest
import torch

from oracle.seeded import seeded_input
from tests import emu_ops, optim_ref, panel_ref
from tests import engine_cases as EC
from tests import engine_ref as ER
from tests.test_backward_launch_trace import _DISC_OPS, tracing
from tests.test_loss_allconstraint_host_logic import reduce_sum_frames, reduce_sum_frames_bwd
from tests.test_loss_host_logic import gauss_reg, gauss_reg_bwd, reduce_sum, reduce_sum_bwd
from tests.test_lpips_host_logic import _LPIPS_OPS

SHAPE = (1, 3, 5, 16, 16)
TN = EC.time_n_compress(False)    # the cut networks halve time once
NOISE = {"latent": (1, 16, 3, 4, 4), "all": (2, 4, 3, 4, 4)}
INDICES = [0, 2, 3]
RTOL, GRAD_TOL, GRAD_FLOOR, STEP_TOL = 1e-4, 5e-4, 1e-3, 1e-5
OPT = EC.YAML_OPT["params"]


def emu_recon_panels(x, xrec, boost):
    return tuple(t.contiguous() for t in panel_ref.panels(x, xrec, boost))


@contextlib.contextmanager
def emulated(trace=False):
    """every kernel wrapper the engines reach, emulated; trace: also record the top-level ops calls -> the list of lines"""
    from cvvae_amd import ops
    with pytest.MonkeyPatch.context() as mp:
        for f in (reduce_sum, reduce_sum_bwd, gauss_reg, gauss_reg_bwd, reduce_sum_frames, reduce_sum_frames_bwd):
            mp.setattr(ops, f.__name__, f)
        mp.setattr(ops, "recon_panels", emu_recon_panels)
        optim_ref.pretend_gpu(mp)
        with (tracing() if trace else emu_ops.patched(whole_model=True)) as lines:
            if not trace:
                for n, fn in {**_DISC_OPS, **_LPIPS_OPS}.items():
                    mp.setattr(ops, n, fn)
            yield lines


def _rel(a, b, floor=0.0):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(floor if floor else 1e-30))


def _close(name, got, want, rtol=RTOL):
    got, want = float(got), float(want)
    assert abs(got - want) <= rtol * max(abs(want), 1e-6), (name, got, want)


def _group(name):
    return "loss.logvar" if name.startswith("loss.logvar") else name.split(".")[0 if not name.startswith("loss.") else 1]


_BUILT = {}


def _engine(kind, **kw):
    key = (kind, tuple(sorted(kw.items())))
    if key not in _BUILT:
        _BUILT[key] = EC.build(kind, False, **kw)
    return copy.deepcopy(_BUILT[key])


CASES = [("latent", None, 0), ("latent", 0.999, 2), ("all", 0.999, 0), ("all", None, 2)]


@pytest.mark.parametrize("kind,ema,disc_start_iter", CASES, ids=[f"{k}-ema{e}-start{d}" for k, e, d in CASES])
def test_four_iterations_against_the_fp64_restatement(kind, ema, disc_start_iter):
    e = _engine(kind, ema_decay=ema, disc_start_iter=disc_start_iter)
    x = seeded_input(SHAPE, 12)
    e.sample_generator, twin = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    seen = []
    backward = e.manual_backward
    e.manual_backward = lambda loss: (seen.append({n for n, p in e.named_parameters() if p.requires_grad}), backward(loss))
    logged = []
    e.log_fn = lambda logs, step: logged.append((step, sorted(logs)))
    trainable = {n for n, p in e.named_parameters() if p.requires_grad}
    ae_names = {n for n in trainable if not n.startswith("loss.discriminator.")}
    want_idx = [0, 0, 0, 1] if disc_start_iter else [0, 1, 0, 1]
    cfg = EC.net_cfg(kind, False)
    with emulated():
        for it in range(4):
            draws = kind == "latent" and it == 2          # this iteration draws its frames from the generator
            e.frame_indices = None if draws else INDICES
            state = {k: v.detach().clone() for k, v in e.state_dict().items()}
            opts = e.optimizers()
            idx = want_idx[it]
            lr = [g["lr"] for g in opts[idx].param_groups]
            before = {n: (p.detach().clone(), {k: v.clone() for k, v in opts[idx].state.get(p, {}).items()})
                      for n, p in e.named_parameters() if n in (ae_names if idx == 0 else trainable - ae_names)}
            noise = torch.randn(NOISE[kind], generator=twin)
            indices = INDICES
            if draws:
                indices = torch.cat([torch.tensor([0]), torch.randint(1, TN + 1, (2,), generator=twin) + torch.arange(2) * TN]).tolist()
            loss = e.training_step({"frames": x}, it)
            assert e.global_step == it + 1 and logged[-1][0] == it + 1
            # which optimizer, which parameters were live in the backward, all restored
            assert seen[-1] == (ae_names if idx == 0 else trainable - ae_names), (it, idx)
            assert {n for n, p in e.named_parameters() if p.requires_grad} == trainable
            assert [s.last_epoch for s in e.lr_schedulers()] == [it + 1, it + 1]
            # loss, logs, gradients against the restatement of THIS iteration
            ref_loss, ref_log, ref_grads = ER.iteration(kind, state, x, cfg, noise=noise, indices=indices, optimizer_idx=idx, global_step=it,
                                                        time_n_compress=TN)
            _close("loss", loss, ref_loss)
            logs = dict(e.last_logs)
            if idx == 0:
                _close("log loss", logs.pop("loss"), ref_loss)
            assert sorted(logs) == sorted(ref_log) == [k for k in logged[-1][1] if k != "loss"], (it, sorted(logs), sorted(ref_log))
            for k in ref_log:
                if k.startswith("train/scalars/logvar"):   # (the log holds the live parameter: it has moved with the step)
                    _close(k, state["loss." + k.rsplit("/", 1)[1]], ref_log[k])
                else:
                    _close(k, logs[k], ref_log[k], 2 * GRAD_TOL if k.endswith("d_weight") else RTOL)
            params = dict(e.named_parameters())
            assert set(ref_grads) == set(before), (it, sorted(set(ref_grads) ^ set(before))[:5])
            scale = {}
            for n, g in ref_grads.items():
                if g is not None:
                    scale[_group(n)] = max(scale.get(_group(n), 0.0), float(g.norm()))
            for n, g in ref_grads.items():
                if g is None:      # the discriminator's unused temb_proj
                    assert params[n].grad is None or float(params[n].grad.abs().max()) == 0.0, n
                    continue
                assert params[n].grad is not None, (it, n)
                err = _rel(params[n].grad, g, GRAD_FLOOR * scale[_group(n)])
                assert err < GRAD_TOL, (it, n, err)
            for n in trainable - set(before):
                assert n not in ref_grads
            # the update: AdamW from the engine's own gradients, clipped to norm 1 over the optimizer's parameters
            with_grad = [n for n in before if params[n].grad is not None]
            norm = math.sqrt(sum(float(params[n].grad.double().pow(2).sum()) for n in with_grad))
            coef = min(1.0, 1.0 / (norm + 1e-6))
            _close("grad norm", opts[idx].last_grad_norm, norm, 1e-5)
            for n in with_grad:
                p0, st0 = before[n]
                t = int(opts[idx].state[params[n]]["step"])
                assert t == (int(st0["step"]) if st0 else 0) + 1
                m0 = st0["exp_avg"] if st0 else torch.zeros_like(p0)
                v0 = st0["exp_avg_sq"] if st0 else torch.zeros_like(p0)
                m2, v2, p2, _, _ = optim_ref.adamw64(params[n].grad, p0, m0, v0, t, lr[0], OPT["betas"][0], OPT["betas"][1], OPT["eps"],
                                                     OPT["weight_decay"], coef)
                st = opts[idx].state[params[n]]
                assert _rel(params[n], p2) < STEP_TOL and _rel(st["exp_avg"], m2) < STEP_TOL and _rel(st["exp_avg_sq"], v2) < STEP_TOL, (it, n)
            assert all(torch.equal(p, state[n]) for n, p in e.named_parameters() if n not in before)     # nothing else moved
            # the EMA
            e.on_train_batch_end()
            if ema:
                n_up = it + 1
                assert int(e.model_ema.num_updates) == n_up
                omd = 1.0 - min(float(torch.tensor(ema, dtype=torch.float32)), (1 + n_up) / (10 + n_up))
                for n, p in e.named_parameters():
                    if p.requires_grad:
                        s_name = n.replace(".", "")
                        want = optim_ref.ema64(state["model_ema." + s_name], p, omd)
                        assert _rel(getattr(e.model_ema, s_name), want) < STEP_TOL, (it, n)
            else:
                assert not hasattr(e, "model_ema")
    assert [len(s) > 0 for s in seen] == [True] * 4
    # the warm-up of the generator's cosine schedule and the constant discriminator schedule
    assert e.optimizers()[0].param_groups[0]["lr"] == pytest.approx(2 * EC.BASE_LR * 4 / 1000)
    assert e.optimizers()[1].param_groups[0]["lr"] == EC.BASE_LR


def test_validation_step_its_ema_pass_and_the_meter():
    e = _engine("latent", ema_decay=0.5)
    x = seeded_input(SHAPE, 12)
    e.sample_generator, e.frame_indices = torch.Generator().manual_seed(5), INDICES

    class Meter:
        calls = []

        def update(self, a, b):
            self.calls.append((a, b))
    e.validation_meter = Meter()
    with emulated():
        for it in range(2):
            e.training_step({"frames": x}, it)
            e.on_train_batch_end()
        before = [p.detach().clone() for p in e.parameters()]
        versions = [p._version for p in e.parameters()]
        twin = torch.Generator()
        twin.set_state(e.sample_generator.get_state())
        state = {k: v.detach().clone() for k, v in e.state_dict().items()}
        out = e.validation_step({"frames": x}, 0)
    assert e.training and e.encoder.training and not e.loss.perceptual_loss.training
    assert all(torch.equal(p, q) for p, q in zip(before, e.parameters())), "the _ema pass did not restore the weights"
    assert all(p._version > v for p, v in zip(e.parameters(), versions) if p.requires_grad)   # ... and the weight caches saw both swaps
    keys = ["kl_loss", "loss/total", "loss/nll", "loss/rec", "loss/rec2d", "loss/g", "scalars/logvar", "scalars/logvar_2d", "scalars/d_weight",
            "loss/disc", "logits/real", "logits/fake"]
    assert sorted(out) == sorted([f"val/{k}" for k in keys] + [f"val_ema/{k}" for k in keys])
    assert all(k in e.last_logs for k in out)
    assert float(out["val/scalars/d_weight"]) == 1.0 and float(out["val/loss/g"]) != 0.0          # eval(): the discriminator is on, weight 1
    assert float(out["val/loss/rec"]) != float(out["val_ema/loss/rec"])
    assert len(Meter.calls) == 1 and Meter.calls[0][0] is x and tuple(Meter.calls[0][1].shape) == SHAPE
    # the plain pass against the restatement in eval mode, from the state before the call
    noise = torch.randn(NOISE["latent"], generator=twin)
    for idx in (0, 1):
        _, ref_log, _ = ER.iteration("latent", state, x, EC.net_cfg("latent", False), noise=noise, indices=INDICES, optimizer_idx=idx,
                                     global_step=2, split="val", training=False, want_grads=False, time_n_compress=TN)
        for k, v in ref_log.items():
            _close(k, out[k], v)


@pytest.mark.parametrize("kind", ["latent", "all"])
def test_log_images_keys_shapes_and_values(kind):
    e = _engine(kind, ema_decay=0.5)
    x = seeded_input(SHAPE, 12)
    e.sample_generator, e.frame_indices = torch.Generator().manual_seed(5), INDICES
    with emulated():
        e.training_step({"frames": x}, 0)
        e.on_train_batch_end()
        before = [p.detach().clone() for p in e.parameters()]
        log = e.log_images({"frames": x})
    want = ["inputs", "reconstructions", "reconstructions_2d" if kind == "latent" else "rec_d", "diff", "diff_boost",
            "reconstructions_ema", "diff_ema", "diff_boost_ema"]
    assert list(log) == want
    assert all(torch.equal(p, q) for p, q in zip(before, e.parameters()))
    for k, v in log.items():
        assert tuple(v.shape) == (3 if k == "reconstructions_2d" else 5, 3, 16, 16) and not v.requires_grad, k
    assert torch.equal(log["inputs"], panel_ref.frames(x))
    back = lambda t: t.view(1, 5, 3, 16, 16).permute(0, 2, 1, 3, 4)  # noqa: E731
    for post in ("", "_ema"):
        _, _, d, db = panel_ref.panels(x, back(log["reconstructions" + post]), 3.0)
        assert torch.equal(log["diff" + post], d) and torch.equal(log["diff_boost" + post], db)
    assert not torch.equal(log["reconstructions"], log["reconstructions_ema"])


def test_apply_ckpt_round_trips_and_the_converter_reads_the_result(tmp_path, capsys):
    from cvvae_amd import checkpoint
    from lvdm.models.autoencoder import build_from_config
    e = _engine("latent", ema_decay=0.999)
    with torch.no_grad():
        for p in e.parameters():
            if p.requires_grad:
                p.add_(0.01)                 # the weights now differ from the shadows and from a fresh seeded engine
    sd = e.state_dict()
    ckpt, st = str(tmp_path / "last.ckpt"), str(tmp_path / "last.safetensors")
    torch.save({"state_dict": sd, "global_step": 7}, ckpt)
    from safetensors.torch import save_file
    save_file({k: v.contiguous() for k, v in sd.items()}, st)
    for path, key in ((ckpt, "ckpt_path"), (st, "ckpt_engine")):
        cfg = EC.config("latent", False, ema_decay=0.999, **{key: path})
        f = build_from_config(cfg)
        assert "Restored vae weights with 0 missing and 0 unexpected keys" in capsys.readouterr().out
        got = f.state_dict()
        assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd), path
    with pytest.raises(NotImplementedError):
        e.apply_ckpt(str(tmp_path / "last.bin"))
    partial = {k: v for k, v in sd.items() if k.startswith("encoder.")}
    partial["not.a.key"] = torch.zeros(1)
    e.apply_ckpt(partial)
    out = capsys.readouterr().out
    assert "1 unexpected keys" in out and "Unexpected Keys: ['not.a.key']" in out and "Missing Keys" in out
    # the converter takes the engine's checkpoint as it is: the weights, or their EMA shadows
    widths = EC.net_cfg("latent", False)
    for use_ema in (False, True):
        dst = str(tmp_path / f"vae{int(use_ema)}")
        checkpoint.convert_training_checkpoint(ckpt, dst, family="sd3", use_ema=use_ema, **widths)
        from safetensors.torch import load_file
        conv = load_file(os.path.join(dst, "diffusion_pytorch_model.safetensors"))
        src = sd["model_ema.encoderconv_inweight"] if use_ema else sd["encoder.conv_in.weight"]
        assert torch.equal(conv["encoder.conv_in.weight"], src)
        assert not torch.equal(sd["model_ema.encoderconv_inweight"], sd["encoder.conv_in.weight"])


@pytest.mark.parametrize("kind", ["latent", "all"])
def test_an_iteration_issues_exactly_the_launches_of_the_hand_assembled_sequence(kind):
    """one generator and one discriminator iteration: same ops calls, same order, same arguments (the tracer of
    tests/test_backward_launch_trace.py); the engine adds no launch to the path"""
    x = seeded_input(SHAPE, 12)
    a, b = _engine(kind, ema_decay=0.999), _engine(kind, ema_decay=0.999)
    a.sample_generator, a.frame_indices = torch.Generator().manual_seed(5), INDICES
    with emulated(trace=True) as lines:
        for it in range(2):
            a.training_step({"frames": x}, it)
            a.on_train_batch_end()
        engine_lines = list(lines)
    hand = EC.ByHand(kind, EC.modules_of(b), ema=b.model_ema, tn=TN)
    hand.ema_model, hand.generator, hand.frame_indices = b, torch.Generator().manual_seed(5), INDICES
    with emulated(trace=True) as lines:
        for it in range(2):
            hand.step(x, it)
        hand_lines = list(lines)
    assert len(engine_lines) > 100 and any(ln.startswith("mt_adamw(") for ln in engine_lines) and any(ln.startswith("mt_ema(") for ln in engine_lines)
    assert not any(ln.startswith("recon_panels(") for ln in engine_lines)
    first = next((i for i, (p, q) in enumerate(zip(engine_lines, hand_lines)) if p != q), None)
    assert first is None, (first, engine_lines[first][:200], hand_lines[first][:200])
    assert len(engine_lines) == len(hand_lines)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
