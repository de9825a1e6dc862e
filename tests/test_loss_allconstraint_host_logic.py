"""CPU check of the HOST logic of LPIPSWithDiscriminatorAndAllConstraint (cvvae_amd/loss.py): with the ops wrappers replaced by
plain-torch emulations of their documented arithmetic (those of tests/test_loss_host_logic.py, plus cvvae_reduce_sum_frames / _bwd
emulated here: the target is materialised by the header's rule and handed to the emulated plain reduction), LPIPS by a small
differentiable stand-in and the discriminator by elementwise torch ops, the class must reproduce the fp64 restatement
(tests/allconstraint_ref.py) under torch.autograd: the loss, every log entry and every gradient, for all three `target_type`s and
both optimizer branches.  This is where a wrong divisor (2 B T frames for the 3-D term, B T' for the 2-D one), a doubled copy that
is not the stride-0 view, a wrong group start 1 + n (t' - 1) or a draw that is not the reference's shows.

Tolerance: 1e-4 relative, as tests/test_loss_host_logic.py (fp32 emulation against fp64; a wiring mistake changes a value by a
factor)."""
import pytest
import torch

from oracle.seeded import seeded_input
from tests import allconstraint_ref as R
from tests import loss_ref
from tests.test_loss_host_logic import Disc, Perceptual, _close, emulated, reduce_sum, reduce_sum_bwd

B, H, W, N = 2, 6, 7, 2
SEEN = []   # (mode, index, group, clip strides) of every emulated frame-map launch


def _target(clip, mode, index, group):
    """the header's rule, in fp32: GATHER picks frames; GROUP_MEAN keeps frame 0 and averages left to right with one multiply"""
    from cvvae_amd import _lib as L
    c = clip.detach().float()
    if mode == L.FMAP_GATHER:
        return c[:, :, list(index)]
    t = c.shape[2]
    assert (t - 1) % group == 0
    out = [c[:, :, :1]]
    for s in range(1, t, group):
        acc = c[:, :, s]
        for q in range(1, group):
            acc = acc + c[:, :, s + q]
        out.append((acc * (torch.tensor(1.0) / group)).unsqueeze(2))
    return torch.cat(out, dim=2)


def reduce_sum_frames(op, a, clip, mode, *, index=None, group=None):
    assert a.is_contiguous() and not a.requires_grad and not clip.requires_grad
    SEEN.append((mode, None if index is None else list(index), group, tuple(clip.stride())))
    return reduce_sum(op, a, _target(clip, mode, index, group))


def reduce_sum_frames_bwd(op, a, clip, coef, mode, *, index=None, group=None):
    return reduce_sum_bwd(op, a, _target(clip, mode, index, group), coef, True, False)[0]


def _problem(dtype, t):
    tp = 1 + (t - 1) // N
    x = seeded_input((B, 3, t, H, W), 1).to(dtype)
    x2 = torch.cat([x, x], dim=0)
    leaves = {
        "base": (x2 + 0.3 * seeded_input((2 * B, 3, t, H, W), 2).to(dtype)).requires_grad_(True),
        "xhat2d": (0.8 * x[:, :, :tp] + 0.2 * seeded_input((B, 3, tp, H, W), 3).to(dtype)).requires_grad_(True),
        "last": torch.tensor([0.3, -0.4, 0.5], dtype=dtype).requires_grad_(True),
        "moments": (1.5 * seeded_input((2 * B, 8, 2, 3, 3), 4).to(dtype)).requires_grad_(True),
    }
    with torch.no_grad():
        leaves["base"][0, 0, 0, 0, :3] = x[0, 0, 0, 0, :3]  # exact zeros in x - xhat
    feat = seeded_input((2 * B, 3, t, H, W), 5).to(dtype)
    feat[0, 0, 0, 0, :3] = 0
    noise = seeded_input((2 * B, 4, 2, 3, 3), 6).to(dtype)
    return x, leaves, feat, noise


def _xhat(leaves, feat, z):
    return leaves["base"] + leaves["last"].view(1, 3, 1, 1, 1) * feat + 0.01 * z[:, :3, :1, :1, :1]


def _run(monkeypatch, target_type, t=5, indices=None, **s):
    from cvvae_amd import ops
    from cvvae_amd.loss import DiagonalGaussianRegularizer, LPIPSWithDiscriminatorAndAllConstraint
    s = dict(dict(optimizer_idx=0, global_step=20, training=True, rec_loss="l1", disc_loss="hinge", weights=None, perceptual_weight=0.8,
                  learn_logvar=True, logvar_init=0.2, disc_factor=1.0, disc_weight=1.0, rec2d_weight=0.6), **s)
    m = LPIPSWithDiscriminatorAndAllConstraint(
        disc_start=10, logvar_init=s["logvar_init"], disc_factor=s["disc_factor"], disc_weight=s["disc_weight"],
        perceptual_weight=s["perceptual_weight"], disc_loss=s["disc_loss"], rec_loss=s["rec_loss"], dims=3,
        learn_logvar=s["learn_logvar"], regularization_weights={"kl_loss": 1e-2}, discriminator=Disc(), time_n_compress=N,
        rec2d_weight=s["rec2d_weight"], target_type=target_type)
    m.perceptual_loss = Perceptual()
    m.train(s["training"])
    x, lv, feat, noise = _problem(torch.float32, t)
    del SEEN[:]
    with emulated(monkeypatch) as mp:
        mp.setattr(ops, "reduce_sum_frames", reduce_sum_frames)
        mp.setattr(ops, "reduce_sum_frames_bwd", reduce_sum_frames_bwd)
        z, rlog = DiagonalGaussianRegularizer()(lv["moments"], noise=noise)
        loss, log = m(x, _xhat(lv, feat, z), lv["xhat2d"], regularization_log=rlog, optimizer_idx=s["optimizer_idx"],
                      global_step=s["global_step"], last_layer=lv["last"], weights=s["weights"], frame_indices=indices)
        assert loss.dim() == 0
        if loss.requires_grad:
            loss.backward()
    x64, lr, feat64, noise64 = _problem(torch.float64, t)
    disc = Disc(torch.float64)
    logvar = torch.tensor(s["logvar_init"], dtype=torch.float64, requires_grad=True)
    logvar2 = torch.tensor(s["logvar_init"], dtype=torch.float64, requires_grad=True)
    z64, kl = loss_ref.gauss_reg_ref(lr["moments"], noise64)
    w = s["weights"].double() if isinstance(s["weights"], torch.Tensor) else s["weights"]
    rloss, rlog64 = R.all_constraint_ref(
        x64, _xhat(lr, feat64, z64), lr["xhat2d"], logvar=logvar, logvar_2d=logvar2, discriminator=disc, perceptual=Perceptual(),
        perceptual_weight=s["perceptual_weight"], rec_loss=s["rec_loss"], disc_loss=s["disc_loss"], disc_start=10,
        disc_factor=s["disc_factor"], disc_weight=s["disc_weight"], time_n_compress=N, rec2d_weight=s["rec2d_weight"],
        target_type=target_type, indices=None if indices is None else torch.tensor(indices),
        regularization_weights={"kl_loss": 1e-2}, regularization_log={"kl_loss": kl}, optimizer_idx=s["optimizer_idx"],
        global_step=s["global_step"], last_layer=lr["last"], weights=w, training=s["training"])
    if rloss.requires_grad:
        rloss.backward()
    got = {"loss": loss.detach(), **{"log:" + k: v for k, v in log.items()}}
    want = {"loss": rloss.detach(), **{"log:" + k: v for k, v in rlog64.items()}}
    grads = {**{n: (lv[n].grad, lr[n].grad) for n in lv}, "disc.gain": (m.discriminator.gain.grad, disc.gain.grad),
             "disc.bias": (m.discriminator.bias.grad, disc.bias.grad), "logvar": (m.logvar.grad, logvar.grad),
             "logvar_2d": (m.logvar_2d.grad, logvar2.grad)}
    return s, got, want, grads, list(log)


def _compare(got, want, grads):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert got[k].dim() == 0 and not got[k].requires_grad or k == "loss", k
        _close(k, got[k], want[k])
    for name, (g, r) in grads.items():
        if r is None or float(r.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) == 0.0, name
        else:
            _close("grad " + name, g, r)


SETTINGS = [dict(), dict(optimizer_idx=1), dict(rec_loss="l2", weights=0.7), dict(global_step=0),
            dict(training=False, global_step=0), dict(perceptual_weight=0.0, disc_factor=0.5, disc_weight=0.3),
            dict(optimizer_idx=1, disc_loss="vanilla")]


@pytest.mark.parametrize("target_type", ["slice", "random", "mean"])
@pytest.mark.parametrize("setting", SETTINGS, ids=[",".join(f"{k}={v}" for k, v in s.items()) or "default" for s in SETTINGS])
def test_loss_logs_and_gradients_match_the_restatement(monkeypatch, target_type, setting):
    import json
    import os
    s, got, want, grads, keys = _run(monkeypatch, target_type, indices=[0, 2, 3] if target_type == "random" else None, **setting)
    _compare(got, want, grads)
    names = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_names_allconstraint.json")))
    names = names["LPIPSWithDiscriminatorAndAllConstraint"]
    if s["optimizer_idx"] == 0:
        assert keys == ["train/kl_loss"] + names["log_keys_generator"]
        assert all(grads[n][1] is not None for n in ("base", "xhat2d", "last", "moments", "logvar", "logvar_2d"))
        from cvvae_amd import _lib as L
        want_launch = {"slice": [], "random": [(L.FMAP_GATHER, [0, 2, 3], None)], "mean": [(L.FMAP_GROUP_MEAN, None, N)]}[target_type]
        assert [e[:3] for e in SEEN] == want_launch
        assert all(e[3] == (3 * 5 * H * W, 5 * H * W, H * W, W, 1) for e in SEEN)  # the inputs themselves: no copy, no doubled tensor
    else:
        assert keys == names["log_keys_discriminator"] and SEEN == []
        if s["global_step"] >= 10 or not s["training"]:
            assert grads["disc.gain"][1] is not None and grads["base"][0] is None


def test_pixel_sum_reads_the_inputs_through_a_stride_0_dimension(monkeypatch):
    """cat([inputs, inputs]) never exists for the pixel term: the plain reduction sees [2,B,3,T,H,W] with outer stride 0"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    from cvvae_amd.loss import LPIPSWithDiscriminatorAndAllConstraint
    m = LPIPSWithDiscriminatorAndAllConstraint(disc_start=0, dims=3, perceptual_weight=0.0, discriminator=Disc(), time_n_compress=N)
    x, lv, feat, _ = _problem(torch.float32, 5)
    seen = []
    with emulated(monkeypatch) as mp:
        real = ops.reduce_sum
        mp.setattr(ops, "reduce_sum", lambda op, a, b=None: (seen.append((op, tuple(a.shape), None if b is None else tuple(b.stride()),
                                                                           None if b is None else b.data_ptr())), real(op, a, b))[1])
        m(x, lv["base"], lv["xhat2d"], regularization_log={}, optimizer_idx=0, global_step=1, last_layer=lv["base"])
    two = [e for e in seen if e[0] == L.RED_ABS_DIFF]
    assert (L.RED_ABS_DIFF, (2, B, 3, 5, H, W), (0, *x.stride()), x.data_ptr()) in two
    assert (L.RED_ABS_DIFF, (B, 3, 3, H, W), tuple(x[:, :, ::N].stride()), x.data_ptr()) in two and len(two) == 2
    s = ops._reduce_shape(lv["base"].detach().unflatten(0, (2, B)), x.unsqueeze(0).expand(2, *x.shape))
    assert (list(s.n), s.L, list(s.sa), list(s.sb)) == ([1, 1, 2], x.numel(), [0, 0, x.numel()], [0, 0, 0])


@pytest.mark.parametrize("t", [5, 6, 9])
def test_the_random_draw_is_the_references_under_a_seeded_global_generator(monkeypatch, t):
    torch.manual_seed(1234 + t)
    want = R.random_indices(t, N)
    from cvvae_amd import ops
    from cvvae_amd.loss import LPIPSWithDiscriminatorAndAllConstraint
    m = LPIPSWithDiscriminatorAndAllConstraint(disc_start=99, dims=3, perceptual_weight=0.0, discriminator=Disc(), time_n_compress=N,
                                               target_type="random")
    x = seeded_input((1, 3, t, H, W), 1)
    del SEEN[:]
    torch.manual_seed(1234 + t)
    with emulated(monkeypatch) as mp:  # (t = 6: T' = 1 + (T - 1) // n frames, the last partial group is never drawn from)
        mp.setattr(ops, "reduce_sum_frames", reduce_sum_frames)
        m(x, torch.cat([x, x]) * 0.5, torch.zeros(1, 3, 1 + (t - 1) // N, H, W), regularization_log={}, optimizer_idx=0,
          global_step=0, last_layer=None)
    assert len(SEEN) == 1 and SEEN[0][1] == want.tolist() and len(want) == 1 + (t - 1) // N
    assert want[0] == 0 and all(1 + N * i <= int(v) <= N * (i + 1) for i, v in enumerate(want[1:]))
    # generator= seeds the draw without touching the global generator
    from cvvae_amd.loss import LPIPSWithDiscriminatorAndAllConstraint as A
    m = A(disc_start=0, dims=3, discriminator=Disc(), time_n_compress=N, target_type="random")
    a = m.draw_frame_indices(t, torch.Generator().manual_seed(3))
    state = torch.get_rng_state()
    b = m.draw_frame_indices(t, torch.Generator().manual_seed(3))
    assert torch.equal(a, b) and torch.equal(state, torch.get_rng_state())


@pytest.mark.parametrize("target_type", ["slice", "random", "mean"])
def test_image_batches_of_one_frame(monkeypatch, target_type):
    """T = 1 (d = 0): the 2-D target is the frame itself under every rule"""
    s, got, want, grads, _ = _run(monkeypatch, target_type, t=1)
    _compare(got, want, grads)
    assert float(got["log:train/loss/rec2d"]) > 0.0


def test_value_errors_before_any_launch(monkeypatch):
    from cvvae_amd import ops
    from cvvae_amd.loss import LPIPSWithDiscriminatorAndAllConstraint as A
    x = seeded_input((1, 3, 6, H, W), 1)
    r = torch.cat([x, x])
    kw = dict(regularization_log={}, optimizer_idx=0, global_step=0, last_layer=None)

    def boom(*a, **k):
        raise AssertionError("a launch")

    with emulated(monkeypatch) as mp:
        for f in ("reduce_sum", "reduce_sum_bwd", "reduce_sum_frames", "reduce_sum_frames_bwd"):
            mp.setattr(ops, f, boom, raising=False)
        mk = lambda tt: A(disc_start=9, dims=3, perceptual_weight=0.0, discriminator=Disc(), time_n_compress=N, target_type=tt)  # noqa: E731
        with pytest.raises(ValueError, match='target_type="mean"'):
            mk("mean")(x, r, torch.zeros(1, 3, 3, H, W), **kw)                   # (6 - 1) % 2 != 0
        for tt, frames in (("slice", 2), ("random", 4), ("mean", 2)):
            xx = x if tt != "mean" else x[:, :, :5]
            with pytest.raises(ValueError, match="reconstructions_2d"):
                mk(tt)(xx, torch.cat([xx, xx]), torch.zeros(1, 3, frames, H, W), **kw)
        with pytest.raises(ValueError, match="frame_indices"):
            mk("random")(x, r, torch.zeros(1, 3, 3, H, W), frame_indices=[0, 1], **kw)
        with pytest.raises(ValueError, match="frame_indices"):
            mk("random")(x, r, torch.zeros(1, 3, 3, H, W), frame_indices=[0, 1, 6], **kw)
        with pytest.raises(ValueError, match=r"\[2B,3,T,H,W\]"):
            mk("slice")(x, x, torch.zeros(1, 3, 3, H, W), **kw)
        with pytest.raises(NotImplementedError, match="weights"):
            boomless = mk("slice")
            mp.setattr(ops, "reduce_sum", lambda op, a, b=None: torch.zeros(()))
            boomless(x, r, torch.zeros(1, 3, 3, H, W), weights=torch.ones(2, 3, 6, H, W), **kw)
        with pytest.raises(NotImplementedError, match="optimizer_idx 2"):
            mk("slice")(x, r, torch.zeros(1, 3, 3, H, W), **dict(kw, optimizer_idx=2))
