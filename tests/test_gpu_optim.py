"""The update step on the MI355X: the four multi-tensor passes of csrc/optim_kernels.hip against the header's formulas in fp64, on a
tensor list that puts every edge of the chunk geometry into ONE launch (tests/optim_ref.py edge_list: numel 0, 1 (0-dim), 7, chunk - 1,
chunk, chunk + 1, 3 chunk + 5, a view that starts 4 bytes into its buffer, a tensor without a gradient; steps t in {1, 2, 7, 1000} inside
the launch), then the optimizer, the EMA and the weight caches together on a small sd3 encoder.

Bounds, derived from fp32's format (ulp at the stated magnitude), not measured:
    m: 3 ulp(max(|m|, |G|))      v: 4 ulp(max(v, G^2))      p: 3 (ulp(|p|) + 2^-20 |delta|)      shadow: 3 ulp(max(|s|, |p|))
with G = coef g and delta = p' - p in fp64.  torch.optim.AdamW in fp32 on the CPU has to meet the same bounds on the same inputs (it
uses 0.55, 1.29 and 1.26 of the 3 / 4 / 3 units): that guards the yardstick.

Gradient norm: the longest chain of fp32 additions is 8 per group x CHUNK / 2048 = 4 groups of a thread (32), 6 butterfly steps and 3
across the waves inside a chunk, then ceil(n_chunks / 256) = 1 serial step, 6 and 3 in the second stage: 51 at these sizes, so the
relative error against fp64 is at most (51 + 2) 2^-24 = 3.2e-6 (< 1e-5)."""
import math

import pytest
import torch
import torch.nn as nn

from tests import optim_ref as R

LR = R.YAML_LR
B1, B2 = R.YAML_ADAMW["betas"]
EPS, WD = R.YAML_ADAMW["eps"], R.YAML_ADAMW["weight_decay"]
COEF = 0.37
NORM_PATH = 8 * (R.CHUNK // 2048) + 6 + 3 + 1 + 6 + 3


@pytest.fixture(scope="module")
def edge():
    return R.edge_list(0)


def _coef32(coef):
    return None if coef is None else torch.tensor(coef, dtype=torch.float32)


def _adamw_bounds(d, coef):
    """fp64 results and the bounds for entry d"""
    v = R.views(d, d)
    c32 = _coef32(coef)
    m2, v2, p2, G, delta = R.adamw64(v["g"], v["p"], v["m"], v["v"], d["t"], LR, B1, B2, EPS, WD, None if c32 is None else c32.item())
    bm = 3 * R.ulp32(torch.maximum(v["m"].double().abs(), G.abs()))
    bv = 4 * R.ulp32(torch.maximum(v["v"].double(), G * G))
    bp = 3 * (R.ulp32(v["p"].double()) + 2.0 ** -20 * delta.abs())
    return (m2, bm), (v2, bv), (p2, bp)


def _worst(got, want, bound):
    return float(((got.double() - want).abs() / bound).max()) if got.numel() else 0.0


@pytest.mark.parametrize("coef", [None, COEF])
def test_torch_adamw_on_the_cpu_meets_the_bounds(edge, coef):
    """the guard of the yardstick: no GPU involved"""
    worst = [0.0, 0.0, 0.0]
    for d in edge:
        if not d["has_grad"] or d["n"] == 0:
            continue
        v = {k: x.clone() for k, x in R.views(d, d).items()}
        p = nn.Parameter(v["p"])
        p.grad = v["g"] * _coef32(coef) if coef is not None else v["g"]
        opt = torch.optim.AdamW([p], lr=LR, **R.YAML_ADAMW)
        opt.state[p] = {"step": torch.tensor(float(d["t"] - 1)), "exp_avg": v["m"], "exp_avg_sq": v["v"]}
        opt.step()
        for i, (got, (want, bound)) in enumerate(zip((v["m"], v["v"], p.detach()), _adamw_bounds(d, coef))):
            worst[i] = max(worst[i], _worst(got, want, bound))
    print(f"torch CPU AdamW, coef {coef}: fractions of the m / v / p bounds {worst}")
    assert max(worst) <= 1.0, worst


def _device_copy(edge):
    """fresh device copies of every buffer, and the views over them"""
    out = []
    for d in edge:
        bufs = {k: d[k].cuda() for k in d if k.endswith("_buf")}
        out.append((bufs, R.views(d, bufs)))
    return out


def _list(edge, dev, fields):
    """MultiTensorList over the entries that have a gradient (all of them for the EMA)"""
    from cvvae_amd import ops
    sel = [i for i, d in enumerate(edge) if d["has_grad"] or "g" not in fields]
    mtl = ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda")
    kw = {f: [dev[i][1][{"shadow": "s"}.get(f, f)] for i in sel] for f in fields}
    if "m" in fields:
        kw["step_size"] = [LR / (1.0 - B1 ** edge[i]["t"]) for i in sel]
        kw["bias2_sqrt"] = [math.sqrt(1.0 - B2 ** edge[i]["t"]) for i in sel]
    return mtl.set(**kw), sel


def _untouched(edge, dev, written):
    """a written view's buffer keeps its bits in front of and behind the view (the guard band); every other buffer keeps all of them"""
    for d, (bufs, _) in zip(edge, dev):
        lo, hi = d["off"], d["off"] + d["n"]
        for k in ("g", "p", "m", "v", "s"):
            after, before = bufs[k + "_buf"].cpu().view(torch.int32), d[k + "_buf"].view(torch.int32)
            if k in written and (d["has_grad"] or k == "s"):
                assert torch.equal(after[:lo], before[:lo]) and torch.equal(after[hi:], before[hi:]), (d["n"], k)
            else:
                assert torch.equal(after, before), (d["n"], k)


@pytest.mark.gpu
@pytest.mark.parametrize("coef", [None, COEF])
def test_adamw_pass_on_every_edge_in_one_launch(edge, coef):
    from cvvae_amd import ops
    dev = _device_copy(edge)
    mtl, sel = _list(edge, dev, ("g", "p", "m", "v"))
    assert mtl.n_chunks == 1 + 1 + 1 + 1 + 2 + 4 + 2                      # one launch, 12 chunks, 8 tensors (one of them empty)
    c = None if coef is None else torch.tensor([COEF], dtype=torch.float32, device="cuda")
    ops.mt_adamw(mtl, LR, B1, B2, EPS, WD, c)
    torch.cuda.synchronize()
    worst = [0.0, 0.0, 0.0]
    for i in sel:
        v = dev[i][1]
        for j, (k, (want, bound)) in enumerate(zip(("m", "v", "p"), _adamw_bounds(edge[i], coef))):
            w = _worst(v[k].cpu(), want, bound)
            worst[j] = max(worst[j], w)
            assert w <= 1.0, (edge[i]["n"], edge[i]["off"], edge[i]["t"], k, w)
    print(f"mt_adamw, coef {coef}: fractions of the m / v / p bounds {worst}")
    _untouched(edge, dev, ("p", "m", "v"))


@pytest.mark.gpu
def test_ema_pass_on_every_edge_in_one_launch(edge):
    from cvvae_amd import ops
    dev = _device_copy(edge)
    mtl, sel = _list(edge, dev, ("p", "shadow"))
    assert len(sel) == len(edge)
    omd = float(torch.tensor(1.0) - torch.tensor(2.0 / 11.0))            # LitEma's first update: decay = (1 + 1) / (10 + 1)
    ops.mt_ema(mtl, omd)
    torch.cuda.synchronize()
    worst = 0.0
    for d, (_, v) in zip(edge, dev):
        s0, p0 = R.views(d, d)["s"], R.views(d, d)["p"]
        want = R.ema64(s0, p0, omd)
        bound = 3 * R.ulp32(torch.maximum(s0.double().abs(), p0.double().abs()))
        w = _worst(v["s"].cpu(), want, bound)
        worst = max(worst, w)
        assert w <= 1.0, (d["n"], d["off"], w)
    print(f"mt_ema: fraction of the shadow bound {worst}")
    _untouched(edge, dev, ("s",))


def _norm64(edge):
    return math.sqrt(sum(float((R.views(d, d)["g"].double() ** 2).sum()) for d in edge if d["has_grad"]))


@pytest.mark.gpu
def test_grad_norm_is_accurate_deterministic_and_gives_torchs_coefficient(edge):
    from cvvae_amd import ops
    dev = _device_copy(edge)
    mtl, _ = _list(edge, dev, ("g",))
    want = _norm64(edge)
    outs = [ops.mt_grad_norm(mtl, mx) for mx in (1.0, 1.0, 1e6)]
    torch.cuda.synchronize()
    a, b, big = (o.cpu() for o in outs)
    rel = abs(float(a[0].double()) - want) / want
    print(f"mt_grad_norm: {float(a[0])} vs fp64 {want}: relative error {rel:.3e} (bound {(NORM_PATH + 2) * 2.0 ** -24:.3e})")
    assert NORM_PATH == 51 and (NORM_PATH + 2) * 2.0 ** -24 < 1e-5
    assert rel <= (NORM_PATH + 2) * 2.0 ** -24
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))         # two runs, the same bits
    assert float(a[0]) > 1.0                                              # the clip is active at max_norm 1
    for out, mx in ((a, 1.0), (big, 1e6)):
        c = torch.tensor(mx, dtype=torch.float32) / (out[0] + 1e-6)
        assert torch.equal(out[1], torch.clamp(c, max=1.0)), (out, mx)
    assert float(big[1]) == 1.0 and 0.0 < float(a[1]) < 1.0
    _untouched(edge, dev, ())


@pytest.mark.gpu
def test_scale_is_bit_equal_to_the_fp32_product(edge):
    from cvvae_amd import ops
    dev = _device_copy(edge)
    mtl, sel = _list(edge, dev, ("g",))
    c = torch.tensor([COEF], dtype=torch.float32, device="cuda")
    ops.mt_scale(mtl, c)
    torch.cuda.synchronize()
    for i in sel:
        want = R.views(edge[i], edge[i])["g"] * torch.tensor(COEF, dtype=torch.float32)
        assert torch.equal(dev[i][1]["g"].cpu().view(torch.int32), want.view(torch.int32)), edge[i]["n"]
    _untouched(edge, dev, ("g",))


@pytest.mark.gpu
def test_one_nan_gradient_element_poisons_norm_coefficient_and_step_as_torchs_does(edge):
    from cvvae_amd import ops
    dev = _device_copy(edge)
    dev[6][1]["g"][R.CHUNK + 17] = float("nan")
    mtl, sel = _list(edge, dev, ("g", "p", "m", "v"))
    out2 = ops.mt_grad_norm(mtl, 1.0)
    ops.mt_adamw(mtl, LR, B1, B2, EPS, WD, out2[1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out2).all())
    # torch: clip_grad_norm_ multiplies every gradient by the NaN coefficient, and AdamW then writes NaN everywhere
    assert all(bool(torch.isnan(dev[i][1]["p"]).all()) for i in sel)
    p = nn.Parameter(torch.ones(3))
    p.grad = torch.tensor([1.0, float("nan"), 2.0])
    torch.nn.utils.clip_grad_norm_([p], 1.0)
    torch.optim.AdamW([p], lr=LR, **R.YAML_ADAMW).step()
    assert bool(torch.isnan(p).all())


@pytest.mark.gpu
def test_optimizer_over_the_edge_list_equals_the_bare_passes(edge):
    """cvvae_amd.optim.AdamW(max_grad_norm) = mt_grad_norm + mt_adamw on the parameters that have a gradient; the one without keeps
    its bits and gets no state; torch's state layout"""
    from cvvae_amd import ops
    from cvvae_amd.optim import AdamW
    dev, ref = _device_copy(edge), _device_copy(edge)
    params = []
    for d, (_, v) in zip(edge, dev):
        p = nn.Parameter(v["p"])
        assert p.data_ptr() == v["p"].data_ptr()
        if d["has_grad"]:
            p.grad = v["g"]
        params.append(p)
    opt = AdamW(params, lr=LR, max_grad_norm=1.0, **R.YAML_ADAMW)
    for d, (_, v), p in zip(edge, dev, params):
        if d["has_grad"]:
            opt.state[p] = {"step": torch.tensor(float(d["t"] - 1)), "exp_avg": v["m"], "exp_avg_sq": v["v"]}
    versions = [p._version for p in params]
    opt.step()
    mtl, sel = _list(edge, ref, ("g", "p", "m", "v"))
    out2 = ops.mt_grad_norm(mtl, 1.0)
    ops.mt_adamw(mtl, LR, B1, B2, EPS, WD, out2[1])
    torch.cuda.synchronize()
    assert torch.equal(opt.last_grad_norm, out2[0]) and opt.last_grad_norm.shape == () and opt.last_grad_norm.is_cuda
    for i, (d, p) in enumerate(zip(edge, params)):
        if d["has_grad"]:
            st = opt.state[p]
            assert float(st["step"]) == d["t"] and st["step"].device.type == "cpu" and p._version > versions[i]
            for k, t in (("p", p.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
                assert torch.equal(t.view(torch.int32), ref[i][1][k].view(torch.int32)), (d["n"], k)
            assert torch.equal(p.grad, R.views(d, d)["g"].cuda())          # gradients are left unscaled
        else:
            assert p not in opt.state and p._version == versions[i] and torch.equal(p.detach().cpu(), R.views(d, d)["p"])


# ---- the optimizer, the EMA and the weight caches together ----
# the three-level sd3 encoder of tests/test_training_config_path.py (configs/cvvae_sd3_constraint_training.yaml:10-23, block widths cut)
SMALL_ENCODER = dict(in_channels=3, out_channels=16, down_block_types=["DownEncoderBlock3D"] * 3, block_out_channels=[128, 256, 256],
                     layers_per_block=1, norm_num_groups=32, act_fn="silu", double_z=True, mid_block_add_attention=True, causal=True,
                     half_3d=True)
LATENT_BAND = 4e-5   # relative, fp32 network (README.md, round 4)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.gpu
def test_training_step_with_the_kernel_update_matches_torchs_and_the_caches_follow():
    from cvvae_amd.optim import AdamW
    from lvdm.modules.diffusionmodules.vae_models3d_sd3 import Encoder3D
    from lvdm.modules.ema import LitEma
    from oracle.seeded import seeded_input, seeded_state_dict
    lr = 1e-3
    nets = [Encoder3D(**SMALL_ENCODER) for _ in range(2)]
    sd = seeded_state_dict({k: v.shape for k, v in nets[0].state_dict().items()}, 7)
    for n in nets:
        n.load_state_dict(sd, strict=True)
        n.float().cuda().train()
    ours, theirs = nets
    x = seeded_input((1, 3, 5, 16, 16), 21).cuda()

    def latents(net):   # the taped training pass: its weight cache is checked on train() / eval() transitions only
        return net(x)

    def loss_of(z):
        return 100.0 * z.pow(2).mean()

    before = {n: p.detach().clone() for n, p in theirs.named_parameters()}
    # ours: clip + AdamW in two sweeps, EMA in one
    opt = AdamW(ours.parameters(), lr=lr, max_grad_norm=1.0, **R.YAML_ADAMW)
    ema = LitEma(ours)
    z1 = latents(ours)
    loss_of(z1).backward()
    opt.step()
    ema(ours)
    # theirs: torch's clip, torch's AdamW, the per-parameter EMA loop
    t_opt = torch.optim.AdamW(theirs.parameters(), lr=lr, **R.YAML_ADAMW)
    shadow = {n: p.detach().clone() for n, p in theirs.named_parameters()}
    zt1 = latents(theirs)
    loss_of(zt1).backward()
    assert torch.equal(z1, zt1)
    t_norm = torch.nn.utils.clip_grad_norm_(theirs.parameters(), 1.0)
    t_opt.step()
    decay = torch.minimum(torch.tensor(0.9999), torch.tensor(2, dtype=torch.int32) / torch.tensor(11, dtype=torch.int32))
    with torch.no_grad():
        for n, p in theirs.named_parameters():
            shadow[n].sub_((1.0 - decay).cuda() * (shadow[n] - p))
    torch.cuda.synchronize()
    assert float(t_norm) > 1.0 and float(opt.last_grad_norm) == pytest.approx(float(t_norm), rel=1e-5)   # the clip is active
    worst = 0.0
    for (n, p), (_, q) in zip(ours.named_parameters(), theirs.named_parameters()):
        delta = (q.detach().double() - before[n].double()).abs().cpu()
        bound = 3 * (R.ulp32(before[n].double().cpu()) + 2.0 ** -20 * delta)
        w = _worst(p.detach().cpu(), q.detach().double().cpu(), bound)
        worst = max(worst, w)
        assert w <= 1.0, (n, w)
        assert q.grad is None or bool((delta > 0).any()), n
    print(f"parameters after one step, ours vs torch's: fraction of the p bound {worst}")
    # the next pass sees the step without any cache invalidation call
    z2, zt2 = latents(ours).detach(), latents(theirs).detach()
    assert _rel(z2, z1.detach()) > 10 * LATENT_BAND
    assert _rel(z2, zt2) <= LATENT_BAND, _rel(z2, zt2)
    # the EMA swap for validation: shadow weights in, live weights back
    ema.store(ours.parameters())
    ema.copy_to(ours)
    z_ema = latents(ours).detach()
    theirs.load_state_dict(shadow, strict=False)
    zt_ema = latents(theirs).detach()
    assert _rel(z_ema, z2) > 10 * LATENT_BAND                              # the shadow is 9/11 of the way: other weights
    assert _rel(z_ema, zt_ema) <= LATENT_BAND, _rel(z_ema, zt_ema)
    ema.restore(ours.parameters())
    z3 = latents(ours).detach()
    assert torch.equal(z3, z2)
    assert int(ema.num_updates) == 1 and all(p.is_leaf for p in ours.parameters())
