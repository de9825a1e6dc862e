"""Time one evaluation of the training loss on an MI355X: LPIPSWithDiscriminatorAndDomainConstraint + DiagonalGaussianRegularizer,
generator branch and discriminator branch, forward + backward, at inputs [1,3,17,256,256], 2-D reconstructions [1,3,5,256,256] and
moments [1,32,5,32,32]; (a) through cvvae_amd.loss on libcvvae_hip.so and (b) with the same arithmetic written as eager torch
ops (the reference's formulas: full-size temporaries, torch.sum / torch.mean) on the same GPU, the two interleaved call by call.
The discriminator is an elementwise stand-in in both (no discriminator network ships yet).  Variants: `lpips` (the perceptual
term on; BOTH paths call cvvae_amd.lpips.LPIPS, so the difference is the passes around it) and `pixel` (perceptual_weight = 0: the
new passes alone); reconstructions in fp32 and bf16.

    timeout -k 10 900 python tools/loss_step.py                  # writes profiles/loss_step.json
    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d <dir> -o loss -- python tools/loss_step.py --only hip --variant pixel --iters 3 --out <dir>/x.json
    (and --only torch for the baseline's kernel count; counters and traces go in runs of their own)

Each figure is the median host time of `--iters` calls, every call between two device synchronisations, after `--warmup` untimed
calls.  There is no CPU path.  No speed bar is asserted; the ratio is recorded (DESIGN.md 3.8 discusses it)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvvae_amd import _lib  # noqa: E402
from cvvae_amd.loss import DiagonalGaussianRegularizer, LPIPSWithDiscriminatorAndDomainConstraint  # noqa: E402
from tools.lpips_step import seeded_weights  # noqa: E402


class Disc(nn.Module):
    """elementwise stand-in: 5-D clip -> 5-D logits"""

    def __init__(self):
        super().__init__()
        self.gain = nn.Parameter(torch.tensor(1.7))
        self.bias = nn.Parameter(torch.tensor(-0.2))

    def forward(self, x):
        return self.gain.to(x.dtype) * torch.tanh(2.0 * x[:, :1]) + self.bias.to(x.dtype) * x[:, 1:2]


def frames(x):
    b, c, t, h, w = x.shape
    return x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)


def torch_regulariser(moments, noise):
    mean, logvar = torch.chunk(moments, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    z = mean + torch.exp(0.5 * logvar) * noise
    kl = 0.5 * torch.sum(mean ** 2 + torch.exp(logvar) - 1.0 - logvar, dim=[1, 2, 3, 4])
    return z, {"kl_loss": torch.sum(kl) / kl.shape[0]}


def torch_loss(m, inputs, recs, recs2d, rlog, idx, last_layer):
    """the reference's forward (discriminator_loss.py:392-585, target_type "slice") in eager torch ops on the module's parameters"""
    x, r = frames(inputs), frames(recs)
    t2, r2 = frames(inputs[:, :, ::m.time_n_compress]), frames(recs2d)
    rec2d = torch.abs(t2.contiguous() - r2.contiguous())
    rec = torch.abs(x.contiguous() - r.contiguous())
    if m.perceptual_weight > 0:
        rec = rec + m.perceptual_weight * m.perceptual_loss(x.contiguous(), r.contiguous())
    nll = rec / torch.exp(m.logvar) + m.logvar
    n2 = rec2d / torch.exp(m.logvar_2d) + m.logvar_2d
    n2 = torch.sum(n2) / n2.shape[0]
    nll = torch.sum(nll) / nll.shape[0] + m.rec2d_weight * n2
    if idx == 0:
        g_loss = -torch.mean(m.discriminator(recs.contiguous()))
        ng = torch.autograd.grad(nll, last_layer, retain_graph=True)[0]
        gg = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
        d_weight = torch.clamp(torch.norm(ng) / (torch.norm(gg) + 1e-4), 0.0, 1e4).detach() * m.discriminator_weight
        loss = nll + d_weight * m.disc_factor * g_loss
        for k in rlog:
            if k in m.regularization_weights:
                loss = loss + m.regularization_weights[k] * rlog[k]
        return loss
    real = m.discriminator(inputs.contiguous().detach())
    fake = m.discriminator(recs.contiguous().detach())
    return m.disc_factor * 0.5 * (torch.mean(F.relu(1.0 - real)) + torch.mean(F.relu(1.0 + fake)))


def interleaved(fns, warmup, iters):
    """median host ms of each callable, the callables taking turns"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "iters": iters} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", choices=["hip", "torch"], help="one path alone (kernel traces)")
    ap.add_argument("--variant", choices=["lpips", "pixel"], help="one variant alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/loss_step.py measures on an MI355X; no GPU found (there is no CPU path)")
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(11)
    T, S = a.frames, a.size
    T2 = (T - 1) // 4 + 1
    x = (torch.rand((1, 3, T, S, S), generator=g) * 2 - 1).cuda()
    res = {"inputs": [1, 3, T, S, S], "reconstructions_2d": [1, 3, T2, S, S], "moments": [1, 32, T2, S // 8, S // 8],
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernel_sources": _lib.source_fingerprint(),
           "baseline": "the same formulas as eager torch ops, same GPU, interleaved; LPIPS is cvvae_amd.lpips in both", "runs": {}}
    reg = DiagonalGaussianRegularizer()
    for variant in ([a.variant] if a.variant else ["lpips", "pixel"]):
        for dtype in (torch.float32, torch.bfloat16):
            m = LPIPSWithDiscriminatorAndDomainConstraint(disc_start=0, dims=3, perceptual_weight=1.0 if variant == "lpips" else 0.0,
                                                          regularization_weights={"kl_loss": 1e-6}, discriminator=Disc())
            seeded_weights(m.perceptual_loss)
            m.perceptual_loss.to(dtype)
            m = m.cuda().train()
            base = (x + 0.3 * (torch.rand(x.shape, generator=g) * 2 - 1).cuda()).clamp(-1, 1).to(dtype)
            base2 = (x[:, :, ::4] + 0.2 * (torch.rand((1, 3, T2, S, S), generator=g) * 2 - 1).cuda()).clamp(-1, 1).to(dtype)
            mom0 = torch.randn((1, 32, T2, S // 8, S // 8), generator=g).cuda().to(dtype)
            noise = torch.randn((1, 16, T2, S // 8, S // 8), generator=g).cuda().to(dtype)
            last0 = torch.tensor([1.0, 1.0, 1.0], device="cuda", dtype=dtype)

            def step(hip, idx):
                mom = mom0.clone().requires_grad_(True)
                last = last0.clone().requires_grad_(True)
                z, rlog = reg(mom, noise=noise) if hip else torch_regulariser(mom, noise)
                rec = base * last.view(1, 3, 1, 1, 1) + 1e-3 * z[:, :3, :1, :1, :1]
                rec2 = base2.clone().requires_grad_(True)
                if hip:
                    loss, _ = m(x, rec, rec2, regularization_log=rlog, optimizer_idx=idx, global_step=1, last_layer=last)
                else:
                    loss = torch_loss(m, x, rec, rec2, rlog, idx, last)
                m.zero_grad(set_to_none=True)
                loss.backward()
                return loss.detach(), (last.grad if idx == 0 else m.discriminator.gain.grad.clone())

            fns = {}
            for idx, branch in ((0, "generator"), (1, "discriminator")):
                for path in (["hip", "torch"] if not a.only else [a.only]):
                    fns[f"{branch}_{path}"] = (lambda p=path, i=idx: step(p == "hip", i))
            run = interleaved(fns, a.warmup, a.iters)
            if not a.only:
                for idx, branch in ((0, "generator"), (1, "discriminator")):
                    run[f"{branch}_torch_over_hip"] = run[f"{branch}_torch"]["median_ms"] / run[f"{branch}_hip"]["median_ms"]
                    (lh, gh), (lt, gt) = step(True, idx), step(False, idx)
                    run[f"{branch}_loss_hip_vs_torch"] = [float(lh), float(lt)]
                    run[f"{branch}_grad_rel_l2_hip_vs_torch"] = float((gh.float() - gt.float()).norm() / gt.float().norm())
            res["runs"][f"{variant}_{str(dtype)[6:]}"] = run
            print(variant, str(dtype)[6:], json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
