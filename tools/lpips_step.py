"""Time one training-sized LPIPS call on an MI355X: forward + backward of `LPIPS(inputs, reconstructions)` over 2N = 34 frames of
256x256 with the gradient into `reconstructions` only (what a training step does), in bf16 and fp32, (a) through cvvae_amd.lpips
on libcvvae_hip.so and (b) through the plain-torch restatement of the reference's LPIPS.forward on PyTorch-ROCm's own kernels
(MIOpen convolutions, ATen elementwise ops, torch.autograd), on the same GPU and the same seeded weights.

    timeout 900 python tools/lpips_step.py                 # writes profiles/lpips_step.json
    timeout 900 rocprofv3 --kernel-trace --stats -d <dir> -o lpips -- python tools/lpips_step.py --hip-only --iters 3 --out <dir>/x.json

Each figure is the median host time of `--iters` calls, every call between two device synchronisations, after `--warmup` untimed
calls of the same shape.  There is no CPU path: without a GPU the script fails.  No speed bar is asserted; the HIP / torch ratio
is recorded (DESIGN.md discusses it)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvvae_amd import _lib  # noqa: E402
from cvvae_amd.lpips import PLAN, LPIPS  # noqa: E402


def seeded_weights(m: LPIPS, seed: int = 3):
    """He-scaled conv weights (features stay O(1) through 13 layers), non-negative lin weights -- no trained weights exist offline"""
    g = torch.Generator().manual_seed(seed)
    sd = m.state_dict()
    for k, v in sd.items():
        if k.startswith("net.") and k.endswith(".weight"):
            fan_in = v[0].numel()
            sd[k] = (torch.rand(v.shape, generator=g) * 2 - 1) * (6.0 / fan_in) ** 0.5
        elif k.startswith("net."):
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
        elif k.startswith("lin"):
            sd[k] = torch.rand(v.shape, generator=g) / v.shape[1] ** 0.5
    m.load_state_dict(sd)
    return m


def torch_lpips(inp, tgt, p):
    """the reference's LPIPS.forward (lvdm/modules/autoencoding/lpips/loss/lpips.py:46-64) in plain torch ops"""
    def trunk(x):
        x = (x - p["scaling_layer.shift"]) / p["scaling_layer.scale"]
        outs = []
        for name, pool, convs in PLAN:
            if pool:
                x = F.max_pool2d(x, 2, 2)
            for i in convs:
                x = F.relu(F.conv2d(x, p[f"net.{name}.{i}.weight"], p[f"net.{name}.{i}.bias"], padding=1))
            outs.append(x)
        return outs

    def nrm(x, eps=1e-10):
        return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True) + eps) + eps)

    val = 0
    for kk, (a, b) in enumerate(zip(trunk(inp), trunk(tgt))):
        val = val + F.conv2d((nrm(a) - nrm(b)) ** 2, p[f"lin{kk}.model.1.weight"]).mean([2, 3], keepdim=True)
    return val


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=17)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--hip-only", action="store_true", help="skip the torch baseline (kernel traces of the HIP path alone)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lpips_step.py measures on an MI355X; no GPU found (there is no CPU path)")
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(11)
    shape = (a.pairs, 3, a.size, a.size)
    x = (torch.rand(shape, generator=g) * 2 - 1).cuda()
    xrec0 = (x.cpu() + 0.3 * (torch.rand(shape, generator=g) * 2 - 1)).clamp(-1, 1).cuda()
    res = {"shape": list(shape), "frames": 2 * a.pairs, "gradient_into": "target", "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "kernel_sources": _lib.source_fingerprint(), "runs": {}}
    for dtype in (torch.bfloat16, torch.float32):
        name = str(dtype)[6:]
        m = seeded_weights(LPIPS().eval()).to(dtype).cuda()
        p = {k: v.detach() for k, v in m.state_dict().items()}
        xi, xr = x.to(dtype), xrec0.to(dtype)

        def hip_step():
            r = xr.clone().requires_grad_(True)
            m(xi, r).sum().backward()
            return r.grad

        def torch_step():
            r = xr.clone().requires_grad_(True)
            torch_lpips(xi, r, p).sum().backward()
            return r.grad

        run = {"hip": timed(hip_step, a.warmup, a.iters)}
        if not a.hip_only:
            run["torch"] = timed(torch_step, a.warmup, a.iters)
            run["torch_over_hip"] = run["torch"]["median_ms"] / run["hip"]["median_ms"]
            gh, gt = hip_step().float(), torch_step().float()
            run["grad_rel_l2_hip_vs_torch"] = float((gh - gt).norm() / gt.norm())
        res["runs"][name] = run
        print(name, json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
