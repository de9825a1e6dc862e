"""Time the discriminator passes of csrc/disc_kernels.hip on an MI355X at the shapes the 3-D PatchGAN discriminator has on a
[1,3,17,256,256] clip, (a) through cvvae_amd.ops / cvvae_amd.disc_ops on libcvvae_hip.so and (b) as the same ops in eager torch on
the same GPU (channels-last-3d views of the same NDHWC buffers), the two interleaved sample by sample.

    timeout -k 10 600 python tools/disc_ops_step.py                 # writes profiles/disc_ops.json

Ops: the downsample pool and its adjoint at [1,9,128,128,128] and [1,5,64,64,256]; GroupNorm + LeakyReLU forward (statistics + apply)
and backward (cvvae_leaky_bwd + cvvae_gn_bwd_input_params), the apply pass and cvvae_leaky_bwd alone, at [1,5,64,64,128],
[1,3,32,32,256] and [1,3,32,32,512]; the bare LeakyReLU and its backward at [1,9,128,128,64].  bf16 and fp32.

Two figures per op and path, each the median of `--iters` samples after `--warmup` untimed ones:
  streamed_us  device time (events) of one sweep of back-to-back calls over K distinct buffer sets, per call -- K chosen so that the
               sweep moves >= 1 GiB where 32 sets allow it (the 256 MiB Infinity Cache then cannot hold the operands; `footprint_mib`
               says when it can).  `hbm_fraction` = bytes / streamed time / 6.3 TB/s, bytes = the tensors each pass must read and
               write once (`bytes`), so a pass that reads an operand twice shows as a lower fraction.
  call_us      host time of ONE call between two device synchronisations: what a caller in a chain of dependent launches waits for.
There is no CPU path.  No speed bar is asserted; DESIGN.md 3.9 states the result."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvvae_amd import _lib, disc_ops, ops  # noqa: E402

HBM_BYTES_PER_S = 6.3e12   # the figure DESIGN.md uses
SLOPE, EPS, GROUPS = 0.2, 1e-6, 32


def ncdhw(t):
    """the channels-last-3d view torch's ops take: same memory"""
    return t.permute(0, 4, 1, 2, 3)


def torch_pool(v):
    if v.shape[2] % 2 == 1:
        v = torch.cat([v[:, :, :1], v], dim=2)
    return F.avg_pool3d(v, kernel_size=2, stride=2)


def build(op, shape, dtype, k, g):
    """k independent (hip, torch) call pairs of one op on their own buffers, and the bytes one call must move"""
    B, T, H, W, C = shape
    n, es = B * T * H * W * C, torch.finfo(dtype).bits // 8
    rnd = lambda s=shape: torch.randn(s, generator=g, device="cuda").to(dtype)  # noqa: E731
    hip, ref = [], []
    if op in ("pool_fwd", "pool_bwd"):
        oshape = ops.avgpool3d_down_shape(shape)
        no = math.prod(oshape)
        for _ in range(k):
            if op == "pool_fwd":
                x = rnd()
                hip.append(lambda x=x: ops.avgpool3d_down(x))
                ref.append(lambda x=x: torch_pool(ncdhw(x)))
            else:
                gy = rnd(oshape)
                xr = ncdhw(rnd()).requires_grad_(True)
                yr = torch_pool(xr)
                hip.append(lambda gy=gy: ops.avgpool3d_down_bwd(gy, shape))
                ref.append(lambda yr=yr, xr=xr, gy=gy: torch.autograd.grad(yr, xr, ncdhw(gy), retain_graph=True))
        return hip, ref, (n + no) * es
    w = 1.0 + 0.2 * torch.randn(C, generator=g, device="cuda")
    b = 0.3 * torch.randn(C, generator=g, device="cuda")
    for _ in range(k):
        x = rnd()
        if op == "gn_leaky_fwd":          # must read x and write y (the statistics pass reads x a second time)
            hip.append(lambda x=x: disc_ops.group_norm_leaky(x, w, b, GROUPS, EPS, SLOPE))
            ref.append(lambda x=x: F.leaky_relu(F.group_norm(ncdhw(x), GROUPS, w.to(dtype), b.to(dtype), EPS), SLOPE))
            nbytes = 2 * n * es
        elif op == "gn_leaky_bwd":        # cvvae_leaky_bwd + cvvae_gn_bwd_input_params: must read y, gy, x and write gx
            gy = rnd()
            xa = x.clone().requires_grad_(True)
            wa, ba = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
            ya = disc_ops.group_norm_leaky(xa, wa, ba, GROUPS, EPS, SLOPE)
            xr = ncdhw(x).clone(memory_format=torch.channels_last_3d).requires_grad_(True)
            wr, br = w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
            yr = F.leaky_relu(F.group_norm(xr, GROUPS, wr, br, EPS), SLOPE)
            hip.append(lambda ya=ya, ins=(xa, wa, ba), gy=gy: torch.autograd.grad(ya, ins, gy, retain_graph=True))
            ref.append(lambda yr=yr, ins=(xr, wr, br), gy=gy: torch.autograd.grad(yr, ins, ncdhw(gy), retain_graph=True))
            nbytes = 4 * n * es
        elif op == "apply":
            sc, sh = ops.gn_stats(x, w, b, EPS, groups=GROUPS)
            scb, shb = sc.to(dtype)[:, None, None, None, :], sh.to(dtype)[:, None, None, None, :]
            hip.append(lambda x=x, t=(sc, sh): ops.gn_leaky_apply(x, t, SLOPE))
            ref.append(lambda x=x, scb=scb, shb=shb: F.leaky_relu(torch.addcmul(shb, x, scb), SLOPE))
            nbytes = 2 * n * es
        elif op == "bare_fwd":
            hip.append(lambda x=x: ops.gn_leaky_apply(x, None, SLOPE))
            ref.append(lambda x=x: F.leaky_relu(x, SLOPE))
            nbytes = 2 * n * es
        elif op == "leaky_bwd":
            gy = rnd()
            hip.append(lambda y=x, gy=gy: ops.leaky_bwd(y, gy, SLOPE))
            ref.append(lambda y=x, gy=gy: torch.where(y > 0, gy, SLOPE * gy))
            nbytes = 3 * n * es
        else:
            raise ValueError(op)
    return hip, ref, nbytes


def measure(paths, warmup, iters):
    """paths: {name: [callables on distinct buffers]} -> per name the median streamed and single-call times, the paths taking turns"""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    streamed, single = {p: [] for p in paths}, {p: [] for p in paths}
    for it in range(warmup + iters):
        for p, fns in paths.items():
            torch.cuda.synchronize()
            ev0.record()
            for f in fns:
                f()
            ev1.record()
            torch.cuda.synchronize()
            t_sweep = ev0.elapsed_time(ev1) * 1e3 / len(fns)
            f = fns[it % len(fns)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t_call = (time.perf_counter() - t0) * 1e6
            if it >= warmup:
                streamed[p].append(t_sweep)
                single[p].append(t_call)
    return {p: {"streamed_us": statistics.median(streamed[p]), "streamed_min_us": min(streamed[p]), "streamed_max_us": max(streamed[p]),
                "call_us": statistics.median(single[p])} for p in paths}


CASES = [("pool_fwd", (1, 9, 128, 128, 128)), ("pool_bwd", (1, 9, 128, 128, 128)),
         ("pool_fwd", (1, 5, 64, 64, 256)), ("pool_bwd", (1, 5, 64, 64, 256)),
         ("gn_leaky_fwd", (1, 5, 64, 64, 128)), ("gn_leaky_bwd", (1, 5, 64, 64, 128)), ("apply", (1, 5, 64, 64, 128)),
         ("leaky_bwd", (1, 5, 64, 64, 128)),
         ("gn_leaky_fwd", (1, 3, 32, 32, 256)), ("gn_leaky_bwd", (1, 3, 32, 32, 256)), ("apply", (1, 3, 32, 32, 256)),
         ("leaky_bwd", (1, 3, 32, 32, 256)),
         ("gn_leaky_fwd", (1, 3, 32, 32, 512)), ("gn_leaky_bwd", (1, 3, 32, 32, 512)), ("apply", (1, 3, 32, 32, 512)),
         ("leaky_bwd", (1, 3, 32, 32, 512)),
         ("bare_fwd", (1, 9, 128, 128, 64)), ("leaky_bwd", (1, 9, 128, 128, 64))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", choices=["hip", "torch"], help="one path alone (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_ops.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/disc_ops_step.py measures on an MI355X; no GPU found (there is no CPU path)")
    torch.cuda.set_device(0)
    res = {"clip": [1, 3, 17, 256, 256], "warmup": a.warmup, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "kernel_sources": _lib.source_fingerprint(),
           "baseline": "the same ops as eager torch on channels-last-3d views of the same buffers, same GPU, interleaved", "runs": {}}
    for dtype in (torch.bfloat16, torch.float32):
        for op, shape in CASES:
            g = torch.Generator(device="cuda").manual_seed(17)
            probe = build(op, shape, dtype, 1, g)[2]
            k = max(2, min(32, math.ceil(2 ** 30 / probe)))
            hip, ref, nbytes = build(op, shape, dtype, k, g)
            paths = {p: f for p, f in (("hip", hip), ("torch", ref)) if not a.only or a.only == p}
            run = measure(paths, a.warmup, a.iters)
            run.update(shape=list(shape), bytes=nbytes, buffer_sets=k, footprint_mib=k * nbytes / 2 ** 20)
            for p in paths:
                run[p]["hbm_fraction"] = nbytes / (run[p]["streamed_us"] * 1e-6) / HBM_BYTES_PER_S
            if not a.only:
                run["torch_over_hip_streamed"] = run["torch"]["streamed_us"] / run["hip"]["streamed_us"]
                run["torch_over_hip_call"] = run["torch"]["call_us"] / run["hip"]["call_us"]
            key = f"{op}_{'x'.join(map(str, shape))}_{str(dtype)[6:]}"
            res["runs"][key] = run
            print(key, json.dumps(run), flush=True)
            del hip, ref, paths
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
