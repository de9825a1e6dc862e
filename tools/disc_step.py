"""Time the 3-D PatchGAN discriminator (cvvae_amd/discriminator.py) on an MI355X at the training clip [1,3,17,256,256], in bf16 and
fp32, (a) as the module on libcvvae_hip.so and (b) as the same network in eager torch on the same GPU (its own containers,
channels_last_3d tensors), the two interleaved sample by sample.

    timeout -k 10 1100 python tools/disc_step.py                    # writes profiles/disc_net.json

Per dtype, each figure the median device time (events) of `--iters` samples after `--warmup` untimed ones:
  forward         torch.no_grad()
  disc_step       forward + backward with a DETACHED input (parameter gradients only: the first layer's input gradient is skipped)
  gen_step        forward + backward with an attached input and trainable parameters (what the loss's generator branch walks)
  first_dgrad     the first layer's input gradient alone, [1,9,128,128,64] -> [1,17,256,256,8]: the direct gather kernel
                  (cvvae_conv333_s2_dgrad_small) and grad3d.dgrad333's zero-stuffed MFMA path, interleaved, with the largest
                  difference of the two results
There is no CPU path.  No speed bar is asserted; DESIGN.md 3.11 states the result."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvvae_amd import _lib, discriminator as D  # noqa: E402
from cvvae_amd.loss import weights_init  # noqa: E402

CLIP = (1, 3, 17, 256, 256)


def timed(fn):
    if isinstance(fn, tuple):
        fn[0]()
        fn = fn[1]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def interleaved(fns, warmup, iters):
    """{name: median us} of the callables, run round-robin"""
    for _ in range(warmup):
        for f in fns.values():
            timed(f)
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            samples[k].append(timed(f))
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
            for k, v in samples.items()}


def step(net, x, attached, eager):
    """(prepare, run): `prepare` -- outside the timed window -- clears the gradients and makes the input leaf; `run` is forward + backward"""
    box = {}

    def prepare():
        net.zero_grad(set_to_none=True)
        box["x"] = x.clone().requires_grad_(attached)

    def run():
        y = net.forward_eager(box["x"]) if eager else net(box["x"])
        y.float().mean().backward()
    return prepare, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_net.json"))
    ap.add_argument("--dtypes", default="bfloat16,float32")
    ap.add_argument("--no-eager", action="store_true", help="skip the eager-torch baseline")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/disc_step.py measures on an MI355X; no GPU found")
    out = {"clip": list(CLIP), "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
           "source_fingerprint": _lib.source_fingerprint(), "dtypes": {}}
    for name in a.dtypes.split(","):
        dtype = getattr(torch, name)
        torch.manual_seed(0)
        net = D.get_cvvae_discriminator().apply(weights_init).to(dtype).cuda().train()
        x = (torch.rand(CLIP, device="cuda") * 2 - 1).to(dtype)
        xe = x.contiguous(memory_format=torch.channels_last_3d)
        ref = None if a.no_eager else D.get_cvvae_discriminator().to(dtype).cuda().train().to(memory_format=torch.channels_last_3d)
        if ref is not None:
            ref.load_state_dict(net.state_dict())
        res = {}

        def fwd(n, xx, eager):
            def run():
                with torch.no_grad():
                    return n.forward_eager(xx) if eager else n(xx)
            return run
        for label, attached in (("forward", None), ("disc_step", False), ("gen_step", True)):
            fns = {"hip": fwd(net, x, False) if attached is None else step(net, x, attached, False)}
            if ref is not None:
                fns["eager"] = fwd(ref, xe, True) if attached is None else step(ref, xe, attached, True)
            res[label] = interleaved(fns, a.warmup, a.iters)
            print(name, label, res[label], flush=True)
        if ref is not None:
            with torch.no_grad():
                ya, yb = net(x).float(), ref.forward_eager(xe).float()
            res["logits_rel_diff_vs_eager"] = float((ya - yb).norm() / yb.norm())
        # the first layer's input gradient, both ways, on one gradient tensor
        wc = net._cache()
        gv = torch.randn(1, 9, 128, 128, 64, device="cuda").to(dtype)
        in_shape = (1, 17, 256, 256)
        res["first_dgrad"] = interleaved({"direct": lambda: D.first_layer_dgrad(wc, gv, in_shape, 3, direct=True),
                                          "zero_stuffed": lambda: D.first_layer_dgrad(wc, gv, in_shape, 3, direct=False)},
                                         a.warmup, a.iters)
        da, db = D.first_layer_dgrad(wc, gv, in_shape, 3, direct=True), D.first_layer_dgrad(wc, gv, in_shape, 3, direct=False)
        res["first_dgrad"]["max_abs_diff"] = float((da.float() - db.float()).abs().max())
        res["first_dgrad"]["max_abs"] = float(db.float().abs().max())
        es = torch.finfo(dtype).bits // 8
        res["first_dgrad"]["bytes_gy_plus_gx"] = (gv.numel() + da.numel()) * es
        print(name, "first_dgrad", res["first_dgrad"], flush=True)
        out["dtypes"][name] = res
        del net, ref
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:      # (after every dtype: a partial run still leaves its figures)
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
