"""Time ONE WHOLE CV-VAE training iteration on an MI355X -- a generator iteration and a discriminator iteration -- through
  (a) `engine`: AutoencodingEngineWithLatentConstraint.training_step + on_train_batch_end (cvvae_amd/autoencoder.py), and
  (b) `hand`:   the hand-assembled sequence of the same public calls (tests/engine_cases.py ByHand) on a second copy of the modules,
the two taking turns sample by sample in ONE process, on the same clip.  Shape [1,3,17,256,256], the shipped widths, the training
YAML's entries (tests/engine_cases.py latent_config: loss `LPIPSWithDiscriminatorAndDomainConstraint` with `target_type: random` and
`frame_maps: true`, `cvvae_amd.optim.AdamW` with `max_grad_norm: 1.0`), in two set-ups: bf16 networks, and fp32 modules under
torch.autocast(bfloat16).  `--config file.yaml` takes the model from a training YAML instead (a `ckpt_path` that is no file is dropped).

    timeout -k 10 900 python tools/train_iteration.py             # writes profiles/train_iteration.json

Per path and iteration kind: the median / min / max over `--iters` samples of the time between two device events around the call
(host time the device does not hide is in it), the host's own time in the call (perf_counter, no synchronisation) and the peak of
allocated device memory during the call (both copies of the modules are resident).  The criterion recorded with the figures: the
engine's median lies within the hand-assembled sequence's own min-max spread of the same run; if it does not, a cProfile listing of
one engine iteration is attached (all frames by cumulative time, and the engine's own frames by their own time).  The panels pass of log_images (ops.recon_panels) is timed at the same shape with its bytes moved
(2 reads + 4 writes per element) against 6.3e12 bytes/s: reported only.  There is no CPU path."""
import argparse
import copy
import cProfile
import io
import json
import os
import pstats
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvvae_amd import _lib, ops  # noqa: E402
from lvdm.models.autoencoder import build_from_config  # noqa: E402
from tests import engine_cases as EC  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SHAPE = (1, 3, 17, 256, 256)
SHIPPED = dict(block_out_channels=[128, 256, 512, 512], layers_per_block=2)


def load_config(path):
    if path is None:
        return EC.latent_config(SHIPPED, target_type="random")
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    params = cfg["model"]["params"]
    for k in ("ckpt_path", "ckpt_engine"):
        if isinstance(params.get(k), str) and not os.path.isfile(params[k]):
            print(f"{k}: {params[k]!r} is no file, dropped")
            params.pop(k)
    return cfg


def sample(fn):
    """-> (device ms, host ms, peak allocated bytes) of one call"""
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), host, torch.cuda.max_memory_allocated()


def stats(rows):
    ms, host, peak = zip(*rows)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "host_median_ms": statistics.median(host),
            "peak_allocated_gib": max(peak) / 2 ** 30, "iters": len(ms)}


def measure(cfg, setup, warmup, iters):
    torch.manual_seed(0)
    a = EC.seed_engine(build_from_config(copy.deepcopy(cfg))).train()      # seeded weights: finite activations at every layer
    b = copy.deepcopy(a)
    mp = cfg["model"]["params"]
    if setup == "bf16":
        a, b = EC.to_device(a, torch.bfloat16), EC.to_device(b, torch.bfloat16)
        x = torch.rand(SHAPE, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
    else:
        a, b = a.cuda(), b.cuda()
        x = torch.rand(SHAPE, device="cuda").mul_(2).sub_(1)
    autocast = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=setup != "bf16")  # noqa: E731
    a.sample_generator = torch.Generator("cuda").manual_seed(1)
    hand = EC.ByHand("latent", EC.modules_of(b), lr=a.learning_rate, lr_g_factor=mp.get("lr_g_factor", 1.0), ema=getattr(b, "model_ema", None),
                     tn=a.loss.time_n_compress, optimizer_config=mp.get("optimizer_config"), lr_g_scheduler_config=mp.get("lr_g_scheduler_config"))
    hand.ema_model, hand.generator = b, torch.Generator("cuda").manual_seed(1)
    batch = {a.input_key: x}

    def engine_it(i):
        with autocast():
            a.training_step(batch, i)
        a.on_train_batch_end()

    def hand_it(i):
        with autocast():
            hand.step(x, i)

    paths = {"engine": engine_it, "hand": hand_it}
    for _ in range(warmup):
        for fn in paths.values():
            fn(0)
            fn(1)
    torch.cuda.synchronize()
    rows = {(p, k): [] for p in paths for k in ("generator", "discriminator")}
    for _ in range(iters):
        for p, fn in paths.items():            # sample by sample: engine generator, engine discriminator, hand generator, hand discriminator
            rows[(p, "generator")].append(sample(lambda: fn(0)))
            rows[(p, "discriminator")].append(sample(lambda: fn(1)))
    out = {"setup": setup, "global_step_after": [a.global_step, hand.global_step]}
    for kind in ("generator", "discriminator"):
        e, h = stats(rows[("engine", kind)]), stats(rows[("hand", kind)])
        inside = h["min_ms"] <= e["median_ms"] <= h["max_ms"]
        out[kind] = {"engine": e, "hand": h, "engine_over_hand_median": e["median_ms"] / h["median_ms"],
                     "engine_median_within_hand_spread": inside}
        if not inside:
            prof = cProfile.Profile()
            prof.enable()
            engine_it(0 if kind == "generator" else 1)
            torch.cuda.synchronize()
            prof.disable()
            s, own = io.StringIO(), io.StringIO()
            pstats.Stats(prof, stream=s).strip_dirs().sort_stats("cumulative").print_stats(30)
            pstats.Stats(prof, stream=own).strip_dirs().sort_stats("tottime").print_stats(r"autoencoder\.py")   # the engine's own frames
            out[kind]["cprofile_of_one_engine_iteration"] = s.getvalue().splitlines()
            out[kind]["cprofile_engine_own_frames"] = own.getvalue().splitlines()
    # the panels pass at this shape
    with torch.no_grad():
        xrec = (x.float() + 0.1 * torch.randn(SHAPE, device="cuda")).to(x.dtype)
        for _ in range(3):
            ops.recon_panels(x, xrec, 3.0)
        r = stats([sample(lambda: ops.recon_panels(x, xrec, 3.0)) for _ in range(max(iters, 20))])
    nbytes = 6 * x.numel() * x.element_size()
    r.update(bytes_moved=nbytes, bytes_per_s=nbytes / (r["median_ms"] * 1e-3), frac_of_hbm=nbytes / (r["median_ms"] * 1e-3) / HBM_BYTES_PER_S,
             dtype=str(x.dtype)[6:])
    out["recon_panels"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=None, help="a training YAML (model.target an engine of lvdm.models.autoencoder)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--setups", default="bf16,fp32_autocast")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_iteration.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/train_iteration.py measures on an MI355X; no GPU found (there is no CPU path)")
    torch.cuda.set_device(0)
    cfg = load_config(a.config)
    res = {"what": "one whole training iteration (forward, loss, backward, clip, AdamW, schedulers, EMA hook) of "
                   + cfg["model"]["target"].rsplit(".", 1)[1] + " and of the hand-assembled sequence of the same calls",
           "shape": list(SHAPE), "config": a.config or "tests/engine_cases.py latent_config (the training YAML's entries, frame_maps: true)",
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernel_sources": _lib.source_fingerprint(),
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "timing": "device events around each call, paths interleaved sample by sample in one process",
           "runs": {}}
    for setup in a.setups.split(","):
        try:
            res["runs"][setup] = measure(cfg, setup, a.warmup, a.iters)
        except (RuntimeError, NotImplementedError, ValueError, TypeError) as e:   # a set-up the modules refuse: recorded, the others still run
            if "HIP error" in str(e) or "illegal memory" in str(e):
                raise
            res["runs"][setup] = {"setup": setup, "error": f"{type(e).__name__}: {str(e)[:400]}"}
        print(setup, json.dumps({k: v for k, v in res["runs"][setup].items()}, default=str)[:2000], flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
