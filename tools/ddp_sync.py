"""Time the data-parallel gradient exchange (cvvae_amd/ddp.py) on an MI355X, on the two optimizer lists of the sd3 engine
(AutoencodingEngineWithLatentConstraint at the shipped widths, fp32 gradients): the autoencoder's parameters and the discriminator's.

  1. `pack`: ops.mt_pack of a whole list into the slots of its bucket (ONE launch, 8 bytes per element) against `torch`, the sequence
     it replaces: torch._foreach_div into fresh tensors followed by the flatten, torch.cat (16 bytes per element, two or more
     launches).  Samples interleaved, median of 10 after 3 warm-ups; microseconds and GB/s of each path's own bytes.
  2. `iteration`: a whole generator and a whole discriminator iteration (training_step + on_train_batch_end, shape [1,3,17,256,256])
     of an engine under data_parallel() at world size 1 against an equal engine without it, sample by sample in one process, in the
     two set-ups of tools/train_iteration.py; that tool's figures from profiles/train_iteration.json (the parent commit's) are
     copied next to them.  Expected cost: one more sweep over the gradients.  Recorded, not gated.
  3. `allreduce`: the all-reduce of each bucket over RCCL, one process per device -- only when more than one GPU is visible;
     otherwise the record says so.

    timeout -k 10 900 python tools/ddp_sync.py                    # writes profiles/ddp_sync.json

--wide measures the fp32 bucket for 16-bit gradients (GradientSync(wide_gradients=True)) on the same two lists stored in bf16, and
writes profiles/ddp_sync_wide.json:

  a. `pack`: ops.mt_pack_wide at divisor 8 (ONE launch, 6 bytes per element) against the per-dtype torch path of sync() that it
     replaces, as sync() runs it without the keyword: torch.cat of the flattened gradients, div_, one copy_ per tensor on the way back
     (12 bytes per element, a launch per tensor and two more).  Condition: the kernel is not slower; the ratio is recorded.
  b. `adamw`: ops.mt_adamw_master_wide (fp32 gradient, 30 bytes per parameter) against ops.mt_adamw_master (bf16 gradient, 28) on the
     same list, each on its own copy of the state.  Condition: at most 30 / 28 times the box's +-3 % spread, 1.10.
  c. `allreduce`: the all-reduce of each bucket over RCCL in bf16 (2 bytes per parameter) and in fp32 (4) -- only when more than one
     GPU is visible; otherwise the record says that the figure is still unmeasured.

    timeout -k 10 300 python tools/ddp_sync.py --wide

There is no CPU path."""
import argparse
import copy
import datetime
import json
import os
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvvae_amd import _lib, ddp, ops  # noqa: E402
from lvdm.models.autoencoder import build_from_config  # noqa: E402
from tests import engine_cases as EC  # noqa: E402
from tools.train_iteration import SHAPE, SHIPPED, sample, stats  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
WORLD = 8.0      # the divisor of the pack measurement: the eight GPUs of a node


def interleaved(fns, warmup, iters):
    """median device-event microseconds of each callable, the callables taking turns"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "iters": iters} for k, v in ts.items()}


def pack_against_torch(shapes, warmup, iters):
    gen = torch.Generator("cuda").manual_seed(3)
    grads = [torch.randn(s, generator=gen, device="cuda") * 0.01 for s in shapes]
    numels = [g.numel() for g in grads]
    n = sum(numels)
    offsets, total = ddp.slot_layout(numels)
    flat = torch.zeros(total, device="cuda")
    slots = [flat[o:o + k] for o, k in zip(offsets, numels)]
    mtl = ops.MultiTensorList(numels, "cuda").set(g=grads, shadow=slots)

    def torch_sequence():
        return torch.cat([t.reshape(-1) for t in torch._foreach_div(grads, WORLD)])
    run = interleaved({"pack": lambda: ops.mt_pack(mtl, WORLD), "torch": torch_sequence}, warmup, iters)
    same = torch.equal(torch.cat([s for s in slots]), torch_sequence())
    for k, nbytes in (("pack", 8), ("torch", 16)):
        run[k].update(bytes_per_element=nbytes, gb_per_s=nbytes * n / (run[k]["median_us"] * 1e-6) / 1e9)
        run[k]["frac_of_hbm"] = run[k]["gb_per_s"] * 1e9 / HBM_BYTES_PER_S
    return {"elements": n, "tensors": len(shapes), "chunks": mtl.n_chunks, "bucket_elements": total, **run,
            "torch_over_pack": run["torch"]["median_us"] / run["pack"]["median_us"], "same_bits": same}


# ---- --wide: the fp32 bucket for 16-bit gradients ----
ADAMW = (4.0e-5, 0.9, 0.98, 1.0e-4, 0.01)      # lr, betas, eps, weight decay of the shipped YAML
ADAMW_WIDE_BOUND = 1.10                        # 30 / 28 bytes x the +-3 % spread of a box


def wide_pack_against_torch(shapes, warmup, iters, dtype=torch.bfloat16):
    gen = torch.Generator("cuda").manual_seed(3)
    grads = [(torch.randn(s, generator=gen, device="cuda") * 0.01).to(dtype) for s in shapes]
    theirs = [g.clone() for g in grads]        # the torch path writes its gradients in place
    numels = [g.numel() for g in grads]
    n = sum(numels)
    offsets, total = ddp.slot_layout(numels)
    flat = torch.zeros(total, device="cuda")
    slots = [flat[o:o + k] for o, k in zip(offsets, numels)]
    mtl = ops.MultiTensorList(numels, "cuda", dtype).set(g=grads, shadow=slots)

    def torch_sequence():                      # cvvae_amd/ddp.py sync(), the per-dtype path, the exchange itself left out
        cat = torch.cat([g.reshape(-1) for g in theirs])
        cat.div_(WORLD)
        for g, part in zip(theirs, cat.split(numels)):
            g.copy_(part.view(g.shape))
    run = interleaved({"pack_wide": lambda: ops.mt_pack_wide(mtl, WORLD), "torch": torch_sequence}, warmup, iters)
    same = torch.equal(torch.cat(slots), torch.div(torch.cat([g.reshape(-1) for g in grads]).float(), torch.tensor(WORLD, device="cuda")))
    for k, nbytes in (("pack_wide", 6), ("torch", 12)):
        run[k].update(bytes_per_element=nbytes, gb_per_s=nbytes * n / (run[k]["median_us"] * 1e-6) / 1e9)
        run[k]["frac_of_hbm"] = run[k]["gb_per_s"] * 1e9 / HBM_BYTES_PER_S
    run["torch"]["launches"] = len(shapes) + 2
    return {"elements": n, "tensors": len(shapes), "chunks": mtl.n_chunks, "bucket_elements": total, **run,
            "torch_over_pack_wide": run["torch"]["median_us"] / run["pack_wide"]["median_us"], "same_bits_as_fp32_division": same}


def wide_adamw_against_master(shapes, warmup, iters, dtype=torch.bfloat16):
    gen = torch.Generator("cuda").manual_seed(4)
    numels = [int(torch.Size(s).numel()) for s in shapes]
    n = sum(numels)
    lists = {}
    for name, gdtype in (("adamw_master_wide", torch.float32), ("adamw_master", dtype)):
        master = [torch.randn(s, generator=gen, device="cuda") for s in shapes]
        fields = dict(g=[(torch.randn(s, generator=gen, device="cuda") * 0.01).to(gdtype) for s in shapes], p=[w.to(dtype) for w in master],
                      m=[torch.zeros_like(w) for w in master], v=[torch.zeros_like(w) for w in master], shadow=master)
        lists[name] = ops.MultiTensorList(numels, "cuda", dtype).set(step_size=[ADAMW[0] / 0.1] * len(shapes), bias2_sqrt=[0.02 ** 0.5] * len(shapes),
                                                                     **fields)
    run = interleaved({"adamw_master_wide": lambda: ops.mt_adamw_master_wide(lists["adamw_master_wide"], *ADAMW),
                       "adamw_master": lambda: ops.mt_adamw_master(lists["adamw_master"], *ADAMW)}, warmup, iters)
    for k, nbytes in (("adamw_master_wide", 30), ("adamw_master", 28)):
        run[k].update(bytes_per_element=nbytes, gb_per_s=nbytes * n / (run[k]["median_us"] * 1e-6) / 1e9)
        run[k]["frac_of_hbm"] = run[k]["gb_per_s"] * 1e9 / HBM_BYTES_PER_S
    ratio = run["adamw_master_wide"]["median_us"] / run["adamw_master"]["median_us"]
    return {"elements": n, "tensors": len(shapes), **run, "wide_over_master": ratio, "expected_by_bytes": 30 / 28, "bound": ADAMW_WIDE_BOUND,
            "within_bound": ratio <= ADAMW_WIDE_BOUND}


def wide(shapes, a):
    res = {"what": "the fp32 bucket for 16-bit gradients (GradientSync(wide_gradients=True)) on the bf16 lists of "
                   "AutoencodingEngineWithLatentConstraint: the widening pack pass against the per-dtype torch path of sync() it replaces, "
                   "the master AdamW pass with an fp32 gradient against the one with a bf16 gradient, the all-reduce over RCCL in both widths",
           "device": torch.cuda.get_device_name(0), "kernel_sources": _lib.source_fingerprint(), "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "timing": "device events around each call, paths interleaved sample by sample in one process; median of "
                     f"{a.iters} after {a.warmup} warm-ups", "divisor": WORLD, "pack": {}, "adamw": {}}
    for name, sh in shapes.items():
        res["pack"][name] = wide_pack_against_torch(sh, a.warmup, a.iters)
        print("pack", name, json.dumps(res["pack"][name]), flush=True)
        torch.cuda.empty_cache()
        res["adamw"][name] = wide_adamw_against_master(sh, a.warmup, a.iters)
        print("adamw", name, json.dumps(res["adamw"][name]), flush=True)
        torch.cuda.empty_cache()
    res["pack_wide_not_slower_than_torch"] = all(v["pack_wide"]["median_us"] <= v["torch"]["median_us"] for v in res["pack"].values())
    res["adamw_wide_within_bound"] = all(v["within_bound"] for v in res["adamw"].values())
    totals = {k: ddp.slot_layout([int(torch.Size(s).numel()) for s in sh])[1] for k, sh in shapes.items()}
    sizes = {f"{k}:{w}": n for k, n in totals.items() for w in ("bf16", "fp32")}
    res["allreduce"] = allreduce(sizes)
    if isinstance(res["allreduce"], str):
        res["allreduce"] = "the RCCL figure (4 against 2 bytes per 16-bit parameter) is still unmeasured: " + res["allreduce"]
    return res


def iterations(cfg, setup, warmup, iters):
    torch.manual_seed(0)
    a = EC.seed_engine(build_from_config(copy.deepcopy(cfg))).train()
    b = copy.deepcopy(a)
    if setup == "bf16":
        a, b = EC.to_device(a, torch.bfloat16), EC.to_device(b, torch.bfloat16)
        x = torch.rand(SHAPE, device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
    else:
        a, b = a.cuda(), b.cuda()
        x = torch.rand(SHAPE, device="cuda").mul_(2).sub_(1)
    a.data_parallel()
    for e in (a, b):
        e.sample_generator = torch.Generator("cuda").manual_seed(1)
    batch = {a.input_key: x}

    def it(e, i):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=setup != "bf16"):
            e.training_step(batch, i)
        e.on_train_batch_end()
    paths = {"data_parallel": a, "plain": b}
    for _ in range(warmup):
        for e in paths.values():
            it(e, 0)
            it(e, 1)
    torch.cuda.synchronize()
    rows = {(p, k): [] for p in paths for k in ("generator", "discriminator")}
    for _ in range(iters):
        for p, e in paths.items():
            rows[(p, "generator")].append(sample(lambda: it(e, 0)))
            rows[(p, "discriminator")].append(sample(lambda: it(e, 1)))
    out = {"setup": setup, "pack_path": "torch (bf16 gradients; the fp32 logvars on the kernel)" if setup == "bf16" else "kernel"}
    for kind in ("generator", "discriminator"):
        d, p = stats(rows[("data_parallel", kind)]), stats(rows[("plain", kind)])
        out[kind] = {"data_parallel": d, "plain": p, "data_parallel_over_plain_median": d["median_ms"] / p["median_ms"],
                     "extra_ms_median": d["median_ms"] - p["median_ms"]}
    return out


def parent_figures():
    path = os.path.join(ROOT, "profiles", "train_iteration.json")
    if not os.path.isfile(path):
        return "profiles/train_iteration.json is missing"
    with open(path) as f:
        rec = json.load(f)
    return {"kernel_sources": rec.get("kernel_sources"),
            "runs": {s: {k: r[k]["engine"]["median_ms"] for k in ("generator", "discriminator") if k in r} for s, r in rec.get("runs", {}).items()}}


# ---- 3. the all-reduce over RCCL: one process per device ----
def allreduce_child(a):
    torch.cuda.set_device(a.rank)
    import torch.distributed as dist
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{a.port}", rank=a.rank, world_size=a.world,
                            timeout=datetime.timedelta(seconds=120))
    try:
        out = {}
        for name, n in json.loads(a.sizes).items():
            dtype = torch.bfloat16 if name.endswith(":bf16") else torch.float32      # (--wide names its buffers "<list>:<width>")
            t = torch.ones(n, device="cuda", dtype=dtype)
            run = interleaved({"allreduce": lambda: dist.all_reduce(t)}, 3, 10)["allreduce"]
            # a ring moves 2 (world - 1) / world of the buffer in and out of every device
            run["bus_gb_per_s"] = 2 * (a.world - 1) / a.world * t.element_size() * n / (run["median_us"] * 1e-6) / 1e9
            out[name] = run
        if a.rank == 0:
            with open(a.out, "w") as f:
                json.dump(out, f)
    finally:
        dist.destroy_process_group()


def allreduce(sizes):
    world = torch.cuda.device_count()
    if world < 2:
        return "not measured: one GPU visible"
    from tests.ddp_ref import free_port
    port = free_port()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "allreduce.json")
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--allreduce-rank", str(r), "--world", str(world),
                                   "--port", str(port), "--sizes", json.dumps(sizes), "--out", out]) for r in range(world)]
        try:
            codes = [p.wait(timeout=300) for p in procs]
        except subprocess.TimeoutExpired:
            codes = None
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                p.wait()
        if codes is None or any(codes) or not os.path.isfile(out):
            return f"not measured: the {world} RCCL processes ended with {codes}"
        with open(out) as f:
            return {"world": world, "backend": "nccl (RCCL)", "buckets": json.load(f)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--setups", default="bf16,fp32_autocast")
    ap.add_argument("--wide", action="store_true", help="measure the fp32 bucket for 16-bit gradients instead")
    ap.add_argument("--out", default=None, help="default: profiles/ddp_sync.json, with --wide profiles/ddp_sync_wide.json")
    ap.add_argument("--allreduce-rank", dest="rank", type=int, default=None)
    ap.add_argument("--world", type=int, default=0)
    ap.add_argument("--port", type=int, default=0)
    ap.add_argument("--sizes", default="{}")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ddp_sync.py measures on an MI355X; no GPU found (there is no CPU path)")
    if a.rank is not None:
        return allreduce_child(a)
    torch.cuda.set_device(0)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "ddp_sync_wide.json" if a.wide else "ddp_sync.json")
    cfg = EC.latent_config(SHIPPED, target_type="random")
    res = {"what": "the data-parallel gradient exchange of AutoencodingEngineWithLatentConstraint: the pack pass against the torch "
                   "sequence it replaces, whole iterations with data_parallel() at world size 1, the all-reduce over RCCL",
           "device": torch.cuda.get_device_name(0), "kernel_sources": _lib.source_fingerprint(), "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "timing": "device events around each call, paths interleaved sample by sample in one process; median of "
                     f"{a.iters} after {a.warmup} warm-ups", "divisor": WORLD, "pack": {}, "iteration": {}}
    engine = build_from_config(copy.deepcopy(cfg))
    lists = {"autoencoder": engine.get_autoencoder_params(), "discriminator": engine.get_discriminator_params()}
    shapes = {k: [tuple(p.shape) for p in v] for k, v in lists.items()}
    del engine, lists
    if a.wide:
        res = wide(shapes, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    for name, sh in shapes.items():
        res["pack"][name] = pack_against_torch(sh, a.warmup, a.iters)
        print("pack", name, json.dumps(res["pack"][name]), flush=True)
        torch.cuda.empty_cache()
    res["pack_not_slower_than_torch"] = all(v["pack"]["median_us"] <= v["torch"]["median_us"] for v in res["pack"].values())
    for setup in a.setups.split(","):
        res["iteration"][setup] = iterations(cfg, setup, 2, a.iters)
        print("iteration", setup, json.dumps(res["iteration"][setup]), flush=True)
        torch.cuda.empty_cache()
    res["iteration_parent_commit"] = {"from": "profiles/train_iteration.json (tools/train_iteration.py, `engine` path, median ms)",
                                      "figures": parent_figures()}
    res["allreduce"] = allreduce({k: ddp.slot_layout([int(torch.Size(s).numel()) for s in sh])[1] for k, sh in shapes.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
