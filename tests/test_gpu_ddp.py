"""Data-parallel training on a real MI355X (cvvae_amd/ddp.py, csrc/optim_kernels.hip cvvae_mt_pack).

a. the pack pass at every edge of the chunk geometry in ONE launch per divisor, bit for bit against torch.div on the device;
b. world size 1 (a one-rank gloo group): four iterations of an engine under data_parallel() equal an engine without it bit for bit;
c. two ranks drive the real kernels on ONE card (two fresh child processes, gloo, transport "host"): each rank's synchronised
   gradient is g_0 / 2 + g_1 / 2 bit for bit, and after four iterations the replicas' states are bit-equal;
d. the same worker over RCCL, one device per rank (needs two GPUs).

The kernels are deterministic and the exchange of two ranks is one commutative addition, so every comparison here is an equality."""
import argparse
import copy
import datetime
import os
import subprocess
import sys
import time

import pytest
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.seeded import seeded_input  # noqa: E402
from tests import ddp_ref, optim_ref  # noqa: E402
from tests import engine_cases as EC  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (1, 3, 5, 32, 32)
INDICES = [0, 2]
SENTINEL = 7.25
CHILD_LIMIT = 180.0


# ---- a. the pack pass ----
@pytest.fixture(scope="module")
def edge_case():
    """optim_ref.edge_list with the gradients replaced by ddp_ref.special_values; destinations laid out as GradientSync lays its
    slots, each followed by GUARD elements, in one buffer filled with a sentinel"""
    from cvvae_amd import ddp
    entries = optim_ref.edge_list(3)
    gen = torch.Generator().manual_seed(11)
    srcs = []
    for d in entries:
        buf = ddp_ref.special_values(d["off"] + d["n"] + optim_ref.GUARD, gen).cuda()
        view = buf[d["off"]:d["off"] + d["n"]].view(() if d["n"] == 1 else (d["n"],))
        srcs.append((buf, view if d["has_grad"] else None))
    numels = [d["n"] for d in entries]
    offsets, total = ddp.slot_layout([n + optim_ref.GUARD for n in numels])
    assert any(d["off"] == 1 for d in entries) and any(not d["has_grad"] for d in entries)
    return entries, srcs, numels, offsets, total


@pytest.mark.parametrize("divisor", [1, 2, 3, 8])
def test_pack_at_its_edges_in_one_launch(edge_case, divisor):
    from cvvae_amd import ops
    entries, srcs, numels, offsets, total = edge_case
    flat = torch.full((total,), SENTINEL, dtype=torch.float32, device="cuda")
    dsts = [flat[o:o + n] for o, n in zip(offsets, numels)]
    assert all(d.data_ptr() % 16 == 0 for d in dsts)
    assert sum(s[1] is not None and s[1].data_ptr() % 16 == 4 for s in srcs) == 1        # the source 4 bytes into its buffer
    before = [b.clone() for b, _ in srcs]
    mtl = ops.MultiTensorList(numels, "cuda").set(g=[g for _, g in srcs], shadow=dsts)
    ops.mt_pack(mtl, float(divisor))
    torch.cuda.synchronize()
    touched = torch.zeros(total, dtype=torch.bool, device="cuda")
    for (buf, g), dst, o, n in zip(srcs, dsts, offsets, numels):
        touched[o:o + n] = True
        if g is None:
            assert n > 0 and float(dst.abs().max()) == 0.0 and not bool(torch.signbit(dst).any())     # the None slot: all +0
            continue
        # torch.div on the device with the divisor as a 0-dim DEVICE tensor: a Python scalar would make torch multiply by its
        # reciprocal (measured here: the pack differs from torch.div(g, 3.0) in the last bit and equals the two below) ...
        want = torch.div(g.reshape(-1), torch.tensor(float(divisor), device="cuda"))
        assert ddp_ref.same_bits_or_both_nan(dst, want), (n, divisor)
        # ... and the host's division, which is the C++ operator
        assert ddp_ref.same_bits_or_both_nan(dst, torch.div(g.reshape(-1).cpu(), torch.tensor(float(divisor)))), (n, divisor)
        if divisor == 1 and n:
            assert ddp_ref.same_bits_or_both_nan(dst, g.reshape(-1))
    # the guards behind every destination and the alignment gaps: the sentinel, untouched; the sources: unchanged
    assert bool((flat[~touched] == SENTINEL).all())
    assert all(ddp_ref.same_bits_or_both_nan(b, c) for (b, _), c in zip(srcs, before))
    if divisor == 3:     # the case that tells a division from a product with the reciprocal
        g = torch.cat([g.reshape(-1) for _, g in srcs if g is not None])
        fin = torch.isfinite(g)
        three = torch.tensor(3.0, device="cuda")
        assert not torch.equal((g / three)[fin], (g * (1.0 / three))[fin])


def test_pack_refuses_what_it_has_no_kernel_for():
    from cvvae_amd import ops
    t = torch.zeros(8, device="cuda")
    mtl = ops.MultiTensorList([8], "cuda").set(g=[t], shadow=[t.clone()])
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.mt_pack(mtl, bad)
    with pytest.raises(ValueError):
        ops.mt_pack(ops.MultiTensorList([8], "cuda").set(g=[t]), 2.0)            # no destination was ever set
    empty = ops.MultiTensorList([0, 0], "cuda").set(g=[None, t[:0]], shadow=[t[:0], t[:0]])
    assert empty.n_chunks == 0
    ops.mt_pack(empty, 2.0)                                                       # n_chunks = 0 is allowed
    torch.cuda.synchronize()


# ---- b. world size 1 ----
@pytest.fixture(scope="module")
def one_rank_group():
    made = not dist.is_initialized()
    if made:
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{ddp_ref.free_port()}", rank=0, world_size=1,
                                timeout=datetime.timedelta(seconds=60))
        group = dist.group.WORLD
    else:
        group = dist.new_group([dist.get_rank()], backend="gloo")
    try:
        yield group
    finally:
        if made:
            dist.destroy_process_group()


_BUILT = {}


def _engine(kind, dtype, device="cuda"):
    if kind not in _BUILT:
        _BUILT[kind] = EC.build(kind, True, ema_decay=0.999)
    e = EC.to_device(copy.deepcopy(_BUILT[kind]), dtype, device)
    e.sample_generator, e.frame_indices = torch.Generator(device).manual_seed(5), INDICES
    return e


def _differences(a, b):
    sa, sb = ddp_ref.engine_state(a), ddp_ref.engine_state(b)
    assert sorted(sa) == sorted(sb)
    return [k for k in sa if sa[k].dtype != sb[k].dtype or sa[k].shape != sb[k].shape or not torch.equal(sa[k], sb[k])]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["latent", "all"])
def test_world_size_one_equals_the_engine_without_it_bit_for_bit(one_rank_group, kind, dtype):
    a, b = _engine(kind, dtype), _engine(kind, dtype)
    assert a.data_parallel(one_rank_group) is a
    x = seeded_input(SHAPE, 12).to(dtype).cuda()
    for it in range(4):
        la, lb = a.training_step({"frames": x}, it), b.training_step({"frames": x}, it)
        a.on_train_batch_end()
        b.on_train_batch_end()
        assert torch.equal(la, lb) and bool(torch.isfinite(la)), (it, float(la), float(lb))
        assert sorted(a.last_logs) == sorted(b.last_logs)
        diff = [k for k in a.last_logs if not torch.equal(a.last_logs[k], b.last_logs[k])]
        assert not diff, (it, diff)
        bad = _differences(a, b)
        assert not bad, (it, len(bad), bad[:8])
        opt = a.optimizers()[it % 2]
        assert torch.equal(opt.last_grad_norm, b.optimizers()[it % 2].last_grad_norm)
        # after sync() every gradient the kernel took lies in its slot; a gradient of another dtype stays where backward put it
        sync = a.gradient_sync(opt)
        assert sync.calls == it // 2 + 1 and sync.world == 1 and sync.transport == "host"
        n_slot = 0
        for p, o, n in zip(sync.params, sync.layout(), sync.numels):
            if p.grad is None:
                continue
            if p.dtype == torch.float32:
                assert p.grad.data_ptr() == sync.flat.data_ptr() + 4 * o and p.grad.is_contiguous() and p.grad.shape == p.shape
                n_slot += 1
            else:
                assert n == 0 and p.grad.dtype == dtype
        # fp32: every gradient sits in the bucket; bf16 networks: the loss's fp32 logvars do (generator iterations), the rest not
        assert n_slot > 10 if dtype == torch.float32 else n_slot == sum(p.dtype == torch.float32 and p.grad is not None for p in sync.params)
        assert (sync.flat is not None) == (n_slot > 0)
        if dtype == torch.bfloat16 and it % 2 == 0:
            assert n_slot >= 1
    if dtype == torch.bfloat16:
        # the method of test_training_step_does_not_synchronise_the_host: two more iterations under torch's synchronisation check
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for it in range(4, 6):
                loss = a.training_step({"frames": x}, it)
                a.on_train_batch_end()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert a.global_step == 6 and bool(torch.isfinite(loss))


# ---- c / d. two ranks: the worker (a fresh process per rank) and its parents ----
def _child(args):
    torch.set_num_threads(4)
    dist.init_process_group(args.backend, init_method=f"tcp://127.0.0.1:{args.port}", rank=args.rank, world_size=args.world,
                            timeout=datetime.timedelta(seconds=60))
    try:
        device = f"cuda:{args.rank if args.backend == 'nccl' else 0}"
        torch.cuda.set_device(device)
        xs = [seeded_input(SHAPE, 30 + r).to(device) for r in range(args.world)]
        per_rank = []
        for r in range(args.world):       # unsynchronised copies, run here: every rank's own gradient of the first iteration
            e = _engine("latent", torch.float32, device)
            e.training_step({"frames": xs[r]}, 0)
            per_rank.append([None if p.grad is None else p.grad.detach().cpu() for g in e.optimizers()[0].param_groups for p in g["params"]])
            del e
        want = ddp_ref.mean_in_rank_order(per_rank)          # g_0 / 2 + g_1 / 2 on the host in fp32 -- not (g_0 + g_1) / 2
        e = _engine("latent", torch.float32, device)
        e.data_parallel(transport=args.transport)
        losses = []
        for it in range(4):
            losses.append(float(e.training_step({"frames": xs[args.rank]}, it)))
            if it == 0:
                sync = e.gradient_sync(e.optimizers()[0])
                assert sync.world == args.world and sync.transport == args.transport and sync.flat.is_cuda
                got = [p.grad for p in sync.params]
                assert [g is None for g in got] == [w is None for w in want]
                bad = [i for i, (g, w) in enumerate(zip(got, want)) if w is not None and not torch.equal(g.cpu(), w)]
                assert not bad, f"rank {args.rank}: {len(bad)} synchronised gradients differ from g_0/2 + g_1/2, first {bad[:5]}"
                assert all(g.data_ptr() == sync.flat.data_ptr() + 4 * o for g, o in zip(got, sync.layout()) if g is not None)
            e.on_train_batch_end()
        torch.save({"state": {k: v.detach().cpu() for k, v in ddp_ref.engine_state(e).items()}, "losses": losses}, args.out)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    print(f"DDP-CHILD rank {args.rank} done: losses {losses}")
    return 0


def _two_ranks(tmp_path, backend, transport):
    port = ddp_ref.free_port()
    outs = [str(tmp_path / f"rank{r}.pt") for r in range(2)]
    logs = [open(str(tmp_path / f"rank{r}.log"), "w+") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), "--world", "2", "--port", str(port),
                               "--backend", backend, "--transport", transport, "--out", outs[r]],
                              cwd=ROOT, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(2)]
    deadline = time.monotonic() + CHILD_LIMIT
    failed = None
    try:
        while any(p.poll() is None for p in procs) and failed is None:
            if time.monotonic() > deadline:
                failed = f"no exit within {CHILD_LIMIT:.0f} s"
            elif any(p.poll() not in (None, 0) for p in procs):
                failed = f"exit codes {[p.poll() for p in procs]}"
            else:
                time.sleep(0.05)
        if failed is None and any(p.returncode != 0 for p in procs):
            failed = f"exit codes {[p.returncode for p in procs]}"
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
        text = []
        for f in logs:
            f.seek(0)
            text.append(f.read())
            f.close()
    print("\n".join(text))
    assert failed is None, failed + "\n" + "\n".join(t[-3000:] for t in text)
    a, b = (torch.load(o) for o in outs)
    assert sorted(a["state"]) == sorted(b["state"])
    diff = [k for k in a["state"] if not torch.equal(a["state"][k], b["state"][k])]
    assert not diff, (len(diff), diff[:8])
    assert any(k.startswith("opt1:") for k in a["state"]) and any(k.startswith("ema:") for k in a["state"])
    assert a["losses"][0] != b["losses"][0], "the two ranks saw the same data"


def test_two_ranks_on_one_card_over_gloo(tmp_path):
    _two_ranks(tmp_path, "gloo", "host")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_ranks_over_rccl(tmp_path):
    _two_ranks(tmp_path, "nccl", "device")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--backend", required=True)
    ap.add_argument("--transport", required=True)
    ap.add_argument("--out", required=True)
    sys.exit(_child(ap.parse_args()))
