"""Data-parallel training on the CPU (cvvae_amd/ddp.py, AbstractAutoencoder.data_parallel): the bucket layout as pure host code, and
two and three `gloo` ranks (spawned, as tests/test_dist_gloo.py does) running a small engine on the emulated kernels
(tests/test_train_engine_host_logic.py `emulated` plus tests/ddp_ref.py's pack pass), a different seeded batch per rank.

What is compared bit for bit has no tolerance.  The one band is for three ranks: the worker probes the exchange with a seeded
log-uniform vector of the bucket's length and demands equality with sum_r(g_r / world) when the probe comes out as the rank-order
sum, else |got - want| <= 1 ulp at the magnitude sum_r |g_r / world|; it reports which of the two applied.  The "host" transport adds
in rank order by construction (cvvae_amd/ddp.py _sum_in_rank_order), so equality applies; gloo's own ring all-reduce, which adds each
chunk in another rotation of the ranks, measured 2.0 of those ulps on these gradients and would miss the band."""
import copy
import datetime
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import ddp_ref

SHAPE = (1, 3, 5, 16, 16)
INDICES = [0, 2, 3]
JOIN_LIMIT = 240.0


# ---- layout: pure host code ----
def test_slots_are_aligned_disjoint_and_in_list_order():
    from cvvae_amd import ddp
    numels = [5, 0, 1, 8, 8191, 4, 3, 0]
    offsets, total = ddp.slot_layout(numels)
    assert len(offsets) == len(numels) and all(o % 4 == 0 for o in offsets) and total % 4 == 0
    assert offsets == sorted(offsets) and offsets[0] == 0
    for (o, n), nxt in zip(zip(offsets, numels), offsets[1:] + [total]):
        assert o + n <= nxt and nxt - (o + n) < 4          # disjoint, and a gap is only what alignment asks for
    assert offsets[1] == offsets[2] == 8                   # an empty tensor gets an empty slot
    params = [torch.nn.Parameter(torch.zeros(n)) for n in numels] + [torch.nn.Parameter(torch.zeros(6, dtype=torch.bfloat16))]
    sync = ddp.GradientSync(params)
    assert sync.layout() == offsets + [total] and sync.total == total and sync.numels[-1] == 0   # a bf16 parameter: an empty slot
    assert sync.world == 1 and sync.ranges == [(0, total)]
    with pytest.raises(ValueError):
        ddp.GradientSync(params + params[:1])
    with pytest.raises(ValueError):
        ddp.GradientSync(params, transport="carrier pigeon")


def test_bucket_ranges_cut_at_slot_starts_only():
    from cvvae_amd import ddp
    numels = [100, 100, 1000, 4, 4, 4]
    offsets, total = ddp.slot_layout(numels)
    assert ddp.bucket_ranges(offsets, total, None) == [(0, total)]
    assert ddp.bucket_ranges([], 0, 64) == []
    for nbytes in (1, 16, 800, 801, 4000, 4 * total, 1 << 30):
        r = ddp.bucket_ranges(offsets, total, nbytes)
        assert r[0][0] == 0 and r[-1][1] == total and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(a < b for a, b in r)
        assert all(a in offsets for a, _ in r)
        # a range exceeds the limit only when it is a single slot
        assert all((b - a) * 4 <= nbytes or sum(a <= o < b for o in offsets) == 1 for a, b in r)
    assert ddp.bucket_ranges(offsets, total, 800) == [(0, 200), (200, 1200), (1200, 1212)]
    with pytest.raises(ValueError):
        ddp.bucket_ranges(offsets, total, 0)


def test_pack_entry_point_contract():
    """the checks cvvae_mt_pack makes before it launches (no GPU is touched), and the None a list's field may hold"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    lib = L.load()
    p = 64     # any non-null table address: every call below returns before a launch
    assert "cvvae_mt_pack" in L.PROTOTYPES
    for dt in (L.F16, L.BF16, L.F32Q):
        assert lib.cvvae_mt_pack(dt, p, p, 1, 2.0, None) == -2
    assert lib.cvvae_mt_pack(L.F32, None, None, 0, 2.0, None) == 0          # n_chunks = 0 is allowed
    assert lib.cvvae_mt_pack(L.F32, None, p, 1, 2.0, None) == -1
    assert lib.cvvae_mt_pack(L.F32, p, p, 1 << 40, 2.0, None) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.cvvae_mt_pack(L.F32, p, p, 1, bad, None) == -1
    t = torch.zeros(5)
    mtl = ops.MultiTensorList([5, 3], "cpu").set(g=[t, None], shadow=[t, t[:3]])
    assert mtl._image[0, 0] == t.data_ptr() and mtl._image[1, 0] == 0 and mtl._image[1, 4] == t.data_ptr()
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mt_pack(mtl, 2.0)                                                # CPU tensors: no fallback


def test_world_size_one_packs_and_views_without_a_process_group(monkeypatch):
    """no torch.distributed at all: sync() still packs into the slots and hands out the views; None keeps None; the guard gaps stay 0"""
    from cvvae_amd import ddp
    count = {}
    ddp_ref.pretend_gpu(monkeypatch, count)
    gen = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in ((3, 5), (7,), (), (2, 2))]
    grads = [torch.randn(p.shape, generator=gen) for p in params]
    for p, g in zip(params[:3], grads):
        p.grad = g.clone()
    sync = ddp.GradientSync(params)
    sync.sync()
    assert count == {"mt_pack": 1} and sync._mtl.tensors.get("g") is None
    for p, g, o, n in zip(params, grads, sync.layout(), sync.numels):
        if p is params[3]:
            assert p.grad is None
            continue
        assert torch.equal(p.grad, g) and p.grad.is_contiguous() and p.grad.shape == p.shape
        assert p.grad.data_ptr() == sync.flat.data_ptr() + 4 * o
    used = torch.zeros(sync.total, dtype=torch.bool)
    for o, n in zip(sync.layout(), sync.numels[:3]):
        used[o:o + n] = True
    assert float(sync.flat[~used].abs().max()) == 0.0
    # set_to_none=False: the gradient IS the slot; the pack runs in place
    params[0].grad.mul_(2.0)
    sync.sync()
    assert torch.equal(params[0].grad, 2.0 * grads[0]) and params[0].grad.data_ptr() == sync.flat.data_ptr()


# ---- spawned ranks ----
def _engine_worker_context():
    from tests.test_train_engine_host_logic import emulated
    return emulated()


def _build(kind="latent"):
    from tests import engine_cases as EC
    return EC.build(kind, False, ema_decay=0.999)


def _seed(e):
    e.sample_generator, e.frame_indices = torch.Generator().manual_seed(5), INDICES
    return e


def _opt_params(e, i):
    return [p for g in e.optimizers()[i].param_groups for p in g["params"]]


def _mode_train(rank, world):
    from oracle.seeded import seeded_input
    from tests import optim_ref
    xs = [seeded_input(SHAPE, 30 + r) for r in range(world)]
    with _engine_worker_context(), pytest.MonkeyPatch.context() as mpatch:
        ddp_ref.pretend_gpu(mpatch)
        base = _build()
        per_rank = []
        for r in range(world):          # unsynchronised copies: every rank's own gradient of the first iteration
            e = _seed(copy.deepcopy(base))
            e.training_step({"frames": xs[r]}, 0)
            per_rank.append([None if p.grad is None else p.grad.detach().clone() for p in _opt_params(e, 0)])
        want = ddp_ref.mean_in_rank_order(per_rank)
        scale = ddp_ref.magnitude(per_rank)
        e = _seed(copy.deepcopy(base))
        if rank:                        # a replica that starts elsewhere: data_parallel() must bring it to rank 0's state
            with torch.no_grad():
                for t in list(e.parameters()) + [b for b in e.model_ema.buffers() if b.is_floating_point()]:
                    t.add_(0.25 * rank)
                e.model_ema.num_updates += 3 * rank
        e.data_parallel()
        state0 = ddp_ref.digest({"p:" + n: p for n, p in e.named_parameters()})
        same_start = state0 == ddp_ref.digest({"p:" + n: p for n, p in base.named_parameters()})
        losses, report = [], {}
        for it in range(4):
            losses.append(float(e.training_step({"frames": xs[rank]}, it)))
            if it == 0:
                sync = e.gradient_sync(e.optimizers()[0])
                # (log-uniform magnitudes: sums of values on one binary grid would be exact in every order)
                probe = [optim_ref.log_uniform((sync.total,), torch.Generator().manual_seed(70 + r)) for r in range(world)]
                mine = probe[rank].clone()
                sync._exchange(mine, sync.ranges)      # the exchange the gradients went through
                in_order = probe[0].clone()
                for t in probe[1:]:
                    in_order = in_order + t
                report["rank_order"] = bool(torch.equal(mine, in_order))
                got = [p.grad for p in _opt_params(e, 0)]
                assert [g is None for g in got] == [w is None for w in want]
                exact = all(torch.equal(g, w) for g, w in zip(got, want) if w is not None)
                report["exact"] = exact
                worst = max(float(((g.double() - w.double()).abs() / optim_ref.ulp32(s.double())).max())
                            for g, w, s in zip(got, want, scale) if w is not None and w.numel())
                report["worst_ulp"] = worst
                if report["rank_order"] or world == 2:
                    assert exact, f"the synchronised gradient is not sum_r(g_r / world) in rank order (worst {worst} ulp)"
                else:
                    assert worst <= 1.0, worst
                flat = sync.flat
                assert all(g.data_ptr() == flat.data_ptr() + 4 * o for g, o in zip(got, sync.layout()) if g is not None)
                report["norm"] = float(e.optimizers()[0].last_grad_norm)
            e.on_train_batch_end()
        return {"losses": losses, "state": ddp_ref.digest(ddp_ref.engine_state(e)), "same_start": same_start, "report": report,
                "calls": [s.calls for s in e._dp["syncs"].values()]}


def _mode_disagree(rank, world):
    from cvvae_amd import ddp
    gen = torch.Generator().manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen)) for n in (5, 9, 2, 7)]
    for p in params:
        p.grad = torch.ones_like(p)
    if rank == 1:
        params[2].grad = None
    ddp.GradientSync(params).sync()
    return "no error"


def _mode_plain(rank, world):
    """the torch path (CPU tensors as they are: fp32, bf16 and a non-contiguous gradient) and the kernel path over several ranges"""
    from cvvae_amd import ddp
    gen = torch.Generator().manual_seed(2)
    shapes = [(5,), (300,), (4, 6), (1000,), ()]
    mk = lambda r: [torch.randn(s, generator=torch.Generator().manual_seed(100 * r + i)) for i, s in enumerate(shapes)]  # noqa: E731
    per_rank = [mk(r) for r in range(world)]
    out = {}
    # torch path
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes] + [torch.nn.Parameter(torch.zeros(6, dtype=torch.bfloat16))]
    for p, g in zip(params, per_rank[rank]):
        p.grad = g.clone()
    params[2].grad = per_rank[rank][2].t().contiguous().t()          # same values, other strides
    params[5].grad = torch.full((6,), float(rank + 1), dtype=torch.bfloat16)
    sync = ddp.GradientSync(params, check_first=1)
    sync.sync()
    want = ddp_ref.mean_in_rank_order(per_rank)
    out["torch_path"] = all(torch.equal(p.grad, w) for p, w in zip(params, want)) and sync.flat is None
    out["bf16"] = params[5].grad.tolist() == [sum((r + 1) / world for r in range(world))] * 6 if world == 2 else True
    # kernel path, emulated, three ranges
    with pytest.MonkeyPatch.context() as mpatch:
        ddp_ref.pretend_gpu(mpatch)
        params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
        for p, g in zip(params, per_rank[rank]):
            p.grad = g.clone()
        params[1].grad = None if rank == 0 else params[1].grad       # ... and one rank-dependent hole, past the checked calls
        sync = ddp.GradientSync(params, bucket_bytes=1300, check_first=0)
        sync.sync()
        per_rank[0][1] = None
        want = ddp_ref.mean_in_rank_order(per_rank)
        out["ranges"] = len(sync.ranges)
        out["kernel_path"] = all(torch.equal(p.grad, w) for p, w in zip(params, want) if p.grad is not None)
        out["hole"] = (params[1].grad is None) == (rank == 0)
    return out


def _mode_validate(rank, world):
    from oracle.seeded import seeded_input
    from cvvae_amd import ops
    from cvvae_amd.metrics import ReconstructionMeter
    from tests import metrics_ref
    xs = [seeded_input(SHAPE, 30 + r) for r in range(world)]
    with _engine_worker_context(), pytest.MonkeyPatch.context() as mpatch:
        ddp_ref.pretend_gpu(mpatch)

        def fake(a, b, quantize=True, want_ssim=True):
            sse, psnr, ssim = metrics_ref.frame_metrics(a, b, quantize, want_ssim)
            return sse, psnr, (ssim.float() if want_ssim else None)
        mpatch.setattr(ops, "frame_metrics", fake)
        base = _build()
        single = []
        for r in range(world):
            e = _seed(copy.deepcopy(base))
            single.append(e.validation_step({"frames": xs[r]}, 0))
        e = _seed(copy.deepcopy(base)).data_parallel()
        got = e.validation_step({"frames": xs[rank]}, 0)
        assert sorted(got) == sorted(single[0]) and all(e.last_logs[k] is got[k] for k in got)
        bad = []
        for k in got:
            acc = single[0][k].float()
            for s in single[1:]:
                acc = acc + s[k].float()
            want = (acc / world).to(single[0][k].dtype)
            ok = torch.equal(got[k], want) if world == 2 else abs(float(got[k]) - float(want)) <= 2.4e-7 * abs(float(want))
            if not ok:
                bad.append((k, float(got[k]), float(want)))
        differ = any(float(single[0][k]) != float(single[1][k]) for k in got)
        # the meter: every rank scores its own pair of clips; compute(group) is the pooled figure on every rank
        pairs = []
        for r in range(world):
            g = torch.Generator().manual_seed(200 + r)
            a = torch.randint(0, 256, (2 + r, 12, 13, 3), generator=g, dtype=torch.uint8)
            b = (a.int() + torch.randint(-9, 10, a.shape, generator=g)).clamp(0, 255).to(torch.uint8)
            b[0] = a[0]
            pairs.append((a, b))
        pooled = ReconstructionMeter()
        for a, b in pairs:
            pooled.update(a, b)
        mine = ReconstructionMeter()
        mine.update(*pairs[rank])
        local = mine.compute()
        return {"bad": bad, "differ": differ, "meter": mine.compute(dist.group.WORLD), "pooled": pooled.compute(), "local": local,
                "local_again": mine.compute()}


MODES = {"train": _mode_train, "disagree": _mode_disagree, "plain": _mode_plain, "validate": _mode_validate}


def _worker(rank, world, port, mode, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        q.put((rank, "ok", MODES[mode](rank, world)))
    except BaseException as err:  # noqa: BLE001 -- the parent judges it
        q.put((rank, type(err).__name__, str(err)))
    finally:
        dist.destroy_process_group()


def _run(world, mode):
    """-> {rank: (status, payload)}; the parent waits with a limit and terminates what is left when a rank is missing"""
    import queue
    import time
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = ddp_ref.free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, mode, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, deadline = {}, time.monotonic() + JOIN_LIMIT
    try:
        while len(res) < world:
            try:
                rank, status, payload = q.get(timeout=max(deadline - time.monotonic(), 0.01))
            except queue.Empty:
                break
            res[rank] = (status, payload)
        for p in procs:
            p.join(timeout=max(deadline - time.monotonic(), 0.01) if len(res) == world else 0.01)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    assert len(res) == world, f"ranks {sorted(set(range(world)) - set(res))} did not report within {JOIN_LIMIT:.0f} s"
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_engine_replicas_average_their_gradients_and_stay_bit_equal(world):
    res = _run(world, "train")
    assert all(s == "ok" for s, _ in res.values()), res
    out = [res[r][1] for r in range(world)]
    for r, o in enumerate(out):
        print(f"\n[ddp host] world {world} rank {r}: gloo adds in rank order: {o['report']['rank_order']}; gradients bit-equal to the "
              f"rank-order sum: {o['report']['exact']}; worst ulp {o['report'].get('worst_ulp', 0.0)}; norm {o['report']['norm']:.6e}")
        assert o["same_start"], "data_parallel() did not bring the replica to rank 0's state"
        assert o["calls"] == [2, 2]
    # parameters, optimizer state and EMA buffers after four iterations: bit-equal across the ranks
    for r in range(1, world):
        diff = [k for k in out[0]["state"] if out[0]["state"][k] != out[r]["state"].get(k)]
        assert sorted(out[0]["state"]) == sorted(out[r]["state"]) and not diff, (r, len(diff), diff[:6])
    assert any(k.startswith("opt1:") for k in out[0]["state"]) and any(k.startswith("ema:") for k in out[0]["state"])
    assert len({o["report"]["norm"] for o in out}) == 1           # last_grad_norm: the averaged gradient's, the same everywhere
    assert len({o["losses"][0] for o in out}) == world, "the ranks saw the same data"


def test_ranks_that_disagree_about_a_gradient_all_raise():
    res = _run(2, "disagree")
    for r in range(2):
        status, msg = res[r]
        assert status == "RuntimeError" and "parameter 2" in msg and "rank 1: no gradient" in msg, (r, status, msg)


@pytest.mark.parametrize("world", [2, 3])
def test_torch_path_and_bucket_ranges(world):
    res = _run(world, "plain")
    assert all(s == "ok" for s, _ in res.values()), res
    for r in range(world):
        o = res[r][1]
        assert o["ranges"] == 4 and o["hole"], o       # [0, 308), [308, 332), the 1000-element slot alone, the last slot
        assert o["torch_path"] and o["bf16"] and o["kernel_path"], (r, o)     # the host transport adds in rank order


def test_validation_logs_and_the_meter_are_pooled_over_the_ranks():
    res = _run(2, "validate")
    assert all(s == "ok" for s, _ in res.values()), res
    for r in range(2):
        o = res[r][1]
        assert not o["bad"], o["bad"][:4]
        assert o["differ"]
        assert o["meter"]["frames"] == o["pooled"]["frames"] == 5 and o["meter"]["identical_frames"] == 2
        assert o["local"]["frames"] == 2 + r and o["local_again"] == o["local"]        # the meter's own sums stay
        for k in ("psnr", "ssim"):
            assert o["meter"][k] == pytest.approx(o["pooled"][k], rel=1e-12)
        assert o["meter"]["lpips"] is None
