"""The fp32 gradient bucket for 16-bit parameters on a real MI355X (cvvae_amd/ddp.py GradientSync(wide_gradients=True),
csrc/optim_kernels.hip cvvae_mt_pack_wide / cvvae_mt_adamw_master_wide, cvvae_amd/optim.py `main_grad`).

a. the widening pack pass at every edge of the chunk geometry in ONE launch per divisor, bit for bit against torch.div(g.float(), d)
   on the device, over the special values of the 16-bit format;
b. the AdamW pass that reads an fp32 gradient for a 16-bit parameter on the same edge list: master, m and v have the bits of the fp32
   pass on fp32 copies, p is the rounded master, and fed float(g16) all four have the bits of the master pass fed g16;
c. world size 1: four iterations of a bf16 engine on master weights under data_parallel(wide_gradients=True) equal the engine without
   data_parallel bit for bit, every 16-bit gradient lying in its slot as `main_grad`; two more under torch's synchronisation check;
d. two ranks drive the real kernels on ONE card (two fresh child processes, gloo, transport "host"): each rank's `main_grad` is
   float(g_0) / 2 + float(g_1) / 2 bit for bit, and after four iterations the replicas' states are bit-equal; the same over RCCL
   where two GPUs are visible;
e. one NaN element in one 16-bit gradient poisons the norm, the coefficient and the step.

The kernels are deterministic and the exchange of two ranks is one commutative addition, so every comparison here is an equality."""
import argparse
import copy
import datetime
import math
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
from tests import ddp_ref, ddp_wide_ref, optim_ref  # noqa: E402
from tests import engine_cases as EC  # noqa: E402
from tests import master_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (1, 3, 5, 32, 32)
INDICES = [0, 2]
SENTINEL = 7.25
CHILD_LIMIT = 180.0
LR = optim_ref.YAML_LR
B1, B2 = optim_ref.YAML_ADAMW["betas"]
EPS, WD = optim_ref.YAML_ADAMW["eps"], optim_ref.YAML_ADAMW["weight_decay"]
COEF = 0.37
CHUNK = optim_ref.CHUNK
GUARD = optim_ref.GUARD
_EDGES = {}


def _edge(dtype):
    if dtype not in _EDGES:
        _EDGES[dtype] = M.edge_list16(dtype)
    return _EDGES[dtype]


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- a. the pack pass ----
@pytest.fixture(scope="module", params=M.DTYPES16, ids=["bf16", "fp16"])
def pack_case(request):
    """master_ref.edge_list16's geometry (element counts, the view 2 bytes into its buffer, the tensor without a gradient) with the
    sources replaced by ddp_wide_ref.special_values16; destinations laid out as GradientSync lays its slots, each followed by GUARD
    elements"""
    from cvvae_amd import ddp
    dtype = request.param
    entries = _edge(dtype)
    gen = torch.Generator().manual_seed(11)
    srcs = []
    for e in entries:
        off, n = e["off"]["g"], e["n"]
        buf = ddp_wide_ref.special_values16(off + n + GUARD, dtype, gen).cuda()
        view = buf[off:off + n].view(() if n == 1 else (n,))
        srcs.append((buf, view if e["has_grad"] else None))
    numels = [e["n"] for e in entries]
    assert sorted(set(numels)) == sorted({0, 1, 7, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 3, 3 * CHUNK + 5, 1000})
    offsets, total = ddp.slot_layout([n + GUARD for n in numels])
    return dtype, entries, srcs, numels, offsets, total


@pytest.mark.parametrize("divisor", [1, 2, 3, 8])
def test_pack_wide_at_its_edges_in_one_launch(pack_case, divisor):
    from cvvae_amd import ops
    dtype, entries, srcs, numels, offsets, total = pack_case
    flat = torch.full((total,), SENTINEL, dtype=torch.float32, device="cuda")
    dsts = [flat[o:o + n] for o, n in zip(offsets, numels)]
    assert all(d.data_ptr() % 16 == 0 for d in dsts)
    assert sum(s[1] is not None and s[1].data_ptr() % 16 == 2 for s in srcs) >= 1        # a source 2 bytes into its buffer
    assert sum(s[1] is None for s in srcs) == 1
    before = [b.clone() for b, _ in srcs]
    mtl = ops.MultiTensorList(numels, "cuda", dtype).set(g=[g for _, g in srcs], shadow=dsts)
    ops.mt_pack_wide(mtl, float(divisor))
    torch.cuda.synchronize()
    touched = torch.zeros(total, dtype=torch.bool, device="cuda")
    d_dev = torch.tensor(float(divisor), device="cuda")
    classes = set()
    for (buf, g), dst, o, n in zip(srcs, dsts, offsets, numels):
        touched[o:o + n] = True
        if g is None:
            assert n > 0 and float(dst.abs().max()) == 0.0 and not bool(torch.signbit(dst).any())     # the None slot: all +0
            continue
        wide = g.reshape(-1).float()
        assert wide.dtype == torch.float32 and torch.equal(wide.to(dtype).view(torch.int16)[~torch.isnan(wide)],
                                                           g.reshape(-1).view(torch.int16)[~torch.isnan(wide)])    # exact widening
        # the divisor as a 0-dim DEVICE tensor: a Python scalar would make torch multiply by its reciprocal
        assert ddp_ref.same_bits_or_both_nan(dst, torch.div(wide, d_dev)), (n, divisor)
        # ... and the host's division, which is the C++ operator
        assert ddp_ref.same_bits_or_both_nan(dst, torch.div(wide.cpu(), torch.tensor(float(divisor)))), (n, divisor)
        if divisor == 1 and n:
            assert ddp_ref.same_bits_or_both_nan(dst, wide)
        if n >= 1000:
            fi = torch.finfo(dtype)
            a = wide.abs()
            classes |= {k for k, hit in (("nan", torch.isnan(wide)), ("inf", torch.isinf(wide)), ("-0", (wide == 0) & torch.signbit(wide)),
                                         ("sub", (a > 0) & (a < fi.tiny)), ("tiny", a == fi.tiny), ("max", a == fi.max)) if bool(hit.any())}
    assert classes == {"nan", "inf", "-0", "sub", "tiny", "max"}, classes
    # the guards behind every destination and the alignment gaps: the sentinel, untouched; the sources: unchanged
    assert bool((flat[~touched] == SENTINEL).all())
    assert all(torch.equal(b.view(torch.int16), c.view(torch.int16)) for (b, _), c in zip(srcs, before))
    if divisor == 3:     # the case that tells a division from a product with the reciprocal
        g = torch.cat([g.reshape(-1).float() for _, g in srcs if g is not None])
        fin = torch.isfinite(g)
        three = torch.tensor(3.0, device="cuda")
        assert not torch.equal((g / three)[fin], (g * (1.0 / three))[fin])


def test_pack_wide_refuses_what_it_has_no_kernel_for():
    from cvvae_amd import ops
    t = torch.zeros(8, device="cuda")
    h = t.bfloat16()
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.mt_pack_wide(ops.MultiTensorList([8], "cuda", torch.bfloat16).set(g=[h], shadow=[t]), bad)
    with pytest.raises(ValueError):
        ops.mt_pack_wide(ops.MultiTensorList([8], "cuda", torch.bfloat16).set(g=[h]), 2.0)     # no destination was ever set
    with pytest.raises(NotImplementedError):
        ops.mt_pack_wide(ops.MultiTensorList([8], "cuda").set(g=[t], shadow=[t.clone()]), 2.0)  # an fp32 list is cvvae_mt_pack's
    with pytest.raises(NotImplementedError):
        ops.mt_pack(ops.MultiTensorList([8], "cuda", torch.bfloat16).set(g=[h], shadow=[t]), 2.0)   # and a 16-bit one is not
    empty = ops.MultiTensorList([0, 0], "cuda", torch.float16).set(g=[None, h[:0].half()], shadow=[t[:0], t[:0]])
    assert empty.n_chunks == 0
    ops.mt_pack_wide(empty, 2.0)                                                  # n_chunks = 0 is allowed
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


# ---- b. the AdamW pass with an fp32 gradient ----
FIELDS = ("g", "p", "m", "v", "w")


def _device_copy(edge, grad32=None):
    """per entry (buffers on the device, views); grad32(e) -> an fp32 gradient buffer laid out as e's 16-bit one (`g32_buf`, view `g32`)"""
    out = []
    for e in edge:
        bufs = {k: e[k].cuda() for k in e if k.endswith("_buf")}
        views = M.views16(e, bufs)
        if grad32 is not None:
            bufs["g32_buf"] = grad32(e).cuda()
            off = e["off"]["g"]
            views["g32"] = bufs["g32_buf"][off:off + e["n"]].view(views["g"].shape)
        out.append((bufs, views))
    return out


def _scalars(edge, sel):
    return dict(step_size=[LR / (1.0 - B1 ** edge[i]["t"]) for i in sel], bias2_sqrt=[math.sqrt(1.0 - B2 ** edge[i]["t"]) for i in sel])


def _list(edge, dev, dtype, g):
    """the list of the tensors that have a gradient: g = "g32" (the wide pass), "g" (the master pass) or "ref" (the fp32 pass on fp32
    copies of master, m and v fed the g32 views)"""
    from cvvae_amd import ops
    sel = [i for i, e in enumerate(edge) if e["has_grad"]]
    pick = lambda k: [dev[i][1][k] for i in sel]  # noqa: E731
    if g == "ref":
        mtl = ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda")
        return mtl.set(g=pick("g32"), p=[t.clone() for t in pick("w")], m=[t.clone() for t in pick("m")], v=[t.clone() for t in pick("v")],
                       **_scalars(edge, sel)), sel
    mtl = ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda", dtype)
    return mtl.set(g=pick(g), p=pick("p"), m=pick("m"), v=pick("v"), shadow=pick("w"), **_scalars(edge, sel)), sel


def _untouched(edge, dev, written, g32=None):
    """a written view's buffer keeps its bits in front of and behind the view; every other buffer keeps all of them"""
    for e, (bufs, _) in zip(edge, dev):
        for k in FIELDS:
            lo, hi = e["off"][k], e["off"][k] + e["n"]
            after, before = _bits(bufs[k + "_buf"].cpu()), _bits(e[k + "_buf"])
            if k in written and e["has_grad"]:
                assert torch.equal(after[:lo], before[:lo]) and torch.equal(after[hi:], before[hi:]), (e["n"], k)
            else:
                assert torch.equal(after, before), (e["n"], k)
        if g32 is not None:
            assert torch.equal(_bits(bufs["g32_buf"].cpu()), _bits(g32(e))), e["n"]


@pytest.mark.parametrize("coef", [None, COEF], ids=["nocoef", "coef"])
@pytest.mark.parametrize("dtype", M.DTYPES16, ids=["bf16", "fp16"])
def test_adamw_master_wide_pass_on_every_edge_in_one_launch(dtype, coef):
    from cvvae_amd import ops
    edge = _edge(dtype)
    c = None if coef is None else torch.tensor([COEF], dtype=torch.float32, device="cuda")
    hp = (LR, B1, B2, EPS, WD, c)
    # 1. a gradient no 16-bit value holds (float(g16) / 3, what an average over three ranks looks like): the fp32 pass is the yardstick
    third = lambda e: torch.div(e["g_buf"].float(), torch.tensor(3.0))  # noqa: E731
    dev = _device_copy(edge, third)
    mtl, sel = _list(edge, dev, dtype, "g32")
    ref, _ = _list(edge, dev, dtype, "ref")
    assert mtl.n_chunks == ref.n_chunks == 1 + 1 + 1 + 1 + 2 + 4 + 2 + 2 + 2          # one launch, 10 tensors (one of them empty)
    mis = {(dev[i][1]["g32"].data_ptr() % 16, dev[i][1]["p"].data_ptr() % 16) for i in sel if edge[i]["n"] > CHUNK}
    assert {(0, 0), (4, 2), (0, 2)} <= mis                                            # g and p aligned or not, separately
    assert not all(torch.equal(dev[i][1]["g32"].to(dtype).float(), dev[i][1]["g32"]) for i in sel)
    ops.mt_adamw_master_wide(mtl, *hp)
    ops.mt_adamw(ref, *hp)
    torch.cuda.synchronize()
    for j, i in enumerate(sel):
        e, v = edge[i], dev[i][1]
        for k, f in (("w", "p"), ("m", "m"), ("v", "v")):
            assert _same_bits(v[k], ref.tensors[f][j]), (e["n"], e["off"], e["t"], k)
        assert _same_bits(v["p"], v["w"].to(dtype)), (e["n"], e["off"])
        assert e["n"] == 0 or not torch.equal(v["w"].cpu(), M.views16(e, e)["w"])     # the master moved
    _untouched(edge, dev, ("p", "m", "v", "w"), third)                                # g16 and g32 among the untouched
    # 2. the gradient exactly float(g16): all four outputs have the bits of the master pass fed g16
    exact = lambda e: e["g_buf"].float()  # noqa: E731
    dev, dev16 = _device_copy(edge, exact), _device_copy(edge)
    mtl, sel = _list(edge, dev, dtype, "g32")
    narrow, _ = _list(edge, dev16, dtype, "g")
    ops.mt_adamw_master_wide(mtl, *hp)
    ops.mt_adamw_master(narrow, *hp)
    torch.cuda.synchronize()
    for i in sel:
        for k in ("p", "w", "m", "v"):
            assert _same_bits(dev[i][1][k], dev16[i][1][k]), (edge[i]["n"], edge[i]["off"], k)
    _untouched(edge, dev, ("p", "m", "v", "w"), exact)


# ---- e. a NaN ----
def test_one_nan_in_a_16_bit_gradient_poisons_norm_coefficient_and_step():
    from cvvae_amd import ops
    dtype = torch.bfloat16
    edge = _edge(dtype)
    dev = _device_copy(edge, lambda e: torch.zeros(e["g_buf"].shape))
    dev[6][1]["g"][CHUNK + 17] = float("nan")
    sel = [i for i, e in enumerate(edge) if e["has_grad"]]
    pack = ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda", dtype).set(g=[dev[i][1]["g"] for i in sel], shadow=[dev[i][1]["g32"] for i in sel])
    ops.mt_pack_wide(pack, 2.0)
    mtl, _ = _list(edge, dev, dtype, "g32")
    norm = ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda").set(g=[dev[i][1]["g32"] for i in sel])
    partials = torch.empty(norm.n_chunks, dtype=torch.float32, device="cuda")
    ops.mt_sumsq(norm, partials)
    out2 = ops.mt_norm_finish(partials, 1.0)
    ops.mt_adamw_master_wide(mtl, LR, B1, B2, EPS, WD, out2[1])
    torch.cuda.synchronize()
    assert int(torch.isnan(torch.cat([dev[i][1]["g32"].reshape(-1) for i in sel])).sum()) == 1      # one element of one slot
    assert bool(torch.isnan(out2).all())
    for i in sel:                      # as torch: the NaN coefficient reaches every gradient, AdamW then writes NaN everywhere
        assert all(bool(torch.isnan(dev[i][1][k]).all()) for k in ("p", "w", "m", "v")), edge[i]["n"]


# ---- c. world size 1 ----
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


def _engine(kind, device="cuda"):
    """the fp32 engine of tests/engine_cases.py on the device, its networks cast to bf16 on fp32 master weights"""
    if kind not in _BUILT:
        _BUILT[kind] = EC.build(kind, True, ema_decay=0.999)
    e = copy.deepcopy(_BUILT[kind]).to(device).master_weights()
    e.sample_generator, e.frame_indices = torch.Generator(device).manual_seed(5), INDICES
    return e


def _differences(a, b):
    sa, sb = ddp_ref.engine_state(a), ddp_ref.engine_state(b)
    assert sorted(sa) == sorted(sb)
    return [k for k in sa if sa[k].dtype != sb[k].dtype or sa[k].shape != sb[k].shape or not torch.equal(sa[k], sb[k])]


def _in_their_slots(sync):
    """after sync(): every 16-bit parameter with a gradient has it as main_grad in its slot and no .grad; -> (16-bit, fp32) counts"""
    n16 = n32 = 0
    for p, o, n in zip(sync.params, sync.layout(), sync.numels):
        assert n == p.numel()
        if p.dtype == torch.float32:
            if p.grad is not None:
                assert p.grad.data_ptr() == sync.flat.data_ptr() + 4 * o
                n32 += 1
        elif getattr(p, "main_grad", None) is not None:
            g = p.main_grad
            assert p.grad is None and g.dtype == torch.float32 and g.shape == p.shape and g.is_contiguous()
            assert g.data_ptr() == sync.flat.data_ptr() + 4 * o
            n16 += 1
        else:
            assert p.grad is None
    return n16, n32


def test_world_size_one_equals_the_master_engine_without_it_bit_for_bit(one_rank_group):
    a, b = _engine("latent"), _engine("latent")
    assert a.data_parallel(one_rank_group, wide_gradients=True) is a
    x = seeded_input(SHAPE, 12).to(torch.bfloat16).cuda()
    for it in range(4):
        la, lb = a.training_step({"frames": x}, it), b.training_step({"frames": x}, it)
        a.on_train_batch_end()
        b.on_train_batch_end()
        assert torch.equal(la, lb) and bool(torch.isfinite(la)), (it, float(la), float(lb))
        assert sorted(a.last_logs) == sorted(b.last_logs)
        diff = [k for k in a.last_logs if not torch.equal(a.last_logs[k], b.last_logs[k])]
        assert not diff, (it, diff)
        opt = a.optimizers()[it % 2]
        assert opt.master_weights and torch.equal(opt.last_grad_norm, b.optimizers()[it % 2].last_grad_norm)
        bad = _differences(a, b)
        assert not bad, (it, len(bad), bad[:8])
        sync = a.gradient_sync(opt)
        assert sync.calls == it // 2 + 1 and sync.world == 1 and sync.wide_gradients and sync.flat is not None
        n16, n32 = _in_their_slots(sync)
        assert n16 > 10 and (n32 >= 1 if it % 2 == 0 else n32 == 0)  # the generator's list holds the loss's fp32 logvars
        assert n16 == sum(p.dtype == torch.bfloat16 and p in opt.state for p in sync.params)
    assert any(k.endswith(":master") for k in ddp_ref.engine_state(a))
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


# ---- d. two ranks: the worker (a fresh process per rank) and its parents ----
def _opt_grads(e, i=0):
    return [p.main_grad if getattr(p, "main_grad", None) is not None else p.grad for g in e.optimizers()[i].param_groups for p in g["params"]]


def _child(args):
    torch.set_num_threads(4)
    dist.init_process_group(args.backend, init_method=f"tcp://127.0.0.1:{args.port}", rank=args.rank, world_size=args.world,
                            timeout=datetime.timedelta(seconds=60))
    try:
        device = f"cuda:{args.rank if args.backend == 'nccl' else 0}"
        torch.cuda.set_device(device)
        xs = [seeded_input(SHAPE, 30 + r).to(torch.bfloat16).to(device) for r in range(args.world)]
        per_rank = []
        for r in range(args.world):       # unsynchronised copies, run here: every rank's own gradient of the first iteration
            e = _engine("latent", device)
            e.training_step({"frames": xs[r]}, 0)
            per_rank.append([None if g is None else g.detach().cpu() for g in _opt_grads(e)])
            del e
        dtypes = {g.dtype for g in per_rank[0] if g is not None}
        assert dtypes == {torch.bfloat16, torch.float32}, dtypes                # the networks' gradients and the loss's logvar
        want = ddp_wide_ref.mean_in_rank_order16(per_rank)    # float(g_0) / 2 + float(g_1) / 2 on the host in fp32
        e = _engine("latent", device)
        e.data_parallel(transport=args.transport, wide_gradients=True)
        losses = []
        for it in range(4):
            losses.append(float(e.training_step({"frames": xs[args.rank]}, it)))
            if it == 0:
                sync = e.gradient_sync(e.optimizers()[0])
                assert sync.world == args.world and sync.transport == args.transport and sync.flat.is_cuda and sync.wide_gradients
                got = _opt_grads(e)
                assert [g is None for g in got] == [w is None for w in want]
                assert all(g.dtype == torch.float32 for g in got if g is not None)
                bad = [i for i, (g, w) in enumerate(zip(got, want)) if w is not None and not torch.equal(g.cpu(), w)]
                assert not bad, f"rank {args.rank}: {len(bad)} synchronised gradients differ from g_0/2 + g_1/2, first {bad[:5]}"
                assert all(g.data_ptr() == sync.flat.data_ptr() + 4 * o for g, o in zip(got, sync.layout()) if g is not None)
                assert all(p.grad is None for p in sync.params if p.dtype == torch.bfloat16)
                n16 = sum(p.dtype == torch.bfloat16 and p.main_grad is not None for p in sync.params)
                n32 = sum(p.dtype == torch.float32 and p.grad is not None for p in sync.params)
                assert n16 > 10 and n32 >= 1, (n16, n32)
            e.on_train_batch_end()
        torch.save({"state": {k: v.detach().cpu() for k, v in ddp_ref.engine_state(e).items()}, "losses": losses}, args.out)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    print(f"DDP-WIDE-CHILD rank {args.rank} done: losses {losses}")
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
    assert any(k.endswith(":master") for k in a["state"])
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
