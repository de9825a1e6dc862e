"""engine.master_weights() without a GPU (cvvae_amd/autoencoder.py): the `latent` case of tests/engine_cases.py with bf16 networks on
the emulated kernels (tests/test_train_engine_host_logic.py `emulated` plus tests/master_ref.py) for four iterations -- every trainable
parameter is its master rounded to bf16, bit for bit; the masters left their seeds; the EMA shadows are fp32 and equal, bit for bit,
the EMA recomputed from the recorded masters with the documented arithmetic; master_state_dict() has state_dict()'s keys and fp32
values -- the calls that must raise, and two `gloo` ranks whose masters, moments and shadows stay bit-equal over three iterations."""
import contextlib
import copy
import datetime
import os

import pytest
import torch

from oracle.seeded import seeded_input
from tests import ddp_ref
from tests import engine_cases as EC
from tests import master_ref as M
from tests.test_train_engine_host_logic import INDICES, SHAPE, emulated

JOIN_LIMIT = 300.0
_BUILT = {}


def _engine(**kw):
    key = repr(sorted(kw.items()))
    if key not in _BUILT:
        _BUILT[key] = EC.build("latent", False, **kw)
    return copy.deepcopy(_BUILT[key])


@contextlib.contextmanager
def emulated_with_masters(count=None):
    with emulated(), pytest.MonkeyPatch.context() as mp:
        M.pretend_gpu(mp, count)
        yield


def test_four_iterations_on_master_weights():
    e = _engine(ema_decay=0.999)
    fp32 = {n: p.detach().clone() for n, p in e.named_parameters()}
    trainable = [n for n, p in e.named_parameters() if p.requires_grad]
    keys = list(e.state_dict())
    x = seeded_input(SHAPE, 12).to(torch.bfloat16)
    e.sample_generator = torch.Generator().manual_seed(5)
    e.frame_indices = INDICES
    count = {}
    with emulated_with_masters(count):
        assert e.master_weights() is e
        cast = [n for n in trainable if e.get_parameter(n).dtype == torch.bfloat16]
        assert cast and sorted(set(trainable) - set(cast)) == sorted(n for n in trainable if n.startswith("loss.logvar"))
        assert all(p.dtype == torch.bfloat16 for n, p in e.named_parameters() if not n.startswith("loss.logvar"))   # the frozen ones too
        # before the first step: the seeds are the fp32 values, the shadows their copies, master_state_dict() holds them
        for n in cast:
            assert torch.equal(e.master_of(e.get_parameter(n)), fp32[n]) and torch.equal(e.get_parameter(n).detach(), fp32[n].bfloat16())
        msd = e.master_state_dict()
        assert list(msd) == list(e.state_dict()) == keys
        assert all(msd[n].dtype == torch.float32 and torch.equal(msd[n], fp32[n]) for n in trainable)
        shadow = {}
        for n in trainable:
            s = getattr(e.model_ema, e.model_ema.m_name2s_name[n])
            assert s.dtype == torch.float32 and torch.equal(s, fp32[n])
            assert n not in cast or s.data_ptr() != e.master_of(e.get_parameter(n)).data_ptr()       # a copy of the seed
            shadow[n] = fp32[n].clone()
        opts = e.optimizers()
        assert all(o.master_weights for o in opts)
        for o in opts:                                    # the seeds went to the optimizers themselves, not as copies
            for p in (p for g in o.param_groups for p in g["params"]):
                if p.dtype == torch.bfloat16:
                    assert o.master(p) is e._master["seeds"][p]
        for it in range(4):
            loss = e.training_step({"frames": x}, it)
            e.on_train_batch_end()
            assert bool(torch.isfinite(loss))
            decay = torch.minimum(torch.tensor(0.999), torch.tensor(2 + it, dtype=torch.int32) / torch.tensor(11 + it, dtype=torch.int32))
            for n in trainable:
                p = e.get_parameter(n)
                m = e.master_of(p)
                assert (m is not None) == (n in cast), n
                if m is not None:
                    assert m.dtype == torch.float32 and torch.equal(p.detach(), m.bfloat16()), (it, n)
                shadow[n].sub_((1.0 - decay) * (shadow[n] - (p.detach() if m is None else m)))
        assert count["mt_adamw_master"] == 4 and count["mt_adamw"] == 2 and count["mt_norm_finish"] == 4 and count["mt_ema"] == 4
        assert count["mt_sumsq"] == 6 and "mt_grad_norm" not in count   # generator: fp32 logvars + bf16; discriminator: bf16 alone
        moved = [n for n in cast if not torch.equal(e.master_of(e.get_parameter(n)), fp32[n])]
        # the masters left their seeds: all but the few whose gradient is zero or rounding noise and whose value is 0 (a bias in
        # front of a normalisation, to_k's bias under the softmax) -- and none moved that no optimizer stepped
        stepped = {p for o in opts for p in o.state}
        assert all(e.get_parameter(n) in stepped for n in moved) and len(moved) > 0.8 * len(cast), (len(moved), len(cast))
        assert {n.split(".")[0 if not n.startswith("loss.") else 1] for n in moved} == {"encoder", "decoder", "discriminator"}
        stood = [n for n in cast if torch.equal(e.get_parameter(n).detach(), fp32[n].bfloat16())]
        print(f"{len(cast)} bf16 parameters; {len(stood)} of them still show their first bf16 value after 2 steps each")
        for n in trainable:
            s = getattr(e.model_ema, e.model_ema.m_name2s_name[n])
            assert s.dtype == torch.float32 and torch.equal(s, shadow[n]), n
        msd, sd = e.master_state_dict(), e.state_dict()
        assert list(msd) == list(sd) == keys
        for k in keys:
            if k in trainable:
                assert msd[k].dtype == torch.float32
                assert torch.equal(msd[k], e.master_of(e.get_parameter(k))) if k in cast else torch.equal(msd[k], sd[k])
            else:
                assert msd[k].dtype == sd[k].dtype and torch.equal(msd[k], sd[k])
        # a late call
        with pytest.raises(RuntimeError, match="before the first training_step"):
            e.master_weights()


def test_the_calls_that_raise():
    e = _engine(ema_decay=0.999)
    with pytest.raises(NotImplementedError, match="loss scaling"):
        e.master_weights(torch.float16)
    with pytest.raises(ValueError):
        e.master_weights(torch.float32)
    t = _engine(optimizer_config=dict(target="torch.optim.AdamW", params=dict(betas=[0.9, 0.98])))
    before = [p.dtype for p in t.parameters()]
    with pytest.raises(ValueError, match=r"cvvae_amd\.optim\.AdamW"):
        t.master_weights()
    assert [p.dtype for p in t.parameters()] == before      # refused before anything was cast
    assert all(p.dtype == torch.float32 for p in e.parameters())
    e.master_weights()
    with pytest.raises(RuntimeError):
        e.master_weights()                                    # twice
    late = _engine(ema_decay=0.999)
    late.optimizers()
    with pytest.raises(RuntimeError, match="before the first training_step"):
        late.master_weights()


def _rank(rank, world, port, out):
    """one replica: its own start, its own seeds, its own data; three iterations; the digests of its state to `out`"""
    import json
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        torch.manual_seed(100 + rank)
        e = EC.build("latent", False, ema_decay=0.999)
        if rank:                              # another start on the other rank: the broadcast must carry rank 0's
            with torch.no_grad():
                for p in e.parameters():
                    p.add_(0.01 * torch.randn(p.shape))
            e._build_ema()
        x = seeded_input(SHAPE, 12 + rank).to(torch.bfloat16)
        e.sample_generator = torch.Generator().manual_seed(5)
        e.frame_indices = INDICES
        with emulated_with_masters():
            e.master_weights()
            if rank:                          # and seeds that the broadcast of the 16-bit parameters alone would not repair
                with torch.no_grad():
                    for s in e._master["seeds"].values():
                        s.add_(1e-5)
            e.data_parallel()
            for it in range(3):
                e.training_step({"frames": x}, it)
                e.on_train_batch_end()
            state = ddp_ref.engine_state(e)
            state.update({"master:" + n: e.master_of(p) for n, p in e.named_parameters() if e.master_of(p) is not None})
        with open(out, "w") as fh:
            json.dump(ddp_ref.digest(state), fh)
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_keep_masters_moments_and_shadows_bit_equal(tmp_path):
    import json
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = ddp_ref.free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, str(tmp_path / f"r{r}.json"))) for r in range(2)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(timeout=JOIN_LIMIT)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    assert [p.exitcode for p in procs] == [0, 0]
    a, b = (json.load(open(tmp_path / f"r{r}.json")) for r in range(2))
    assert sorted(a) == sorted(b)
    masters = [k for k in a if k.startswith("master:")]
    moments = [k for k in a if k.startswith("opt") and k.rsplit(":", 1)[1] in ("exp_avg", "exp_avg_sq", "master")]
    shadows = [k for k in a if k.startswith("ema:")]
    assert masters and moments and shadows
    assert [k for k in a if a[k] != b[k]] == []
