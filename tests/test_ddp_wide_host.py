"""The fp32 gradient bucket for 16-bit parameters, what holds without a GPU: the two C entry points (cvvae_mt_pack_wide,
cvvae_mt_adamw_master_wide: exported, typed, declared, refusing bad arguments before any launch, ABI still 14),
cvvae_amd.ddp.GradientSync(wide_gradients=True) and cvvae_amd.optim.AdamW(master_weights=True)'s reading of `main_grad` on the
emulated launches (tests/ddp_wide_ref.py), and the engine's refusal of the switch without master weights.  Every comparison of values
is an equality: the emulated passes are the documented arithmetic and a world of one rank divides by 1."""
import contextlib
import copy
import ctypes
import os

import pytest
import torch
import torch.nn as nn

from tests import ddp_wide_ref as W
from tests import optim_ref as R

EINVAL, EUNSUPPORTED = -1, -2
NEW = ["cvvae_mt_pack_wide", "cvvae_mt_adamw_master_wide"]
HP = dict(lr=R.YAML_LR, **R.YAML_ADAMW)


# ---- the C entry points ----
def test_the_two_entry_points_are_exported_typed_and_declared_and_the_abi_is_still_14():
    from cvvae_amd import _lib, ops
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "cvvae.h")).read()
    assert "#define CVVAE_ABI_VERSION 14" in header
    for n in NEW:
        assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header, n
        assert getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1]
    assert _lib.PROTOTYPES["cvvae_mt_pack_wide"] == _lib.PROTOTYPES["cvvae_mt_pack"]
    assert _lib.PROTOTYPES["cvvae_mt_adamw_master_wide"] == _lib.PROTOTYPES["cvvae_mt_adamw_master"]
    assert ctypes.sizeof(_lib.MTTensor) == 48 and _lib.MTTensor.shadow.offset == 32      # the struct keeps its layout
    assert callable(ops.mt_pack_wide) and callable(ops.mt_adamw_master_wide)


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL (host) pointer: the checks below never dereference or launch
    hp = (4e-5, 0.9, 0.98, 1e-4, 0.01)
    for dt in (L.F32, L.F32Q, 9):
        assert lib.cvvae_mt_pack_wide(dt, p, p, 1, 2.0, None) == EUNSUPPORTED
        assert lib.cvvae_mt_adamw_master_wide(dt, p, p, 1, *hp, None, None) == EUNSUPPORTED
    for dt in (L.BF16, L.F16):
        assert lib.cvvae_mt_pack_wide(dt, None, p, 1, 2.0, None) == EINVAL
        assert lib.cvvae_mt_pack_wide(dt, p, None, 1, 2.0, None) == EINVAL
        assert lib.cvvae_mt_pack_wide(dt, p, p, -1, 2.0, None) == EINVAL
        assert lib.cvvae_mt_pack_wide(dt, p, p, 1 << 40, 2.0, None) == EINVAL
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert lib.cvvae_mt_pack_wide(dt, p, p, 1, bad, None) == EINVAL
        assert lib.cvvae_mt_pack_wide(dt, None, None, 0, 2.0, None) == 0                        # an empty list: no error, no launch
        assert lib.cvvae_mt_adamw_master_wide(dt, None, p, 1, *hp, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master_wide(dt, p, None, 1, *hp, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master_wide(dt, p, p, -1, *hp, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master_wide(dt, p, p, 1 << 40, *hp, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master_wide(dt, p, p, 1, -1.0, 0.9, 0.98, 1e-4, 0.01, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master_wide(dt, p, p, 1, 4e-5, 1.0, 0.98, 1e-4, 0.01, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master_wide(dt, p, p, 1, 4e-5, 0.9, float("nan"), 1e-4, 0.01, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master_wide(dt, None, None, 0, *hp, None, None) == 0
    # the entries they stand beside keep their contracts
    for dt in (L.BF16, L.F16):
        assert lib.cvvae_mt_pack(dt, p, p, 1, 2.0, None) == EUNSUPPORTED


def test_the_wrappers_have_no_cpu_path():
    from cvvae_amd import ops
    mtl = ops.MultiTensorList([5], "cpu", torch.bfloat16)
    z16, z32 = torch.zeros(5, dtype=torch.bfloat16), torch.zeros(5)
    mtl.set(g=[z32.clone()], p=[z16.clone()], m=[z32], v=[z32.clone()], shadow=[z32.clone()], step_size=[1.0], bias2_sqrt=[1.0])
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mt_adamw_master_wide(mtl, 4e-5, 0.9, 0.98, 1e-4, 0.01)
    mtl.set(g=[z16])
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mt_pack_wide(mtl, 2.0)


# ---- GradientSync and AdamW on the emulated launches ----
SPECS = [((5, 3), torch.float32, True), ((7,), torch.bfloat16, True), ((4,), torch.bfloat16, False), ((), torch.float32, True),
         ((R.CHUNK + 9,), torch.bfloat16, True), ((3,), torch.float32, False), ((), torch.bfloat16, True)]


def _mixed(seed=0):
    """one group: fp32 and bf16 parameters with and without a gradient, 0-dim ones, one larger than a chunk -> (params, grads)"""
    gen = torch.Generator().manual_seed(seed)
    params, grads = [], []
    for shape, dt, has_grad in SPECS:
        p = nn.Parameter(torch.randn(shape, generator=gen).to(dt))
        g = (0.5 * torch.randn(shape, generator=gen)).to(dt) if has_grad else None
        p.grad = None if g is None else g.clone()
        params.append(p)
        grads.append(g)
    return params, grads


def test_wide_sync_gives_every_parameter_an_aligned_slot_and_sets_main_grad(monkeypatch):
    from cvvae_amd import ddp
    count = {}
    W.pretend_gpu(monkeypatch, count)
    params, grads = _mixed()
    sync = ddp.GradientSync(params, wide_gradients=True)
    numels = [p.numel() for p in params]
    assert sync.wide_gradients and sync.numels == numels                     # a bf16 parameter has a slot of its element count
    assert (sync.layout(), sync.total) == ddp.slot_layout(numels)            # slot_layout is the same function
    assert all(o % 4 == 0 for o in sync.layout())
    sync.sync()
    assert count == {"mt_pack": 1, "mt_pack_wide": 1}                        # one launch per source dtype present
    assert sync.flat.dtype == torch.float32 and sync.flat.numel() == sync.total
    used = torch.zeros(sync.total, dtype=torch.bool)
    for (shape, dt, has_grad), p, g, o, n in zip(SPECS, params, grads, sync.layout(), numels):
        slot = sync.flat[o:o + n]
        used[o:o + n] = True
        if dt == torch.float32:
            assert not hasattr(p, "main_grad")
            if has_grad:
                assert p.grad.data_ptr() == sync.flat.data_ptr() + 4 * o and torch.equal(p.grad, g) and p.grad.shape == p.shape
            else:
                assert p.grad is None and float(slot.abs().max()) == 0.0
        elif has_grad:
            mg = p.main_grad
            assert p.grad is None                                             # the 16-bit gradient is freed
            assert mg.dtype == torch.float32 and mg.shape == p.shape and mg.is_contiguous()
            assert mg.data_ptr() == sync.flat.data_ptr() + 4 * o and torch.equal(mg, g.float())
        else:
            assert p.grad is None and p.main_grad is None and float(slot.abs().max()) == 0.0 and not bool(torch.signbit(slot).any())
    assert int((~used).sum()) > 0 and float(sync.flat[~used].abs().max()) == 0.0      # the gaps stay zero
    assert all(m.tensors.get("g") is None for m in [sync._mtl] + [m for _, _, m in sync._wide])
    # the next iteration: another parameter goes without a gradient; the slot it filled is zeroed and its main_grad cleared
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()
    params[1].grad = None
    sync.sync()
    assert count == {"mt_pack": 2, "mt_pack_wide": 2}
    o = sync.layout()[1]
    assert params[1].main_grad is None and params[1].grad is None and float(sync.flat[o:o + 7].abs().max()) == 0.0
    assert torch.equal(params[4].main_grad, grads[4].float())


def test_a_gradient_the_kernel_cannot_take_keeps_the_torch_path(monkeypatch):
    from cvvae_amd import ddp
    count = {}
    W.pretend_gpu(monkeypatch, count)
    gen = torch.Generator().manual_seed(3)
    params = [nn.Parameter(torch.randn(4, 6, generator=gen).bfloat16()), nn.Parameter(torch.randn(5, generator=gen).bfloat16())]
    g0 = torch.randn(6, 4, generator=gen).bfloat16().t()                      # not contiguous
    g1 = torch.randn(5, generator=gen).bfloat16()
    assert not g0.is_contiguous()
    params[0].grad, params[1].grad = g0, g1.clone()
    sync = ddp.GradientSync(params, wide_gradients=True)
    sync.sync()
    assert count == {"mt_pack_wide": 1}                                       # no fp32 parameter: no fp32 launch
    assert params[0].grad is g0 and params[0].main_grad is None and float(sync.slots[0].abs().max()) == 0.0
    assert params[1].grad is None and torch.equal(params[1].main_grad, g1.float())


def test_without_the_keyword_the_same_list_behaves_as_before(monkeypatch):
    from cvvae_amd import ddp
    count = {}
    W.pretend_gpu(monkeypatch, count)
    params, grads = _mixed()
    sync = ddp.GradientSync(params)
    assert not sync.wide_gradients
    assert sync.numels == [p.numel() if p.dtype == torch.float32 else 0 for p in params]       # a bf16 parameter: an empty slot
    sync.sync()
    assert count == {"mt_pack": 1} and sync._wide == []
    for p, g in zip(params, grads):
        assert not hasattr(p, "main_grad")
        if p.dtype == torch.bfloat16:
            assert (p.grad is None) == (g is None) and (g is None or (p.grad.dtype == torch.bfloat16 and torch.equal(p.grad, g)))
        elif g is not None:
            assert torch.equal(p.grad, g) and sync.flat.data_ptr() <= p.grad.data_ptr() < sync.flat.data_ptr() + 4 * sync.total


def test_adamw_reads_main_grad_with_one_norm_and_one_launch_per_dtype_and_width(monkeypatch):
    """AdamW(master_weights=True) after a wide sync() of one rank = the same optimizer on the 16-bit gradients themselves, bit for bit
    (float(g) / 1 is float(g)): parameters, masters, moments, the norm.  Launches: one norm (a sumsq per list, one finish), one AdamW
    launch per (dtype, width)"""
    from cvvae_amd import ddp
    from cvvae_amd.optim import AdamW
    count, calls = {}, []
    W.pretend_gpu(monkeypatch, count, calls)
    (pa, ga), (pb, _) = _mixed(), _mixed()
    a = AdamW(pa, max_grad_norm=1.0, master_weights=True, **HP)
    b = AdamW(pb, max_grad_norm=1.0, master_weights=True, **HP)
    sync = ddp.GradientSync(pa, wide_gradients=True)
    for it in range(2):
        sync.sync()
        count.clear()
        del calls[:]
        a.step()
        assert count == {"mt_sumsq": 2, "mt_norm_finish": 1, "mt_adamw": 1, "mt_adamw_master_wide": 1}, count
        names = [(n, args[0].dtype) for n, args in calls if n != "mt_norm_finish"]
        # the partials: fp32 parameters first, then bf16 -- whose fp32 main_grads the fp32 instance reads; then the wide step
        assert names == [("mt_sumsq", torch.float32), ("mt_sumsq", torch.float32), ("mt_adamw_master_wide", torch.bfloat16)]
        wide_norm = calls[1][1][0]
        assert [int(n) for n in wide_norm.numels] == [7, R.CHUNK + 9, 1]
        count.clear()
        b.step()
        assert count == {"mt_sumsq": 2, "mt_norm_finish": 1, "mt_adamw": 1, "mt_adamw_master": 1}
        assert torch.equal(a.last_grad_norm, b.last_grad_norm)
        for p, q in zip(pa, pb):
            assert torch.equal(p.detach(), q.detach()) and sorted(a.state.get(p, {})) == sorted(b.state.get(q, {}))
            for k, v in a.state.get(p, {}).items():
                assert v.dtype == b.state[q][k].dtype and torch.equal(v, b.state[q][k]), (it, k)
        for p, g in zip(pa, ga):      # gradients are left unscaled, in the slot
            if g is not None and p.dtype == torch.bfloat16:
                assert torch.equal(p.main_grad, g.float()) and p.main_grad.data_ptr() >= sync.flat.data_ptr()
        a.zero_grad()
        assert all(p.grad is None and getattr(p, "main_grad", None) is None for p in pa)      # zero_grad() clears main_grad
        for p, g in zip(pa, ga):
            p.grad = None if g is None else g.clone()
    assert pa[2] not in a.state and pa[5] not in a.state                      # no gradient: no state


def test_a_16_bit_gradient_beside_a_main_grad_is_one_more_launch_of_its_width(monkeypatch):
    from cvvae_amd.optim import AdamW
    count = {}
    W.pretend_gpu(monkeypatch, count)
    gen = torch.Generator().manual_seed(7)
    ps = [nn.Parameter(torch.randn(6, generator=gen).bfloat16()) for _ in range(2)]
    ps[0].grad = torch.randn(6, generator=gen).bfloat16()
    ps[1].main_grad = torch.randn(6, generator=gen)
    opt = AdamW(ps, max_grad_norm=1.0, master_weights=True, **HP)
    before = [p.detach().clone() for p in ps]
    opt.step()
    assert count == {"mt_sumsq": 2, "mt_norm_finish": 1, "mt_adamw_master": 1, "mt_adamw_master_wide": 1}
    assert all("master" in opt.state[p] and opt.state[p]["exp_avg"].dtype == torch.float32 for p in ps)
    assert not any(torch.equal(opt.master(p), b.float()) for p, b in zip(ps, before))


def test_without_master_weights_nothing_reads_main_grad(monkeypatch):
    from cvvae_amd.optim import AdamW
    count = {}
    W.pretend_gpu(monkeypatch, count)
    p = nn.Parameter(torch.ones(6, dtype=torch.bfloat16))
    p.main_grad = torch.ones(6)
    opt = AdamW([p], max_grad_norm=1.0, **HP)
    opt.step()
    assert count == {} and p not in opt.state and bool((p.detach() == 1.0).all())
    opt.zero_grad()
    assert p.main_grad is not None                                            # not this optimizer's to clear


def test_clip_grad_norm_scales_main_grad_in_its_slot(monkeypatch):
    from cvvae_amd import ddp
    from cvvae_amd.optim import clip_grad_norm_
    count = {}
    W.pretend_gpu(monkeypatch, count)
    params, grads = _mixed()
    sync = ddp.GradientSync(params, wide_gradients=True)
    sync.sync()
    count.clear()
    norm = clip_grad_norm_(params, 0.5)
    assert count == {"mt_grad_norm": 1, "mt_scale": 1}
    want = torch.cat([g.float().reshape(-1) for g in grads if g is not None])
    assert abs(float(norm) - float(want.norm())) <= 1e-5 * float(want.norm()) and float(norm) > 0.5
    coef = torch.tensor(0.5) / (norm + 1e-6)
    for p, g in zip(params, grads):
        if g is not None:
            got = p.grad if p.dtype == torch.float32 else p.main_grad
            assert torch.equal(got, g.float() * coef) and got.data_ptr() >= sync.flat.data_ptr()
    with pytest.raises(NotImplementedError):
        clip_grad_norm_(params, 0.5, norm_type=1.0)                           # torch's function does not know main_grad


# ---- the engine ----
_BUILT = {}


def _engine():
    from tests import engine_cases as EC
    if "latent" not in _BUILT:
        _BUILT["latent"] = EC.build("latent", False, ema_decay=0.999)
    return copy.deepcopy(_BUILT["latent"])


@contextlib.contextmanager
def _emulated(count=None):
    from tests.test_train_engine_host_logic import emulated
    with emulated(), pytest.MonkeyPatch.context() as mp:
        W.pretend_gpu(mp, count)
        yield


def test_the_engine_refuses_wide_gradients_without_master_weights():
    with _emulated():
        e = _engine()
        assert e.data_parallel(wide_gradients=True) is e
        with pytest.raises(ValueError, match="master_weights"):
            e.gradient_sync(e.optimizers()[0])
        with pytest.raises(ValueError, match="master_weights"):
            e.gradient_sync(torch.optim.AdamW([nn.Parameter(torch.zeros(3))]))       # a foreign optimizer
        e = _engine()
        with pytest.raises(NotImplementedError):
            e.master_weights(torch.float16)                                   # fp16 engines stay refused


def test_two_engine_iterations_under_a_wide_sync_equal_the_engine_without_it():
    from oracle.seeded import seeded_input
    from tests import ddp_ref
    from tests.test_train_engine_host_logic import INDICES, SHAPE
    x = seeded_input(SHAPE, 12).to(torch.bfloat16)
    count = {}
    with _emulated(count):
        a, b = _engine(), _engine()
        for e in (a, b):
            e.sample_generator, e.frame_indices = torch.Generator().manual_seed(5), INDICES
            e.master_weights()
        a.data_parallel(wide_gradients=True)
        for it in range(2):
            count.clear()
            la = a.training_step({"frames": x}, it)
            # the generator's list holds the loss's fp32 logvars beside the bf16 networks, the discriminator's is bf16 alone
            assert (count.get("mt_pack", 0), count["mt_pack_wide"]) == ((1, 1) if it == 0 else (0, 1)), count
            assert count["mt_adamw_master_wide"] == 1 and "mt_adamw_master" not in count
            lb = b.training_step({"frames": x}, it)
            a.on_train_batch_end()
            b.on_train_batch_end()
            assert torch.equal(la, lb) and bool(torch.isfinite(la))
            assert torch.equal(a.optimizers()[it].last_grad_norm, b.optimizers()[it].last_grad_norm)
            sync = a.gradient_sync(a.optimizers()[it])
            n16 = 0
            for p, o in zip(sync.params, sync.layout()):
                if p.dtype == torch.bfloat16 and getattr(p, "main_grad", None) is not None:
                    assert p.grad is None and p.main_grad.data_ptr() == sync.flat.data_ptr() + 4 * o
                    n16 += 1
            assert n16 > 10
            sa, sb = ddp_ref.engine_state(a), ddp_ref.engine_state(b)
            assert sorted(sa) == sorted(sb)
            bad = [k for k in sa if sa[k].dtype != sb[k].dtype or not torch.equal(sa[k], sb[k])]
            assert not bad, (it, len(bad), bad[:8])
