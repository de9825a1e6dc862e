"""16-bit parameters on fp32 master weights, what holds without a GPU: the C entry points (cvvae_mt_adamw_master, cvvae_mt_sumsq,
cvvae_mt_norm_finish: exported, typed, declared, refusing bad arguments before any launch, ABI still 14), the stall that motivates the
feature and its cure, cvvae_amd.optim.AdamW(master_weights=True)'s state, seeds, state dict and version counters on the emulated
kernels (tests/master_ref.py), and the one norm over a list of mixed dtypes.

The stall.  lr 4e-5, betas (0.9, 0.98), eps 1e-4, weight decay 0.01, a constant gradient 0.5: one step moves a weight of size 1 by
about 4e-5, half a bf16 ulp at 1.0 is 3.9e-3, so torch.optim.AdamW on a bf16 parameter leaves it at exactly 1.0 after 400 steps, where
the fp32 run stands at 0.98383522.  With master weights p must be round_bf16(master) = 0.984375 exactly (the nearest rounding boundary
is 1.4e-3 from the fp32 value) and the master within 1e-4 of the fp32 run: 400 steps x 3 x (ulp(1) + 2^-20 x 4e-5), the per-step bound
3 (ulp(|p|) + 2^-20 |delta|) of tests/test_gpu_optim.py with fp32's ulp of 2^-24 just below 1, where the weight lives from the first
step on: 400 x 3 x (5.96e-8 + 3.8e-11) = 7.2e-5, rounded up to 1e-4."""
import copy
import ctypes
import os

import pytest
import torch
import torch.nn as nn

from tests import master_ref as M
from tests import optim_ref as R

EINVAL, EUNSUPPORTED = -1, -2
NEW = ["cvvae_mt_adamw_master", "cvvae_mt_sumsq", "cvvae_mt_norm_finish"]
HP = dict(lr=R.YAML_LR, **R.YAML_ADAMW)


def test_the_three_entry_points_are_exported_typed_and_declared_and_the_abi_is_still_14():
    from cvvae_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "cvvae.h")).read()
    assert "#define CVVAE_ABI_VERSION 14" in header
    for n in NEW:
        assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header, n
        assert getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1]
    assert ctypes.sizeof(_lib.MTTensor) == 48 and _lib.MTTensor.shadow.offset == 32      # the struct keeps its layout
    from cvvae_amd import ops
    for n in ("mt_adamw_master", "mt_sumsq", "mt_norm_finish"):
        assert callable(getattr(ops, n))


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL (host) pointer: the checks below never dereference or launch
    hp = (4e-5, 0.9, 0.98, 1e-4, 0.01)
    for dt in (L.F32, L.F32Q, 9):
        assert lib.cvvae_mt_adamw_master(dt, p, p, 1, *hp, None, None) == EUNSUPPORTED
    for dt in (L.F32Q, 9):
        assert lib.cvvae_mt_sumsq(dt, p, p, 1, p, None) == EUNSUPPORTED
    for dt in (L.BF16, L.F16):
        assert lib.cvvae_mt_adamw_master(dt, None, p, 1, *hp, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master(dt, p, None, 1, *hp, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master(dt, p, p, -1, *hp, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master(dt, p, p, 1 << 40, *hp, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master(dt, p, p, 1, -1.0, 0.9, 0.98, 1e-4, 0.01, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master(dt, p, p, 1, 4e-5, 1.0, 0.98, 1e-4, 0.01, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master(dt, p, p, 1, 4e-5, 0.9, float("nan"), 1e-4, 0.01, None, None) == EINVAL
        assert lib.cvvae_mt_adamw_master(dt, None, None, 0, *hp, None, None) == 0          # an empty list: no error, no launch
    for dt in (L.F32, L.BF16, L.F16):
        assert lib.cvvae_mt_sumsq(dt, None, p, 1, p, None) == EINVAL
        assert lib.cvvae_mt_sumsq(dt, p, None, 1, p, None) == EINVAL
        assert lib.cvvae_mt_sumsq(dt, p, p, 1, None, None) == EINVAL
        assert lib.cvvae_mt_sumsq(dt, p, p, -1, p, None) == EINVAL
        assert lib.cvvae_mt_sumsq(dt, None, None, 0, p, None) == 0
    assert lib.cvvae_mt_norm_finish(None, 1, 1.0, p, None) == EINVAL
    assert lib.cvvae_mt_norm_finish(p, 1, 1.0, None, None) == EINVAL
    assert lib.cvvae_mt_norm_finish(p, -1, 1.0, p, None) == EINVAL
    assert lib.cvvae_mt_norm_finish(p, 1 << 40, 1.0, p, None) == EINVAL


def test_the_wrappers_have_no_cpu_path():
    from cvvae_amd import ops
    mtl = ops.MultiTensorList([5], "cpu", torch.bfloat16)
    z16, z32 = torch.zeros(5, dtype=torch.bfloat16), torch.zeros(5)
    mtl.set(g=[z16], p=[z16.clone()], m=[z32], v=[z32.clone()], shadow=[z32.clone()], step_size=[1.0], bias2_sqrt=[1.0])
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mt_adamw_master(mtl, 4e-5, 0.9, 0.98, 1e-4, 0.01)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mt_sumsq(mtl, torch.zeros(1))
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mt_norm_finish(torch.zeros(1), 1.0)


def _constant_gradient_run(opt, p, steps, grad):
    for _ in range(steps):
        p.grad = torch.full_like(p, grad)
        opt.step()


def test_a_bf16_parameter_stalls_under_torchs_step_and_learns_on_master_weights(monkeypatch):
    from cvvae_amd.optim import AdamW
    S = M.STALL
    # the parent's behaviour: torch's step, and ours without the keyword, leave the bf16 weights at exactly 1.0
    for cls in (torch.optim.AdamW, AdamW):
        p = nn.Parameter(torch.full((S["n"],), S["start"], dtype=torch.bfloat16))
        _constant_gradient_run(cls([p], **HP), p, S["steps"], S["grad"])
        assert bool((p.detach() == 1.0).all()), cls
    # fp32, the yardstick
    q = nn.Parameter(torch.full((S["n"],), S["start"]))
    _constant_gradient_run(torch.optim.AdamW([q], **HP), q, S["steps"], S["grad"])
    assert abs(float(q.detach()[0]) - S["fp32_end"]) < 1e-6 and float(q.detach().bfloat16()[0]) == S["bf16_end"]
    # master weights on the emulated kernels
    count = {}
    M.pretend_gpu(monkeypatch, count)
    p = nn.Parameter(torch.full((S["n"],), S["start"], dtype=torch.bfloat16))
    opt = AdamW([p], master_weights=True, **HP)
    _constant_gradient_run(opt, p, S["steps"], S["grad"])
    assert count == {"mt_adamw_master": S["steps"]}
    master = opt.master(p)
    print(f"after {S['steps']} steps: p {float(p.detach()[0])}, master {float(master[0])!r}, fp32 torch {float(q.detach()[0])!r}, "
          f"|master - fp32| {float((master - q.detach()).abs().max()):.3e}")
    assert p.dtype == torch.bfloat16 and bool((p.detach().float() == S["bf16_end"]).all())
    assert master.dtype == torch.float32 and float((master - q.detach()).abs().max()) <= 1e-4


def _mixed(dtype=torch.bfloat16, seed=0):
    """one group: fp32, 16-bit, 16-bit without a gradient, fp32 0-dim, 16-bit larger than a chunk"""
    gen = torch.Generator().manual_seed(seed)
    shapes = [((5, 3), torch.float32, True), ((7,), dtype, True), ((4,), dtype, False), ((), torch.float32, True),
              ((R.CHUNK + 9,), dtype, True)]
    params = []
    for shape, dt, has_grad in shapes:
        p = nn.Parameter(torch.randn(shape, generator=gen).to(dt))
        if has_grad:
            p.grad = (0.5 * torch.randn(shape, generator=gen)).to(dt)
        params.append(p)
    return params


@pytest.mark.parametrize("dtype", M.DTYPES16, ids=["bf16", "fp16"])
def test_state_dtypes_seeds_lookup_and_version_counters(monkeypatch, dtype):
    from cvvae_amd.optim import AdamW
    count = {}
    M.pretend_gpu(monkeypatch, count)
    params = _mixed(dtype)
    opt = AdamW(params, max_grad_norm=1.0, master_weights=True, **HP)
    seed = params[1].detach().float() + 1e-4        # not representable in 16 bits: the seed, not p.float(), must be the master
    opt.seed_master(params[1], seed)
    assert opt.master(params[1]) is seed and opt.master(params[4]) is None and opt.master(params[0]) is None
    with pytest.raises(ValueError):
        opt.seed_master(params[4], torch.zeros(3))
    with pytest.raises(ValueError):
        opt.seed_master(params[4], params[4].detach().clone())       # 16-bit
    before, seed0 = [p.detach().clone() for p in params], seed.clone()
    p4_float = params[4].detach().float()
    versions = [p._version for p in params]
    opt.step()
    assert count == {"mt_sumsq": 2, "mt_norm_finish": 1, "mt_adamw": 1, "mt_adamw_master": 1}
    assert opt.last_grad_norm.shape == () and opt.last_grad_norm.dtype == torch.float32
    for i, p in enumerate(params):
        if p.grad is None:
            assert p not in opt.state and p._version == versions[i] and torch.equal(p, before[i])
            continue
        st = opt.state[p]
        assert p._version > versions[i]
        # what moved: the fp32 value (one step of 4e-5 is below the 16-bit spacing: a 16-bit p may stand)
        start = seed0 if i == 1 else before[i].float()
        assert not torch.equal(st["master"] if p.dtype == dtype else p.detach(), start)
        assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and st["step"].dim() == 0 and float(st["step"]) == 1.0
        assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32 and st["exp_avg"].shape == p.shape
        if p.dtype == dtype:
            assert sorted(st) == ["exp_avg", "exp_avg_sq", "master", "step"]
            assert st["master"].dtype == torch.float32 and opt.master(p) is st["master"]
            assert torch.equal(p.detach(), st["master"].to(dtype))
        else:
            assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and opt.master(p) is None
    assert opt.state[params[1]]["master"] is seed                     # the seed itself, updated in place: no copy
    with pytest.raises(RuntimeError):
        opt.seed_master(params[1], seed.clone())                      # after the first step
    # the unseeded master started from p.float(): one step of the documented arithmetic from there
    coef = min(1.0, 1.0 / (float(opt.last_grad_norm) + 1e-6))
    lone = R.adamw64(params[4].grad.float(), p4_float, torch.zeros_like(p4_float), torch.zeros_like(p4_float), 1, HP["lr"], *HP["betas"],
                     HP["eps"], HP["weight_decay"], coef)[2]
    assert float((opt.master(params[4]).double() - lone).abs().max()) < 1e-6
    # without the keyword the lookup and the seeds are refused / empty
    plain = AdamW(_mixed(dtype), **HP)
    assert plain.master(plain.param_groups[0]["params"][1]) is None
    with pytest.raises(RuntimeError):
        plain.seed_master(plain.param_groups[0]["params"][1], seed)


@pytest.mark.parametrize("dtype", M.DTYPES16, ids=["bf16", "fp16"])
def test_without_the_keyword_a_16_bit_group_is_torchs_step_bit_for_bit(monkeypatch, dtype):
    from cvvae_amd.optim import AdamW
    count = {}
    M.pretend_gpu(monkeypatch, count)
    ours, theirs = [[p for p in _mixed(dtype) if p.dtype == dtype] for _ in range(2)]
    a, b = AdamW(ours, **HP), torch.optim.AdamW(theirs, **HP)
    for _ in range(3):
        a.step()
        b.step()
    assert count == {}
    for p, q in zip(ours, theirs):
        assert torch.equal(p, q)
        for k in a.state.get(p, {}):
            assert a.state[p][k].dtype == b.state[q][k].dtype and torch.equal(a.state[p][k], b.state[q][k]), k
    assert "master" not in a.state[ours[0]] and a.state[ours[0]]["exp_avg"].dtype == dtype


def test_refused_options_cover_16_bit_device_parameters_with_the_keyword(monkeypatch):
    from cvvae_amd.optim import AdamW
    half = [nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))]
    for name in ("amsgrad", "maximize", "capturable", "differentiable"):
        AdamW(half, master_weights=True, **{name: True})             # CPU parameters: the base class serves them
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for name in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=name):
            AdamW(half, master_weights=True, **{name: True})
        AdamW(half, **{name: True})                                   # without the keyword: torch's path, as before
    import inspect
    assert inspect.signature(AdamW).parameters["master_weights"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(AdamW).parameters["master_weights"].default is False


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_state_dict_round_trips_fp32_bit_for_bit_and_p_follows_the_master(monkeypatch):
    from cvvae_amd.optim import AdamW
    M.pretend_gpu(monkeypatch)
    params = _mixed()
    opt = AdamW(params, max_grad_norm=1.0, master_weights=True, **HP)
    for _ in range(3):
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert sorted(sd["state"]) == [0, 1, 3, 4]
    for i in (1, 4):
        assert all(sd["state"][i][k].dtype == torch.float32 for k in ("exp_avg", "exp_avg_sq", "master"))
        assert not torch.equal(sd["state"][i]["master"], sd["state"][i]["master"].bfloat16().float())   # bits a cast would lose
    fresh = _mixed(seed=1)                                              # other weights: the load must overwrite the 16-bit ones
    other = AdamW(fresh, max_grad_norm=1.0, master_weights=True, **HP)
    versions = [p._version for p in fresh]
    other.load_state_dict(sd)
    for i, p in enumerate(fresh):
        if i not in sd["state"]:
            continue
        for k, v in sd["state"][i].items():
            got = other.state[p][k]
            assert got.dtype == v.dtype and torch.equal(_bits(got) if v.dim() else got, _bits(v) if v.dim() else v), (i, k)
        if p.dtype == torch.bfloat16:
            assert torch.equal(p.detach(), other.master(p).to(torch.bfloat16)) and p._version > versions[i]
            assert torch.equal(p.detach(), params[i].detach())
    again = other.state_dict()
    for i in sd["state"]:
        for k, v in sd["state"][i].items():
            assert torch.equal(again["state"][i][k], v)
    # both continue identically
    for p, q in zip(params, fresh):
        if p.grad is not None:
            q.grad = p.grad.clone()
        if p.dtype == torch.float32:
            q.data.copy_(p.data)
    opt.step()
    other.step()
    for p, q in zip(params, fresh):
        assert p.grad is None or torch.equal(p, q)


def test_a_plain_torch_adamw_state_dict_loads(monkeypatch):
    from cvvae_amd.optim import AdamW
    theirs = [p for p in _mixed() if p.dtype == torch.bfloat16]
    t_opt = torch.optim.AdamW(theirs, **HP)
    for _ in range(2):
        t_opt.step()
    sd = copy.deepcopy(t_opt.state_dict())
    assert sd["state"][0]["exp_avg"].dtype == torch.bfloat16
    M.pretend_gpu(monkeypatch)
    ours = [p for p in _mixed() if p.dtype == torch.bfloat16]
    for p, q in zip(ours, theirs):
        p.data.copy_(q.data)
    opt = AdamW(ours, master_weights=True, **HP)
    opt.load_state_dict(sd)
    for i, p in enumerate(ours):
        if i not in sd["state"]:
            assert p not in opt.state
            continue
        st = opt.state[p]
        assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == st["master"].dtype == torch.float32
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"].float()) and torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"].float())
        assert torch.equal(st["master"], theirs[i].detach().float()) and torch.equal(p.detach(), st["master"].bfloat16())
        assert float(st["step"]) == 2.0 and st["step"].dtype == torch.float32
    opt.step()
    assert float(opt.state[ours[0]]["step"]) == 3.0


def test_one_norm_over_the_mixed_list_fp32_partials_first(monkeypatch):
    from cvvae_amd.optim import AdamW
    calls = []
    M.pretend_gpu(monkeypatch, calls=calls)
    gen = torch.Generator().manual_seed(4)
    spec = [(torch.bfloat16, 7), (torch.float32, R.CHUNK + 3), (torch.float16, 5), (torch.bfloat16, 2 * R.CHUNK), (torch.float32, 1)]
    params = []
    for dt, n in spec:
        p = nn.Parameter(torch.randn(n, generator=gen).to(dt))
        p.grad = torch.randn(n, generator=gen).to(dt)
        params.append(p)
    opt = AdamW(params, max_grad_norm=1.0, master_weights=True, **HP)
    opt.step()
    names = [n for n, _ in calls]
    assert names == ["mt_sumsq", "mt_sumsq", "mt_sumsq", "mt_norm_finish", "mt_adamw_master", "mt_adamw_master"]
    lists = [a[0] for n, a in calls if n == "mt_sumsq"]
    assert [m.dtype for m in lists] == [torch.float32, torch.bfloat16, torch.float16]
    assert [m.n_chunks for m in lists] == [3, 3, 1]
    slices = [a[1] for n, a in calls if n == "mt_sumsq"]
    partials = calls[3][1][0]
    assert partials.numel() == 7 and partials.dtype == torch.float32
    at = 0
    for m, s in zip(lists, slices):      # side by side in ONE workspace, fp32 first
        assert s.data_ptr() == partials.data_ptr() + 4 * at and s.numel() == m.n_chunks
        at += m.n_chunks
    want = [float((g.float() ** 2).sum()) for g in (params[1].grad[:R.CHUNK], params[1].grad[R.CHUNK:], params[4].grad, params[0].grad,
                                                    params[3].grad[:R.CHUNK], params[3].grad[R.CHUNK:], params[2].grad)]
    assert partials.tolist() == pytest.approx(want, rel=1e-6)
    # the coefficient: torch's clip_grad_norm_ on float copies, within the norm's existing bound (tests/test_gpu_optim.py: 1e-5 relative)
    copies = [nn.Parameter(p.detach().float()) for p in params]
    for c, p in zip(copies, params):
        c.grad = p.grad.float().clone()
    t_norm = torch.nn.utils.clip_grad_norm_(copies, 1.0)
    assert float(t_norm) > 1.0
    assert float(opt.last_grad_norm) == pytest.approx(float(t_norm), rel=1e-5)
    coef = calls[4][1][-1]
    assert coef.numel() == 1 and float(coef) == pytest.approx(1.0 / (float(t_norm) + 1e-6), rel=1e-5)
    assert float(calls[5][1][-1]) == float(coef)
    # an all-fp32 list keeps the one-call norm
    calls.clear()
    count = {}
    M.pretend_gpu(monkeypatch, count)
    q = nn.Parameter(torch.ones(3))
    q.grad = torch.ones(3)
    AdamW([q], max_grad_norm=1.0, master_weights=True, **HP).step()
    assert count == {"mt_grad_norm": 1, "mt_adamw": 1}


def test_the_stand_alone_clip_keeps_sending_16_bit_gradients_to_torch(monkeypatch):
    from cvvae_amd.optim import clip_grad_norm_
    count = {}
    M.pretend_gpu(monkeypatch, count)
    p = nn.Parameter(torch.ones(8, dtype=torch.bfloat16))
    p.grad = torch.full((8,), 2.0, dtype=torch.bfloat16)
    q = nn.Parameter(torch.ones(8, dtype=torch.bfloat16))
    q.grad = p.grad.clone()
    assert torch.equal(clip_grad_norm_([p], 1.0), torch.nn.utils.clip_grad_norm_([q], 1.0)) and torch.equal(p.grad, q.grad)
    assert count == {}
