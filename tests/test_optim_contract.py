"""The contract of the update step (cvvae_amd/optim.py, lvdm/modules/ema.py, lvdm/lr_scheduler.py) that holds without a GPU: the C entry
points of csrc/optim_kernels.hip (exported, typed, declared, refusing bad arguments before any launch; ABI version unchanged), the
training loop's import paths without transformers / pytorch_lightning, the optimizer's constructor and the options that raise, the
schedules' closed forms, and LitEma's buffer names, state_dict keys and arithmetic."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn as nn

from oracle.ref_loader import REF_ROOT as REFERENCE
from tests import optim_ref as R

ENTRIES = ["cvvae_mt_workspace_bytes", "cvvae_mt_grad_norm", "cvvae_mt_scale", "cvvae_mt_adamw", "cvvae_mt_ema"]
EINVAL, EUNSUPPORTED = -1, -2


def test_entry_points_are_exported_with_prototypes_and_the_abi_version_stays():
    from cvvae_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "cvvae.h")).read()
    assert "#define CVVAE_ABI_VERSION 14" in header
    for n in ENTRIES:
        assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header, n
        assert getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1]
    assert f"#define CVVAE_MT_CHUNK {_lib.MT_CHUNK}" in header and _lib.MT_CHUNK % 2048 == 0
    assert ctypes.sizeof(_lib.MTChunk) == 16 and ctypes.sizeof(_lib.MTTensor) == 48
    assert _lib.MTTensor.step_size.offset == 40 and _lib.MTTensor.bias2_sqrt.offset == 44
    assert "optim_kernels.hip" in _lib.TRAINING_ONLY_SOURCES
    assert "optim_kernels.hip" in open(os.path.join(_lib._HERE, "csrc", "Makefile")).read()
    assert lib.cvvae_mt_workspace_bytes(0) >= 4 and lib.cvvae_mt_workspace_bytes(1000) == 4000 and lib.cvvae_mt_workspace_bytes(-1) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # a non-NULL (host) pointer: the checks below never dereference or launch
    hp = (4e-5, 0.9, 0.98, 1e-4, 0.01)
    for dt in (L.F16, L.BF16, L.F32Q, 9):   # only fp32 lists
        assert lib.cvvae_mt_grad_norm(dt, p, p, 1, 1.0, p, p, None) == EUNSUPPORTED
        assert lib.cvvae_mt_scale(dt, p, p, 1, p, None) == EUNSUPPORTED
        assert lib.cvvae_mt_adamw(dt, p, p, 1, *hp, None, None) == EUNSUPPORTED
        assert lib.cvvae_mt_ema(dt, p, p, 1, 1e-4, None) == EUNSUPPORTED
    assert lib.cvvae_mt_grad_norm(L.F32, None, p, 1, 1.0, p, p, None) == EINVAL
    assert lib.cvvae_mt_grad_norm(L.F32, p, None, 1, 1.0, p, p, None) == EINVAL
    assert lib.cvvae_mt_grad_norm(L.F32, p, p, 1, 1.0, None, p, None) == EINVAL
    assert lib.cvvae_mt_grad_norm(L.F32, p, p, 1, 1.0, p, None, None) == EINVAL
    assert lib.cvvae_mt_grad_norm(L.F32, p, p, -1, 1.0, p, p, None) == EINVAL
    assert lib.cvvae_mt_scale(L.F32, p, p, 1, None, None) == EINVAL                  # the device coefficient
    assert lib.cvvae_mt_scale(L.F32, None, p, 1, p, None) == EINVAL
    assert lib.cvvae_mt_adamw(L.F32, None, p, 1, *hp, None, None) == EINVAL
    assert lib.cvvae_mt_adamw(L.F32, p, None, 1, *hp, None, None) == EINVAL
    assert lib.cvvae_mt_adamw(L.F32, p, p, 1, -1.0, 0.9, 0.98, 1e-4, 0.01, None, None) == EINVAL
    assert lib.cvvae_mt_adamw(L.F32, p, p, 1, 4e-5, 1.0, 0.98, 1e-4, 0.01, None, None) == EINVAL
    assert lib.cvvae_mt_adamw(L.F32, p, p, 1, 4e-5, 0.9, float("nan"), 1e-4, 0.01, None, None) == EINVAL
    assert lib.cvvae_mt_ema(L.F32, None, p, 1, 1e-4, None) == EINVAL
    assert lib.cvvae_mt_ema(L.F32, p, p, 1 << 40, 1e-4, None) == EINVAL
    # an empty list is no error and no launch
    assert lib.cvvae_mt_scale(L.F32, None, None, 0, p, None) == 0
    assert lib.cvvae_mt_adamw(L.F32, None, None, 0, *hp, None, None) == 0
    assert lib.cvvae_mt_ema(L.F32, None, None, 0, 1e-4, None) == 0


def test_wrappers_have_no_cpu_path():
    from cvvae_amd import ops
    mtl = ops.MultiTensorList([5], "cpu").set(g=[torch.zeros(5)])
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mt_grad_norm(mtl, 1.0)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mt_ema(mtl, 0.1)


def test_chunk_table_partitions_every_tensor():
    from cvvae_amd import ops
    C = R.CHUNK
    numels = [0, 1, 7, C - 1, C, C + 1, 3 * C + 5]
    mtl = ops.MultiTensorList(numels, "cpu")
    rows = mtl.chunks.numpy().view([("start", "<i8"), ("tensor", "<i4"), ("n", "<i4")]).reshape(-1)
    assert mtl.n_chunks == len(rows) == 0 + 1 + 1 + 1 + 1 + 2 + 4
    seen = {}
    for r in rows:
        assert 0 < r["n"] <= C and r["start"] % C == 0 and r["start"] == seen.get(int(r["tensor"]), 0)
        seen[int(r["tensor"])] = int(r["start"] + r["n"])
    assert seen == {i: n for i, n in enumerate(numels) if n}
    assert list(rows["tensor"]) == sorted(rows["tensor"])
    assert ops.MultiTensorList([], "cpu").n_chunks == 0


def test_training_loop_imports_resolve_without_transformers_or_lightning(monkeypatch):
    for mod in ("transformers", "pytorch_lightning"):
        monkeypatch.setitem(sys.modules, mod, None)   # `import transformers` now raises ImportError
    for mod in ("lvdm.lr_scheduler", "lvdm.modules.ema", "cvvae_amd.optim"):
        monkeypatch.delitem(sys.modules, mod, raising=False)
    import importlib
    assert callable(importlib.import_module("lvdm.lr_scheduler").get_scheduler)
    assert issubclass(importlib.import_module("lvdm.modules.ema").LitEma, nn.Module)
    assert issubclass(importlib.import_module("cvvae_amd.optim").AdamW, torch.optim.AdamW)


def test_adamw_constructs_from_the_yaml_and_refuses_what_has_no_kernel(monkeypatch):
    from cvvae_amd.optim import AdamW
    net = nn.Linear(3, 2)
    opt = AdamW(net.parameters(), lr=R.YAML_LR, **R.YAML_ADAMW)
    assert isinstance(opt, torch.optim.AdamW) and opt.max_grad_norm is None and opt.last_grad_norm is None
    assert list(opt.defaults["betas"]) == [0.9, 0.98] and opt.defaults["eps"] == 1e-4 and opt.defaults["weight_decay"] == 0.01
    assert AdamW(net.parameters(), max_grad_norm=1.0).max_grad_norm == 1.0
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            AdamW(net.parameters(), max_grad_norm=bad)
    with pytest.raises(ValueError):
        AdamW(net.parameters(), lr=-1.0)                      # the base class's own checks stay
    # CPU parameters: every option the base class has is still served, by the base class
    for opt_name in ("amsgrad", "maximize", "capturable", "differentiable"):
        AdamW(net.parameters(), **{opt_name: True})
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))   # fp32 device parameters: the kernel path
    for opt_name in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=opt_name):
            AdamW(net.parameters(), **{opt_name: True})
    opt = AdamW(net.parameters())
    with pytest.raises(NotImplementedError):
        opt.add_param_group({"params": [nn.Parameter(torch.zeros(2))], "amsgrad": True})
    assert len(opt.param_groups) == 1
    AdamW(net.half().parameters(), amsgrad=True)              # 16-bit parameters never reach the kernels


def test_sparse_gradients_raise_as_torch_does(monkeypatch):
    from cvvae_amd.optim import AdamW
    p = nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.sparse_coo_tensor([[0], [1]], [1.0], (4, 3))
    for pretend in (False, True):
        if pretend:
            monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
        with pytest.raises(RuntimeError, match="sparse"):
            AdamW([p]).step()


def _cosine(s, W=1000, N=60000, r=0.005):
    if s < W:
        return s / max(1, W)
    return max(0.0, 0.5 * ((1 + r) + (1 - r) * math.cos(math.pi * (s - W) / max(1, N - W))))


def _multipliers(sched_args, steps):
    from lvdm.lr_scheduler import get_scheduler
    opt = torch.optim.SGD([nn.Parameter(torch.zeros(1))], lr=1.0)
    sch = get_scheduler(optimizer=opt, **sched_args)
    assert type(sch) is torch.optim.lr_scheduler.LambdaLR
    fn = sch.lr_lambdas[0]
    return [fn(s) for s in steps]


def test_scheduler_values_match_the_closed_forms():
    W, N = 1000, 60000
    steps = [0, 1, W - 1, W, (W + N) // 2, N, N + 10]
    got = _multipliers(R.YAML_COSINE, steps)
    for s, g in zip(steps, got):
        assert g == pytest.approx(_cosine(s), rel=1e-12, abs=1e-15), s
    assert got[0] == 0.0 and got[3] == 1.0 and got[4] == pytest.approx(0.5025) and got[5] == pytest.approx(0.005)
    assert _multipliers(dict(name="cosine", num_warmup_steps=0, num_training_steps=10), [0, 5, 10]) == pytest.approx([1.0, 0.5, 0.0], abs=1e-15)
    assert _multipliers(dict(name="constant"), steps) == [1.0] * len(steps)
    assert _multipliers(dict(name="constant_with_warmup", num_warmup_steps=W), [0, 1, W - 1, W, N]) == [0.0, 1 / W, (W - 1) / W, 1.0, 1.0]
    assert _multipliers(dict(name="linear", num_warmup_steps=W, num_training_steps=N), steps) == pytest.approx(
        [0.0, 1 / W, (W - 1) / W, 1.0, 0.5, 0.0, 0.0])


def test_scheduler_drives_the_optimizer_and_refuses_what_is_missing():
    from lvdm.lr_scheduler import get_scheduler
    from cvvae_amd.optim import AdamW
    p = nn.Parameter(torch.zeros(3))
    opt = AdamW([p], lr=R.YAML_LR, **R.YAML_ADAMW)
    sch = get_scheduler(optimizer=opt, **R.YAML_COSINE)
    assert opt.param_groups[0]["lr"] == 0.0
    p.grad = torch.ones(3)
    for s in (1, 2, 3):
        opt.step()
        sch.step()
        assert opt.param_groups[0]["lr"] == pytest.approx(R.YAML_LR * s / 1000)
    with pytest.raises(ValueError, match="num_warmup_steps"):
        get_scheduler("cosine", opt)
    with pytest.raises(ValueError, match="num_training_steps"):
        get_scheduler("cosine", opt, num_warmup_steps=10)
    with pytest.raises(ValueError, match="num_training_steps"):
        get_scheduler("linear", opt, num_warmup_steps=10)
    with pytest.raises(ValueError, match="num_warmup_steps"):
        get_scheduler("constant_with_warmup", opt)
    for name in ("polynomial", "cosine_with_restarts", "nope"):
        with pytest.raises(NotImplementedError):
            get_scheduler(name, opt, 10, 100)


class _Two(nn.Module):
    def __init__(self):
        super().__init__()
        self.block = nn.Sequential(nn.Linear(3, 4), nn.Linear(4, 2))
        self.head = nn.Linear(2, 2, bias=False)
        self.block[0].bias.requires_grad_(False)


def test_litema_buffer_names_and_state_dict_keys():
    from lvdm.modules.ema import LitEma
    net = _Two()
    ema = LitEma(net, decay=0.999)
    assert ema.m_name2s_name == {"block.0.weight": "block0weight", "block.1.weight": "block1weight", "block.1.bias": "block1bias",
                                 "head.weight": "headweight"}
    assert list(ema.state_dict().keys()) == ["decay", "num_updates", "block0weight", "block1weight", "block1bias", "headweight"]
    assert ema.decay.dtype == torch.float32 and ema.num_updates.dtype == torch.int32 and int(ema.num_updates) == 0
    assert int(LitEma(net, use_num_upates=False).num_updates) == -1
    for n, s in ema.m_name2s_name.items():
        assert torch.equal(getattr(ema, s), net.get_parameter(n)) and getattr(ema, s).data_ptr() != net.get_parameter(n).data_ptr()
    with pytest.raises(ValueError):
        LitEma(net, decay=1.5)
    # what cvvae_amd/checkpoint.py --ema reads: 'model_ema.' + the parameter's name without dots
    from cvvae_amd.checkpoint import extract_codec_state
    sd = {"model_ema." + k: v for k, v in ema.state_dict().items()}
    sd.update(net.state_dict())
    want = {n: p.shape for n, p in net.named_parameters() if p.requires_grad}
    out = extract_codec_state(sd, want, use_ema=True)
    assert set(out) == set(want)


def _drive(cls, net, updates, seed=3):
    gen = torch.Generator().manual_seed(seed)
    ema = cls(net, decay=0.9999)
    for _ in range(updates):
        with torch.no_grad():
            for p in net.parameters():
                if p.requires_grad:
                    p.add_(0.1 * torch.randn(p.shape, generator=gen))
        ema(net)
    return ema


def test_litema_follows_the_documented_arithmetic_and_survives_reload():
    from lvdm.modules.ema import LitEma
    torch.manual_seed(0)
    net = _Two()
    shadow = {n: p.detach().clone() for n, p in net.named_parameters() if p.requires_grad}
    gen = torch.Generator().manual_seed(3)
    ema = LitEma(net, decay=0.9999)
    for n_up in range(1, 13):
        with torch.no_grad():
            for p in net.parameters():
                if p.requires_grad:
                    p.add_(0.1 * torch.randn(p.shape, generator=gen))
        ema(net)
        decay = torch.minimum(torch.tensor(0.9999), torch.tensor(1 + n_up, dtype=torch.int32) / torch.tensor(10 + n_up, dtype=torch.int32))
        for n, p in net.named_parameters():
            if p.requires_grad:
                shadow[n].sub_((1.0 - decay) * (shadow[n] - p.detach()))
        if n_up == 5:   # a reload in the middle: the host mirror of num_updates is re-read
            other = LitEma(_Two())
            other.load_state_dict(ema.state_dict())
            ema = other
    assert int(ema.num_updates) == 12
    for n, s in ema.m_name2s_name.items():
        assert torch.equal(getattr(ema, s), shadow[n]), n
    ema.reset_num_updates()
    assert int(ema.num_updates) == 0
    before = ema.headweight.clone()
    ema(net)
    assert int(ema.num_updates) == 1                       # decay = 2 / 11 again, not 0.9999
    assert torch.allclose(ema.headweight, before - (1 - 2 / 11) * (before - net.head.weight.detach()), rtol=1e-6, atol=1e-7)


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "lvdm", "modules", "ema.py")), reason="needs the reference checkout")
def test_litema_agrees_with_the_reference_class_over_12_updates():
    import importlib.util
    from lvdm.modules.ema import LitEma
    spec = importlib.util.spec_from_file_location("_reference_ema", os.path.join(REFERENCE, "lvdm", "modules", "ema.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                            # pure torch
    torch.manual_seed(0)
    a, b = _Two(), _Two()
    b.load_state_dict(a.state_dict())
    ours, theirs = _drive(LitEma, a, 12), _drive(mod.LitEma, b, 12)
    assert ours.m_name2s_name == theirs.m_name2s_name
    assert list(ours.state_dict().keys()) == list(theirs.state_dict().keys())
    assert int(ours.num_updates) == int(theirs.num_updates) == 12 and torch.equal(ours.decay, theirs.decay)
    for k, v in theirs.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k
    # and the swap for validation
    ours.store(a.parameters())
    theirs.store(b.parameters())
    ours.copy_to(a)
    theirs.copy_to(b)
    assert all(torch.equal(x, y) for x, y in zip(a.parameters(), b.parameters()))
    ours.restore(a.parameters())
    theirs.restore(b.parameters())
    assert all(torch.equal(x, y) for x, y in zip(a.parameters(), b.parameters()))
    assert all(p.is_leaf for p in a.parameters())
