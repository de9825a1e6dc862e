"""The host side of the update step on a CPU: the four cvvae_amd.ops.mt_* launches are replaced by fp32 torch emulations of the
arithmetic include/cvvae.h documents (tests/optim_ref.py) and CPU tensors pretend to be device tensors, so everything around the
kernels -- torch's state and state_dict, per-tensor step counts inside one launch, the scheduler, the clip coefficient's route, the
version counters and the pointer-table uploads -- runs as it does on the GPU.  Tolerance: 1e-6 relative on parameters and moments
(fp32 against fp32 with the operations in another order)."""
import copy

import pytest
import torch
import torch.nn as nn

from tests import optim_ref as R

TOL = 1e-6


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(6, 5)
        self.b = nn.Linear(5, 4)
        self.late = nn.Parameter(torch.ones(4))            # no gradient in the first two steps
        self.logvar = nn.Parameter(torch.zeros(()))        # 0-dim, as the loss's logvar
        self.unused = nn.Parameter(torch.ones(3))          # never gets a gradient

    def loss(self, x, step):
        y = self.b(torch.tanh(self.a(x)))
        if step >= 2:
            y = y * self.late
        return (y.pow(2).mean() / self.logvar.exp() + self.logvar) * 30.0


def _pair(seed=0):
    torch.manual_seed(seed)
    a = _Net()
    b = copy.deepcopy(a)
    return a, b


def _groups(net):
    return [dict(params=[net.a.weight, net.a.bias, net.late, net.unused]),
            dict(params=[net.b.weight, net.b.bias, net.logvar], lr=3e-3, weight_decay=0.1)]


def _same(ours, theirs, o_opt, t_opt):
    for (n, p), q in zip(ours.named_parameters(), theirs.parameters()):
        assert _rel(p, q) <= TOL, (n, _rel(p, q))
        assert (p in o_opt.state) == (q in t_opt.state), n
        if p in o_opt.state:
            so, st = o_opt.state[p], t_opt.state[q]
            assert set(so) == set(st) == {"step", "exp_avg", "exp_avg_sq"}
            assert so["step"].device.type == "cpu" and so["step"].dtype == torch.float32 and so["step"].dim() == 0
            assert float(so["step"]) == float(st["step"]), n
            assert _rel(so["exp_avg"], st["exp_avg"]) <= TOL and _rel(so["exp_avg_sq"], st["exp_avg_sq"]) <= TOL, n


def _run(steps, ours, theirs, o_opt, t_opt, x, first=0, o_sch=None, t_sch=None, clip=None):
    for s in range(first, first + steps):
        for net, opt, sch in ((ours, o_opt, o_sch), (theirs, t_opt, t_sch)):
            opt.zero_grad(set_to_none=True)
            net.loss(x, s).backward()
            if clip is not None and opt is t_opt:
                torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
            opt.step()
            if sch is not None:
                sch.step()


def test_five_steps_match_torch_with_two_groups_a_scheduler_and_a_late_parameter(monkeypatch):
    from cvvae_amd.optim import AdamW
    ours, theirs = _pair()
    count = {}
    R.pretend_gpu(monkeypatch, count)
    x = torch.randn(7, 6)
    o_opt = AdamW(_groups(ours), lr=1e-2, **R.YAML_ADAMW)
    t_opt = torch.optim.AdamW(_groups(theirs), lr=1e-2, **R.YAML_ADAMW)
    lam = lambda s: 1.0 / (1 + s)  # noqa: E731
    o_sch, t_sch = (torch.optim.lr_scheduler.LambdaLR(o, [lam, lambda s: 0.5 ** s]) for o in (o_opt, t_opt))
    _run(5, ours, theirs, o_opt, t_opt, x, o_sch=o_sch, t_sch=t_sch)
    _same(ours, theirs, o_opt, t_opt)
    assert count == {"mt_adamw": 2 * 5}                                    # one launch per group and step, no clip
    assert float(o_opt.state[ours.late]["step"]) == 3 and float(o_opt.state[ours.a.weight]["step"]) == 5   # lagging inside one launch
    assert ours.unused not in o_opt.state and torch.equal(ours.unused, torch.ones(3))
    assert o_opt.state[ours.logvar]["exp_avg"].shape == ()
    assert o_opt.param_groups[0]["lr"] == t_opt.param_groups[0]["lr"] != 1e-2
    assert not torch.equal(ours.logvar.detach(), torch.zeros(()))


def test_state_dict_goes_into_torch_and_back_after_step_3(monkeypatch):
    from cvvae_amd.optim import AdamW
    ours, theirs = _pair(1)
    R.pretend_gpu(monkeypatch)
    x = torch.randn(7, 6)
    o_opt = AdamW(_groups(ours), lr=1e-2, **R.YAML_ADAMW)
    t_opt = torch.optim.AdamW(_groups(theirs), lr=1e-2, **R.YAML_ADAMW)
    _run(3, ours, theirs, o_opt, t_opt, x)
    # swap the optimizers' states: ours continues from torch's state_dict and torch from ours
    sd_o, sd_t = copy.deepcopy(o_opt.state_dict()), copy.deepcopy(t_opt.state_dict())
    assert sd_o["param_groups"][0].keys() == sd_t["param_groups"][0].keys() and sd_o["state"].keys() == sd_t["state"].keys()
    o_opt2 = AdamW(_groups(ours), lr=1e-2, **R.YAML_ADAMW)
    t_opt2 = torch.optim.AdamW(_groups(theirs), lr=1e-2, **R.YAML_ADAMW)
    o_opt2.load_state_dict(sd_t)
    t_opt2.load_state_dict(sd_o)
    _run(2, ours, theirs, o_opt2, t_opt2, x, first=3)
    _same(ours, theirs, o_opt2, t_opt2)
    assert float(o_opt2.state[ours.a.weight]["step"]) == 5 and float(o_opt2.state[ours.late]["step"]) == 3


def test_max_grad_norm_matches_clip_then_step_and_leaves_gradients_unscaled(monkeypatch):
    from cvvae_amd.optim import AdamW
    ours, theirs = _pair(2)
    count = {}
    R.pretend_gpu(monkeypatch, count)
    x = torch.randn(7, 6) * 3
    o_opt = AdamW(_groups(ours), lr=1e-2, max_grad_norm=1.0, **R.YAML_ADAMW)
    t_opt = torch.optim.AdamW(_groups(theirs), lr=1e-2, **R.YAML_ADAMW)
    _run(1, ours, theirs, o_opt, t_opt, x, first=2, clip=1.0)
    raw = [p.grad.clone() for p in ours.parameters() if p.grad is not None]
    total = torch.stack([g.norm() for g in raw]).norm()
    assert float(total) > 1.0                                              # the clip is active
    assert o_opt.last_grad_norm.shape == () and float(o_opt.last_grad_norm) == pytest.approx(float(total), rel=1e-6)
    _run(3, ours, theirs, o_opt, t_opt, x, first=3, clip=1.0)
    _same(ours, theirs, o_opt, t_opt)
    assert count == {"mt_grad_norm": 4, "mt_adamw": 8}                     # one norm over BOTH groups per step; no scale sweep
    scaled = [p.grad for p in theirs.parameters() if p.grad is not None]
    mine = [p.grad for p in ours.parameters() if p.grad is not None]
    assert any(not torch.allclose(a, b) for a, b in zip(mine, scaled))    # ours are what backward wrote


def test_clip_grad_norm_scales_in_place_and_returns_the_norm(monkeypatch):
    from cvvae_amd import optim
    ours, theirs = _pair(3)
    x = torch.randn(7, 6) * 3
    for net in (ours, theirs):
        net.loss(x, 5).backward()
    want = torch.nn.utils.clip_grad_norm_(theirs.parameters(), 0.5)
    count = {}
    R.pretend_gpu(monkeypatch, count)
    got = optim.clip_grad_norm_(ours.parameters(), 0.5)
    assert count == {"mt_grad_norm": 1, "mt_scale": 1}
    assert got.shape == () and float(got) == pytest.approx(float(want), rel=1e-6)
    for p, q in zip(ours.parameters(), theirs.parameters()):
        assert (p.grad is None) == (q.grad is None)
        if p.grad is not None:
            assert _rel(p.grad, q.grad) <= TOL
    # norm types the kernels do not have go to torch
    n_inf = optim.clip_grad_norm_(ours.parameters(), 0.5, norm_type=float("inf"))
    assert count == {"mt_grad_norm": 1, "mt_scale": 1} and float(n_inf) == float(max(p.grad.abs().max() for p in ours.parameters() if p.grad is not None))


def test_groups_the_kernels_do_not_take_run_torchs_own_step(monkeypatch):
    from cvvae_amd.optim import AdamW
    ours, theirs = _pair(4)
    x = torch.randn(7, 6)
    o_opt = AdamW(_groups(ours), lr=1e-2, max_grad_norm=1.0, **R.YAML_ADAMW)       # CPU tensors, no pretending: torch's path
    t_opt = torch.optim.AdamW(_groups(theirs), lr=1e-2, **R.YAML_ADAMW)
    from cvvae_amd import ops
    monkeypatch.setattr(ops, "mt_adamw", lambda *a, **k: pytest.fail("CPU tensors must not reach the kernels"))
    _run(3, ours, theirs, o_opt, t_opt, x, first=1, clip=1.0)
    for p, q in zip(ours.parameters(), theirs.parameters()):
        assert torch.equal(p, q)
    assert float(o_opt.last_grad_norm) > 0


def test_versions_move_on_step_copy_to_and_restore(monkeypatch):
    from cvvae_amd.optim import AdamW
    from lvdm.modules.ema import LitEma
    net, _ = _pair(5)
    net.unused.requires_grad_(False)
    count = {}
    R.pretend_gpu(monkeypatch, count)
    opt = AdamW(net.parameters(), lr=1e-2, **R.YAML_ADAMW)
    ema = LitEma(net, decay=0.5, use_num_upates=False)
    net.loss(torch.randn(7, 6), 0).backward()
    updated = [p for p in net.parameters() if p.grad is not None]
    idle = [p for p in net.parameters() if p.grad is None]
    assert {id(net.late), id(net.unused)} == {id(p) for p in idle}
    v0 = {p: p._version for p in net.parameters()}
    opt.step()
    assert all(p._version > v0[p] for p in updated) and all(p._version == v0[p] for p in idle)
    # EMA: one launch over every trainable parameter
    live = {n: p.detach().clone() for n, p in net.named_parameters()}
    ema(net)
    assert count["mt_ema"] == 1
    for n, s in ema.m_name2s_name.items():
        assert not hasattr(ema, "unused") and n != "unused"
        moved = not torch.equal(live[n], getattr(ema, s))
        assert moved == any(net.get_parameter(n) is p for p in updated), n
    trainable = [p for p in net.parameters() if p.requires_grad]
    v1 = {p: p._version for p in net.parameters()}
    ema.store(net.parameters())
    ema.copy_to(net)
    assert all(p._version > v1[p] for p in trainable) and net.unused._version == v1[net.unused]
    assert all(torch.equal(net.get_parameter(n), getattr(ema, s)) for n, s in ema.m_name2s_name.items())
    v2 = {p: p._version for p in net.parameters()}
    ema.restore(net.parameters())
    assert all(p._version > v2[p] for p in net.parameters())
    assert all(torch.equal(p, live[n]) and p.is_leaf and p.grad_fn is None for n, p in net.named_parameters())


def test_pointer_table_is_uploaded_only_when_a_pointer_moved(monkeypatch):
    from cvvae_amd import ops
    from cvvae_amd.optim import AdamW
    net, _ = _pair(6)
    R.pretend_gpu(monkeypatch)
    uploads = []
    real = ops.MultiTensorList._upload
    monkeypatch.setattr(ops.MultiTensorList, "_upload", lambda self, img: (uploads.append(self), real(self, img))[1])
    # the per-tensor scalars sit in the same table and move with every step count: pin them to look at the pointers alone
    monkeypatch.setattr(ops.MultiTensorList, "set", _set_without_scalars(ops.MultiTensorList.set))
    opt = AdamW(net.parameters(), lr=1e-2, **R.YAML_ADAMW)
    x = torch.randn(7, 6)
    net.loss(x, 5).backward()
    opt.step()
    assert len(uploads) == 1
    lists = list(opt._lists.d.values())
    assert len(lists) == 1 and lists[0].uploads == 1
    opt.step()                                               # the same gradient tensors, the same p / m / v: nothing to upload
    opt.zero_grad(set_to_none=False)                         # zeroed in place: the pointers stay
    opt.step()
    assert len(uploads) == 1
    held = [p.grad for p in net.parameters()]                # (kept alive, so that no fresh gradient lands on a freed one's address)
    opt.zero_grad(set_to_none=True)
    net.loss(x, 5).backward()                                # fresh gradient tensors
    opt.step()
    assert len(uploads) == 2 and lists[0].uploads == 2 and list(opt._lists.d.values()) == lists
    del held
    # EMA: p and shadow pointers never move
    from lvdm.modules.ema import LitEma
    ema = LitEma(net)
    for _ in range(3):
        ema(net)
    assert ema._list[1].uploads == 1


def _set_without_scalars(real):
    def set_(self, step_size=None, bias2_sqrt=None, **fields):
        n = self.n_tensors
        return real(self, step_size=[1.0] * n if step_size is not None else None, bias2_sqrt=[1.0] * n, **fields)
    return set_
