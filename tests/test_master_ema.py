"""lvdm.modules.ema.LitEma(fp32_shadows=True) without a GPU: fp32 shadows of 16-bit parameters (from p.float() or from the mapping given
to the constructor) that stay fp32, with `decay`, through .to(bfloat16) / .half(); the update reading the masters a callable hands
it; the documented arithmetic over 12 updates, in fp32, where a bf16 shadow stands still; unchanged names and keys."""
import pytest
import torch
import torch.nn as nn

from tests import master_ref as M


class _Two(nn.Module):   # tests/test_optim_contract.py's, with a parameter that stays fp32 beside the 16-bit ones
    def __init__(self):
        super().__init__()
        self.block = nn.Sequential(nn.Linear(3, 4), nn.Linear(4, 2))
        self.head = nn.Linear(2, 2, bias=False)
        self.block[0].bias.requires_grad_(False)
        self.to(torch.bfloat16)
        self.logvar = nn.Parameter(torch.zeros(()))


KEYS = ["decay", "num_updates", "logvar", "block0weight", "block1weight", "block1bias", "headweight"]


def test_shadows_are_fp32_keep_names_and_keys_and_survive_casts():
    from lvdm.modules.ema import LitEma
    torch.manual_seed(0)
    net = _Two()
    plain = LitEma(net, decay=0.9999)
    assert plain.block0weight.dtype == torch.bfloat16 and float(plain.to(torch.bfloat16).decay) == 1.0    # what the keyword is for
    masters = {net.head.weight: torch.randn(2, 2)}
    ema = LitEma(net, 0.9999, True, fp32_shadows=True, masters=masters)
    assert list(ema.state_dict().keys()) == KEYS == list(LitEma(net).state_dict().keys())
    assert ema.m_name2s_name == plain.m_name2s_name
    for n, s in ema.m_name2s_name.items():
        shadow, p = getattr(ema, s), net.get_parameter(n)
        assert shadow.dtype == torch.float32 and shadow.shape == p.shape
        if p in masters:
            assert torch.equal(shadow, masters[p]) and shadow.data_ptr() != masters[p].data_ptr()
        else:
            assert torch.equal(shadow, p.detach().float())
    with pytest.raises(TypeError):
        LitEma(net, 0.9999, True, True)                       # keyword-only
    kept = {k: v.clone() for k, v in ema.state_dict().items()}
    for cast in (lambda m: m.to(torch.bfloat16), lambda m: m.half(), lambda m: m.to("cpu", torch.bfloat16), lambda m: m.float()):
        ema = cast(ema)
        for k, v in ema.state_dict().items():
            assert v.dtype == kept[k].dtype and torch.equal(v, kept[k]), k
    assert float(ema.decay) == float(torch.tensor(0.9999)) and ema.num_updates.dtype == torch.int32


@pytest.mark.parametrize("pretend", [False, True], ids=["torch", "emulated-kernel"])
def test_the_update_reads_the_masters_and_follows_the_documented_arithmetic_over_12_updates(monkeypatch, pretend):
    from lvdm.modules.ema import LitEma
    count = {}
    if pretend:
        M.pretend_gpu(monkeypatch, count)
    torch.manual_seed(0)
    net = _Two()
    trainable = {n: p for n, p in net.named_parameters() if p.requires_grad}
    masters = {p: p.detach().float() + 1e-3 * torch.randn(p.shape) for n, p in trainable.items() if p.dtype == torch.bfloat16}
    shadow = {n: masters[p].clone() if p in masters else p.detach().clone() for n, p in trainable.items()}
    start = {n: s.clone() for n, s in shadow.items()}
    ema = LitEma(net, decay=0.9999, fp32_shadows=True, masters=masters)
    stalled = LitEma(net, decay=0.9999)
    gen = torch.Generator().manual_seed(3)
    for n_up in range(1, 13):
        with torch.no_grad():
            for p in trainable.values():      # steps far below the bf16 spacing: only the masters (and the fp32 logvar) move
                src = masters.get(p, p)
                src.add_(1e-5 * torch.randn(p.shape, generator=gen))
        ema(net, masters=masters.get)
        stalled(net)
        decay = torch.minimum(torch.tensor(0.9999), torch.tensor(1 + n_up, dtype=torch.int32) / torch.tensor(10 + n_up, dtype=torch.int32))
        for n, p in trainable.items():
            shadow[n].sub_((1.0 - decay) * (shadow[n] - masters.get(p, p).detach()))
    assert int(ema.num_updates) == 12
    assert count == ({"mt_ema": 24} if pretend else {})
    for n, s in ema.m_name2s_name.items():
        got = getattr(ema, s)
        assert got.dtype == torch.float32 and torch.equal(got, shadow[n]), n
        assert not torch.equal(got, start[n]), n
    for n, p in trainable.items():            # the 16-bit shadows of the plain class never left the 16-bit weights
        if p.dtype == torch.bfloat16:
            assert torch.equal(getattr(stalled, ema.m_name2s_name[n]), p.detach())
    # copy_to writes the rounded shadows, restore puts the 16-bit weights back
    before = [p.detach().clone() for p in net.parameters()]
    ema.store(net.parameters())
    ema.copy_to(net)
    for n, p in trainable.items():
        assert torch.equal(p.detach(), shadow[n].to(p.dtype)), n
    ema.restore(net.parameters())
    assert all(torch.equal(p.detach(), b) for p, b in zip(net.parameters(), before))


def test_a_reload_keeps_the_fp32_shadows_and_the_converter_reads_them():
    from cvvae_amd.checkpoint import extract_codec_state
    from lvdm.modules.ema import LitEma
    torch.manual_seed(1)
    net = _Two()
    ema = LitEma(net, decay=0.999, fp32_shadows=True)
    with torch.no_grad():
        ema.headweight.add_(1e-4)
    other = LitEma(_Two(), fp32_shadows=True)
    other.load_state_dict(ema.state_dict())
    assert other.headweight.dtype == torch.float32 and torch.equal(other.headweight, ema.headweight)
    sd = {"model_ema." + k: v for k, v in ema.state_dict().items()}
    sd.update(net.state_dict())
    want = {n: p.shape for n, p in net.named_parameters() if p.requires_grad}
    out = extract_codec_state(sd, want, use_ema=True)
    assert set(out) == set(want) and all(v.dtype == torch.float32 for v in out.values())
    assert torch.equal(out["head.weight"], ema.headweight)
