"""CPU check of the HOST logic of the frozen LDM (SD2.1-family) decoder's input-gradient pass (cvvae_amd/grad.py,
`ldm2d_decoder_backward` over `engine.ldm2d_decoder`'s tape): with every kernel replaced by the plain-PyTorch emulation of its
documented arithmetic (tests/emu_ops.py), the taped forward must reproduce the golden reconstruction of the reference's own
`DecoderWith3DWrapper` and the backward walk its autograd gradient (tests/golden/ldm2d_dec_grad_*.npz, written by
tools/make_ldm_grad_fixture.py from that class) -- i.e. the right tensors are taped, `nin_shortcut` / `mid.attn_1.*` are the names
walked, the upsample convs are taken at the upsampled size and `post_quant_conv` is transposed with the forward's padding.
Bound: 1e-4 relative L2, what tests/test_grad_host_logic.py holds the SD3 decoder's wiring to (the fixture's own fp32 error against
fp64 is 3e-6).  (The kernels themselves run on the GPU: tests/test_gpu_train_constraint.py.)"""
import os

import numpy as np
import pytest
import torch

from oracle.golden_cases import LDM_CASES
from oracle.seeded import seeded_input, seeded_state_dict
from tests import emu_ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"ldm2d_dec_t3_8": "ldm2d_dec_grad_t3_8", "ldm2d_dec_4d_6x4": "ldm2d_dec_grad_4d_6x4"}


def frozen_decoder(cfg, wseed, **kw):
    from cvvae_amd.constraint_ldm import DecoderWith3DWrapper
    m = DecoderWith3DWrapper(**cfg, **kw)
    m.load_state_dict(seeded_state_dict({k: v.shape for k, v in m.state_dict().items()}, wseed), strict=True)
    return m.eval().requires_grad_(False)


@pytest.mark.parametrize("case", list(CASES))
def test_ldm_decoder_backward_wiring(case):
    from cvvae_amd import engine, grad
    _, cfg, shape, wseed, xseed = LDM_CASES[case]
    fix = np.load(os.path.join(GOLDEN, CASES[case] + ".npz"))
    want_y = torch.from_numpy(np.load(os.path.join(GOLDEN, case + ".npz"))["out"])
    want = torch.from_numpy(fix["dz_fp32"])
    m = frozen_decoder(cfg, wseed)
    z = seeded_input(shape, xseed)
    z5 = z if z.dim() == 5 else z.unsqueeze(2)
    cot = seeded_input(tuple(want_y.shape), int(fix["cot_seed"]))
    cot5 = cot if cot.dim() == 5 else cot.unsqueeze(2)
    with emu_ops.patched(), torch.no_grad():
        wc = engine.WeightCache(m)
        tape = []
        y = engine.ldm2d_decoder(wc, z5, m._cfg, tape)
        assert torch.equal(y, engine.ldm2d_decoder(wc, z5, m._cfg)), "the taped forward must be the inference forward"
        gz = grad.ldm2d_decoder_backward(wc, tape, cot5)
    y = y if z.dim() == 5 else y.squeeze(2)
    assert float((y - want_y).norm() / want_y.norm()) < 1e-4
    ops_seen = [e["op"] for e in tape]
    assert ops_seen.count("resnet") == 2 + 3 * len(cfg["ch_mult"]) and ops_seen.count("up") == len(cfg["ch_mult"]) - 1
    assert ops_seen.count("attn") == 1 and ops_seen[-1] == "out" and tape[-1]["post_quant_conv"] is True
    assert (tape[-1]["B"], tape[-1]["T"], tape[-1]["zin"]) == (z5.shape[0], z5.shape[2], 4)
    gz = gz if z.dim() == 5 else gz.squeeze(2)
    assert gz.shape == want.shape
    err = float((gz - want).norm() / want.norm())
    print(f"\n[ldm decoder backward wiring {case}] rel L2 {err:.2e}")
    assert err < 1e-4, err


def test_ldm_decoder_backward_without_post_quant_conv():
    """legacy=False: no post_quant_conv, conv_in's input gradient is the latents' -- against autograd over the emulated forward with
    legacy=True's 1x1 layer set to the identity (the two decoders then compute the same function)"""
    from cvvae_amd import engine, grad
    _, cfg, shape, wseed, xseed = LDM_CASES["ldm2d_dec_t3_8"]
    a = frozen_decoder(cfg, wseed)
    sd = a.state_dict()
    sd["post_quant_conv.weight"] = torch.eye(4).reshape(4, 4, 1, 1)
    sd["post_quant_conv.bias"] = torch.zeros(4)
    a.load_state_dict(sd)
    from cvvae_amd.constraint_ldm import DecoderWith3DWrapper
    b = DecoderWith3DWrapper(**cfg, legacy=False)
    b.load_state_dict({k: v for k, v in sd.items() if not k.startswith("post_quant_conv.")}, strict=True)
    b = b.eval().requires_grad_(False)
    z = seeded_input(shape, xseed)
    cot = seeded_input((1, 3, 3, 64, 64), 77)
    got = []
    with emu_ops.patched(), torch.no_grad():
        for m in (a, b):
            wc, tape = engine.WeightCache(m), []
            engine.ldm2d_decoder(wc, z, m._cfg, tape)
            assert tape[-1]["post_quant_conv"] is (m is a)
            got.append(grad.ldm2d_decoder_backward(wc, tape, cot))
    assert float((got[0] - got[1]).norm() / got[0].norm()) < 1e-5


def test_ldm_decoder_node_under_autograd_and_its_refusals():
    """the module's own route: z.requires_grad -> one autograd node (taped / begin_node / backward_pass / node_grads); a second
    backward under retain_graph walks the same tape to the same bits; a trainable parameter raises; no_grad and a detached z take
    the inference pass"""
    _, cfg, shape, wseed, xseed = LDM_CASES["ldm2d_dec_4d_6x4"]
    fix = np.load(os.path.join(GOLDEN, "ldm2d_dec_grad_4d_6x4.npz"))
    want = torch.from_numpy(fix["dz_fp32"])
    m = frozen_decoder(cfg, wseed)
    z = seeded_input(shape, xseed).requires_grad_(True)
    cot = seeded_input((2, 3, 48, 32), int(fix["cot_seed"]))
    with emu_ops.patched(whole_model=True):
        y = m(z)
        assert y.requires_grad and type(y.grad_fn.next_functions[0][0]).__name__.startswith("Decoder2DInputGradFn")  # (under the 4-D squeeze)
        loss = (y * cot).sum()
        loss.backward(retain_graph=True)
        g1 = z.grad.clone()
        z.grad = None
        loss.backward()
        assert torch.equal(z.grad, g1)
        with torch.no_grad():
            y0 = m(z)
        assert not y0.requires_grad and torch.equal(y0, y.detach())
        yd = m(z.detach())
        assert yd.grad_fn is None and torch.equal(yd, y0)
        m.conv_in.weight.requires_grad_(True)
        with pytest.raises(NotImplementedError, match="input gradient"):
            m(z)
    assert float((g1 - want).norm() / want.norm()) < 1e-4
