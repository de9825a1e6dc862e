"""CPU pin of the LAUNCH SEQUENCES of the training path: forward plus backward of every taped network (cvvae_amd/grad.py, grad3d.py,
discriminator.py, lpips.py over the shared helpers of cvvae_amd/backward.py) must issue the same calls of `cvvae_amd.ops`, in the
same order, with the same arguments as the recording in tests/golden/backward_launch_trace.json.  The later scenarios pin the
INFERENCE programs too (eval, no_grad: both 3-D families on a clip and on a single frame, the frozen SD2.1-family 2-D halves).

The tracer runs on the plain-PyTorch emulations of the ops (tests/emu_ops.patched(whole_model=True) plus the discriminator's and
LPIPS' emulations of tests/test_disc_net_host_logic.py and tests/test_lpips_host_logic.py); no GPU, no library.  It wraps every public
function of `cvvae_amd.ops` and writes one line per TOP-LEVEL call (calls an emulation makes itself are not recorded): the op's name,
then every parameter of the op by name (the call's arguments bound to the signature, defaults filled in: the launch, not how the
call spells it) and the result -- a tensor as shape and dtype, a packed weight as cout / cin / k / folded / time_folds /
batch_stride, a GroupNorm record as its geometry, scalars, tuples and strings by value, None as None.  No addresses, no values of
tensors.  Per scenario the fixture holds the number of calls, the count per op name (so that a failure says where) and the sha256 of
the joined lines; the test compares all three.

The fixture is regenerated ONLY by a change that MEANS to alter the launch sequence (a new launch, another operand, another order):

    python -m tests.test_backward_launch_trace          # from the repository root; rewrites tests/golden/backward_launch_trace.json

A refactor of the host code must leave it alone: it was recorded from the code before the helpers moved into backward.py and passes
unchanged on both."""
import collections
import contextlib
import dataclasses
import hashlib
import inspect
import json
import os

import numpy as np
import pytest
import torch

from oracle.seeded import seeded_input, seeded_state_dict
from tests import disc_ref, emu_ops
from tests.test_disc_net_host_logic import (emu_avgpool3d_down_bwd, emu_avgpool3d_down_out, emu_conv333_s2_dgrad_small,
                                            emu_gn_leaky_apply_out, emu_leaky_bwd)
from tests.test_lpips_host_logic import _LPIPS_OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "backward_launch_trace.json")
SD3 = dict(block_out_channels=[128, 256, 256], layers_per_block=1)
V3 = dict(ch=128, ch_mult=(1, 2, 2), num_res_blocks=1)
C2D = dict(in_channels=16, out_channels=3, up_block_types=["UpDecoderBlock2D"] * 3, block_out_channels=[128, 256, 256],
           layers_per_block=1, norm_num_groups=32, act_fn="silu", mid_block_add_attention=True)
_DISC_OPS = dict(avgpool3d_down=emu_avgpool3d_down_out, avgpool3d_down_bwd=emu_avgpool3d_down_bwd, gn_leaky_apply=emu_gn_leaky_apply_out,
                 leaky_bwd=emu_leaky_bwd, conv333_s2_dgrad_small=emu_conv333_s2_dgrad_small)


def _show(v) -> str:
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    if isinstance(v, torch.Tensor):
        return f"T{list(v.shape)}{str(v.dtype)[6:]}"
    if isinstance(v, (torch.dtype, torch.device)):
        return str(v)
    if isinstance(v, (tuple, list)):
        return "(" + ",".join(_show(e) for e in v) + ")"
    if isinstance(v, dict):
        return "{" + ",".join(f"{k}:{_show(e)}" for k, e in sorted(v.items())) + "}"
    if dataclasses.is_dataclass(v) and hasattr(v, "batch_stride"):     # a packed weight
        return "PW(" + ",".join(f"{f}={_show(getattr(v, f))}" for f in ("cout", "cin", "k", "folded", "time_folds", "batch_stride")) + ")"
    if isinstance(v, emu_ops.FakePart):                                   # GroupNorm records of a producer
        return "GN(" + ",".join(f"{f}={getattr(v, f)}" for f in ("rows", "C", "groups", "frames", "slabs")) + ")"
    return type(v).__name__


@contextlib.contextmanager
def tracing():
    """the emulated ops with every public function of cvvae_amd.ops wrapped; yields the list of lines"""
    from cvvae_amd import ops
    lines, depth = [], [0]

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def f(*a, **k):
            if depth[0]:
                return fn(*a, **k)
            depth[0] += 1
            try:
                out = fn(*a, **k)
            finally:
                depth[0] -= 1
            bound = sig.bind(*a, **k)       # every parameter by name, defaults filled in: the launch, not how the call spells it
            bound.apply_defaults()
            lines.append(f"{name}({', '.join(f'{n}={_show(v)}' for n, v in bound.arguments.items())}) -> {_show(out)}")
            return out
        return f
    with emu_ops.patched(whole_model=True), pytest.MonkeyPatch.context() as mp:
        for n, fn in {**_DISC_OPS, **_LPIPS_OPS}.items():
            mp.setattr(ops, n, fn)
        mp.setattr(ops, "_need_gpu", lambda t: None)
        for n, fn in list(vars(ops).items()):
            if not n.startswith("_") and inspect.isfunction(fn):
                mp.setattr(ops, n, wrap(n, fn))
        yield lines


def _load(m, seed):
    m.load_state_dict(seeded_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed), strict=True)
    return m


def _step(net, x, need_x=True):
    """forward + backward of net in its current mode"""
    xa = x.clone().requires_grad_(need_x)
    y = net(xa)
    (y * seeded_input(tuple(y.shape), 4)).sum().backward()


def _sd3(part):
    import cvvae_amd
    return getattr(_load(cvvae_amd.CVVAESD3Model(**SD3), 7), part).train()


def sd3_encoder():
    _step(_sd3("encoder"), seeded_input((1, 3, 5, 16, 24), 11))


def sd3_decoder():
    _step(_sd3("decoder"), seeded_input((1, 16, 3, 4, 6), 13))


def vae3d_encoder_causal():
    import cvvae_amd
    _step(_load(cvvae_amd.CVVAEModel(causal_encoder=True, **V3), 9).encoder.train(), seeded_input((1, 3, 5, 16, 24), 14))


def vae3d_decoder():
    import cvvae_amd
    _step(_load(cvvae_amd.CVVAEModel(**V3), 10).decoder.train(), seeded_input((1, 4, 3, 4, 6), 15))


def frozen_decoder():
    _step(_sd3("decoder").requires_grad_(False), seeded_input((1, 16, 3, 4, 6), 13))


def tail_only_probe():
    """two last-layer probes (Net3DTailFn's backward alone), then the step's real backward"""
    dec = _sd3("decoder")
    za = seeded_input((1, 16, 3, 4, 6), 13).requires_grad_(True)
    ya = dec(za)
    cot = seeded_input(tuple(ya.shape), 6)
    for _ in range(2):
        torch.autograd.grad((ya * cot).sum(), dec.get_last_layer(), retain_graph=True)
    (ya * seeded_input(tuple(ya.shape), 5)).sum().backward()


def recompute():
    for part, shape, seed in (("encoder", (1, 3, 5, 16, 24), 11), ("decoder", (1, 16, 3, 4, 6), 13)):
        net = _sd3(part)
        net.recompute = True
        _step(net, seeded_input(shape, seed))


def constraint_decoder2d():
    from cvvae_amd.constraint import DecoderWith3DWrapper
    m = _load(DecoderWith3DWrapper(**C2D), 5).eval().requires_grad_(False)
    _step(m, seeded_input((2, 16, 1, 5, 4), 9))       # (the host-logic test's latent with the fewer elements)


def _disc(need_x, frozen):
    from cvvae_amd.discriminator import DiscFn, get_cvvae_discriminator
    z = np.load(os.path.join(ROOT, "tests", "golden", "disc_net_ref.npz"))
    net = get_cvvae_discriminator()
    net.load_state_dict(disc_ref.seeded_state())
    net.train().requires_grad_(not frozen)
    named = list(net.named_parameters())
    xa = torch.from_numpy(z["x"]).float().requires_grad_(need_x)
    y = DiscFn.apply(xa, net, tuple(n for n, _ in named), *[p for _, p in named])
    (y * torch.from_numpy(z["c"]).float()).sum().backward()


def _lpips(need0, need1):
    from cvvae_amd.lpips import LPIPS
    from tests import lpips_ref
    m = LPIPS().eval()
    m.load_state_dict(lpips_ref.lpips_state_dict(3), strict=True)
    x0 = seeded_input((2, 3, 16, 16), 5)
    x1 = (x0 + 0.3 * seeded_input((2, 3, 16, 16), 6)).clamp(-1, 1)
    m(x0.requires_grad_(need0), x1.requires_grad_(need1)).sum().backward()


LDM = dict(ch=128, out_ch=3, ch_mult=(1, 2, 2), num_res_blocks=1, attn_resolutions=[], in_channels=3, resolution=32, z_channels=4)


def _ldm2d_decoder(legacy):
    """the frozen SD2.1-family decoder: taped forward + input gradient (legacy: with post_quant_conv)"""
    from cvvae_amd.constraint_ldm import DecoderWith3DWrapper
    m = _load(DecoderWith3DWrapper(legacy=legacy, **LDM), 5).eval().requires_grad_(False)
    _step(m, seeded_input((2, 4, 1, 5, 4), 9))


def _ldm2d_encoder(legacy):
    from cvvae_amd.constraint_ldm import EncoderWith3DWrapper
    m = _load(EncoderWith3DWrapper(legacy=legacy, **LDM), 6).eval()
    with torch.no_grad():
        m(seeded_input((1, 3, 2, 16, 24), 10))


def _inference(model):
    """the untaped programs: encode + decode of a clip, then of a single frame (the temporally folded path)"""
    model.eval()
    with torch.no_grad():
        for shape in ((1, 3, 5, 16, 24), (1, 3, 1, 16, 24)):
            model.decode(model.encode(seeded_input(shape, 12)).latent_dist.mode())


def sd3_inference():
    import cvvae_amd
    _inference(_load(cvvae_amd.CVVAESD3Model(**SD3), 7))


def vae3d_inference():
    import cvvae_amd
    _inference(_load(cvvae_amd.CVVAEModel(causal_encoder=True, **V3), 9))


def sd3_no_mid_attention():
    import cvvae_amd
    from cvvae_amd.constraint import DecoderWith3DWrapper
    m = _load(cvvae_amd.CVVAESD3Model(mid_block_add_attention=False, **SD3), 7).eval()
    with torch.no_grad():
        m.encoder(seeded_input((1, 3, 5, 16, 24), 11))
        m.decoder(seeded_input((1, 16, 3, 4, 6), 13))
    d = _load(DecoderWith3DWrapper(**dict(C2D, mid_block_add_attention=False)), 5).eval().requires_grad_(False)
    _step(d, seeded_input((2, 16, 1, 5, 4), 9))


SCENARIOS = {
    "sd3_encoder": sd3_encoder,
    "sd3_decoder": sd3_decoder,
    "vae3d_encoder_causal": vae3d_encoder_causal,
    "vae3d_decoder": vae3d_decoder,
    "frozen_decoder": frozen_decoder,
    "tail_only_probe": tail_only_probe,
    "recompute": recompute,
    "constraint_decoder2d": constraint_decoder2d,
    "disc_input_and_parameters": lambda: _disc(True, False),
    "disc_detached_input": lambda: _disc(False, False),
    "disc_frozen_parameters": lambda: _disc(True, True),
    "lpips_input": lambda: _lpips(True, False),
    "lpips_target": lambda: _lpips(False, True),
    "lpips_both": lambda: _lpips(True, True),
    "ldm2d_decoder_legacy": lambda: _ldm2d_decoder(True),
    "ldm2d_decoder_plain": lambda: _ldm2d_decoder(False),
    "ldm2d_encoder_legacy": lambda: _ldm2d_encoder(True),
    "ldm2d_encoder_plain": lambda: _ldm2d_encoder(False),
    "sd3_inference": sd3_inference,
    "vae3d_inference": vae3d_inference,
    "sd3_no_mid_attention": sd3_no_mid_attention,
}


def record(name: str) -> dict:
    with tracing() as lines:
        SCENARIOS[name]()
    ops_count = collections.Counter(ln.split("(", 1)[0] for ln in lines)
    return {"calls": len(lines), "per_op": dict(sorted(ops_count.items())), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest()}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_covers_every_scenario(golden):
    assert sorted(golden) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_launch_sequence_is_the_recorded_one(golden, name):
    got, want = record(name), golden[name]
    assert got["per_op"] == want["per_op"], {k: (got["per_op"].get(k), want["per_op"].get(k))
                                             for k in set(got["per_op"]) | set(want["per_op"]) if got["per_op"].get(k) != want["per_op"].get(k)}
    assert got["calls"] == want["calls"]
    assert got["sha256"] == want["sha256"], "same ops, same counts: an argument, a shape or the order moved"


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump({n: record(n) for n in SCENARIOS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)
