"""The 3-D PatchGAN discriminator as a module (cvvae_amd/discriminator.py): import paths, the reference's state_dict() names and
shapes (tests/golden/disc_net_names.json, written from the reference's own module by tools/make_disc_fixture.py), construction
from the training config's dictionary, the constructor flags that are not built, the new C entry point and the wrapper's argument
checks -- none of which launches a kernel."""
import ctypes
import importlib
import json
import os

import pytest
import torch

from tests import disc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# configs/cvvae_sd3_constraint_training.yaml: model.params.loss_config.params.discriminator_config
YAML_DISC = {"target": "lvdm.modules.autoencoding.lpips.model.model.NLayerDiscriminator3D",
             "params": {"input_nc": 3, "ndf": 64, "n_layers": 4, "use_actnorm": False, "causal": False, "half_3d": False}}


def _names():
    with open(os.path.join(ROOT, "tests", "golden", "disc_net_names.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


def test_the_three_import_paths_resolve_to_one_class():
    from cvvae_amd import discriminator as D
    a = importlib.import_module("lvdm.modules.autoencoding.lpips.model.model")
    b = importlib.import_module("models.discriminator")
    importlib.import_module("lvdm.modules.autoencoding.lpips.model")
    for m in (a, b):
        assert m.NLayerDiscriminator3D is D.NLayerDiscriminator3D and m.ResnetBlockDown3D is D.ResnetBlockDown3D
        assert m.weights_init is D.weights_init
    assert b.get_cvvae_discriminator is D.get_cvvae_discriminator
    from cvvae_amd import loss
    assert D.weights_init is loss.weights_init


def test_state_dict_names_and_shapes_are_the_reference_modules():
    from cvvae_amd.discriminator import get_cvvae_discriminator
    net = get_cvvae_discriminator()
    want = _names()
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert sum(p.numel() for p in net.parameters()) == 29015041
    assert "main.2.temb_proj.weight" in got and "main.2.nin_shortcut.weight" in got and "main.11.nin_shortcut.weight" not in got
    assert disc_ref.shapes() == want                       # the yardstick's own table
    net.load_state_dict(disc_ref.seeded_state(), strict=True)
    for m in net.modules():
        if isinstance(m, torch.nn.GroupNorm):
            assert m.num_groups == 32 and m.eps == 1e-5


def test_the_training_configs_dictionary_builds_it_with_weights_init():
    from cvvae_amd import loss
    from cvvae_amd.discriminator import NLayerDiscriminator3D
    torch.manual_seed(0)
    net = loss._instantiate(YAML_DISC).apply(loss.weights_init)
    assert type(net) is NLayerDiscriminator3D
    w = net.main[2].conv1.weight
    assert abs(float(w.detach().std()) - 0.02) < 1e-3 and abs(float(w.detach().mean())) < 1e-3        # every Conv3d: N(0, 0.02)
    assert torch.equal(net.main[3].weight, torch.ones(128))                          # GroupNorm is no "BatchNorm": left alone


@pytest.mark.parametrize("flag", ["use_actnorm", "causal", "half_3d"])
def test_constructor_flags_that_are_not_built_raise(flag):
    from cvvae_amd.discriminator import NLayerDiscriminator3D
    with pytest.raises(NotImplementedError):
        NLayerDiscriminator3D(**{flag: True})


def test_block_flags_that_are_not_built_raise():
    from cvvae_amd.discriminator import ResnetBlockDown3D
    for kw in (dict(), dict(half_3d=False, causal=True), dict(half_3d=False, conv_shortcut=True)):   # (half_3d defaults to True)
        with pytest.raises(NotImplementedError):
            ResnetBlockDown3D(in_channels=64, out_channels=128, dropout=0.0, **kw)
    blk = ResnetBlockDown3D(in_channels=64, out_channels=128, dropout=0.0, half_3d=False)
    assert sorted(n for n, _ in blk.named_children()) == ["conv1", "conv2", "dropout", "nin_shortcut", "norm1", "norm2", "temb_proj"]


def test_the_c_entry_point_is_exported_and_declared():
    from cvvae_amd import _lib
    lib = _lib.load()
    n = "cvvae_conv333_s2_dgrad_small"
    with open(os.path.join(ROOT, "include", "cvvae.h")) as f:
        header = f.read()
    assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header
    assert getattr(lib, n).restype is ctypes.c_int32 and list(getattr(lib, n).argtypes) == _lib.PROTOTYPES[n][1]
    assert lib.cvvae_abi_version() == 14 == _lib.ABI_VERSION
    assert "#define CVVAE_ABI_VERSION 14" in header


def test_the_c_entry_point_refuses_before_it_launches():
    """argument checks of the library itself (host code: null pointers and bad extents return before any HIP call)"""
    from cvvae_amd import _lib
    lib = _lib.load()
    f = lib.cvvae_conv333_s2_dgrad_small
    ok = dict(dtype=_lib.BF16, gy=4096, stride=64, w=8192, gx=16384, B=1, T=5, H=6, W=7, To=3, Ho=3, Wo=4, cin=3, cout=64)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["dtype"], a["gy"], a["stride"], a["w"], a["gx"], a["B"], a["T"], a["H"], a["W"], a["To"], a["Ho"], a["Wo"], a["cin"],
                 a["cout"], None)
    assert call(gy=None) == -1 and call(w=None) == -1 and call(gx=None) == -1 and call(B=0) == -1 and call(cin=0) == -1
    assert call(To=2) == -1 and call(Ho=4) == -1 and call(Wo=3) == -1          # not the forward's output extents
    assert call(cin=9) == -2 and call(cout=60) == -2 and call(dtype=7) == -2
    assert call(stride=56) == -2 and call(stride=68) == -2                       # shorter than Cout; no multiple of 8
    assert call(cout=152, stride=152) == -2 and call(cin=8, cout=80, stride=80) == -2   # the weight table does not fit 64 KiB of LDS
    assert call(gy=4100) == -2                                                   # not 16-byte aligned


def test_the_wrapper_refuses_bad_arguments_without_launching(monkeypatch):
    from cvvae_amd import _lib, ops
    lib = _lib.load()
    monkeypatch.setattr(ops, "_need_gpu", lambda t: None)
    monkeypatch.setattr(ops, "_stream", lambda t: pytest.fail("reached the launch"))
    gy = torch.zeros(2, 3, 3, 4, 64)
    w = torch.zeros(64, 3, 3, 3, 3)
    with pytest.raises(NotImplementedError):
        ops.conv333_s2_dgrad_small(gy, torch.zeros(64, 9, 3, 3, 3), (2, 5, 6, 7), 9)           # Cin > 8
    with pytest.raises(NotImplementedError):
        ops.conv333_s2_dgrad_small(torch.zeros(2, 3, 3, 4, 64), torch.zeros(60, 3, 3, 3, 3), (2, 5, 6, 7), 3)   # Cout % 8
    for shape in ((2, 5, 6, 9), (2, 7, 6, 7), (1, 5, 6, 7)):                                    # gy of another input's shape
        with pytest.raises(ValueError):
            ops.conv333_s2_dgrad_small(gy, w, shape, 3)
    with pytest.raises(ValueError):
        ops.conv333_s2_dgrad_small(torch.zeros(2, 3, 3, 4, 56), w, (2, 5, 6, 7), 3)            # fewer channels than Cout
    with pytest.raises(ValueError):
        ops.conv333_s2_dgrad_small(gy, w, (2, 5, 6, 7), 4)                                     # cin against the weight's
    with pytest.raises(ValueError):
        ops.conv333_s2_dgrad_small(gy.transpose(2, 3), w, (2, 5, 6, 7), 3)                     # not contiguous
    assert lib is _lib.load()
    tab = ops.dgrad_small_table(torch.arange(8 * 3 * 27, dtype=torch.float32).reshape(8, 3, 3, 3, 3))
    assert tuple(tab.shape) == (27, 8, 8) and float(tab[5, 2, 1]) == (2 * 3 + 1) * 27 + 5 and float(tab[:, :, 3:].abs().max()) == 0
