"""The contract of the LPIPS drop-in (cvvae_amd/lpips.py) that holds without a GPU: the reference's state-dict layout, frozen
parameters, the `lvdm...` import path, no network at construction, no CPU fallback, and the argument checks of the new C entry
points (include/cvvae.h ABI 14)."""
import ctypes

import pytest
import torch

from tests import lpips_ref

# the reference's LPIPS().state_dict(): torchvision VGG16 `features` indices inside the five slices, lin weights behind a Dropout
EXPECTED = {
    "scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1),
    "net.slice1.0.weight": (64, 3, 3, 3), "net.slice1.0.bias": (64,), "net.slice1.2.weight": (64, 64, 3, 3), "net.slice1.2.bias": (64,),
    "net.slice2.5.weight": (128, 64, 3, 3), "net.slice2.5.bias": (128,), "net.slice2.7.weight": (128, 128, 3, 3), "net.slice2.7.bias": (128,),
    "net.slice3.10.weight": (256, 128, 3, 3), "net.slice3.10.bias": (256,), "net.slice3.12.weight": (256, 256, 3, 3),
    "net.slice3.12.bias": (256,), "net.slice3.14.weight": (256, 256, 3, 3), "net.slice3.14.bias": (256,),
    "net.slice4.17.weight": (512, 256, 3, 3), "net.slice4.17.bias": (512,), "net.slice4.19.weight": (512, 512, 3, 3),
    "net.slice4.19.bias": (512,), "net.slice4.21.weight": (512, 512, 3, 3), "net.slice4.21.bias": (512,),
    "net.slice5.24.weight": (512, 512, 3, 3), "net.slice5.24.bias": (512,), "net.slice5.26.weight": (512, 512, 3, 3),
    "net.slice5.26.bias": (512,), "net.slice5.28.weight": (512, 512, 3, 3), "net.slice5.28.bias": (512,),
    "lin0.model.1.weight": (1, 64, 1, 1), "lin1.model.1.weight": (1, 128, 1, 1), "lin2.model.1.weight": (1, 256, 1, 1),
    "lin3.model.1.weight": (1, 512, 1, 1), "lin4.model.1.weight": (1, 512, 1, 1),
}


def test_state_dict_layout_is_the_references():
    from cvvae_amd.lpips import LPIPS
    m = LPIPS()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == EXPECTED and len(got) == 33
    assert lpips_ref.STATE_DICT_SHAPES == EXPECTED
    m.load_state_dict(lpips_ref.lpips_state_dict(0), strict=True)


def test_parameters_are_frozen_and_buffers_hold_the_constants():
    from cvvae_amd.lpips import LPIPS
    m = LPIPS()
    assert all(not p.requires_grad for p in m.parameters()) and len(list(m.parameters())) == 31
    bufs = dict(m.named_buffers())
    assert set(bufs) == {"scaling_layer.shift", "scaling_layer.scale"}
    assert torch.equal(bufs["scaling_layer.shift"], torch.tensor([-0.030, -0.088, -0.188])[None, :, None, None])
    assert torch.equal(bufs["scaling_layer.scale"], torch.tensor([0.458, 0.448, 0.450])[None, :, None, None])
    assert m.chns == [64, 128, 256, 512, 512]
    assert list(LPIPS(use_dropout=False).lin0.state_dict()) == ["model.0.weight"]


def test_reference_import_path_resolves_to_the_class():
    from lvdm.modules.autoencoding.lpips.loss.lpips import LPIPS
    import cvvae_amd.lpips
    assert LPIPS is cvvae_amd.lpips.LPIPS


def test_construction_reaches_no_network(monkeypatch):
    import socket
    import urllib.request

    def refuse(*a, **k):
        raise AssertionError("LPIPS() tried to reach the network")

    try:
        import requests
        monkeypatch.setattr(requests, "get", refuse)
    except ImportError:
        pass
    monkeypatch.setattr(urllib.request, "urlopen", refuse)
    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", refuse)
    from cvvae_amd.lpips import LPIPS
    m = LPIPS().eval()
    assert float(getattr(m.net.slice5, "28").weight.abs().max()) > 0  # default-initialised, not empty


def test_from_pretrained_takes_an_existing_local_file_only(tmp_path):
    from cvvae_amd.lpips import LPIPS
    with pytest.raises(FileNotFoundError):
        LPIPS.from_pretrained(str(tmp_path / "vgg.pth"))
    with pytest.raises(FileNotFoundError):
        LPIPS.from_pretrained("vgg_lpips")
    sd = lpips_ref.lpips_state_dict(2)
    torch.save(sd, tmp_path / "vgg.pth")
    m = LPIPS.from_pretrained(str(tmp_path / "vgg.pth"))
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert all(not p.requires_grad for p in m.parameters())


def test_cpu_tensors_raise_the_needs_a_gpu_error():
    from cvvae_amd.lpips import LPIPS
    m = LPIPS().eval()
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x.clone().requires_grad_(True))


NEW_ENTRIES = ["cvvae_lpips_scale_in", "cvvae_lpips_scale_in_bwd", "cvvae_relu", "cvvae_maxpool2x2", "cvvae_relu_pool_bwd",
               "cvvae_lpips_head_workspace_bytes", "cvvae_lpips_head", "cvvae_lpips_head_bwd"]


def test_new_entry_points_are_exported_with_prototypes():
    from cvvae_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "cvvae.h")).read()
    for n in NEW_ENTRIES:
        assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header, n


def test_new_entry_points_refuse_null_and_inconsistent_arguments():
    """CVVAE_EINVAL before any launch: no GPU is touched"""
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # a non-NULL (host) pointer: the checks below never dereference or launch
    E = -1
    assert lib.cvvae_lpips_scale_in(L.F32, L.BF16, None, 1, 4, 4, p, p, 32, p, None) == E
    assert lib.cvvae_lpips_scale_in(L.F32, L.BF16, p, 1, 4, 4, None, p, 32, p, None) == E
    assert lib.cvvae_lpips_scale_in(L.F32, L.BF16, p, 1, 4, 4, p, p, 32, None, None) == E
    assert lib.cvvae_lpips_scale_in(L.F32, L.BF16, p, 1, 4, 4, p, p, 12, p, None) == E     # Cpad % 8
    assert lib.cvvae_lpips_scale_in(L.F32, 9, p, 1, 4, 4, p, p, 32, p, None) == E          # unknown dtype
    assert lib.cvvae_lpips_scale_in_bwd(L.BF16, L.F32, None, 1, 4, 4, 8, p, p, None) == E
    assert lib.cvvae_lpips_scale_in_bwd(L.BF16, L.F32, p, 1, 4, 4, 8, None, p, None) == E
    assert lib.cvvae_lpips_scale_in_bwd(L.BF16, L.F32, p, 1, 4, 4, 8, p, None, None) == E
    assert lib.cvvae_lpips_scale_in_bwd(L.BF16, L.F32, p, 1, 4, 4, 4, p, p, None) == E     # pixel stride < 8
    assert lib.cvvae_relu(L.F16, None, 64, p, None) == E
    assert lib.cvvae_relu(L.F16, p, 64, None, None) == E
    assert lib.cvvae_relu(L.F16, p, 12, p, None) == E                                      # n % 8
    assert lib.cvvae_maxpool2x2(L.F16, None, 1, 4, 4, 64, p, None) == E
    assert lib.cvvae_maxpool2x2(L.F16, p, 1, 4, 4, 64, None, None) == E
    assert lib.cvvae_maxpool2x2(L.F16, p, 1, 1, 4, 64, p, None) == E                       # nothing to pool
    assert lib.cvvae_maxpool2x2(L.F16, p, 1, 4, 4, 60, p, None) == E                       # C % 8
    assert lib.cvvae_relu_pool_bwd(L.F16, None, p, p, 1, 4, 4, 64, p, None) == E
    assert lib.cvvae_relu_pool_bwd(L.F16, p, None, None, 1, 4, 4, 64, p, None) == E        # neither gradient
    assert lib.cvvae_relu_pool_bwd(L.F16, p, p, p, 1, 4, 4, 64, None, None) == E
    assert lib.cvvae_lpips_head(L.F16, None, p, p, 1, 16, 64, p, p, None) == E
    assert lib.cvvae_lpips_head(L.F16, p, None, p, 1, 16, 64, p, p, None) == E
    assert lib.cvvae_lpips_head(L.F16, p, p, None, 1, 16, 64, p, p, None) == E
    assert lib.cvvae_lpips_head(L.F16, p, p, p, 1, 16, 64, None, p, None) == E
    assert lib.cvvae_lpips_head(L.F16, p, p, p, 1, 16, 64, p, None, None) == E
    assert lib.cvvae_lpips_head(L.F16, p, p, p, 1, 16, 96, p, p, None) == -2               # a width no wave mapping exists for
    assert lib.cvvae_lpips_head_bwd(L.F16, None, p, p, p, 1, 16, 64, p, p, None) == E
    assert lib.cvvae_lpips_head_bwd(L.F16, p, p, p, None, 1, 16, 64, p, p, None) == E
    assert lib.cvvae_lpips_head_bwd(L.F16, p, p, p, p, 1, 16, 64, None, None, None) == E   # neither side requested
    assert lib.cvvae_lpips_head_workspace_bytes(1, 16, 96) == 0
    assert lib.cvvae_lpips_head_workspace_bytes(3, 63, 64) == 3 * 2 * 4                    # 32 pixels per workgroup pass -> 2 partials
