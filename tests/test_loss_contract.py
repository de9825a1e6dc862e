"""The contract of the training-loss modules (cvvae_amd/loss.py) that holds without a GPU: the new C entry points of
csrc/loss_kernels.hip (exported, typed, declared, refusing bad arguments before any launch; ABI version unchanged), the
reference's import paths, its parameter names and forward keys (tests/golden/loss_names.json), the options that raise, and no
CPU fallback."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn as nn

NAMES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_names.json")))
ENTRIES = ["cvvae_reduce_workspace_bytes", "cvvae_reduce_sum", "cvvae_reduce_sum_bwd", "cvvae_gauss_reg", "cvvae_gauss_reg_bwd"]
EINVAL, EUNSUPPORTED = -1, -2


def test_entry_points_are_exported_with_prototypes_and_the_abi_version_stays():
    from cvvae_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "cvvae.h")).read()
    assert "#define CVVAE_ABI_VERSION 14" in header
    for n in ENTRIES:
        assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header, n
    ops = ["ABS_DIFF", "SQ_DIFF", "SQ", "IDENT", "HINGE_NEG", "HINGE_POS", "SOFTPLUS_NEG", "SOFTPLUS_POS"]
    for i, n in enumerate(ops):
        assert getattr(_lib, "RED_" + n) == i and f"CVVAE_RED_{n} = {i}" in header, n
    assert ctypes.sizeof(_lib.ReduceShape) == 10 * 8


def _shape(n=(1, 1, 4), L=16):
    from cvvae_amd import _lib as Lb
    s = Lb.ReduceShape()
    for i in range(3):
        s.n[i], s.sa[i], s.sb[i] = n[i], L, L
    s.L = L
    return s


def test_reduce_entry_points_refuse_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # a non-NULL (host) pointer: the checks below never dereference or launch
    s = ctypes.byref(_shape())
    A, I = L.RED_ABS_DIFF, L.RED_IDENT
    # every NULL pointer
    assert lib.cvvae_reduce_sum(A, L.F32, None, L.BF16, p, s, p, p, None) == EINVAL
    assert lib.cvvae_reduce_sum(A, L.F32, p, L.BF16, None, s, p, p, None) == EINVAL          # a two-operand op without b
    assert lib.cvvae_reduce_sum(A, L.F32, p, L.BF16, p, None, p, p, None) == EINVAL
    assert lib.cvvae_reduce_sum(A, L.F32, p, L.BF16, p, s, None, p, None) == EINVAL
    assert lib.cvvae_reduce_sum(A, L.F32, p, L.BF16, p, s, p, None, None) == EINVAL
    assert lib.cvvae_reduce_sum(I, L.F32, p, L.F32, p, s, p, p, None) == EINVAL              # a unary op given a second operand
    assert lib.cvvae_reduce_sum(8, L.F32, p, L.F32, None, s, p, p, None) == EUNSUPPORTED     # unknown op
    assert lib.cvvae_reduce_sum(-1, L.F32, p, L.F32, None, s, p, p, None) == EUNSUPPORTED
    assert lib.cvvae_reduce_sum(I, 7, p, L.F32, None, s, p, p, None) == EUNSUPPORTED         # unknown dtype
    assert lib.cvvae_reduce_sum(A, L.F32, p, L.F32Q, p, s, p, p, None) == EUNSUPPORTED
    for bad in (_shape(n=(1, 0, 4)), _shape(L=0), _shape(n=(1, 1, -2))):
        assert lib.cvvae_reduce_sum(I, L.F32, p, L.F32, None, ctypes.byref(bad), p, p, None) == EINVAL
    neg = _shape()
    neg.sa[2] = -16
    assert lib.cvvae_reduce_sum(I, L.F32, p, L.F32, None, ctypes.byref(neg), p, p, None) == EINVAL

    assert lib.cvvae_reduce_sum_bwd(A, L.F32, None, L.BF16, p, s, p, p, p, None) == EINVAL
    assert lib.cvvae_reduce_sum_bwd(A, L.F32, p, L.BF16, None, s, p, p, p, None) == EINVAL
    assert lib.cvvae_reduce_sum_bwd(A, L.F32, p, L.BF16, p, None, p, p, p, None) == EINVAL
    assert lib.cvvae_reduce_sum_bwd(A, L.F32, p, L.BF16, p, s, None, p, p, None) == EINVAL   # the device coefficient
    assert lib.cvvae_reduce_sum_bwd(A, L.F32, p, L.BF16, p, s, p, None, None, None) == EINVAL  # neither gradient requested
    assert lib.cvvae_reduce_sum_bwd(I, L.F32, p, L.F32, p, s, p, p, None, None) == EINVAL    # a unary op given a second operand
    assert lib.cvvae_reduce_sum_bwd(I, L.F32, p, L.F32, None, s, p, None, p, None) == EINVAL  # ... or asked for its gradient
    assert lib.cvvae_reduce_sum_bwd(8, L.F32, p, L.F32, None, s, p, p, None, None) == EUNSUPPORTED
    assert lib.cvvae_reduce_sum_bwd(I, 9, p, L.F32, None, s, p, p, None, None) == EUNSUPPORTED


def test_gauss_entry_points_refuse_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.cvvae_gauss_reg(L.F32, None, p, p, 1, 4, 4, p, p, None) == EINVAL
    assert lib.cvvae_gauss_reg(L.F32, p, p, None, 1, 4, 4, p, p, None) == EINVAL
    assert lib.cvvae_gauss_reg(L.F32, p, p, p, 1, 4, 4, None, p, None) == EINVAL
    assert lib.cvvae_gauss_reg(L.F32, p, p, p, 1, 4, 4, p, None, None) == EINVAL
    assert lib.cvvae_gauss_reg(L.F32, p, p, p, 0, 4, 4, p, p, None) == EINVAL
    assert lib.cvvae_gauss_reg(L.F32, p, p, p, 1, 4, -1, p, p, None) == EINVAL
    assert lib.cvvae_gauss_reg(5, p, None, p, 1, 4, 4, p, p, None) == EUNSUPPORTED           # unknown dtype (noise may be NULL)
    assert lib.cvvae_gauss_reg_bwd(L.BF16, None, p, p, p, p, 1, 4, 4, None) == EINVAL
    assert lib.cvvae_gauss_reg_bwd(L.BF16, p, p, p, None, p, 1, 4, 4, None) == EINVAL
    assert lib.cvvae_gauss_reg_bwd(L.BF16, p, p, p, p, None, 1, 4, 4, None) == EINVAL
    assert lib.cvvae_gauss_reg_bwd(L.BF16, p, p, p, p, p, 1, 0, 4, None) == EINVAL
    assert lib.cvvae_gauss_reg_bwd(L.F32Q6, p, None, None, p, p, 1, 4, 4, None) == EUNSUPPORTED


def test_workspace_bytes_for_hand_computed_shapes():
    """a workgroup pass covers 256 threads x 8 elements = 2048; one fp32 partial per workgroup; the grid is capped at 2048"""
    from cvvae_amd import _lib as L
    lib = L.load()
    ws = lambda n, l: lib.cvvae_reduce_workspace_bytes(ctypes.byref(_shape(n, l)))  # noqa: E731
    assert ws((1, 1, 1), 1) == 4 and ws((1, 1, 1), 2048) == 4 and ws((1, 1, 1), 2049) == 8
    assert ws((2, 3, 3), 256) == 4 * 3                       # 4608 elements: 3 passes, whatever the split into rows
    assert ws((1, 3, 17), 65536) == 4 * 1632                 # one [1,3,17,256,256] clip
    assert ws((1, 1, 2048), 2048) == 4 * 2048 and ws((1, 1, 2049), 2048) == 4 * 2048
    assert ws((1, 0, 1), 8) == 0 and lib.cvvae_reduce_workspace_bytes(None) == 0


def test_reference_import_paths_resolve_to_the_classes():
    import cvvae_amd.loss as loss
    from lvdm.modules.autoencoding.losses import GeneralLPIPSWithDiscriminator, LPIPSWithDiscriminatorAndDomainConstraint
    from lvdm.modules.autoencoding.regularizers import DiagonalGaussianRegularizer
    assert LPIPSWithDiscriminatorAndDomainConstraint is loss.LPIPSWithDiscriminatorAndDomainConstraint
    assert GeneralLPIPSWithDiscriminator is loss.GeneralLPIPSWithDiscriminator
    assert DiagonalGaussianRegularizer is loss.DiagonalGaussianRegularizer
    assert issubclass(LPIPSWithDiscriminatorAndDomainConstraint, GeneralLPIPSWithDiscriminator)


class TinyDisc3d(nn.Module):
    def __init__(self, ch: int = 4):
        super().__init__()
        self.conv = nn.Conv3d(3, ch, 1)
        self.norm = nn.BatchNorm3d(ch)


@pytest.mark.parametrize("name", ["GeneralLPIPSWithDiscriminator", "LPIPSWithDiscriminatorAndDomainConstraint"])
@pytest.mark.parametrize("learn", [False, True])
def test_names_parameters_and_forward_keys_are_the_references(name, learn):
    import cvvae_amd.loss as loss
    from cvvae_amd.lpips import LPIPS
    torch.manual_seed(0)
    m = getattr(loss, name)(disc_start=5, logvar_init=0.25, dims=3, learn_logvar=learn,
                            discriminator_config={"target": "tests.test_loss_contract.TinyDisc3d", "params": {"ch": 6}})
    want = NAMES[name]
    keys = list(m.state_dict())
    assert sorted(k for k in keys if not k.startswith("discriminator.")) == sorted(want["state_dict"])
    assert sorted(k for k in keys if k.startswith("discriminator.")) == sorted("discriminator." + k for k in TinyDisc3d().state_dict())
    assert m.forward_keys == want["forward_keys"]
    logvars = [m.logvar] + ([m.logvar_2d] if "Domain" in name else [])
    for p in logvars:
        assert p.dim() == 0 and float(p) == 0.25 and p.requires_grad == learn
    assert [id(p) for p in m.get_trainable_autoencoder_parameters()] == ([id(p) for p in logvars] if learn else [])
    assert [id(p) for p in m.get_trainable_parameters()] == [id(p) for p in m.discriminator.parameters()]
    assert isinstance(m.perceptual_loss, LPIPS) and not m.perceptual_loss.training
    assert all(not p.requires_grad for p in m.perceptual_loss.parameters())
    # weights_init: Conv ~ N(0, 0.02), BatchNorm weight ~ N(1, 0.02) and zero bias
    d = m.discriminator
    assert type(d).__name__ == "TinyDisc3d" and d.conv.out_channels == 6  # built from the dotted path, params passed
    assert float(d.conv.weight.abs().max()) < 0.12 and abs(float(d.norm.weight.mean()) - 1.0) < 0.05
    assert float(d.norm.weight.std()) > 0 and float(d.norm.bias.abs().max()) == 0.0


def test_unsupported_options_raise():
    from cvvae_amd.loss import GeneralLPIPSWithDiscriminator as G
    from cvvae_amd.loss import LPIPSWithDiscriminatorAndDomainConstraint as D
    disc = nn.Identity()
    with pytest.raises(NotImplementedError, match="no discriminator network ships yet"):
        G(disc_start=0)
    with pytest.raises(NotImplementedError, match="no discriminator network ships yet"):
        D(disc_start=0, dims=3)
    with pytest.raises(NotImplementedError, match="scale_input_to_tgt_size"):
        G(disc_start=0, scale_input_to_tgt_size=True, discriminator=disc)
    for t in ("mean", "random"):
        with pytest.raises(NotImplementedError, match=f'target_type="{t}"'):
            D(disc_start=0, dims=3, target_type=t, discriminator=disc)
    with pytest.raises(AssertionError):
        D(disc_start=0, dims=3, target_type="median", discriminator=disc)
    with pytest.raises(AssertionError):
        G(disc_start=0, disc_loss="wasserstein", discriminator=disc)
    with pytest.raises(ValueError, match="not both"):
        G(disc_start=0, discriminator=disc, discriminator_config={"target": "torch.nn.Identity"})
    assert not hasattr(G, "log_images")


def test_full_weight_tensors_and_unknown_optimizer_raise(monkeypatch):
    from cvvae_amd import ops
    from cvvae_amd.loss import GeneralLPIPSWithDiscriminator as G
    m = G(disc_start=0, perceptual_weight=0.0, discriminator=nn.Identity())
    x = torch.zeros(1, 3, 4, 4)
    monkeypatch.setattr(ops, "_need_gpu", lambda t: None)
    monkeypatch.setattr(ops, "reduce_sum", lambda op, a, b=None: torch.zeros(()))
    monkeypatch.setattr(torch.cuda, "device", lambda *_a, **_k: __import__("contextlib").nullcontext())
    kw = dict(regularization_log={}, global_step=0, last_layer=None)
    with pytest.raises(NotImplementedError, match="weights"):
        m(x, x, optimizer_idx=0, weights=torch.ones(1, 3, 4, 4), **kw)
    with pytest.raises(NotImplementedError, match="optimizer_idx 2"):
        m(x, x, optimizer_idx=2, **kw)
    with pytest.raises(ValueError, match="4-D"):
        m(x[None], x[None], optimizer_idx=0, **kw)


def test_cpu_tensors_raise_the_no_cpu_path_error():
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    from cvvae_amd.loss import DiagonalGaussianRegularizer, LPIPSWithDiscriminatorAndDomainConstraint
    x = torch.zeros(1, 3, 5, 16, 16)
    m = LPIPSWithDiscriminatorAndDomainConstraint(disc_start=0, dims=3, discriminator=nn.Identity())
    for idx in (0, 1):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(x, x.clone().requires_grad_(True), x[:, :, ::4].clone(), regularization_log={}, optimizer_idx=idx, global_step=1,
              last_layer=None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DiagonalGaussianRegularizer()(torch.zeros(1, 8, 2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.reduce_sum(L.RED_SQ, torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.reduce_sum_bwd(L.RED_SQ, torch.zeros(8), None, torch.zeros(()))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gauss_reg(torch.zeros(1, 8, 4), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gauss_reg_bwd(torch.zeros(1, 8, 4), None, None, torch.zeros(()))
