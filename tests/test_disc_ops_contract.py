"""The contract of the discriminator passes (csrc/disc_kernels.hip, cvvae_amd/disc_ops.py) that holds without a GPU: the four C entry
points are exported, typed and declared under an unchanged ABI version, refuse bad arguments before any launch (checked with host
pointers, which a launch would fault on), and the Python layers have no CPU path."""
import ctypes
import os

import pytest
import torch

ENTRIES = ["cvvae_avgpool3d_down", "cvvae_avgpool3d_down_bwd", "cvvae_gn_leaky_apply", "cvvae_leaky_bwd"]
EINVAL, EUNSUPPORTED = -1, -2


def _p():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)  # a non-NULL HOST pointer: the checks never dereference it or launch


def test_entry_points_are_exported_with_prototypes_and_the_abi_version_stays():
    from cvvae_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "cvvae.h")).read()
    assert "#define CVVAE_ABI_VERSION 14" in header
    for n in ENTRIES:
        assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header, n
        assert getattr(lib, n).restype is ctypes.c_int32 and list(getattr(lib, n).argtypes) == _lib.PROTOTYPES[n][1]
    from cvvae_amd import disc_ops, ops
    for n in ("avgpool3d_down", "avgpool3d_down_bwd", "gn_leaky_apply", "leaky_bwd"):
        assert callable(getattr(ops, n)), n
    assert callable(disc_ops.avg_pool_down3d) and callable(disc_ops.group_norm_leaky)


@pytest.mark.parametrize("name", ["cvvae_avgpool3d_down", "cvvae_avgpool3d_down_bwd"])
def test_pool_entry_points_refuse_bad_arguments_before_any_launch(name):
    from cvvae_amd import _lib as L
    fn = getattr(L.load(), name)
    _keep, p = _p()
    good = dict(B=1, T=3, H=4, W=4, C=8)
    call = lambda dt=L.F32, a=p, b=p, **kw: fn(dt, a, b, *[{**good, **kw}[k] for k in "BTHWC"], None)  # noqa: E731
    assert call(a=None) == EINVAL and call(b=None) == EINVAL
    for k in "BTHWC":
        assert call(**{k: 0}) == EINVAL and call(**{k: -2}) == EINVAL, k
    assert call(H=1) == EINVAL and call(W=1) == EINVAL          # nothing to pool
    assert call(C=12) == EUNSUPPORTED                            # not a multiple of the 8-channel vector
    for dt in (7, -1, L.F32Q, L.F32Q6):
        assert call(dt=dt) == EUNSUPPORTED, dt
    assert call(B=1 << 31, T=2) == EUNSUPPORTED                  # frame count beyond the 32-bit split of the index
    assert call(a=None, C=12) == EINVAL                          # a NULL pointer is reported first


def test_gn_leaky_apply_refuses_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    fn = L.load().cvvae_gn_leaky_apply
    _keep, p = _p()
    assert fn(L.F16, None, p, p, p, 1, 4, 8, 0.2, None) == EINVAL
    assert fn(L.F16, p, p, p, None, 1, 4, 8, 0.2, None) == EINVAL
    assert fn(L.F16, p, None, p, p, 1, 4, 8, 0.2, None) == EINVAL      # one table without the other
    assert fn(L.F16, p, p, None, p, 1, 4, 8, 0.2, None) == EINVAL
    for rows, per_row, C in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (-1, 4, 8), (1, -4, 8), (1, 4, -8)):
        assert fn(L.F16, p, p, p, p, rows, per_row, C, 0.2, None) == EINVAL, (rows, per_row, C)
        assert fn(L.F16, p, None, None, p, rows, per_row, C, 0.2, None) == EINVAL, (rows, per_row, C)
    assert fn(L.F16, p, p, p, p, 1, 4, 12, 0.2, None) == EUNSUPPORTED
    assert fn(L.BF16, p, None, None, p, 1, 4, 12, 0.2, None) == EUNSUPPORTED   # the bare form has the same channel rule
    assert fn(5, p, p, p, p, 1, 4, 8, 0.2, None) == EUNSUPPORTED
    assert fn(L.F32Q, p, None, None, p, 1, 4, 8, 0.2, None) == EUNSUPPORTED


def test_leaky_bwd_refuses_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    fn = L.load().cvvae_leaky_bwd
    _keep, p = _p()
    assert fn(L.F32, None, p, p, 16, 0.2, None) == EINVAL
    assert fn(L.F32, p, None, p, 16, 0.2, None) == EINVAL
    assert fn(L.F32, p, p, None, 16, 0.2, None) == EINVAL
    assert fn(L.F32, p, p, p, 0, 0.2, None) == EINVAL
    assert fn(L.F32, p, p, p, -8, 0.2, None) == EINVAL
    for slope in (0.0, -0.2, float("nan")):                              # the mask comes from the output: slope must be > 0
        assert fn(L.F32, p, p, p, 16, slope, None) == EINVAL, slope
    assert fn(9, p, p, p, 16, 0.2, None) == EUNSUPPORTED
    assert fn(L.F32Q6, p, p, p, 16, 0.2, None) == EUNSUPPORTED


def test_cpu_tensors_raise_the_no_cpu_path_error():
    from cvvae_amd import disc_ops, ops
    x = torch.zeros(1, 3, 4, 4, 8)
    w, b = torch.ones(8), torch.zeros(8)
    for call in (lambda: ops.avgpool3d_down(x), lambda: ops.avgpool3d_down_bwd(torch.zeros(1, 2, 2, 2, 8), x.shape),
                 lambda: ops.gn_leaky_apply(x, None), lambda: ops.leaky_bwd(x, x),
                 lambda: disc_ops.avg_pool_down3d(x), lambda: disc_ops.avg_pool_down3d(x.clone().requires_grad_(True)),
                 lambda: disc_ops.group_norm_leaky(x, w, b, num_groups=2), lambda: disc_ops.group_norm_leaky(x)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_wrappers_refuse_strided_tensors_and_half_an_affine(monkeypatch):
    from cvvae_amd import disc_ops, ops
    monkeypatch.setattr(ops, "_need_gpu", lambda t: None)
    x = torch.zeros(1, 8, 4, 4, 3).permute(0, 4, 2, 3, 1)     # NDHWC shape, NCDHW memory
    assert x.shape == (1, 3, 4, 4, 8) and not x.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        ops.avgpool3d_down(x)
    with pytest.raises(ValueError, match="contiguous"):
        ops.gn_leaky_apply(x, None)
    with pytest.raises(ValueError, match="contiguous"):
        ops.leaky_bwd(x, x)
    with pytest.raises(ValueError, match="pooled shape"):
        ops.avgpool3d_down_bwd(torch.zeros(1, 1, 2, 2, 8), (1, 3, 4, 4, 8))   # T = 3 pools to 2 frames, not 1
    with pytest.raises(ValueError, match="come together"):
        disc_ops.group_norm_leaky(x.contiguous(), torch.ones(8), None)
    with pytest.raises(ValueError, match="slope > 0"):
        disc_ops.group_norm_leaky(x.contiguous(), slope=0.0)
