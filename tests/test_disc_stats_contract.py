"""The contract of the two statistics-producing discriminator passes (cvvae_gn_leaky_apply_stats, cvvae_avgpool3d_down_stats and the
host function cvvae_pass_gn_slabs; csrc/disc_kernels.hip) that holds without a GPU: exported and typed under an unchanged ABI version,
bad arguments refused before any launch (checked with host pointers, which a launch would fault on), a consistent slab count, and no
CPU path in the wrappers."""
import ctypes
import os

import pytest
import torch

ENTRIES = ["cvvae_pass_gn_slabs", "cvvae_avgpool3d_down_stats", "cvvae_gn_leaky_apply_stats"]
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
        assert list(getattr(lib, n).argtypes) == _lib.PROTOTYPES[n][1]
    assert lib.cvvae_pass_gn_slabs.restype is ctypes.c_int64
    assert lib.cvvae_avgpool3d_down_stats.restype is ctypes.c_int32 and lib.cvvae_gn_leaky_apply_stats.restype is ctypes.c_int32


def test_gn_leaky_apply_stats_refuses_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    fn = L.load().cvvae_gn_leaky_apply_stats
    _keep, p = _p()
    good = dict(dt=L.F16, x=p, sc=p, sh=p, y=p, rows=1, per_row=4, C=64, slope=0.2, G=32, part=p)
    call = lambda **kw: fn(*[{**good, **kw}[k] for k in good], None)  # noqa: E731
    assert call(x=None) == EINVAL and call(y=None) == EINVAL
    assert call(sc=None) == EINVAL and call(sh=None) == EINVAL          # one table without the other
    for k in ("rows", "per_row", "C"):
        assert call(**{k: 0}) == EINVAL and call(**{k: -4}) == EINVAL, k
        assert call(**{k: 0}, sc=None, sh=None) == EINVAL, k
    assert call(G=-1) == EINVAL
    assert call(C=12, G=2) == EUNSUPPORTED                              # not a multiple of the 8-channel vector
    assert call(dt=5) == EUNSUPPORTED and call(dt=L.F32Q, sc=None, sh=None) == EUNSUPPORTED
    assert call(G=24) == EUNSUPPORTED                                   # groups do not divide C
    assert call(C=40, G=8) == EUNSUPPORTED                              # 5 channels per group: odd
    assert call(C=4096, G=32) == EUNSUPPORTED                           # more channel vectors than a workgroup has threads
    assert call(rows=65536) == EUNSUPPORTED                             # rows are a grid dimension
    # the plain pass behind out_groups = 0 or out_partials = NULL keeps its own checks
    assert call(G=0, x=None) == EINVAL and call(part=None, C=12) == EUNSUPPORTED and call(G=0, sc=None) == EINVAL


def test_avgpool3d_down_stats_refuses_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    fn = L.load().cvvae_avgpool3d_down_stats
    _keep, p = _p()
    good = dict(dt=L.F32, x=p, y=p, B=1, T=3, H=4, W=4, C=64, G=32, part=p)
    call = lambda **kw: fn(*[{**good, **kw}[k] for k in good], None)  # noqa: E731
    assert call(x=None) == EINVAL and call(y=None) == EINVAL
    for k in "BTHWC":
        assert call(**{k: 0}) == EINVAL and call(**{k: -2}) == EINVAL, k
    assert call(H=1) == EINVAL and call(W=1) == EINVAL                   # nothing to pool
    assert call(G=-32) == EINVAL
    assert call(C=12, G=2) == EUNSUPPORTED
    for dt in (7, -1, L.F32Q, L.F32Q6):
        assert call(dt=dt) == EUNSUPPORTED, dt
    assert call(G=24) == EUNSUPPORTED and call(C=40, G=8) == EUNSUPPORTED and call(C=4096) == EUNSUPPORTED
    assert call(B=65536) == EUNSUPPORTED
    assert call(B=1 << 31, T=2) == EUNSUPPORTED                          # frame count beyond the 32-bit split of the index
    assert call(G=0, x=None) == EINVAL and call(part=None, H=1) == EINVAL and call(part=None, C=12) == EUNSUPPORTED


def test_pass_gn_slabs_is_pure_host_code_and_consistent():
    from cvvae_amd import _lib as L
    lib = L.load()
    f = lib.cvvae_pass_gn_slabs
    assert f(0, 4, 64, 32) == EINVAL and f(1, 0, 64, 32) == EINVAL and f(1, 4, 0, 32) == EINVAL and f(1, 4, 64, 0) == EINVAL
    assert f(1, 4, 12, 2) == EUNSUPPORTED and f(1, 4, 64, 24) == EUNSUPPORTED and f(1, 4, 40, 8) == EUNSUPPORTED
    assert f(1, 4, 4096, 32) == EUNSUPPORTED and f(65536, 4, 64, 32) == EUNSUPPORTED and f(1, 4, 1024, 512) == EUNSUPPORTED
    # cvvae_gn_finalize takes any positive slab count.  The network's tensors (2, 4, 8, 16 channels per group), an odd vector count, tiny and large rows, many rows
    for rows, per_row, C, G in ((1, 9 * 128 * 128, 64, 32), (1, 9 * 64 * 64, 128, 32), (2, 3 * 18 * 14, 256, 32), (2, 1, 512, 32),
                                (1, 5 * 16 * 16, 512, 32), (3, 105, 40, 4), (1, 1 << 30, 96, 8), (4000, 100000, 64, 32),
                                (65535, 7, 2048, 256)):
        slabs = f(rows, per_row, C, G)
        assert 0 < slabs <= per_row and slabs * rows <= max(2048, rows), (rows, per_row, C, G, slabs)
        assert f(rows, per_row, C, G) == slabs      # a function of its arguments: the allocation and the launch agree
    assert f(1, 9 * 128 * 128, 64, 32) > 64         # the first LeakyReLU at [1,3,17,256,256]: enough workgroups to cover the CUs


def test_cpu_tensors_raise_the_no_cpu_path_error():
    from cvvae_amd import ops
    x = torch.zeros(1, 3, 4, 4, 64)
    for call in (lambda: ops.avgpool3d_down(x, gn_out=32), lambda: ops.gn_leaky_apply(x, None, gn_out=32)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
