"""The contract of cvvae_frame_metrics (include/cvvae.h, csrc/metrics_kernels.hip) that holds without a GPU: the symbols are exported,
typed and declared, the ABI version stays 14, every refusal is reached before any launch, and the workspace size is pure host code."""
import ctypes
import os

import pytest

EINVAL, EUNSUPPORTED = -1, -2
ENTRIES = ["cvvae_frame_metrics_workspace_bytes", "cvvae_frame_metrics"]


def test_entry_points_are_exported_with_prototypes_and_the_abi_version_stays():
    from cvvae_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "cvvae.h")).read()
    assert "#define CVVAE_ABI_VERSION 14" in header
    for n in ENTRIES:
        assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header, n
        assert getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1]
    assert "CVVAE_CLIP_NCTHW = 0, CVVAE_CLIP_THWC_U8 = 1" in header and (_lib.CLIP_NCTHW, _lib.CLIP_THWC_U8) == (0, 1)
    assert ctypes.sizeof(_lib.ClipView) == 40 and _lib.ClipView.sb.offset == 8 and _lib.ClipView.sy.offset == 32
    assert "metrics_kernels.hip" in open(os.path.join(_lib._HERE, "csrc", "Makefile")).read()
    assert "metrics_kernels.hip" in _lib.TRAINING_ONLY_SOURCES      # no launch of an encode / decode step comes from it


def _views(L, la=0, da=1, lb=0, db=1, W=13, **kw):
    va, vb = L.ClipView(), L.ClipView()
    for v, lay, dt in ((va, la, da), (vb, lb, db)):
        v.layout, v.dtype = lay, dt
        row = 3 * W if lay == L.CLIP_THWC_U8 else W
        v.sb, v.sc, v.st, v.sy = 3 * 2 * 12 * row, 2 * 12 * row, 12 * row, row
    for k, val in kw.items():
        setattr(va, k, val)
    return va, vb


def test_every_refusal_is_reached_before_any_launch():
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL, 8-byte aligned HOST pointer: the checks never dereference it or launch
    va, vb = _views(L)
    ok = [p, ctypes.byref(va), p, ctypes.byref(vb), 1, 2, 12, 13, 1, 1, p, p, p, p, None]

    def call(**kw):
        names = ["a", "va", "b", "vb", "B", "T", "H", "W", "quantize", "want_ssim", "sse", "psnr", "ssim", "ws", "stream"]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.cvvae_frame_metrics(*args)

    # CVVAE_EINVAL: NULL pointers, extents, strides
    for k in ("a", "va", "b", "vb", "sse", "psnr", "ws"):
        assert call(**{k: None}) == EINVAL, k
    assert call(ssim=None) == EINVAL                      # wanted, nowhere to put it
    for k in ("B", "T", "H", "W"):
        for bad in (0, -1):
            assert call(**{k: bad}) == EINVAL, (k, bad)
    for k in ("sb", "sc", "st", "sy"):
        nv, _ = _views(L, **{k: -1})
        assert call(va=ctypes.byref(nv)) == EINVAL and call(vb=ctypes.byref(nv)) == EINVAL, k
    nv, _ = _views(L, sy=12)
    assert call(va=ctypes.byref(nv)) == EINVAL and call(vb=ctypes.byref(nv)) == EINVAL      # a row is 13 elements
    ua, ub = _views(L, la=L.CLIP_THWC_U8, lb=L.CLIP_THWC_U8)
    assert ua.sy == 39
    ua.sy = 38                                            # ... or 39 bytes
    assert call(va=ctypes.byref(ua), vb=ctypes.byref(ub)) == EINVAL
    odd = ctypes.c_void_p(p.value + 4)
    assert call(sse=odd) == EINVAL and call(ws=odd) == EINVAL and call(psnr=ctypes.c_void_p(p.value + 2)) == EINVAL

    # CVVAE_EUNSUPPORTED: layout, dtype, B with uint8 frames, SSIM's window, the grid's limits
    for bad in (2, -1, 7):
        nv, _ = _views(L, la=bad)
        assert call(va=ctypes.byref(nv)) == EUNSUPPORTED and call(vb=ctypes.byref(nv)) == EUNSUPPORTED, bad
    for bad in (L.F32Q, L.F32Q6, 9, -1):
        nv, _ = _views(L, da=bad)
        assert call(va=ctypes.byref(nv)) == EUNSUPPORTED and call(vb=ctypes.byref(nv)) == EUNSUPPORTED, bad
    ua, _ = _views(L, la=L.CLIP_THWC_U8)
    assert call(va=ctypes.byref(ua), B=2) == EUNSUPPORTED and call(vb=ctypes.byref(ua), B=2) == EUNSUPPORTED
    wide, wide_b = _views(L, W=40)
    assert call(H=10, W=40, va=ctypes.byref(wide), vb=ctypes.byref(wide_b)) == EUNSUPPORTED
    assert call(H=12, W=10) == EUNSUPPORTED
    assert call(B=256, T=256) == EUNSUPPORTED             # B * T frames exceed the grid's second dimension
    huge, huge_b = _views(L, W=(1 << 20) + 1)
    assert call(W=(1 << 20) + 1, va=ctypes.byref(huge), vb=ctypes.byref(huge_b)) == EUNSUPPORTED
    assert call(H=(1 << 20) + 1) == EUNSUPPORTED


def test_workspace_bytes_is_zero_for_refused_extents_and_positive_otherwise():
    from cvvae_amd import _lib as L
    lib = L.load()
    ws = lib.cvvae_frame_metrics_workspace_bytes
    assert ws(1, 1, 11, 11, 1) == 16 and ws(1, 1, 1, 1, 0) == 16          # one tile, two doubles
    assert ws(2, 3, 16 + 10, 32 + 10, 1) == 6 * 16 and ws(2, 3, 17 + 10, 33 + 10, 1) == 6 * 4 * 16
    assert ws(1, 17, 512, 512, 1) == 17 * 32 * 16 * 16 and ws(1, 17, 512, 512, 0) == 17 * 32 * 16 * 16
    for bad in ((0, 1, 12, 12, 1), (1, 0, 12, 12, 1), (1, 1, 0, 12, 0), (1, 1, 12, -3, 0), (1, 1, 10, 40, 1), (1, 1, 40, 10, 1),
                (256, 256, 12, 12, 0), (1, 1, (1 << 20) + 1, 12, 0), (1, 1, 12, (1 << 20) + 1, 1)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1, 10, 40, 0) > 0                                         # PSNR alone has no minimum size


def test_wrapper_has_no_cpu_path():
    import torch
    from cvvae_amd import ops
    f = torch.zeros(1, 12, 13, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.frame_metrics(f, f)
