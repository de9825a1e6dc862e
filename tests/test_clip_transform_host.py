"""The training clip transform without a GPU (cvvae_amd/data.py, lvdm/data/transform.py, include/cvvae.h cvvae_clip_from_frames_u8):
  the tap tables, evaluated in fp64, ARE torch's F.interpolate in fp64 (1e-9), crop windows included, for every case of
  tests/clip_transform_cases.py and both antialias values;
  resized_size / center_crop_origin / draw_random_crop against hand-computed torchvision values, and the draw's use of the generator;
  sample_clip_indices' invariants under a seeded random.Random;
  the lvdm.data.transform factories; the CPU eager path against the fp32 reference;
  the entry point's export, prototype and declaration, ABI 14; its refusals, reached before any launch; ops' ValueErrors."""
import ctypes
import os
import random

import pytest
import torch

import clip_transform_cases as CC
import clip_transform_ref as R

EINVAL, EUNSUPPORTED = -1, -2
AA = pytest.mark.parametrize("antialias", CC.ANTIALIAS, ids=["aa", "plain"])
CASE = pytest.mark.parametrize("case", CC.CASES, ids=[c.name for c in CC.CASES])


def _apply(tab, x, dim):
    """evaluate one axis' tables in fp64 along `dim` of x"""
    xmin, xsize, w, _ = tab
    x = x.movedim(dim, -1)
    cols = [sum(w[i, j] * x[..., int(xmin[i]) + j] for j in range(int(xsize[i]))) for i in range(len(xmin))]
    return torch.stack(cols, -1).movedim(-1, dim)


@CASE
@AA
def test_tables_are_torchs_interpolation_in_fp64(case, antialias):
    from cvvae_amd.data import resample_tables, resized_size
    _, H, W = case.frames
    if case.resize is not None:
        assert resized_size(H, W, case.resize[1], cover=case.resize[0] == "cover") == case.resized
    (top, left), (th, tw) = CC.origin_of(case), case.crop
    ytab = resample_tables(H, case.resized[0], antialias, top, top + th, dtype=torch.float64)
    xtab = resample_tables(W, case.resized[1], antialias, left, left + tw, dtype=torch.float64)
    u = CC.frames_of(case)
    if case.frame_index is not None:
        u = u[torch.tensor(case.frame_index)]
    x = u.permute(3, 0, 1, 2).double()                       # [3,T,H,W]
    got = (_apply(ytab, _apply(xtab, x, 3), 2) / 255 - 0.5) * 2
    want = R.case_reference(case.name, antialias)
    assert got.shape == want.shape == (3, len(case.frame_index or range(case.frames[0]))) + tuple(case.crop)
    err = float((got - want).abs().max())
    print(f"{case.name} antialias={antialias}: tables vs F.interpolate fp64 max|d| {err:.3e}")
    assert err <= 1e-9
    # the tables stay inside the frame, list at least one tap everywhere and their weights sum to 1
    for (mn, sz, w, k), n_in in ((ytab, H), (xtab, W)):
        assert int(mn.min()) >= 0 and int((mn + sz).max()) <= n_in and int(sz.min()) >= 1 and int(sz.max()) == k == w.shape[1]
        assert float((w.sum(1) - 1).abs().max()) < 1e-12
    # the fp32 tables are the fp64 ones rounded once, and a window is a slice of the whole axis
    w32 = resample_tables(H, case.resized[0], antialias, top, top + th)[2]
    assert w32.dtype == torch.float32 and torch.equal(w32, ytab[2].float())
    whole = resample_tables(H, case.resized[0], antialias, dtype=torch.float64)
    assert torch.equal(whole[0][top:top + th], ytab[0]) and torch.equal(whole[2][top:top + th, :ytab[3]], ytab[2])


def test_table_shapes_identity_and_last_position():
    from cvvae_amd.data import resample_tables
    mn, sz, w, k = resample_tables(7, 7, True)
    assert k == 1 and mn.tolist() == list(range(7)) and sz.tolist() == [1] * 7 and w.tolist() == [[1.0]] * 7
    assert resample_tables(7, 7, False, 2, 5)[0].tolist() == [2, 3, 4]
    mn, sz, w, k = resample_tables(4, 8, False)               # the last output position sits on the last input position: one tap
    assert (int(mn[-1]), int(sz[-1]), float(w[-1, 0])) == (3, 1, 1.0) and k == 2
    assert (int(mn[0]), float(w[0, 0]), float(w[0, 1])) == (0, 1.0, 0.0)     # source position clamped at 0
    assert (int(mn[1]), float(w[1, 0]), float(w[1, 1])) == (0, 0.75, 0.25)
    with pytest.raises(ValueError):
        resample_tables(4, 8, False, 3, 9)


def test_sizes_and_crop_origins_are_torchvisions():
    from cvvae_amd.data import center_crop_origin, draw_random_crop, resized_size
    assert resized_size(336, 596, 512) == (512, 908)          # int(512 * 596 / 336) = int(908.19)
    assert resized_size(596, 336, 512) == (908, 512)
    assert resized_size(45, 70, 24) == (24, 37) and resized_size(20, 33, [32]) == (32, 52)
    assert resized_size(45, 70, (24, 30)) == (24, 30)
    assert resized_size(40, 90, (32, 48), cover=True) == (32, 72)        # factors 0.8 and 0.533: 0.8 covers
    assert resized_size(90, 40, (32, 48), cover=True) == (108, 48)       # factors 0.356 and 1.2
    assert center_crop_origin(32, 72, 32, 48) == (0, 12)
    assert center_crop_origin(33, 48, 32, 32) == (0, 8)        # round(0.5) = 0: Python rounds half to even, as torchvision's does
    assert center_crop_origin(35, 51, 32, 32) == (2, 10)       # round(1.5) = 2, round(9.5) = 10
    for fn in (center_crop_origin, draw_random_crop):
        with pytest.raises(ValueError, match="larger"):
            fn(16, 40, 17, 17)
    g, h = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    top = int(torch.randint(0, 512 - 256 + 1, size=(1,), generator=h))
    left = int(torch.randint(0, 908 - 256 + 1, size=(1,), generator=h))
    assert draw_random_crop(512, 908, 256, 256, g) == (top, left)
    assert torch.equal(g.get_state(), h.get_state())           # exactly two draws, in that order
    before = g.get_state()
    assert draw_random_crop(256, 256, 256, 256, g) == (0, 0) and torch.equal(g.get_state(), before)    # equal sizes: no draw
    torch.manual_seed(5)
    a = draw_random_crop(40, 50, 8, 8)                          # no generator: torch's global one
    torch.manual_seed(5)
    assert a == (int(torch.randint(0, 33, size=(1,))), int(torch.randint(0, 43, size=(1,))))


def test_sample_clip_indices_invariants():
    from cvvae_amd.data import sample_clip_indices
    rng = random.Random(3)
    state = rng.getstate()
    assert sample_clip_indices(16, 17, (1, 8), rng) is None and rng.getstate() == state       # too short: no draw
    seen = set()
    for frame_num in (17, 18, 33, 40, 100, 136, 137, 500):
        for _ in range(40):
            idx, stride = sample_clip_indices(frame_num, 17, (1, 8), rng)
            assert len(idx) == 17 and all(b - a == stride for a, b in zip(idx, idx[1:]))
            assert 0 <= idx[0] and idx[-1] < frame_num and 1 <= stride <= 8
            if frame_num < 33:                                   # no stride above 1 fits: drawn or fallen back to, it is 1
                assert stride == 1
            seen.add((frame_num, stride, idx[0]))
    assert len({s for f, s, _ in seen if f == 500}) == 8 and len({i for f, _, i in seen if f == 500}) > 10
    assert {s for f, s, _ in seen if f == 17} == {1} and {i for f, _, i in seen if f == 17} == {0}
    # the fallback: 33 frames cannot hold stride 3 (needs 49); the stride becomes 33 // 17 = 1
    class Fixed:
        def __init__(self, vals): self.vals = list(vals)
        def randint(self, a, b): return self.vals.pop(0)
    r = Fixed([3, 5])
    assert sample_clip_indices(33, 17, (1, 8), r) == ([5 + i for i in range(17)], 1) and r.vals == []     # start drawn from [0, 16]
    r = Fixed([2])
    assert sample_clip_indices(33, 17, (1, 8), r) == ([2 * i for i in range(17)], 2) and r.vals == []     # no slack: no start draw
    r = Fixed([2])
    assert sample_clip_indices(100, 17, (1, 8), r, random_start_frame=False) == ([2 * i for i in range(17)], 2)


def test_factories_return_configured_objects():
    from cvvae_amd.data import ClipTransform, ImageTransform
    from lvdm.data import transform as LT
    from lvdm.util import instantiate_from_config
    t = LT.get_webvid_spatial_transform()
    assert isinstance(t, ClipTransform) and (t.resolution, t.resize_resolution, t.random_crop, t.cover) == ((256, 512), 256, False, False)
    assert t.antialias and t.dtype == torch.float32 and t.device is None
    t = instantiate_from_config({"target": "lvdm.data.transform.get_webvid_spatial_transform",
                                 "params": {"resolution": 256, "resize_resolution": 512, "random_crop": True}})
    assert (t.resolution, t.resize_resolution, t.random_crop, t.cover) == ((256, 256), 512, True, False)
    t = LT.get_video_spatial_transform([32, 48], random_crop=True, antialias=False, dtype=torch.bfloat16)
    assert (t.resolution, t.resize_resolution, t.random_crop, t.cover, t.antialias, t.dtype) == \
        ((32, 48), (32, 48), True, True, False, torch.bfloat16)
    assert t.plan(40, 90, origin=(0, 3)) == (32, 72, 0, 3)
    i = LT.get_image_transform(32)
    assert isinstance(i, ImageTransform) and i.resolution == (32, 32)
    with pytest.raises(ValueError, match="PIL"):
        LT.get_image_transform(32, to_tensor=False)
    import lvdm.data
    assert lvdm.data.get_image_transform is LT.get_image_transform


@CASE
@AA
def test_cpu_eager_path_is_the_fp32_reference(case, antialias):
    t = CC.transform_of(case, antialias)
    origin = None if case.origin == "centre" else case.origin
    got = t(CC.frames_of(case), case.frame_index, origin=origin)
    want = R.case_reference(case.name, antialias, torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    out = torch.full((2,) + tuple(want.shape), 9.0)
    assert t(CC.frames_of(case), case.frame_index, origin=origin, out=out[1]) is not None
    assert torch.equal(out[1], want) and bool((out[0] == 9.0).all())


def test_cpu_paths_of_the_other_entries():
    from cvvae_amd.data import ClipTransform, ImageTransform, collate_clips
    img = CC.frames_of(CC.IMAGE)
    want = R.image_reference(img, CC.IMAGE.resized, CC.IMAGE.crop)
    assert torch.equal(ImageTransform(32)(img), want)
    assert torch.equal(ImageTransform(32)(img[0]), want)       # [H,W,3]: a one-frame clip (add_time_dim)
    # random crop: the generator's draw decides the window
    c = CC.BY_NAME["down_nonint"]
    t = ClipTransform(16, 24, random_crop=True)
    g, h = torch.Generator().manual_seed(2), torch.Generator().manual_seed(2)
    top, left = int(torch.randint(0, 9, (1,), generator=h)), int(torch.randint(0, 22, (1,), generator=h))
    assert torch.equal(t(CC.frames_of(c), generator=g), R.reference(CC.frames_of(c), (24, 37), (top, left), (16, 16), True, dtype=torch.float32))
    assert t.plan(45, 70, torch.Generator().manual_seed(2)) == (24, 37, top, left)
    # collate: samples of different raw resolution into one batch
    a, b = CC.frames_of(c), CC.frames_of(CC.Case("b", (3, 30, 52), None, None, None, None, None))
    tc = ClipTransform(16, 24)
    batch = collate_clips([a, b], tc)["frames"]
    assert batch.shape == (2, 3, 3, 16, 16) and torch.equal(batch[0], tc(a)) and torch.equal(batch[1], tc(b))
    with pytest.raises(ValueError, match="larger"):
        ClipTransform(64, 24)(a)
    with pytest.raises(ValueError, match="uint8"):
        tc(a.float())
    with pytest.raises(ValueError, match="outside"):
        tc(a, [0, 3])
    with pytest.raises(ValueError, match=r"size must be \(h, w\)"):
        ClipTransform(16, 24, cover=True)


def test_entry_point_is_exported_typed_and_declared_and_the_abi_version_stays():
    from cvvae_amd import _lib
    lib = _lib.load()
    n = "cvvae_clip_from_frames_u8"
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "cvvae.h")).read()
    assert "#define CVVAE_ABI_VERSION 14" in header
    assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header
    assert getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1] and len(_lib.PROTOTYPES[n][1]) == 24
    assert "clip_kernels.hip" in open(os.path.join(_lib._HERE, "csrc", "Makefile")).read()
    assert "clip_kernels.hip" in _lib.TRAINING_ONLY_SOURCES     # no launch of an encode / decode step comes from it


NAMES = ["frames", "vin", "T_in", "H", "W", "frame_index", "T_out", "ymin", "ysize", "yw", "kh", "oh", "xmin", "xsize", "xw", "kw", "ow",
         "y_lo", "y_hi", "x_lo", "x_hi", "out", "vout", "stream"]


def test_every_refusal_is_reached_before_any_launch():
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value   # a non-NULL, 8-byte aligned HOST pointer: the checks never dereference it or launch
    T_in, H, W, oh, ow = 5, 40, 60, 16, 24

    def views(**kw):
        vin, vout = L.ClipView(), L.ClipView()
        vin.layout, vin.dtype, vin.sb, vin.sc, vin.st, vin.sy = L.CLIP_THWC_U8, 0, 0, 1, H * W * 3, W * 3
        vout.layout, vout.dtype, vout.sb, vout.sc, vout.st, vout.sy = L.CLIP_NCTHW, L.F32, 0, 4 * oh * ow, oh * ow, ow
        for k, v in kw.items():
            setattr(vin if k.startswith("in_") else vout, k.split("_", 1)[1], v)
        return vin, vout

    def call(view_in=None, view_out=None, **kw):
        dv = views()
        vin, vout = view_in or dv[0], view_out or dv[1]
        args = [p, ctypes.byref(vin), T_in, H, W, None, 4, p, p, p, 3, oh, p, p, p, 3, ow, 2, 30, 0, 60, p, ctypes.byref(vout), None]
        for k, v in kw.items():
            args[NAMES.index(k)] = v
        return lib.cvvae_clip_from_frames_u8(*args)

    # CVVAE_EINVAL
    for k in ("frames", "vin", "ymin", "ysize", "yw", "xmin", "xsize", "xw", "out", "vout"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("T_in", "H", "W", "T_out", "oh", "ow"):
        for bad in (0, -1):
            assert call(**{k: bad}) == EINVAL, (k, bad)
    for k in ("kh", "kw"):
        assert call(**{k: 0}) == EINVAL, k
    for k in ("in_st", "in_sy", "out_sc", "out_st", "out_sy"):
        v = views(**{k: -1})
        assert call(view_in=v[0], view_out=v[1]) == EINVAL, k
    v = views(in_sy=W * 3 - 1)
    assert call(view_in=v[0]) == EINVAL                           # sy smaller than a row of 3W bytes
    v = views(out_sy=ow - 1)
    assert call(view_out=v[1]) == EINVAL
    assert call(out=p + 2) == EINVAL                          # fp32 output off a 4-byte boundary
    v = views(out_dtype=L.BF16)
    assert call(view_out=v[1], out=p + 1) == EINVAL
    for k, bad in (("y_lo", -1), ("y_hi", H + 1), ("y_lo", 30), ("x_lo", -1), ("x_hi", W + 1), ("x_hi", 0)):
        assert call(**{k: bad}) == EINVAL, (k, bad)           # a span that is empty or leaves the frame
    # CVVAE_EUNSUPPORTED
    v = views(in_layout=L.CLIP_NCTHW)
    assert call(view_in=v[0]) == EUNSUPPORTED
    v = views(out_layout=L.CLIP_THWC_U8)
    assert call(view_out=v[1]) == EUNSUPPORTED
    for bad in (L.F32Q, 7, -1):
        v = views(out_dtype=bad)
        assert call(view_out=v[1]) == EUNSUPPORTED, bad
    big = (1 << 20) + 1
    v = views(in_sy=3 * big)
    assert call(view_in=v[0], W=big, x_hi=60) == EUNSUPPORTED
    assert call(H=big) == EUNSUPPORTED
    v = views(out_sy=big)
    assert call(view_out=v[1], ow=big) == EUNSUPPORTED
    assert call(oh=big) == EUNSUPPORTED
    assert call(T_out=65536) == EUNSUPPORTED
    assert call(kh=65) == EUNSUPPORTED                        # one output row's taps do not fit the 64-row LDS stage
    # the order of the header: a bad extent beside an unknown dtype is EINVAL
    v = views(out_dtype=7)
    assert call(view_out=v[1], oh=0) == EINVAL


def test_ops_value_errors_come_before_the_device():
    from cvvae_amd import ops
    n = 4
    tab = ops.ClipAxisTable(torch.zeros(n, dtype=torch.int32), torch.ones(n, dtype=torch.int32), torch.ones(n, 1), 1, 0, 4)
    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    out = torch.empty((3, 2, n, n))
    with pytest.raises(ValueError, match="uint8"):
        ops.clip_from_frames_u8(frames.float(), None, tab, tab, out)
    with pytest.raises(ValueError, match=r"\[T,H,W,3\]"):
        ops.clip_from_frames_u8(frames[..., :2], None, tab, tab, out)
    with pytest.raises(ValueError, match=r"\[T,H,W,3\]"):
        ops.clip_from_frames_u8(frames[0], None, tab, tab, out)
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.clip_from_frames_u8(frames, None, tab, tab, out)          # CPU frames: refused, nothing falls back
    args = dict(frames=frames, frame_index=None, ytab=tab, xtab=tab, out_slot=out)

    def check(match, **kw):
        a = dict(args, **kw)
        with pytest.raises(ValueError, match=match):
            ops.check_clip_operands(_Cuda(a["frames"]), a["frame_index"], a["ytab"], a["xtab"], a["out_slot"])

    check("frame_index", frame_index=torch.zeros(2, dtype=torch.int64))
    check("frame_index", frame_index=torch.zeros((2, 1), dtype=torch.int32))
    check("ytab", ytab=ops.ClipAxisTable(tab.amin.long(), tab.asize, tab.w, 1, 0, 4))
    check("xtab", xtab=ops.ClipAxisTable(tab.amin, tab.asize, tab.w.double(), 1, 0, 4))
    check("xtab", xtab=ops.ClipAxisTable(tab.amin, tab.asize[:3], tab.w, 1, 0, 4))
    check("ytab touches", ytab=ops.ClipAxisTable(tab.amin, tab.asize, tab.w, 1, 0, 9))
    check("fp16 / bf16 / fp32", out_slot=out.double())
    check(r"the slot is \[3,2,4,4\]", out_slot=torch.empty((3, 3, n, n)))
    check(r"the slot is \[3,1,4,4\]", frame_index=torch.zeros(1, dtype=torch.int32))
    check("written in place", out_slot=torch.empty((3, 2, n, 2 * n))[..., ::2])
    ops.check_clip_operands(_Cuda(frames), None, tab, tab, torch.empty((3, 2, n, n + 3))[..., :n])      # padded rows are fine


class _Cuda:
    """a CPU tensor that says it is on the GPU: lets check_clip_operands' later checks be reached on a machine without one (the
    checks only look at dtype, shape, strides and device)"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, k):
        return getattr(self._t, k)
