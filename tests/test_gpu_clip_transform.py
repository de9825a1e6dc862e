"""cvvae_clip_from_frames_u8 on the MI355X, through the C ABI with the output inside a larger poisoned buffer, for every case of
tests/clip_transform_cases.py, both antialias values and every output dtype:
  within tol32 = (kh + kw + 4) * 2^-23 (+ half an ulp of the output dtype below 1) of reference (a): torch's F.interpolate in fp64,
  crop, normalise (tests/clip_transform_ref.py) -- never of torch's fp32 result, whose own error (printed beside the kernel's) is
  far larger; `identity` and `image` bit for bit eager torch; two runs identical bits; no byte outside the slot written;
  tile independence: a crop and a larger crop that contains it at another origin agree bit for bit on the overlap;
  slot 1 of a poisoned batch, padded rows and a slot 1 element off a 16-byte boundary; a frame-strided input view;
  collate_clips, the pinned-CPU upload path, and one engine iteration on a collated batch."""
import ctypes

import pytest
import torch

import clip_transform_cases as CC
import clip_transform_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256
POISON = 0xA5
AA = pytest.mark.parametrize("antialias", CC.ANTIALIAS, ids=["aa", "plain"])
DT = pytest.mark.parametrize("dtype", list(CC.DTYPES.values()), ids=list(CC.DTYPES))


def _tables(H, W, resized, origin, crop, antialias):
    """device tables of a crop window, straight from resample_tables (not through ClipTransform's cache)"""
    from cvvae_amd import ops
    from cvvae_amd.data import resample_tables
    tabs = []
    for n_in, n_out, lo, n in ((H, resized[0], origin[0], crop[0]), (W, resized[1], origin[1], crop[1])):
        mn, sz, w, k = resample_tables(n_in, n_out, antialias, lo, lo + n)
        tabs.append(ops.ClipAxisTable(mn.cuda(), sz.cuda(), w.cuda(), k, int(mn.min()), int((mn + sz).max())))
    return tabs


def _call(frames, resized, origin, crop, antialias, dtype, frame_index=None, shift=0, row_pad=0, slot=0, slots=1):
    """one call through the C ABI: device uint8 frames (a view is read in place) -> slot `slot` of a [slots,3,T,h,w] batch that lies
    `shift` elements behind a 16-byte boundary inside a poisoned buffer, its rows padded by row_pad elements -> that slot on the CPU.
    Asserts that every byte outside the slot's elements still holds the poison."""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    lib = L.load()
    T_in, H, W, _ = frames.shape
    ytab, xtab = _tables(H, W, resized, origin, crop, antialias)
    fi = None if frame_index is None else torch.tensor(frame_index, dtype=torch.int32, device="cuda")
    T = T_in if fi is None else len(frame_index)
    th, tw = crop
    esz = torch.empty((), dtype=dtype).element_size()
    sy = tw + row_pad
    n_el = slots * 3 * T * th * sy
    off = GUARD + shift * esz
    buf = torch.full((off + n_el * esz + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    batch = buf[off:off + n_el * esz].view(dtype).view(slots, 3, T, th, sy)[..., :tw]
    out = batch[slot]
    frames, vin = ops._clip_view(frames)
    vout = L.ClipView()
    vout.layout, vout.dtype, vout.sb = L.CLIP_NCTHW, ops._DT[dtype], 0
    vout.sc, vout.st, vout.sy, _ = out.stride()
    L.check(lib.cvvae_clip_from_frames_u8(frames.data_ptr(), ctypes.byref(vin), T_in, H, W, None if fi is None else fi.data_ptr(), T,
                                          ytab.amin.data_ptr(), ytab.asize.data_ptr(), ytab.w.data_ptr(), ytab.k, th,
                                          xtab.amin.data_ptr(), xtab.asize.data_ptr(), xtab.w.data_ptr(), xtab.k, tw,
                                          ytab.lo, ytab.hi, xtab.lo, xtab.hi, out.data_ptr(), ctypes.byref(vout), ops._stream(frames)),
            "cvvae_clip_from_frames_u8")
    torch.cuda.synchronize()
    got = out.cpu().contiguous()
    batch.view(torch.int16 if esz == 2 else torch.int32)[slot] = 0xA5A5 - (1 << 16) if esz == 2 else 0xA5A5A5A5 - (1 << 32)
    assert bool((buf.cpu() == POISON).all()), "bytes outside the slot were written"
    return got


def _case_call(case, antialias, dtype, **kw):
    return _call(CC.frames_of(case).cuda(), case.resized, CC.origin_of(case), case.crop, antialias, dtype, case.frame_index, **kw)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                     b.view(torch.int16 if b.element_size() == 2 else torch.int32))


@pytest.mark.parametrize("case", CC.CASES, ids=[c.name for c in CC.CASES])
@AA
@DT
def test_kernel_is_within_the_derived_bound_of_torch_fp64(case, antialias, dtype):
    want = R.case_reference(case.name, antialias)
    got = _case_call(case, antialias, dtype)
    kh, kw = R.case_taps(case, antialias)
    tol = R.tol32(kh, kw) + CC.DTYPE_TERM[dtype]
    err = float((got.double() - want).abs().max())
    err_torch = float((R.case_reference(case.name, antialias, torch.float32).double() - want).abs().max())
    print(f"{case.name} antialias={antialias} {dtype}: kernel max|d| {err:.3e}  torch fp32 max|d| {err_torch:.3e}  "
          f"bound {tol:.3e} (kh={kh}, kw={kw})")
    assert got.dtype == dtype and got.shape == want.shape
    assert err <= tol
    assert _bits(got, _case_call(case, antialias, dtype)), "two runs on the same inputs differ"
    if case.name == "identity":        # one tap of weight 1.0 on each axis: (u / 255 - 0.5) * 2 in fp32, rounded once
        assert _bits(got, R.case_reference(case.name, antialias, torch.float32).to(dtype))
    if case.name == "gather":          # frame_index = [8, 0, 4, 4]: output frames 2 and 3 come from the same input frame
        assert _bits(got[:, 2], got[:, 3]) and not _bits(got[:, 0], got[:, 1])


@DT
def test_image_datapipe_is_eager_torch_bit_for_bit(dtype):
    from cvvae_amd.data import ImageTransform
    img = CC.frames_of(CC.IMAGE)
    want = R.image_reference(img, CC.IMAGE.resized, CC.IMAGE.crop).to(dtype)
    t = ImageTransform(32, dtype=dtype)
    assert _bits(t(img.cuda()).cpu(), want)
    assert _bits(t(img[0].cuda()).cpu(), want)               # [H,W,3]
    assert _bits(ImageTransform(32, dtype=dtype, device="cuda")(img).cpu(), want)


@AA
@DT
def test_a_pixels_bits_do_not_depend_on_its_place_in_a_tile(antialias, dtype):
    """crop A (17 x 70 at (40, 90)) inside crop B (60 x 140 at (7, 31)): A's pixels fall in other columns of other 64-column tiles
    and other rows of B's row tiles, in a 1.5x downscale and a 1.7x upscale; then a 6x downscale, where the windows also differ in
    the number of output rows a workgroup takes"""
    for frames_shape, resized in (((2, 150, 260), (100, 173)), ((2, 60, 104), (100, 173))):     # a downscale and an upscale
        case = CC.Case("tile", frames_shape, ("short", 100), resized, None, None, None)
        fr = CC.frames_of(case).cuda()
        a = _call(fr, resized, (40, 90), (17, 70), antialias, dtype)
        b = _call(fr, resized, (7, 31), (60, 140), antialias, dtype)
        assert _bits(a, b[:, :, 33:50, 59:129].contiguous())
        c = _call(fr, resized, (0, 0), resized, antialias, dtype)                              # the whole frame
        assert _bits(a, c[:, :, 40:57, 90:160].contiguous()) and _bits(b, c[:, :, 7:67, 31:171].contiguous())
    # a 6x downscale (13 taps): the 3-row window runs 4 output rows per workgroup, the 30-row window 8, the whole frame 8
    fr = CC.frames_of(CC.Case("tile6", (2, 240, 300), ("short", 40), (40, 50), None, None, None)).cuda()
    a = _call(fr, (40, 50), (10, 12), (3, 20), antialias, dtype)
    b = _call(fr, (40, 50), (4, 5), (30, 40), antialias, dtype)
    c = _call(fr, (40, 50), (0, 0), (40, 50), antialias, dtype)
    assert _bits(a, b[:, :, 6:9, 7:27].contiguous()) and _bits(a, c[:, :, 10:13, 12:32].contiguous())
    assert _bits(b, c[:, :, 4:34, 5:45].contiguous())


@DT
def test_slot_of_a_batch_padded_rows_and_unaligned_base(dtype):
    case = CC.BY_NAME["wide"]
    want = _case_call(case, True, dtype)
    assert _bits(_case_call(case, True, dtype, slot=1, slots=2), want)            # slot 0 and the guards keep the poison
    assert _bits(_case_call(case, True, dtype, shift=1, row_pad=3), want)         # sy > ow, the base 1 element off a 16-byte boundary
    assert _bits(_case_call(case, True, dtype, shift=3, row_pad=1, slot=1, slots=2), want)


def test_frame_strided_input_view_gives_the_bits_of_its_copy():
    case = CC.BY_NAME["down_nonint"]
    fr = CC.frames_of(case).cuda()
    T, H, W, _ = fr.shape
    big = torch.full((2 * T, H + 1, W + 2, 3), 77, dtype=torch.uint8, device="cuda")
    big[::2, :H, 1:W + 1] = fr
    view = big[::2, :H, 1:W + 1]                      # st two padded frames, sy a padded row, the base 3 bytes in
    assert torch.equal(view, fr) and not view.is_contiguous()
    for antialias in CC.ANTIALIAS:
        a = _call(view, case.resized, case.origin, case.crop, antialias, torch.float32)
        assert _bits(a, _call(fr, case.resized, case.origin, case.crop, antialias, torch.float32))


def test_collate_and_the_upload_path_equal_the_single_calls():
    from cvvae_amd.data import ClipTransform, collate_clips
    a = CC.frames_of(CC.BY_NAME["down_nonint"])
    b = CC.frames_of(CC.Case("b", (3, 30, 52), None, None, None, None, None))
    t = ClipTransform(16, 24, dtype=torch.bfloat16)
    batch = collate_clips([a.cuda(), b.cuda()], t)["frames"]
    assert batch.shape == (2, 3, 3, 16, 16) and batch.dtype == torch.bfloat16 and batch.is_cuda
    one_a, one_b = t(a.cuda()), t(b.cuda())
    assert _bits(batch[0].cpu(), one_a.cpu()) and _bits(batch[1].cpu(), one_b.cpu())
    # within the bound of the fp64 reference, through the public object (its cached, sliced tables)
    want = R.reference(a, (24, 37), (4, 10), (16, 16), True)
    assert float((one_a.cpu().double() - want).abs().max()) <= R.tol32(4, 4) + CC.DTYPE_TERM[torch.bfloat16]
    # a pinned CPU tensor with device="cuda": uploaded as uint8, the same bits; frame_indices and a seeded random crop as well
    up = ClipTransform(16, 24, random_crop=True, dtype=torch.bfloat16, device="cuda")
    dev = ClipTransform(16, 24, random_crop=True, dtype=torch.bfloat16)
    g, h = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    got = up(a.pin_memory(), [2, 0], generator=g)
    assert got.is_cuda and got.shape == (3, 2, 16, 16) and _bits(got.cpu(), dev(a.cuda(), [2, 0], generator=h).cpu())
    assert _bits(ClipTransform(16, 24, dtype=torch.bfloat16, device="cuda")(a).cpu(), one_a.cpu())      # pageable memory too
    cpu = collate_clips([a, b], ClipTransform(16, 24, dtype=torch.bfloat16, device="cuda"))["frames"]
    assert cpu.is_cuda and _bits(cpu.cpu(), batch.cpu())


def test_a_collated_batch_goes_through_a_training_step():
    from cvvae_amd.data import ClipTransform, collate_clips
    from tests import engine_cases as EC
    engine = EC.to_device(EC.build("latent", True, ema_decay=0.999), torch.bfloat16)
    engine.sample_generator = torch.Generator("cuda").manual_seed(5)
    engine.frame_indices = [0, 2]
    clip = CC.frames_of(CC.Case("e2e", (9, 45, 70), None, None, None, None, None)).cuda()
    batch = collate_clips([clip], ClipTransform(32, 36, random_crop=True, dtype=torch.bfloat16), frame_indices=[[0, 2, 4, 6, 8]],
                          generator=torch.Generator().manual_seed(1))
    assert batch[engine.input_key].shape == (1, 3, 5, 32, 32)
    for i in range(2):
        loss = engine.training_step(batch, i)
        engine.on_train_batch_end()
        assert bool(torch.isfinite(loss.float()).all())
