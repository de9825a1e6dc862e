"""score_reconstruction_u8 on a seeded CVVAESD3Model (needs the MI355X): the scripts' round trip with a verdict equals frame_metrics of
the separately computed decode_to_frames_u8 output against the frames the encoder saw (resized, truncated to 1 + (T-1)//4*4), bit for
bit; a ReconstructionMeter fed two clips reports their pooled means."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    import cvvae_amd
    from oracle import parity as P
    m = cvvae_amd.CVVAESD3Model()
    P.load_seeded(m, 0)
    return m.to(torch.float16).cuda().eval()


def _frames(T, H, W, seed):
    return torch.randint(0, 256, (T, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).cuda()


def _separately(m, frames, size):
    from cvvae_amd import metrics, ops
    seen = ops.resize_frames_u8(frames, size) if size is not None else frames
    seen = seen[:1 + (seen.shape[0] - 1) // 4 * 4]
    recon = m.decode_to_frames_u8(m.encode_frames_u8(frames, size=size).latent_dist.mode())
    assert recon.shape == seen.shape and recon.dtype == torch.uint8
    return metrics.frame_metrics(seen, recon)


@pytest.mark.parametrize("size", [None, (64, 96)], ids=["as_is", "resized"])
def test_score_reconstruction_u8_is_the_round_trip_scored(model, size):
    frames = _frames(6, 64, 64, 4) if size is None else _frames(6, 90, 120, 4)   # 6 frames: the codec sees 5
    got = model.score_reconstruction_u8(frames, size=size)
    want = _separately(model, frames, size)
    assert set(got) == {"sse", "psnr", "ssim"}
    for k in got:
        assert tuple(got[k].shape) == (1, 5) and got[k].is_cuda and torch.equal(got[k], want[k]), k
    assert got["sse"].dtype == torch.float64 and got["psnr"].dtype == torch.float32 and got["ssim"].dtype == torch.float32
    assert bool(torch.isfinite(got["psnr"]).all()) and bool((got["ssim"].abs() <= 1.0).all())
    with pytest.raises(ValueError):
        model.score_reconstruction_u8(frames.float())


def test_meter_fed_two_clips_reports_their_pooled_means(model):
    from cvvae_amd.metrics import ReconstructionMeter
    meter = ReconstructionMeter()
    a, b = _frames(5, 64, 64, 5), _frames(1, 64, 96, 6)
    ra = model.score_reconstruction_u8(a, meter=meter)
    rb = model.score_reconstruction_u8(b, meter=meter)
    out = meter.compute()
    psnr = torch.cat([ra["psnr"].flatten(), rb["psnr"].flatten()]).double()
    ssim = torch.cat([ra["ssim"].flatten(), rb["ssim"].flatten()]).double()
    assert out["frames"] == 6 and out["identical_frames"] == 0 and out["lpips"] is None
    assert math.isclose(out["psnr"], float(psnr.mean()), rel_tol=1e-12) and math.isclose(out["ssim"], float(ssim.mean()), rel_tol=1e-12)
    meter.reset()
    meter.update(a, a)
    out = meter.compute()
    assert out["frames"] == 5 and out["identical_frames"] == 5 and math.isnan(out["psnr"]) and out["ssim"] == 1.0
