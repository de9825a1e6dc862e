"""API contract of the drop-in wrapper beyond encode/decode, on CPU with the test doubles of test_host_logic.py:
`forward()` (models/modeling_vae.py:114-142 / 440-468), the diffusers-style output types, `encode_latents` (the training engines'
`encode_first_stage`, lvdm/models/diffusion.py:159-171, 380-385), loader leniency, construction-time validation, and the
host-side helpers of bench.py."""
import json
import math
import os
import warnings

import pytest
import torch

from tests.test_host_logic import make


@pytest.mark.parametrize("family", ["sd3", "vae3d"])
def test_forward_matches_encode_decode(family):
    m = make(family)
    g = torch.Generator().manual_seed(0)
    x = torch.rand((1, 3, 9, 64, 64), generator=g) * 2 - 1
    post = m.encode(x).latent_dist
    # sample_posterior=False -> decode(mode())
    out = m(x)
    assert torch.equal(out.sample, m.decode(post.mode()).sample)
    assert torch.equal(m(x, return_dict=False)[0], out.sample)
    assert torch.equal(out[0], out.sample) and torch.equal(out["sample"], out.sample)  # BaseOutput indexing
    # sample_posterior=True with a generator: deterministic under the same seed, equal to decode(sample(generator))
    z = post.sample(generator=torch.Generator().manual_seed(7))
    a = m(x, sample_posterior=True, generator=torch.Generator().manual_seed(7)).sample
    b = m(x, sample_posterior=True, generator=torch.Generator().manual_seed(7)).sample
    assert torch.equal(a, b) and torch.equal(a, m.decode(z).sample)
    assert not torch.equal(a, m(x, sample_posterior=True, generator=torch.Generator().manual_seed(8)).sample)


def test_forward_num_frames_on_4d_input():
    """4-D input (frames folded into the batch): encode unfolds with config.num_video_frames, decode with num_frames."""
    m = make("vae3d", num_video_frames=5)
    g = torch.Generator().manual_seed(1)
    x5 = torch.rand((2, 3, 5, 64, 64), generator=g) * 2 - 1
    x4 = x5.permute(0, 2, 1, 3, 4).reshape(10, 3, 64, 64)
    z5 = m.encode(x5).latent_dist.mode()
    assert torch.equal(m.encode(x4).latent_dist.mode(), z5)
    z4 = z5.permute(0, 2, 1, 3, 4).reshape(-1, *z5.shape[1:2], *z5.shape[3:])  # [(b t') c h w]
    y = m.decode(z4[:, :4], num_frames=z5.shape[2]).sample
    assert torch.equal(y, m.decode(z5[:, :4]).sample)


def test_output_types_and_posterior():
    from cvvae_amd.modeling import AutoencoderKLOutput, DecoderOutput, DiagonalGaussianDistribution
    p = torch.randn(2, 8, 3, 4, 4)
    d = DiagonalGaussianDistribution(p)
    o = AutoencoderKLOutput(latent_dist=d)
    assert o[0] is d and o.latent_dist is d and o["latent_dist"] is d and o.to_tuple() == (d,)
    t = torch.zeros(1)
    assert DecoderOutput(sample=t)[0] is t
    s = d.sample(generator=torch.Generator().manual_seed(0))
    # nll as diffusers: 0.5 * sum(log 2pi + logvar + (x - mean)^2 / var)
    ref = 0.5 * torch.sum(math.log(2 * math.pi) + d.logvar + (s - d.mean) ** 2 / d.var, dim=[1, 2, 3])
    assert torch.allclose(d.nll(s), ref)


@pytest.mark.parametrize("family", ["sd3", "vae3d"])
def test_encode_latents_is_encode_first_stage(family):
    m = make(family)
    g = torch.Generator().manual_seed(2)
    x = torch.rand((3, 3, 5, 64, 64), generator=g) * 2 - 1
    sf = getattr(m.config, "scaling_factor", None)
    z = m.encode_latents(x, sample=False)
    want = torch.cat([m.encode(x[i:i + 1]).latent_dist.mode() for i in range(3)], dim=0)
    assert torch.allclose(z, want * (sf if sf is not None else 1.0))
    # rounds of n samples a time give the same latents (GroupNorm is per sample)
    assert torch.equal(m.encode_latents(x, sample=False, n_samples_a_time=2), z)
    # images: [B,3,H,W] -> [(B T'),z,h,w]
    zi = m.encode_latents(x[:, :, 0], sample=False, scale_factor=1.0)
    assert zi.shape == (3, z.shape[1], 8, 8)
    assert torch.equal(zi, m.encode(x[:, :, :1]).latent_dist.mode()[:, :, 0])
    # sampling is reproducible under a seeded generator
    a = m.encode_latents(x, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, m.encode_latents(x, generator=torch.Generator().manual_seed(5)))


@pytest.mark.parametrize("family", ["sd3", "vae3d"])
def test_decode_latents_is_decode_first_stage(family):
    """DiffusionEngineFor3DVAE.decode_first_stage (lvdm/models/diffusion.py:139-157, 369-377): z / scale_factor, rounds, decode, frames
    folded into the batch; image latents run as one-frame clips"""
    m = make(family)
    g = torch.Generator().manual_seed(3)
    zc = 16 if family == "sd3" else 4
    z = torch.randn((3, zc, 2, 8, 8), generator=g)
    sf = getattr(m.config, "scaling_factor", None) or 1.0
    want = torch.cat([m.decode(z[i:i + 1] * (1.0 / sf)).sample for i in range(3)], dim=0)
    x = m.decode_latents(z)
    assert x.shape == (3 * want.shape[2], 3, 64, 64)
    assert torch.equal(x, want.permute(0, 2, 1, 3, 4).reshape(-1, 3, 64, 64))
    assert torch.equal(m.decode_latents(z, n_samples_a_time=2), x)
    assert torch.equal(m.decode_latents(z, flatten_frames=False), want)
    xi = m.decode_latents(z[:, :, 0], scale_factor=1.0)  # image latents [B,z,h,w]
    assert xi.shape == (3, 3, 64, 64) and torch.equal(xi, m.decode(z[:, :, :1]).sample[:, :, 0])


def test_from_pretrained_ignores_unknown_config_keys_and_extra_tensors(tmp_path):
    import cvvae_amd
    m = cvvae_amd.CVVAEModel()
    m.save_pretrained(tmp_path / "vae3d")
    cfgp = tmp_path / "vae3d" / "config.json"
    cfg = json.loads(cfgp.read_text())
    cfg["some_future_key"] = 1
    cfgp.write_text(json.dumps(cfg))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m2 = cvvae_amd.CVVAEModel.from_pretrained(str(tmp_path), subfolder="vae3d")
    assert any("some_future_key" in str(x.message) for x in w)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    # a sharded checkpoint index gets a clear error
    (tmp_path / "vae3d" / "diffusion_pytorch_model.safetensors.index.json").write_text("{}")
    with pytest.raises(NotImplementedError, match="sharded"):
        cvvae_amd.CVVAEModel.from_pretrained(str(tmp_path), subfolder="vae3d")


def test_unsupported_widths_are_flagged_and_refused_with_a_message():
    """widths the kernels cannot run (not 128 * 2^k): the parameter holder builds (checkpoint tooling works on it) with a
    warning, and a forward pass raises NotImplementedError with the constraint -- never a bare assertion inside a launch."""
    import cvvae_amd
    from cvvae_amd.constraint import Decoder
    with pytest.warns(UserWarning, match="128"):
        m = cvvae_amd.CVVAESD3Model(block_out_channels=[64, 128, 256, 256])
    with pytest.raises(NotImplementedError, match="128"):
        m.encoder(torch.zeros(1, 3, 1, 8, 8))
    with pytest.warns(UserWarning, match="128"):
        m = cvvae_amd.CVVAEModel(ch=96)
    with pytest.raises(NotImplementedError, match="128"):
        m.decoder(torch.zeros(1, 4, 1, 8, 8))
    with pytest.raises(NotImplementedError, match="128"):
        Decoder()(torch.zeros(1, 3, 8, 8))  # the reference class default block_out_channels=(64,)


def test_bench_helpers():
    """bench.py: executed-FLOP accounting follows the kernel's time-fold plan; --gpus N self-launch command line"""
    import bench
    # causal front-2 replicate, 17 frames, stride 1: frame 0 one group, frame 1 two, the rest three
    assert [bench.time_groups(t, 1, 2, 17, True, True) for t in range(4)] == [1, 2, 3, 3]
    assert sum(bench.time_groups(t, 1, 2, 17, True, False) for t in range(17)) == 51
    # symmetric replicate 1+1: first and last frames fold two taps
    assert [bench.time_groups(t, 1, 1, 5, True, True) for t in range(5)] == [2, 3, 3, 3, 2]
    # zero padding: padding frames are skipped without extra weights
    assert [bench.time_groups(t, 1, 1, 5, False, False) for t in range(5)] == [2, 3, 3, 3, 2]
    assert bench.time_groups(0, 1, 1, 1, False, False) == 1
    src = open(bench.__file__).read()
    assert "torch.distributed.run" in src and "--nproc-per-node" in src


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 arrays (float64 kept) in full under the budget; over it, the same seeded sample of every
    output's elements from run to run, within the budget.  --steps below 1 is refused."""
    import numpy as np

    import bench
    g = torch.Generator().manual_seed(0)
    lat, rec, f64 = torch.randn(2, 4, 3, generator=g).bfloat16(), torch.randn(3, 50, 40, generator=g), torch.randn(7, dtype=torch.float64)
    got = bench.dump_outputs(str(tmp_path / "full"), [("latents", lat), ("recon", rec), ("stats", f64), ("none", None)])
    assert got == {"latents": [[2, 4, 3], 24], "recon": [[3, 50, 40], 6000], "stats": [[7], 7]}
    a = np.load(tmp_path / "full" / "latents.npy")
    assert a.dtype == np.float32 and np.array_equal(a, lat.float().numpy())
    assert np.array_equal(np.load(tmp_path / "full" / "recon.npy"), rec.numpy())
    assert np.load(tmp_path / "full" / "stats.npy").dtype == np.float64
    budget = 4 * 1000
    for d in ("s1", "s2"):
        got = bench.dump_outputs(str(tmp_path / d), [("latents", lat), ("recon", rec)], budget)
        assert 4 * sum(n for _, n in got.values()) <= budget and got["recon"] == [[3, 50, 40], int(6000 * budget / 4 / 6024)]
    for n in ("latents", "recon"):
        s1, s2 = np.load(tmp_path / "s1" / (n + ".npy")), np.load(tmp_path / "s2" / (n + ".npy"))
        assert s1.dtype == np.float32 and s1.ndim == 1 and np.array_equal(s1, s2)
    assert np.isin(np.load(tmp_path / "s1" / "recon.npy"), rec.numpy()).all()
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "3", "--dump-outputs", str(tmp_path)])
    assert bench.parse().steps == 3
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_full_is_opt_in(monkeypatch):
    """bench.py: a plain run leaves every extra leg (split, roofline, tolerance modes, parity, CPU baseline, N > 1 check and annex)
    to --full, whose --no-* options still trim it"""
    import bench
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--no-cpu-baseline", "--no-parity"])
    a = bench.parse()
    assert a.full and a.no_cpu_baseline and a.no_parity and not a.no_roofline
