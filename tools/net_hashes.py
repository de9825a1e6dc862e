#!/usr/bin/env python
"""Print the sha256 of what every network program computes on the MI355X, per case and dtype: the output, for the taped networks the
input gradient, for the trainable ones the parameter gradients concatenated in name order.  A refactor of the host programs
(cvvae_amd/engine.py, grad.py, grad3d.py) must print the same lines before and after, against the same built library:

    python tools/net_hashes.py > before.txt        # (CVVAE_LIB may point another tree at the same libcvvae_hip.so)

Inputs and weights are seeded (oracle.seeded); the cases are those of oracle.golden_cases plus one training-mode step of each 3-D
network at the small shapes of tests/test_backward_launch_trace.py.  The kernels sum in fixed orders, so two runs of one commit
print identical lines."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cvvae_amd  # noqa: E402
from cvvae_amd import constraint, constraint_ldm  # noqa: E402
from oracle.golden_cases import CASES, CONSTRAINT_CASES, LDM_CASES  # noqa: E402
from oracle.seeded import seeded_input, seeded_state_dict  # noqa: E402

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
SD3_SMALL = dict(block_out_channels=[128, 256, 256], layers_per_block=1)
V3_SMALL = dict(ch=128, ch_mult=(1, 2, 2), num_res_blocks=1)


def sha(*ts) -> str:
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().float().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:32]


def load(m, seed, dtype):
    m.load_state_dict(seeded_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed), strict=True)
    return m.to(dtype).cuda()


def step(net, x, dtype):
    """forward + backward against a seeded cotangent -> {what: hash}"""
    xa = x.to(dtype).cuda().requires_grad_(True)
    y = net(xa)
    (y * seeded_input(tuple(y.shape), 4).to(dtype).cuda()).sum().backward()
    out = {"out": sha(y), "dx": sha(xa.grad)}
    named = [(n, p) for n, p in sorted(net.named_parameters()) if p.grad is not None]
    if named:
        out["dparams"] = sha(*[p.grad for _, p in named])
    return out


def cases(dtype):
    for name, (cfg, shape, wseed, xseed) in CONSTRAINT_CASES.items():
        m = load(constraint.DecoderWith3DWrapper(**cfg), wseed, dtype).eval().requires_grad_(False)
        yield name, step(m, seeded_input(shape, xseed), dtype)
    for name, (cls, cfg, shape, wseed, xseed) in LDM_CASES.items():
        m = load(getattr(constraint_ldm, cls)(**cfg), wseed, dtype).eval().requires_grad_(False)
        if cls.startswith("Decoder"):
            yield name, step(m, seeded_input(shape, xseed), dtype)
        else:
            with torch.no_grad():
                yield name, {"out": sha(m(seeded_input(shape, xseed).to(dtype).cuda()))}
    for name in ("sd3_t5_64", "sd3_t1_64", "vae3d_t5_64"):
        family, over, shape, wseed, xseed = CASES[name]
        m = load((cvvae_amd.CVVAESD3Model if family == "sd3" else cvvae_amd.CVVAEModel)(**over), wseed, dtype).eval()
        mom = m.encode(seeded_input(shape, xseed).to(dtype).cuda()).latent_dist.parameters
        yield name, {"out": sha(mom, m.decode(mom[:, :mom.shape[1] // 2]).sample)}
    for fam, model, zc in (("sd3", lambda: cvvae_amd.CVVAESD3Model(**SD3_SMALL), 16),
                           ("vae3d", lambda: cvvae_amd.CVVAEModel(causal_encoder=True, **V3_SMALL), 4)):
        m = load(model(), 7, dtype).train()
        yield f"{fam}_encoder_train", step(m.encoder, seeded_input((1, 3, 5, 16, 24), 11), dtype)
        yield f"{fam}_decoder_train", step(m.decoder, seeded_input((1, zc, 3, 4, 6), 13), dtype)


def main():
    for dn, dtype in DTYPES.items():
        for name, hashes in cases(dtype):
            for what, h in hashes.items():
                print(f"{name} {dn} {what} {h}", flush=True)


if __name__ == "__main__":
    main()
