"""Digests of what every multi-tensor update pass (csrc/optim_kernels.hip through cvvae_amd.ops.mt_*) writes on the edge lists of
tests/optim_ref.py and tests/master_ref.py: sha256 over the bytes of every buffer a pass may write, whole buffers with their guard
elements, and over the inputs themselves.  tests/golden/update_pass_digests.json holds the digests of the library as it stood before
the passes were folded onto one chunk walk and one AdamW template; tests/test_gpu_update_parity.py recomputes and compares them, so
a change of the arithmetic -- another FMA contraction, another order of summation -- shows where the fp64 bounds would let it pass.

    python tests/update_parity.py > tests/golden/update_pass_digests.json      # on an MI355X; only to record NEW inputs

A helper, not a test module: pytest does not collect it."""
import hashlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import master_ref as M  # noqa: E402
from tests import optim_ref as R  # noqa: E402

LR = R.YAML_LR
B1, B2 = R.YAML_ADAMW["betas"]
EPS, WD = R.YAML_ADAMW["eps"], R.YAML_ADAMW["weight_decay"]
COEF = 0.37
COEFS = (("nocoef", None), ("coef", COEF))
DTYPES16 = (("bf16", torch.bfloat16), ("fp16", torch.float16))
OMD = float(torch.tensor(1.0) - torch.tensor(2.0 / 11.0))    # test_ema_pass_on_every_edge_in_one_launch's one_minus_decay
PACK_DIVISOR = 3.0
PACK_SENTINEL = 7.25


def sha(tensors):
    """sha256 over the bytes of the tensors, in order"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _bufs(entries, key):
    return [e[key + "_buf"] for e in entries]


def input_digests():
    """the edge lists themselves, on the host: {list: {buffer: sha256}}"""
    out = {"fp32": {k: sha(_bufs(R.edge_list(0), k)) for k in ("g", "p", "m", "v", "s")}}
    for name, dt in DTYPES16:
        out[name] = {k: sha(_bufs(M.edge_list16(dt), k)) for k in ("g", "p", "m", "v", "w")}
    return out


def _to_device(entries):
    return [{k: e[k].cuda() for k in e if k.endswith("_buf")} for e in entries]


def _scalars(entries, sel):
    return dict(step_size=[LR / (1.0 - B1 ** entries[i]["t"]) for i in sel],
                bias2_sqrt=[math.sqrt(1.0 - B2 ** entries[i]["t"]) for i in sel])


def _coef(coef):
    return None if coef is None else torch.tensor([coef], dtype=torch.float32, device="cuda")


def _list32(edge, dev, fields, with_grad_only=True):
    """(MultiTensorList over the fp32 edge list's entries -- those with a gradient unless told otherwise --, their indices)"""
    from cvvae_amd import ops
    sel = [i for i, d in enumerate(edge) if d["has_grad"] or not with_grad_only]
    mtl = ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda")
    kw = {f: [R.views(edge[i], dev[i])[{"shadow": "s"}.get(f, f)] for i in sel] for f in fields}
    if "m" in fields:
        kw.update(_scalars(edge, sel))
    return mtl.set(**kw), sel


def _list16(edge, dev, dtype, fields):
    from cvvae_amd import ops
    sel = [i for i, e in enumerate(edge) if e["has_grad"]]
    mtl = ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda", dtype)
    kw = {f: [M.views16(edge[i], dev[i])[{"shadow": "w"}.get(f, f)] for i in sel] for f in fields}
    if "m" in fields:
        kw.update(_scalars(edge, sel))
    return mtl.set(**kw), sel


def pass_digests():
    """every pass once on the device, each on fresh copies of its inputs: {case: {buffer: sha256}}"""
    from cvvae_amd import ddp, ops
    edge = R.edge_list(0)
    edges16 = {name: M.edge_list16(dt) for name, dt in DTYPES16}
    out = {}

    for tag, coef in COEFS:
        dev = _to_device(edge)
        mtl, _ = _list32(edge, dev, ("g", "p", "m", "v"))
        ops.mt_adamw(mtl, LR, B1, B2, EPS, WD, _coef(coef))
        torch.cuda.synchronize()
        out[f"adamw_{tag}"] = {k: sha(_bufs(dev, k)) for k in ("m", "v", "p")}

    for name, dt in DTYPES16:
        for tag, coef in COEFS:
            dev = _to_device(edges16[name])
            mtl, _ = _list16(edges16[name], dev, dt, ("g", "p", "m", "v", "shadow"))
            ops.mt_adamw_master(mtl, LR, B1, B2, EPS, WD, _coef(coef))
            torch.cuda.synchronize()
            out[f"adamw_master_{name}_{tag}"] = {k: sha(_bufs(dev, k)) for k in ("w", "m", "v", "p")}

    dev = _to_device(edge)
    mtl, sel = _list32(edge, dev, ("p", "shadow"), with_grad_only=False)
    assert len(sel) == len(edge)
    ops.mt_ema(mtl, OMD)
    torch.cuda.synchronize()
    out["ema"] = {"s": sha(_bufs(dev, "s"))}

    dev = _to_device(edge)
    mtl, _ = _list32(edge, dev, ("g",))
    ops.mt_scale(mtl, _coef(COEF))
    torch.cuda.synchronize()
    out["scale"] = {"g": sha(_bufs(dev, "g"))}

    dev = _to_device(edge)
    l32, _ = _list32(edge, dev, ("g",))
    for tag, mx in (("1", 1.0), ("1e6", 1e6)):
        out2 = ops.mt_grad_norm(l32, mx)
        torch.cuda.synchronize()
        out[f"grad_norm_{tag}"] = {"out2": sha([out2])}

    # one mixed list: the fp32 list's partials first, then bf16's, then fp16's
    lists = [l32] + [_list16(edges16[name], _to_device(edges16[name]), dt, ("g",))[0] for name, dt in DTYPES16]
    partials = torch.full((sum(m.n_chunks for m in lists) + R.GUARD,), PACK_SENTINEL, dtype=torch.float32, device="cuda")
    at = 0
    for m in lists:
        ops.mt_sumsq(m, partials[at:at + m.n_chunks])
        at += m.n_chunks
    out2 = ops.mt_norm_finish(partials[:at], 1.0)
    torch.cuda.synchronize()
    out["sumsq_norm_finish_mixed"] = {"partials": sha([partials]), "out2": sha([out2])}

    # the pack pass into one flat bucket laid out as cvvae_amd.ddp lays its slots; the tensor without a gradient is None
    dev = _to_device(edge)
    numels = [d["n"] for d in edge]
    offsets, total = ddp.slot_layout(numels)
    flat = torch.full((total + R.GUARD,), PACK_SENTINEL, dtype=torch.float32, device="cuda")
    gs = [R.views(d, b)["g"] if d["has_grad"] else None for d, b in zip(edge, dev)]
    assert any(g is None for g in gs)
    mtl = ops.MultiTensorList(numels, "cuda").set(g=gs, shadow=[flat[o:o + n] for o, n in zip(offsets, numels)])
    ops.mt_pack(mtl, PACK_DIVISOR)
    torch.cuda.synchronize()
    out["pack"] = {"bucket": sha([flat])}
    return out


def digests():
    return {"inputs": input_digests(), "passes": pass_digests()}


if __name__ == "__main__":
    print(json.dumps(digests(), indent=1, sort_keys=True))
