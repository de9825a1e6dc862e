"""Digests of what the training-side backward passes that are not convolutions write (csrc/bwd_kernels.hip through cvvae_amd.ops):
the GroupNorm backward with and without its affine sums, the per-channel sums, the row-softmax backward, the temporal-attention
backward, the padding adjoint and the 2x2 sum -- sha256 over the bytes of every output, on every non-raising case of the edge tables
in each of its dtypes, and over the inputs themselves.  tests/golden/bwd_pass_digests.json holds the digests of the library as it
stood before these passes were gathered into one file on one GroupNorm-backward element, one per-channel fold and one finish kernel;
tests/test_gpu_bwd_parity.py recomputes and compares them, so a change of the arithmetic -- another FMA contraction, another order of
summation -- shows where the fp64 bounds of the edge tests would let it pass.

    python tests/bwd_parity.py > tests/golden/bwd_pass_digests.json      # on an MI355X; only to record NEW inputs

Two cases stand here only, not in the edge tables: the fused GroupNorm backward with 35 partial [C][2] tables (so that the finish
kernel runs its four-deep loop on that path too) and ops.layernorm_bwd, which composes three of the passes on the one-group view.

A helper, not a test module: pytest does not collect it."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import boundary_edge_cases as BC  # noqa: E402
import boundary_ref as BR  # noqa: E402
import pass_edge_cases as PC  # noqa: E402
import pass_ref as PR  # noqa: E402
import wgrad_edge_cases as WC  # noqa: E402
import wgrad_ref as WR  # noqa: E402

# more than 32 partial tables on the fused path: 5 splits of 512 pixels x 7 rows = 35
GN_PARTS35 = PC._case("gn_bwd_input_params-C128g32-S2049-r7-silu1-add0-parts35", "gn_bwd", dtypes=(PC.F32, PC.BF16), C=128, G=32,
                      S=2049, rows=7, silu=1, add=0, params=1, per_frame=0)
LN_BWD = PC._case("layernorm_bwd-C512-P37", "layernorm", dtypes=(PC.F32, PC.BF16), C=512, P=37, offset=0.0, const_row=-1)

TABLES = ("gn_bwd", "softmax_bwd", "temporal_bwd", "chan", "fold", "upsum", "layernorm_bwd")


def sha(tensors):
    """sha256 over the bytes of the tensors, in order"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _ln_bwd_inputs(dt):
    t = dict(PR.inputs(LN_BWD, dt))
    g = torch.Generator().manual_seed(LN_BWD.seed * 3 + 1000 + (PC.F32, PC.F16, PC.BF16).index(dt))
    t["gy"] = PR._rn(g, LN_BWD["P"], LN_BWD["C"]).to(PR.DTYPE[dt])
    return t


def _gn_bwd(ops, c, dt, d):
    x5 = lambda v: PR._x5(c, v)
    fn = ops.gn_bwd_input_params if c["params"] else ops.gn_bwd_input
    r = fn(x5(d["x"]), x5(d["gy"]), (d["rs"], d["nm"]), d["gamma"], d["beta"], bool(c["silu"]), add=x5(d["add"]) if c["add"] else None,
           per_frame=bool(c.get("per_frame")), groups=c["G"])
    return dict(zip(("gx", "dg", "db"), r if c["params"] else (r,)))


def _upsum(ops, c, dt, d):
    if c.recipe == "tiled_ints":  # built on the device from a formula of the position: nothing on the host to digest
        d = {"g": BR.tiled_ints(c["N"], 2 * c["H"], 2 * c["W"], c["C"], PR.DTYPE[dt], device="cuda")}
    return {"out": ops.upsample2x_sum(d["g"])}


def _chan(ops, c, dt, d):
    r = WR.chan_call(ops, c, d)
    return {"db": r[0]} if c.op == "bias" else {"dg": r[0], "db": r[1]}


def entries():
    """every (table, case name, dtype, host inputs as a thunk, the call on device tensors -> {output name: tensor})"""
    out = []
    for c in PC.gn_bwd_cases() + [GN_PARTS35]:
        out += [("gn_bwd", c, dt, PR.inputs, _gn_bwd) for dt in c.dtypes]
    for c in PC.softmax_bwd_cases():
        out += [("softmax_bwd", c, dt, PR.inputs,
                 lambda ops, c, dt, d: {"gs": ops.softmax_bwd_rows(d["p"], d["gp"], c["n"], c["alpha"], c["ld_o"])}) for dt in c.dtypes]
    for c in PC.temporal_bwd_cases():
        out += [("temporal_bwd", c, dt, PR.inputs,
                 lambda ops, c, dt, d: dict(zip(("gq", "gk", "gv"), ops.temporal_attention_bwd(d["q"], d["k"], d["v"], d["go"]))))
                for dt in c.dtypes]
    for c in WC.chan_cases():
        out += [("chan", c, dt, WR.chan_inputs, _chan) for dt in c.dtypes]
    for c in WC.fold_cases():
        out += [("fold", c, dt, WR.fold_inputs, lambda ops, c, dt, d: {"out": WR.fold_call(ops, c, d)[0]}) for dt in c.dtypes]
    for c in BC.upsum_cases():
        out += [("upsum", c, dt, BR.inputs, _upsum) for dt in c.dtypes]
    out += [("layernorm_bwd", LN_BWD, dt, lambda c, dt: _ln_bwd_inputs(dt),
             lambda ops, c, dt, d: dict(zip(("gx", "dg", "db"), ops.layernorm_bwd(d["x"], d["gy"], d["gamma"], d["beta"], PR.LN_EPS))))
            for dt in LN_BWD.dtypes]
    return [e for e in out if not getattr(e[1], "raises", False)]


def keys():
    return [f"{c.name}/{dt}" for _, c, dt, _, _ in entries()]


def input_digests():
    """the operands themselves, on the host: {table: sha256 over every case's tensors, cases in table order, tensors by name}"""
    hs = {t: hashlib.sha256() for t in TABLES}
    for table, c, dt, inputs, _ in entries():
        t = inputs(c, dt)
        hs[table].update(sha([t[k] for k in sorted(t)]).encode())
    return {t: h.hexdigest() for t, h in hs.items()}


def pass_digests():
    """every case once on the device: {case/dtype: {output name: sha256 of its bytes}}"""
    from cvvae_amd import ops
    out = {}
    for _, c, dt, inputs, call in entries():
        d = {k: v.cuda() for k, v in inputs(c, dt).items()}
        got = call(ops, c, dt, d)
        torch.cuda.synchronize()
        out[f"{c.name}/{dt}"] = {k: sha([v]) for k, v in got.items()}
    return out


def digests():
    return {"inputs": input_digests(), "passes": pass_digests()}


if __name__ == "__main__":
    print(json.dumps(digests(), indent=1, sort_keys=True))
