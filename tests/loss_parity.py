"""Digests of what the passes of the training loss write (csrc/loss_kernels.hip through cvvae_amd.ops): reduce_sum and its adjoint
on every op, dtype pair, tail length and view shape, the frame-mapped pair on every map, clip layout and dtype pair, and the
Gaussian posterior forward and backward -- sha256 over the bytes of every output of every case, and over the inputs themselves.
tests/golden/loss_pass_digests.json holds the digests of the library as it stood before these kernels were folded onto one group
walk and one reduce pair over operand sources; tests/test_gpu_loss_parity.py recomputes and compares them, so a change of the
arithmetic -- another FMA contraction, another order of summation -- shows where the fp64 bands of tests/test_gpu_loss.py would let
it pass.

    python tests/loss_parity.py > tests/golden/loss_pass_digests.json      # on an MI355X; only to record NEW inputs

The shapes are the smallest at which each path can go wrong: 4109 elements are two workgroup tiles and a 5-element tail group,
the element counts around 8 and 2048 the ends of a group and of a tile, 2048 * 2048 + 2048 + 5 one stride of the capped forward
grid; HW = 63 makes groups straddle frames, a frame stride above HW and HW = 256 are the clip's other two layouts; C * S = 420
makes groups straddle the mean / logvar chunks and the rows.

A helper, not a test module: pytest does not collect it."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from cvvae_amd import _lib as L  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
OPS = {"abs_diff": L.RED_ABS_DIFF, "sq_diff": L.RED_SQ_DIFF, "sq": L.RED_SQ, "ident": L.RED_IDENT, "hinge_neg": L.RED_HINGE_NEG,
       "hinge_pos": L.RED_HINGE_POS, "softplus_neg": L.RED_SOFTPLUS_NEG, "softplus_pos": L.RED_SOFTPLUS_POS}
TWO = ("abs_diff", "sq_diff")
N = 4109                            # two workgroup tiles of 2048 and a group of 5
GRID_N = 2048 * 2048 + 2048 + 5     # one stride of the forward grid, one more tile, one more partial group
TABLES = ("reduce", "frames", "gauss")
COEF = -0.37


def sha(tensors):
    """sha256 over the bytes of the tensors, in order"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _rn(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 1.5


# ---- reduce_sum / reduce_sum_bwd ----
def _flat(n, da, db, seed):
    return lambda: {"a": _rn(seed, n).to(DT[da]), **({"b": _rn(seed + 1, n).to(DT[db])} if db else {})}


def _view_run9(d):      # an inner run of 9 from a misaligned base
    return d["a"][:, :, 1:10], d["b"][:, :, 1:10]


def _view_outer3(d):    # three strided outer dimensions over an inner run of 16, against a contiguous tensor
    return d["a"][::2, ::2, ::2, :16], d["b"]


def _view_slice4(d):    # a contiguous tensor against every fourth frame of a clip
    return d["a"], d["b"][:, :, ::4]


VIEWS = {"run9": ((3, 5, 11), (3, 5, 11), _view_run9), "outer3": ((4, 6, 10, 32), (2, 3, 5, 16), _view_outer3),
         "slice4": ((1, 3, 3, 6, 7), (1, 3, 9, 6, 7), _view_slice4)}


def _reduce(op, view=None, b_only_too=False):
    def call(ops, d):
        a, b = view(d) if view else (d["a"], d.get("b"))
        coef = torch.tensor(COEF, device=a.device)
        two = b is not None
        out = {"sum": ops.reduce_sum(OPS[op], a, b)}
        ga, gb = ops.reduce_sum_bwd(OPS[op], a, b, coef, True, two)
        out["ga"] = ga
        if two:
            out["gb"] = gb
        if b_only_too:
            out["ga_alone"] = ops.reduce_sum_bwd(OPS[op], a, b, coef, True, False)[0]
            out["gb_alone"] = ops.reduce_sum_bwd(OPS[op], a, b, coef, False, True)[1]
        return out
    return call


def _reduce_entries():
    out = []
    for i, op in enumerate(OPS):
        for j, dt in enumerate(DT):
            out.append((f"reduce/{op}/{dt}/n{N}", _flat(N, dt, dt if op in TWO else None, 100 + 10 * i + j), _reduce(op, None, op in TWO)))
    for i, op in enumerate(TWO):
        for j, da in enumerate(DT):
            for k, db in enumerate(DT):
                out.append((f"reduce/{op}/{da}-{db}/n{N}", _flat(N, da, db, 300 + 30 * i + 3 * j + k), _reduce(op)))
    for i, n in enumerate((1, 7, 8, 9, 2047, 2048, 2049)):
        for j, dt in enumerate(("bf16", "f32")):
            out.append((f"reduce/sq_diff/{dt}/n{n}", _flat(n, dt, dt, 400 + 2 * i + j), _reduce("sq_diff")))
    for i, (name, (sa, sb, view)) in enumerate(VIEWS.items()):
        for j, dt in enumerate(("bf16", "f32")):
            inputs = lambda sa=sa, sb=sb, dt=dt, s=500 + 4 * i + 2 * j: {"a": _rn(s, *sa).to(DT[dt]), "b": _rn(s + 1, *sb).to(DT[dt])}
            out.append((f"reduce/sq_diff/{dt}/view-{name}", inputs, _reduce("sq_diff", view)))
    out.append(("reduce/sq/bf16/view-run9", lambda: {"a": _rn(520, 3, 5, 11).to(torch.bfloat16)},
                _reduce("sq", lambda d: (d["a"][:, :, 1:10], None))))
    out.append((f"reduce/sq_diff/bf16/n{GRID_N}", _flat(GRID_N, "bf16", "bf16", 530), _reduce("sq_diff")))
    return [("reduce",) + e for e in out]


# ---- reduce_sum_frames / reduce_sum_frames_bwd ----
# clip layouts: (H, W of the clip, the rows trimmed off each end of H by a view)
LAYOUTS = {"hw63": (7, 9, 0), "hw63-stride81": (9, 9, 1), "hw256": (16, 16, 0)}
# frame maps: (frames of the clip, mode, index, group, frames of the target)
MAPS = {"gather0-3": (5, L.FMAP_GATHER, [0, 3], None, 2), "mean2": (5, L.FMAP_GROUP_MEAN, None, 2, 3),
        "mean4": (9, L.FMAP_GROUP_MEAN, None, 4, 3)}


def _frames_entries():
    out = []
    seed = 600
    for lay, (H, W, trim) in LAYOUTS.items():
        for mp, (T, mode, index, group, T2) in MAPS.items():
            for op in TWO:
                for da, dc in (("bf16", "bf16"), ("bf16", "f32"), ("f32", "f32")):
                    seed += 2

                    def inputs(s=seed, T=T, T2=T2, H=H, W=W, trim=trim, da=da, dc=dc):
                        return {"a": _rn(s, 2, 3, T2, H - 2 * trim, W).to(DT[da]), "clip": _rn(s + 1, 2, 3, T, H, W).to(DT[dc])}

                    def call(ops, d, op=op, mode=mode, index=index, group=group, trim=trim):
                        clip = d["clip"][:, :, :, trim:-trim] if trim else d["clip"]
                        coef = torch.tensor(COEF, device=clip.device)
                        return {"sum": ops.reduce_sum_frames(OPS[op], d["a"], clip, mode, index=index, group=group),
                                "ga": ops.reduce_sum_frames_bwd(OPS[op], d["a"], clip, coef, mode, index=index, group=group)}

                    out.append(("frames", f"frames/{op}/{da}-{dc}/{lay}/{mp}", inputs, call))
    return out


# ---- gauss_reg / gauss_reg_bwd ----
# raw logvar entries at and beyond both ends of the clamp [-30, 20] (all exact in bf16 and fp16)
LOW_END = (-30.0, -30.25, -29.75, -31.0, -64.0)
HIGH_END = (20.0, 20.125, 19.875, 21.0, 40.0)
GAUSS = {"2x8x3x5x7": ((2, 8, 3, 5, 7), LOW_END + HIGH_END), "1x32x2x8x8": ((1, 32, 2, 8, 8), LOW_END)}


def _gauss_entries():
    out = []
    seed = 800
    for name, (shape, ends) in GAUSS.items():
        for dt in DT:
            for with_noise in (True, False):
                seed += 3

                def inputs(s=seed, shape=shape, ends=ends, dt=dt, with_noise=with_noise):
                    mom = _rn(s, *shape)
                    lv = mom[:, shape[1] // 2:].reshape(shape[0], -1)      # (a view: the entries land in every sample's logvar chunk)
                    step = lv.shape[1] // len(ends)
                    for k, v in enumerate(ends):
                        lv[:, 3 + k * step] = v
                    z = (shape[0], shape[1] // 2) + shape[2:]
                    d = {"moments": mom.to(DT[dt]), "g_z": _rn(s + 1, *z).to(DT[dt])}
                    if with_noise:
                        d["noise"] = _rn(s + 2, *z).to(DT[dt])
                    return d

                def call(ops, d):
                    coef = torch.tensor(COEF, device=d["moments"].device)
                    z, kl = ops.gauss_reg(d["moments"], d.get("noise"))
                    return {"z": z, "kl_sum": kl, "g": ops.gauss_reg_bwd(d["moments"], d.get("noise"), d["g_z"], coef),
                            "g_kl_alone": ops.gauss_reg_bwd(d["moments"], d.get("noise"), None, coef)}

                out.append(("gauss", f"gauss/{name}/{dt}/{'noise' if with_noise else 'mean'}", inputs, call))
    return out


def entries():
    """every (table, case name, host inputs as a thunk, the calls on device tensors -> {output name: tensor})"""
    return _reduce_entries() + _frames_entries() + _gauss_entries()


def keys():
    return [name for _, name, _, _ in entries()]


def input_digests():
    """the operands themselves, on the host: {table: sha256 over every case's tensors, cases in table order, tensors by name}"""
    hs = {t: hashlib.sha256() for t in TABLES}
    for table, _, inputs, _ in entries():
        t = inputs()
        hs[table].update(sha([t[k] for k in sorted(t)]).encode())
    return {t: h.hexdigest() for t, h in hs.items()}


def pass_digests():
    """every case once on the device: {case: {output name: sha256 of its bytes}}"""
    from cvvae_amd import ops
    out = {}
    for _, name, inputs, call in entries():
        got = call(ops, {k: v.cuda() for k, v in inputs().items()})
        torch.cuda.synchronize()
        out[name] = {k: sha([v]) for k, v in got.items()}
    return out


def digests():
    return {"inputs": input_digests(), "passes": pass_digests()}


if __name__ == "__main__":
    print(json.dumps(digests(), indent=1, sort_keys=True))
