"""16-bit parameters on fp32 master weights on the MI355X: cvvae_mt_adamw_master, cvvae_mt_sumsq and cvvae_mt_norm_finish
(csrc/optim_kernels.hip) on the edge list of tests/optim_ref.py stored in 16 bits (tests/master_ref.py edge_list16: numel 0, 1 (0-dim),
7, chunk - 1, chunk, chunk + 1, 3 chunk + 5, a view that starts 2 bytes into its buffers, one whose g is 16-byte aligned while its p is
not, a tensor without a gradient; steps t in {1, 2, 7, 1000} inside one launch), then cvvae_amd.optim.AdamW(master_weights=True) over it.

The yardstick of the master pass is the EXISTING fp32 pass: master, m and v must carry the bits cvvae_mt_adamw gives on fp32 copies
with g.float() -- the element update is the same expression and must contract to the same FMAs -- and they meet the derived bounds of
tests/test_gpu_optim.py against the fp64 formulas (m: 3 ulp(max(|m|, |G|)), v: 4 ulp(max(v, G^2)), master: 3 (ulp(|w|) + 2^-20 |delta|)).
p is bit-equal to master.to(dtype), torch's round-to-nearest-even conversion; g keeps its bits; so does every guard element in
front of and behind every view.  The norm of 16-bit gradients has the bits of the fp32 passes over g.float(): squares and sums are
fp32 in the same order."""
import math

import pytest
import torch
import torch.nn as nn

from tests import master_ref as M
from tests import optim_ref as R

pytestmark = pytest.mark.gpu
LR = R.YAML_LR
B1, B2 = R.YAML_ADAMW["betas"]
EPS, WD = R.YAML_ADAMW["eps"], R.YAML_ADAMW["weight_decay"]
COEF = 0.37
FIELDS = ("g", "p", "m", "v", "w")
_EDGES = {}


def _edge(dtype):
    if dtype not in _EDGES:
        _EDGES[dtype] = M.edge_list16(dtype)
    return _EDGES[dtype]


def _device_copy(edge):
    out = []
    for e in edge:
        bufs = {k: e[k].cuda() for k in e if k.endswith("_buf")}
        out.append((bufs, M.views16(e, bufs)))
    return out


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _scalars(edge, sel):
    return dict(step_size=[LR / (1.0 - B1 ** edge[i]["t"]) for i in sel], bias2_sqrt=[math.sqrt(1.0 - B2 ** edge[i]["t"]) for i in sel])


def _master_list(edge, dev, dtype):
    from cvvae_amd import ops
    sel = [i for i, e in enumerate(edge) if e["has_grad"]]
    mtl = ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda", dtype)
    pick = lambda k: [dev[i][1][k] for i in sel]  # noqa: E731
    return mtl.set(g=pick("g"), p=pick("p"), m=pick("m"), v=pick("v"), shadow=pick("w"), **_scalars(edge, sel)), sel


def _fp32_list(edge, dev, fields=("g", "p", "m", "v")):
    """the existing passes' list over fp32 copies: g.float() for g, the master for p"""
    from cvvae_amd import ops
    sel = [i for i, e in enumerate(edge) if e["has_grad"]]
    mtl = ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda")
    src = {"g": lambda v: v["g"].float(), "p": lambda v: v["w"].clone(), "m": lambda v: v["m"].clone(), "v": lambda v: v["v"].clone()}
    kw = {f: [src[f](dev[i][1]) for i in sel] for f in fields}
    if "m" in fields:
        kw.update(_scalars(edge, sel))
    return mtl.set(**kw), sel


def _untouched(edge, dev, written):
    """a written view's buffer keeps its bits in front of and behind the view; every other buffer keeps all of them"""
    for e, (bufs, _) in zip(edge, dev):
        for k in FIELDS:
            lo, hi = e["off"][k], e["off"][k] + e["n"]
            after, before = _bits(bufs[k + "_buf"].cpu()), _bits(e[k + "_buf"])
            if k in written and e["has_grad"]:
                assert torch.equal(after[:lo], before[:lo]) and torch.equal(after[hi:], before[hi:]), (e["n"], k)
            else:
                assert torch.equal(after, before), (e["n"], k)


def test_the_edge_list_holds_the_alignment_cases_it_claims():
    edge = _edge(torch.bfloat16)
    dev = _device_copy(edge)
    mis = [tuple(v[k].data_ptr() % 16 for k in FIELDS) for e, (_, v) in zip(edge, dev) if e["n"] == R.CHUNK + 3 or e["n"] == R.CHUNK + 1]
    assert (2, 2, 4, 4, 4) in mis            # every operand starts off a 16-byte boundary: 2 bytes in for g and p
    assert (2, 2, 0, 0, 0) in mis            # the 16-bit operands alone
    assert (0, 2, 0, 0, 0) in mis            # an aligned g beside an unaligned p
    assert (0, 0, 0, 0, 0) in mis


@pytest.mark.parametrize("coef", [None, COEF], ids=["nocoef", "coef"])
@pytest.mark.parametrize("dtype", M.DTYPES16, ids=["bf16", "fp16"])
def test_adamw_master_pass_on_every_edge_in_one_launch(dtype, coef):
    from cvvae_amd import ops
    edge = _edge(dtype)
    dev = _device_copy(edge)
    mtl, sel = _master_list(edge, dev, dtype)
    ref, _ = _fp32_list(edge, dev)
    assert mtl.n_chunks == ref.n_chunks == 1 + 1 + 1 + 1 + 2 + 4 + 2 + 2 + 2          # one launch, 10 tensors (one of them empty)
    c = None if coef is None else torch.tensor([COEF], dtype=torch.float32, device="cuda")
    ops.mt_adamw_master(mtl, LR, B1, B2, EPS, WD, c)
    ops.mt_adamw(ref, LR, B1, B2, EPS, WD, c)                 # the yardstick: the existing fp32 pass on fp32 copies
    torch.cuda.synchronize()
    worst = [0.0, 0.0, 0.0]
    c32 = None if coef is None else torch.tensor(coef, dtype=torch.float32).item()
    for j, i in enumerate(sel):
        e, v = edge[i], dev[i][1]
        where = (e["n"], e["off"], e["t"])
        for k, f in (("w", "p"), ("m", "m"), ("v", "v")):
            assert _same_bits(v[k], ref.tensors[f][j]), (where, k)
        assert _same_bits(v["p"], v["w"].to(dtype)), where
        # and the derived bounds against the fp64 formulas
        h = M.views16(e, e)
        m2, v2, w2, G, delta = R.adamw64(h["g"].float(), h["w"], h["m"], h["v"], e["t"], LR, B1, B2, EPS, WD, c32)
        bounds = ((m2, 3 * R.ulp32(torch.maximum(h["m"].double().abs(), G.abs()))),
                  (v2, 4 * R.ulp32(torch.maximum(h["v"].double(), G * G))),
                  (w2, 3 * (R.ulp32(h["w"].double()) + 2.0 ** -20 * delta.abs())))
        for q, (k, (want, bound)) in enumerate(zip(("m", "v", "w"), bounds)):
            if e["n"]:
                w = float(((v[k].cpu().double() - want).abs() / bound).max())
                worst[q] = max(worst[q], w)
                assert w <= 1.0, (where, k, w)
    print(f"mt_adamw_master {dtype}, coef {coef}: fractions of the m / v / master bounds {worst}")
    _untouched(edge, dev, ("p", "m", "v", "w"))               # g among the untouched: it is read only


def _sumsq_finish(lists, max_norm):
    from cvvae_amd import ops
    partials = torch.empty(sum(m.n_chunks for m in lists), dtype=torch.float32, device="cuda")
    at = 0
    for m in lists:
        ops.mt_sumsq(m, partials[at:at + m.n_chunks])
        at += m.n_chunks
    return ops.mt_norm_finish(partials, max_norm)


def _g_list(edge, dev, dtype, convert=None):
    from cvvae_amd import ops
    sel = [i for i, e in enumerate(edge) if e["has_grad"]]
    gs = [dev[i][1]["g"] if convert is None else dev[i][1]["g"].to(convert) for i in sel]
    return ops.MultiTensorList([edge[i]["n"] for i in sel], "cuda", dtype if convert is None else convert).set(g=gs)


def test_sumsq_and_finish_have_the_bits_of_grad_norm_on_fp32_16_bit_and_mixed_lists():
    from cvvae_amd import ops
    fp32 = R.edge_list(0)
    dev32 = [{k: d[k].cuda() for k in d if k.endswith("_buf")} for d in fp32]
    sel = [i for i, d in enumerate(fp32) if d["has_grad"]]
    g32 = [R.views(fp32[i], dev32[i])["g"] for i in sel]
    l32 = ops.MultiTensorList([fp32[i]["n"] for i in sel], "cuda").set(g=g32)
    for mx in (1.0, 1e6):
        want = ops.mt_grad_norm(l32, mx)
        got, again = _sumsq_finish([l32], mx), _sumsq_finish([l32], mx)
        torch.cuda.synchronize()
        assert _same_bits(got, want) and _same_bits(again, got)              # the fp32 list: the bits of cvvae_mt_grad_norm; twice
    assert float(want[1]) == 1.0 and 0.0 < float(ops.mt_grad_norm(l32, 1.0)[1]) < 1.0
    for dtype in M.DTYPES16:
        edge = _edge(dtype)
        dev = _device_copy(edge)
        l16, lf = _g_list(edge, dev, dtype), _g_list(edge, dev, dtype, torch.float32)
        want = ops.mt_grad_norm(lf, 1.0)                                      # the fp32 result over g.float()
        got, again = _sumsq_finish([l16], 1.0), _sumsq_finish([l16], 1.0)
        torch.cuda.synchronize()
        assert _same_bits(got, want) and _same_bits(again, got) and float(got[0]) > 1.0, dtype
        # mixed: the fp32 list's partials first, then the 16-bit list's = the fp32 pass over both lists' tensors in that order
        both = ops.MultiTensorList(list(l32.numels) + list(lf.numels), "cuda").set(g=list(l32.tensors["g"]) + list(lf.tensors["g"]))
        want = ops.mt_grad_norm(both, 1.0)
        got, again = _sumsq_finish([l32, l16], 1.0), _sumsq_finish([l32, l16], 1.0)
        torch.cuda.synchronize()
        assert _same_bits(got, want) and _same_bits(again, got), dtype
        c = torch.tensor(1.0, dtype=torch.float32) / (got[0].cpu() + 1e-6)
        assert torch.equal(got[1].cpu(), torch.clamp(c, max=1.0))
        _untouched(edge, dev, ())


def test_one_nan_gradient_element_poisons_norm_coefficient_and_step():
    from cvvae_amd import ops
    dtype = torch.bfloat16
    edge = _edge(dtype)
    dev = _device_copy(edge)
    dev[6][1]["g"][R.CHUNK + 17] = float("nan")
    mtl, sel = _master_list(edge, dev, dtype)
    out2 = _sumsq_finish([mtl], 1.0)
    ops.mt_adamw_master(mtl, LR, B1, B2, EPS, WD, out2[1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out2).all())
    for i in sel:                      # as torch: the NaN coefficient reaches every gradient, AdamW then writes NaN everywhere
        assert all(bool(torch.isnan(dev[i][1][k]).all()) for k in ("p", "w", "m", "v")), edge[i]["n"]


def test_optimizer_over_the_edge_list_equals_the_bare_passes_without_a_host_synchronisation():
    """AdamW(max_grad_norm, master_weights=True) over bf16, fp16 and fp32 parameters in ONE group = sumsq per dtype (fp32 first) +
    norm_finish + mt_adamw on the fp32 tensors + mt_adamw_master per 16-bit dtype; the tensor without a gradient keeps its bits and gets
    no state.  The first step runs freely (lazy state, the library); the second runs under torch's synchronisation check."""
    from cvvae_amd import ops
    from cvvae_amd.optim import AdamW
    kinds = (torch.bfloat16, torch.float16)
    fp32 = R.edge_list(0)
    sel32 = [i for i, d in enumerate(fp32) if d["has_grad"]]
    sets = []                          # (ours, the bare passes' copy) per dtype
    for dt in kinds:
        sets.append((_device_copy(_edge(dt)), _device_copy(_edge(dt))))
    ours32, ref32 = ([{k: d[k].cuda() for k in d if k.endswith("_buf")} for d in fp32] for _ in range(2))
    params, metas = [], []
    for dt, (dev, _) in zip(kinds, sets):
        for e, (_, v) in zip(_edge(dt), dev):
            p = nn.Parameter(v["p"])
            assert p.data_ptr() == v["p"].data_ptr()
            if e["has_grad"]:
                p.grad = v["g"]
            params.append(p)
            metas.append((e, v))
    for d, bufs in zip(fp32, ours32):
        v = R.views(d, bufs)
        p = nn.Parameter(v["p"])
        if d["has_grad"]:
            p.grad = v["g"]
        params.append(p)
        metas.append((d, v))
    opt = AdamW(params, lr=LR, max_grad_norm=1.0, master_weights=True, **R.YAML_ADAMW)
    for p, (e, v) in zip(params, metas):
        if e["has_grad"]:
            opt.state[p] = {"step": torch.tensor(float(e["t"] - 1)), "exp_avg": v["m"], "exp_avg_sq": v["v"]}
            if p.dtype != torch.float32:
                opt.state[p]["master"] = v["w"]
    versions = [p._version for p in params]
    opt.step()
    torch.cuda.synchronize()
    # the bare passes, two steps
    lists = [_master_list(_edge(dt), ref, dt)[0] for dt, (_, ref) in zip(kinds, sets)]
    l32 = ops.MultiTensorList([fp32[i]["n"] for i in sel32], "cuda")
    pick = lambda k: [R.views(fp32[i], ref32[i])[k] for i in sel32]  # noqa: E731
    for step in (0, 1):
        for dt, m in zip(kinds, lists):
            sel = [i for i, e in enumerate(_edge(dt)) if e["has_grad"]]
            m.set(step_size=[LR / (1.0 - B1 ** (_edge(dt)[i]["t"] + step)) for i in sel],
                  bias2_sqrt=[math.sqrt(1.0 - B2 ** (_edge(dt)[i]["t"] + step)) for i in sel])
        l32.set(g=pick("g"), p=pick("p"), m=pick("m"), v=pick("v"), step_size=[LR / (1.0 - B1 ** (fp32[i]["t"] + step)) for i in sel32],
                bias2_sqrt=[math.sqrt(1.0 - B2 ** (fp32[i]["t"] + step)) for i in sel32])
        out2 = _sumsq_finish([l32] + lists, 1.0)
        ops.mt_adamw(l32, LR, B1, B2, EPS, WD, out2[1])
        for m in lists:
            ops.mt_adamw_master(m, LR, B1, B2, EPS, WD, out2[1])
        if step == 0:
            torch.cuda.synchronize()
            assert _same_bits(opt.last_grad_norm, out2[0]) and opt.last_grad_norm.shape == () and opt.last_grad_norm.is_cuda
            torch.cuda.set_sync_debug_mode("error")
            try:
                opt.step()
            finally:
                torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert _same_bits(opt.last_grad_norm, out2[0])
    ref_views = [v for (_, ref) in sets for (_, v) in ref] + [R.views(d, b) for d, b in zip(fp32, ref32)]
    for i, (p, (e, _), rv) in enumerate(zip(params, metas, ref_views)):
        if not e["has_grad"]:
            assert p not in opt.state and p._version == versions[i] and _same_bits(p.detach(), rv["p"])
            continue
        st = opt.state[p]
        assert float(st["step"]) == e["t"] + 1 and st["step"].device.type == "cpu" and p._version >= versions[i] + 2
        for k, t in (("p", p.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            assert _same_bits(t, rv[k]), (e["n"], p.dtype, k)
        if p.dtype != torch.float32:
            assert _same_bits(st["master"], rv["w"]) and opt.master(p) is st["master"] and _same_bits(p.detach(), st["master"].to(p.dtype))
        assert _same_bits(p.grad, rv["g"])                                   # gradients are left unscaled
