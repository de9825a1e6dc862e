"""Every built conv instance against an fp64 reference, at the shapes where tiled kernels go wrong (tests/conv_instance_cases.py):
partial spatial tiles, halos at padded borders in both pad modes, a partial N tile, the last K chunk, the boundary frames of
the time folds, To = 1 under two-frame tiles and the odd-frame sibling split.

Per case: the launch must report the declared kernel (ops.PROFILE); the output buffer is pre-filled with NaN and followed by a
sentinel guard, so every logical element must be written and nothing past the end; each element must satisfy
|y - ref| <= a * S + b * |ref| + tiny with S its own convolution over absolute values (conv_instance_cases.compare); fused
statistics must finalize to the fp64 moments of the stored output.  Large launches (the four-wave instance needs 2^19 output
pixels) are compared at sampled pixels: every tile-edge pixel of the boundary frames plus a seeded random set."""
import os

import pytest
import torch

from tests import conv_instance_cases as CI

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
SENTINEL = -7.0  # exact in every storage dtype
SAMPLE_ABOVE = 2e10  # multiply-adds of the reference above which it is evaluated at sampled pixels only (the four-wave case)

_INSTS = CI.instances()
CASES = CI.cases(_INSTS)


def _nan_buffer(shape, dtype):
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)
    buf[n:] = SENTINEL
    return buf, buf[:n].view(shape)


def _to_dev_ndhwc(x):
    return x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def _run_shape(case, s, si, monkeypatch, say):
    from cvvae_amd import ops
    for k, v in case.env().items():
        monkeypatch.setenv(k, v)
    seed = 1000 * si + sum(map(ord, case.id)) % 1000
    t = CI.make_tensors(case, s, seed)
    dt = CI.torch_dtype(case.dtype)
    fast = {CI.F32Q: True, CI.F32Q6: "fp6"}.get(case.dtype, False)
    To, Ho, Wo = s.out_grid
    w = t["w"].to(DEV)
    bias = t["bias"].to(DEV)
    kw = dict(stride=s.stride, pad=s.pad, pad_mode_t=s.mode_t, pad_mode_hw=s.mode_hw, out_mode=s.out_mode, out_f32=s.out_f32)
    if s.rowpack:
        x = ops.ncdhw_to_rowpack(t["x"].to(DEV), dt, s.mode_hw)
        pw = ops.pack_weight_rowpack(w, bias, time_folds=s.time_folds)
        kw["row_packed"] = True
    elif s.gather:
        x = _to_dev_ndhwc(t["x"])
        pw = ops.pack_weight_tapsn(w)
    else:
        x = _to_dev_ndhwc(t["x"])
        if s.batched:
            pw = ops.pack_weight_batched(w, (1, 1, 1), cin_pad=s.Cin, strides=(s.Cin, 1, 0), cout=s.Cout, cin=s.Cin)
        elif s.ups == 2:
            pw = ops.pack_weight_upfold(w, bias, tfold=s.tfold, time_folds=s.time_folds, fast=fast)
        elif s.time_folds:
            pw = ops.pack_weight_tfolds(w, bias, fast=fast)
        else:
            pw = ops.pack_weight(w.reshape(s.Cout, s.Cin, -1), bias, s.k, fast=fast)
    if s.prologue:
        kw.update(prologue=s.prologue, gn=(t["scale"].to(DEV), t["shift"].to(DEV)))
    if s.residual:
        kw["residual"] = _to_dev_ndhwc(t["res"])
    if s.sc_cin:
        pws = ops.pack_weight(t["w2"].reshape(s.Cout, s.sc_cin, 1).to(DEV), t["bias2"].to(DEV), (1, 1, 1), wscale=pw.wscale)
        kw.update(shortcut=(_to_dev_ndhwc(t["x2"]), pws), bias=pw.bias + pws.bias)
    if s.ups:
        kw["upsample2x"] = s.ups
    if case.dtype == CI.F32Q6:
        op_max = CI.operand(s, t).abs().max().item()
        if s.act_bound == "dev":
            kw["act_bound_dev"] = torch.tensor([op_max], dtype=torch.float32, device=DEV)
        else:
            pw.act_bound = 1.25 * op_max  # the ABI's contract: the operand stays inside the stated bound
    if s.gn_out:
        kw["gn_out"] = s.gn_out
    # the stored tensor, NaN-filled, with a guard behind it
    if s.out_mode == 1:
        oshape = (s.B, s.Cout, To, Ho, Wo)
    elif s.out_mode == 2:
        oshape = (s.B, 2 * To - 1, Ho, Wo, s.Cout // 2)
    else:
        oshape = (s.B, To, Ho, Wo, s.Cout)
    buf, out = _nan_buffer(oshape, torch.float32 if s.out_f32 else dt)
    seen = []
    ops.PROFILE = lambda d, pw_, launch: (seen.append(ops.conv_kernel_name(d)), launch())
    try:
        res = ops.conv(x, pw, out=out, **kw)
    finally:
        ops.PROFILE = None
    part = res[1] if s.gn_out else None
    gathered = None
    if s.gather:
        gathered = ops.conv_out_gather(out, 3, torch.cat([t["bias"], torch.zeros(29)]).to(DEV), s.mode_hw, dt)
    stats = None
    if part is not None:
        C = part.C
        one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        sc, sh = ops.gn_finalize(part, one, zero, 1e-6)
        stats = (sc, sh)
    torch.cuda.synchronize()
    assert seen == [s.names[0]], f"{case.id}: launched {seen}, declared {s.names[0]} (force {case.force})"
    got_all = buf.float().cpu()
    n = got_all.numel() - GUARD
    assert (got_all[n:] == SENTINEL).all(), f"{case.id}: wrote past the end of the output"
    assert torch.isfinite(got_all[:n]).all(), f"{case.id}: {int((~torch.isfinite(got_all[:n])).sum())} output elements not written"
    got = out.float().cpu()
    a, b = CI.tolerance(case, s)
    macs = s.pixels * s.Cout * (t["w"][0].numel() if not s.batched else s.Cin)
    if macs > SAMPLE_ABOVE:
        pts = CI.sample_points(case, s, seed)
        ref, S = CI.reference(case, s, t, pts)
        g = got[pts[0], pts[1], pts[2], pts[3]]
        worst, idx, nbad = CI.compare(g, ref, S, a, b)
        where = f"pixel {tuple(int(p[idx[0]]) for p in pts)} ch {idx[1]}" if idx else ""
        what = f"{pts[0].numel()} sampled pixels"
    else:
        ref, S = CI.reference(case, s, t)
        if s.gather:  # the raw taps-in-N columns: a (3,1,1) conv whose weight is the 3x3x3 weight with its taps in N
            wv = torch.zeros(32, s.Cin, 3, 1, 1, dtype=t["w"].dtype)
            wv[:27] = t["w"].permute(3, 4, 0, 1, 2).reshape(27, s.Cin, 3, 1, 1)
            s_raw = CI.Shape(s.B, s.Ti, s.Hi, s.Wi, s.Cin, 32, (3, 1, 1), pad=((1, 1), (0, 0), (0, 0)), mode_t=s.mode_t,
                             prologue=s.prologue, out_f32=True)
            ref, S = CI.reference(case, s_raw, dict(t, w=wv, bias=torch.zeros(32)))
        if s.out_mode != 1:
            got = got.permute(0, 4, 1, 2, 3)
        worst, idx, nbad = CI.compare(got, ref, S, a, b)
        where, what = f"at {idx}", "all elements"
    say(f"  {case.id:64s} shape {si}: launched {'+'.join(s.names)}  worst err/bound {worst:.3f} {where} ({what})")
    assert nbad == 0, f"{case.id} shape {si}: {nbad} elements outside the bound, worst {worst:.3g} {where}"
    ratios = [worst]
    if gathered is not None:
        refg, Sg = CI.reference(case, s, t)
        wg, ig, nb = CI.compare(gathered.float().cpu(), refg, Sg, a, CI.ULP16.get(case.dtype, 2.0 ** -24))
        say(f"  {'':64s} conv_out_gather: worst err/bound {wg:.3f} at {ig}")
        assert nb == 0, f"{case.id}: conv_out_gather {nb} elements outside the bound, worst {wg:.3g} at {ig}"
        ratios.append(wg)
    if stats is not None:
        sc, sh = (v.cpu().double() for v in stats)
        C = sc.shape[1]
        cpg = C // s.gn_out
        rstd = sc.reshape(s.B, s.gn_out, cpg)[:, :, 0]
        mean = (-sh / sc).reshape(s.B, s.gn_out, cpg)[:, :, 0]
        stored = out.float().cpu()
        stored = stored.permute(0, 4, 1, 2, 3) if s.out_mode != 1 else stored
        m_ref, r_ref = CI.group_stats(stored, s.gn_out)
        ws = CI.compare_stats(mean, rstd, m_ref, r_ref)
        say(f"  {'':64s} fused statistics: worst err/tol {ws:.3f} ({part.slabs} records per group)")
        assert ws <= 1.0, f"{case.id}: fused statistics off, worst {ws:.3g} x tolerance"
        ratios.append(ws)
    return max(ratios)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_conv_instance_matches_fp64_reference(case, monkeypatch, capsys):
    torch.set_num_threads(min(16, int(os.environ.get("OMP_NUM_THREADS", "16") or 16)))

    def say(msg):  # one line per launch on the terminal, captured or not: the margins are part of the result
        with capsys.disabled():
            print(msg, flush=True)

    worst = 0.0
    for si, s in enumerate(case.shapes):
        worst = max(worst, _run_shape(case, s, si, monkeypatch, say))
    say(f"{case.id} [{case.inst.family}] worst ratio {worst:.3f}")
