"""CPU checks of the weight-gradient edge tests' own parts (tests/wgrad_ref.py, tests/wgrad_edge_cases.py); the library is loaded
for its host-side plan only, no GPU.

  1. the plan is real: every conv case's declared facts (kernel, slab count, panels per slab, mid-row slab starts, the boundary a
     mid-row slab crosses, FAST eligibility, fused bias) hold for the slab count cvvae_conv_wgrad_workspace_bytes reports;
  2. the fp64 reference equals fp64 autograd of F.conv3d over the padded operand to 1e-12 relative (the small cases);
  3. the bound is honest: an fp32 emulation of the kernels' arithmetic (panels, slabs, the bf16 hi / lo products of fp32 models)
     stays at or below 0.5 of the bound on every element of every case, and so do tests/emu_ops.py's restatements;
  4. the check catches errors: each seeded defect of wgrad_ref.DEFECTS pushes the emulation's worst ratio above 1;
  5. the tables cover the reduce kernel's and the channel sums' loop edges.
Run with -s for the ratios."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_edge_cases as WC
import wgrad_ref as WR
from tests import emu_ops

CONV = WC.conv_cases()
CHAN = WC.chan_cases()
FOLD = WC.fold_cases()
BY_NAME = {c.name: c for c in CONV}
SMALL = [c for c in CONV if c.pixels * c.cin * c.cout * c.ntaps <= 3e8]


def _ids(cs):
    return [c.name for c in cs]


def _lib():
    from cvvae_amd import _lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------------------ 5. coverage
def test_tables_cover_the_loop_edges():
    names = [c.name for c in CONV + CHAN + FOLD]
    assert len(set(names)) == len(names)
    # wgrad_reduce_kernel: the eight-deep slab loop alone, its tail alone, both; every tap count; a narrow last input-channel block
    ns = {c.nslab for c in CONV}
    assert any(n < 8 for n in ns) and 8 in ns and any(n > 8 and n % 8 for n in ns) and any(n > 8 and n % 8 == 0 for n in ns), ns
    assert {c.ntaps for c in CONV} == {1, 3, 9, 27}
    assert any(WC.round_up(c.cin, 8) % 64 for c in CONV) and any(c.cout < 128 for c in CONV)
    # the three kernels, both strides of the DMA ring, both pad modes, the deep pipeline
    assert {(c.kernel, c.xp, c.k[1]) for c in CONV} == {(WC.DMA, False, 3), (WC.REG, True, 3), (WC.REG, True, 1), (WC.REG, False, 1)}
    dma = [c for c in CONV if c.kernel == WC.DMA]
    assert {c.stride[2] for c in dma if c.pmin >= 4} == {1, 2} and {c.mode_hw for c in dma if c.pmin >= 4} == {WC.REP, WC.ZERO}
    assert {c.out_grid[2] for c in dma} >= {1, 63, 64, 65} and {c.dims[3] for c in dma} >= {1, 2}
    assert {c.crosses for c in CONV} >= {"frame", "batch"} and any(c.nan_gap for c in dma)
    fast = [c for c in CONV if c.fast]
    assert any(c.mode_t == WC.REP and c.mode_hw == WC.REP for c in fast) and any(c.mode_hw == WC.ZERO and c.stride[2] == 1 for c in fast)
    assert any(c.stride[2] == 2 for c in fast)
    reg32 = [c for c in CONV if c.kernel == WC.REG and c.xp]
    assert {c.out_grid[2] for c in reg32} >= {1, 31, 32, 33} and any(c.k == (3, 1, 1) for c in reg32) and any(c.nan_gap for c in reg32)
    assert any(c.stride == (2, 2, 2) for c in reg32) and any(c.pmin >= 4 and c.k[1] == 3 for c in reg32) and any(c.pmin >= 4 and c.k[1] == 1 for c in reg32)
    reg16 = [c for c in CONV if c.kernel == WC.REG and not c.xp]
    assert {c.out_grid[2] for c in reg16} >= {1, 127, 128, 129} and any(c.pmin >= 5 and c.out_grid[2] % 128 for c in reg16)
    assert all(BY_NAME[n].k[1] == 3 and WC.BF16 in BY_NAME[n].dtypes for n in WC.REG16_K3_CHILD) and len(WC.REG16_K3_CHILD) == 4
    # chan_sums_kernel / chan_sums_final_kernel (csrc/bwd_kernels.hip)
    for op in ("bias", "gn"):
        assert {c.C for c in CHAN if c.op == op} == {8, 24, 512, 2048}
    for C in (8, 24, 512, 2048):
        ppp = max(256 // (C // 8), 1)
        assert {c.rows * c.S for c in CHAN if c.op == "bias" and c.C == C} >= {4 * ppp - 1, 4 * ppp, 4 * ppp + 1, WC.split_len(C)}
    assert {c.nparts for c in CHAN} >= {1, 8, 25, 32, 33, 57}
    assert all(c.ps > c.C for c in CHAN if c.op == "bias")
    # pad_fold_kernel
    assert any(c.dims[1:] == (1, 1, 1) and c.mode_t == WC.REP for c in FOLD) and {c.C for c in FOLD} == {8, 520}
    assert {(c.pad_t, c.mode_t) for c in FOLD} >= {((2, 0), WC.REP), ((1, 1), WC.REP), ((1, 1), WC.ZERO)} and {c.add for c in FOLD} == {True, False}
    for axis in (1, 2, 3):
        assert any(c.dims[axis] == 1 and (c.mode_t if axis == 1 else c.mode_hw) == WC.REP for c in FOLD)
    assert any(c.vectors > 8192 * 256 for c in FOLD)


# ------------------------------------------------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("case", CONV, ids=_ids(CONV))
def test_declared_plan_holds_in_the_library(case):
    L, lib = _lib()
    for dt in case.dtypes:
        d = WR.conv_desc(L, case, dt)
        nslab = WR.lib_nslab(lib, d)
        f = WR.plan_facts(case, nslab)
        assert nslab == case.nslab, (case.name, dt, nslab)
        assert (f["pmin"], f["pmax"], f["midrow"]) == (case.pmin, case.pmax, case.midrow), (case.name, dt, f)
        assert not case.crosses or case.crosses in f["crossed"], (case.name, f)
        assert lib.cvvae_conv_wgrad_fuses_bias(d) == (1 if case.kernel == WC.DMA else 0)
        assert (case.kernel == WC.DMA) == (dt != WC.F32 and case.k[1] == 3)
        assert WR.fast_eligible(case) == case.fast


@pytest.mark.parametrize("case", CHAN, ids=_ids(CHAN))
def test_declared_parts_hold_in_the_library(case):
    """nparts (rows x splits, what chan_sums_final_kernel loops over) out of cvvae_channel_sums_workspace_bytes"""
    _, lib = _lib()
    rows, S = (1, case.rows * case.S) if case.op == "bias" else (case.rows, case.S)
    assert int(lib.cvvae_channel_sums_workspace_bytes(rows, S, case.C)) == case.nparts * case.C * 2 * 4


# ------------------------------------------------------------------------------------------------------------ 2. the reference
def _pad3(f, pad, mode_t, mode_hw):
    (tf, tb), (hf, hb), (wf, wb) = pad
    if hf or hb or wf or wb:
        f = F.pad(f, (wf, wb, hf, hb, 0, 0), mode="replicate") if mode_hw == WC.REP else F.pad(f, (wf, wb, hf, hb))
    if tf or tb:
        f = F.pad(f, (0, 0, 0, 0, tf, tb), mode="replicate") if mode_t == WC.REP else F.pad(f, (0, 0, 0, 0, tf, tb))
    return f


@pytest.mark.parametrize("case", SMALL, ids=_ids(SMALL))
def test_reference_agrees_with_fp64_autograd(case):
    dt = case.dtypes[-1]
    t = WR.conv_inputs(case, dt)
    f = _pad3(t["a"][..., :case.cin].double().permute(0, 4, 1, 2, 3), case.pad, case.mode_t, case.mode_hw)
    w = torch.zeros(case.cout, case.cin, *case.k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(f, w, None, stride=case.stride)
    gy = t["gy"][..., :case.cout].double()
    assert tuple(y.shape[2:]) == tuple(gy.shape[1:4])
    (y * gy.permute(0, 4, 1, 2, 3)).sum().backward()
    ref = WR.conv_reference(case, dt)
    theirs = w.grad.reshape(case.cout, case.cin, case.ntaps)
    assert (ref["dw"].ref - theirs).abs().max() <= 1e-12 * theirs.abs().max()
    db = gy.reshape(-1, case.cout).sum(0)
    assert (ref["db"].ref - db).abs().max() <= 1e-12 * db.abs().max()
    assert torch.isfinite(ref["dw"].bound).all() and (ref["dw"].bound > 0).all()


def test_small_cases_reach_every_kind_of_case():
    assert {(c.kernel, c.xp, c.k) for c in SMALL} >= {(WC.DMA, False, WC.K333), (WC.REG, True, WC.K333), (WC.REG, True, WC.K311), (WC.REG, False, WC.K111)}
    assert {c.stride for c in SMALL} >= {WC.S1, WC.S222} and {c.mode_hw for c in SMALL} == {WC.REP, WC.ZERO} and any(c.nan_gap for c in SMALL)


@pytest.mark.parametrize("case", FOLD[:-1], ids=_ids(FOLD[:-1]))
def test_fold_reference_agrees_with_fp64_autograd(case):
    t = WR.fold_inputs(case, WC.F32)
    B, T, H, W = case.dims
    x = torch.zeros(B, case.C, T, H, W, dtype=torch.float64, requires_grad=True)
    y = _pad3(x, (case.pad_t, (1, 1), (1, 1)), case.mode_t, case.mode_hw)
    (y * t["gp"].double().permute(0, 4, 1, 2, 3)).sum().backward()
    theirs = x.grad.permute(0, 2, 3, 4, 1) + (t["add"].double() if case.add else 0.0)
    mine = WR.fold_reference(case, WC.F32)["out"].ref
    assert (mine - theirs).abs().max() <= 1e-12 * theirs.abs().max()


# ------------------------------------------------------------------------------------------------------------ 3. the bound
@pytest.mark.parametrize("case", CONV, ids=_ids(CONV))
def test_fp32_emulation_sits_inside_the_bound(case):
    for dt in case.dtypes:
        ref = WR.conv_reference(case, dt)
        assert all(torch.isfinite(c.ref).all() and torch.isfinite(c.bound).all() for c in ref.values())
        w, at, bad = WR.conv_worst(case, dt, WR.conv_emulate(case, dt, case.nslab))
        t = WR.conv_inputs(case, dt)
        # (the gap channels' NaN never reach emu_ops: it slices the real channels, as the kernel must)
        raw = emu_ops.conv_wgrad(t["a"], t["gy"], case.k, stride=case.stride, pad=case.pad, pad_mode_t=case.mode_t, pad_mode_hw=case.mode_hw,
                                 cin=case.cin, cout=case.cout, bias=True)
        w2, at2, _ = WR.conv_worst(case, dt, raw)
        print(f"WGRAD-EDGE-HOST {case.name} {dt}: K = {case.pixels}, emulation err/bound = {w:.4f} at {at}; emu_ops {w2:.4f} at {at2}")
        assert w <= 0.5 and bad == 0, (case.name, dt, w, at)
        assert w2 <= 0.5, (case.name, dt, w2, at2)


def test_split_precision_term_is_the_bf16_formats_own():
    """why fp32 models carry XP_BF16 = 3 * 2^-16 and not the forward convs' XP_ULP (wgrad_ref's docstring): the three-product form
    is right to 3 * 2^-16 per product, and the emulation of a six-pixel sum uses more than half of a bound built on XP_ULP"""
    from conv_instance_cases import XP_ULP
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(1 << 20, generator=g), torch.randn(1 << 20, generator=g)
    (xh, xl), (yh, yl) = WR._split(x), WR._split(y)
    three = xh.double() * yh.double() + xh.double() * yl.double() + xl.double() * yh.double()
    rel = ((three - x.double() * y.double()).abs() / (x.double() * y.double()).abs()).max().item()
    assert XP_ULP < rel <= WR.XP_BF16, rel
    case = BY_NAME["reg32-w1"]
    raw = WR.conv_emulate(case, WC.F32, case.nslab)
    assert WR.conv_worst(case, WC.F32, raw, xp=XP_ULP)[0] > 0.5 >= WR.conv_worst(case, WC.F32, raw)[0]


@pytest.mark.parametrize("case", CHAN, ids=_ids(CHAN))
def test_channel_sums_emulation_sits_inside_the_bound(case):
    for dt in case.dtypes:
        t = WR.chan_inputs(case, dt)
        if case.op == "bias":
            assert torch.isnan(t["gy"][..., case.C:]).all()
            t = {"gy": t["gy"][..., :case.C]}
        w, at, bad = WR.chan_worst(case, dt, WR.chan_call(emu_ops, case, t))
        print(f"WGRAD-EDGE-HOST {case.name} {dt}: emu_ops err/bound = {w:.4f} at {at}")
        assert w <= 0.5 and bad == 0, (case.name, dt, w, at)


@pytest.mark.parametrize("case", FOLD, ids=_ids(FOLD))
def test_pad_fold_emulation_sits_inside_the_bound(case):
    for dt in case.dtypes:
        chk = WR.fold_reference(case, dt)["out"]
        raw = WR.fold_call(emu_ops, case, {k: v.float() for k, v in WR.fold_inputs(case, dt).items()})  # fp32, before the store
        w, idx, bad = WR.compare(raw[0], chk.ref, chk.before_store())
        wr, at, badr = WR.fold_worst(case, dt, (raw[0].to(WR.DTYPE[dt]),))
        print(f"WGRAD-EDGE-HOST {case.name} {dt}: emu_ops err/bound = {w:.4f} before the store, {wr:.4f} rounded at {at}")
        assert w <= 0.5 and bad == 0 and wr <= 1.0 and badr == 0, (case.name, dt, w, wr)


# ------------------------------------------------------------------------------------------------------------ 4. the check catches errors
DEFECT_CASES = {
    "drop_tail": ("dma-deep-causal333-512", "reg32-w33", "reg16-linear-512-row15400", "dma-w63"),
    "panel_twice": ("dma-deep-causal333-512", "dma-deep-stride122-512", "reg32-linear-512-row10000", "reg16-w129"),
    "tap_shift": ("dma-deep-frame133-zero-512", "dma-wi2-rep", "reg32-k311", "dma-stride222-odd"),
    "clamp": ("dma-deep-frame133-zero-512", "dma-wi1-zero", "dma-wi2-zero", "reg32-w31", "dma-nan-gap-72to136"),
    "skip_slab": ("dma-deep-sym333-256", "dma-fast-frame133-zero-128", "reg32-deep-causal333-512", "reg16-8to8-w1"),
    "swap_tail": ("dma-nan-gap-72to136", "dma-conv-in-3of16", "reg32-nan-gap-72to136", "dma-deep-fast-512"),
}


@pytest.mark.parametrize("defect,name", [(d, n) for d in WR.DEFECTS for n in DEFECT_CASES[d]])
def test_seeded_defect_exceeds_the_bound(defect, name):
    case = BY_NAME[name]
    dt = case.dtypes[-1]
    w, at, bad = WR.conv_worst(case, dt, WR.conv_emulate(case, dt, case.nslab, defect=defect))
    print(f"WGRAD-EDGE-HOST defect {defect} on {name} {dt}: err/bound = {w:.1f} at {at} ({bad} elements)")
    assert w > 1.0 and bad >= 1, (defect, name, w)


def test_tap_shift_on_a_one_pixel_row_is_no_defect():
    """Wi = 1 under replicate padding: every column IS the neighbouring column -- why the tap_shift cases start at Wi = 2"""
    case = BY_NAME["dma-wi1-rep"]
    a = WR.conv_emulate(case, WC.BF16, case.nslab)[0]
    assert torch.equal(a, WR.conv_emulate(case, WC.BF16, case.nslab, defect="tap_shift")[0])


def test_compare_flags_nan_and_one_bad_element():
    case = BY_NAME["dma-nan-gap-72to136"]
    ref = WR.conv_reference(case, WC.BF16)
    dw, db = ref["dw"].ref.clone().float(), ref["db"].ref.clone().float()
    assert WR.conv_worst(case, WC.BF16, (dw, db))[0] <= 0.01
    dw[135, 71, 26] = float("nan")
    assert WR.conv_worst(case, WC.BF16, (dw, db))[0] == float("inf")
    dw[135, 71, 26] = float(ref["dw"].ref[135, 71, 26] + 1.5 * ref["dw"].bound[135, 71, 26])
    w, at, bad = WR.conv_worst(case, WC.BF16, (dw, db))
    assert 1.4 < w < 1.6 and bad == 1 and at == "dw(135, 71, 26)"
