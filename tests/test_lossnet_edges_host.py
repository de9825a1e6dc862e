"""CPU checks of the LPIPS / discriminator pass edge tests' own parts (tests/lossnet_ref.py, tests/lossnet_edge_cases.py): no GPU.

For every case and dtype:
  (a) the fp64 reference agrees with torch's own fp64 op or autograd to 1e-12 relative (F.max_pool2d, F.avg_pool3d after the
      torch.cat of frame 0, F.leaky_relu(F.group_norm), F.conv3d(stride=2, padding=1) and the head formula of tests/lpips_ref.py);
  (b) a plain fp32 torch evaluation stays within the per-element bound with worst err / bound <= 0.5, taken BEFORE the store rounding
      against the bound WITHOUT its store term, as tests/test_pass_edges_host.py defines it; rounded to the storage dtype it is held
      to err / bound <= 1 against the whole bound (exact outputs: bit for bit);
  (c) the table holds the edges it claims: the properties are computed from constants copied out of the kernels' headers, each with
      its source line; the slab counts are asked of the library itself (it loads without a GPU);
  (d) every output of a bounded case has at least 90 % of its elements above TINY in magnitude."""
import pytest
import torch

import lossnet_edge_cases as LC
import lossnet_ref as LR
import pass_edge_cases as PC
import pass_ref as PR

BY_OP = LC.by_op()
CASES = [c for c in LC.all_cases() if not c.raises and c.op != "split" and c.recipe != "device"]

# ---- constants of the kernels (a change there must be followed here: the coverage test below is computed from them)
WG = 256               # cvvae_amd/csrc/disc_kernels.hip:17  constexpr int WG = 256
VEC = 8                # disc_kernels.hip:18  constexpr int VEC = 8
MAX_BLOCKS = 2048      # disc_kernels.hip:19  constexpr int MAX_BLOCKS = 2048
DG_MAX_LDS = 64 * 1024  # disc_kernels.hip:345  constexpr int DG_MAX_LDS = 64 * 1024
MAX_STAT_C = WG * VEC  # disc_kernels.hip:431  constexpr int MAX_STAT_C = WG * VEC
RUN_TRIPS = 16         # disc_kernels.hip:516  const int64_t run = 16 * (WG / (C / VEC))
LPIPS_MAX_BLOCKS = 256 * 64   # cvvae_amd/csrc/lpips_kernels.hip:297  if (blocks > 256LL * 64) blocks = 256LL * 64
HEAD_FWD_BLOCKS = 256         # lpips_kernels.hip:289  constexpr int HEAD_FWD_BLOCKS = 256, HEAD_BWD_BLOCKS = 2048
HEAD_BWD_BLOCKS = 2048        # lpips_kernels.hip:289
HEAD_FINAL_WG = 64            # lpips_kernels.hip:217  const long long n = (long long)blockIdx.x * 64 + threadIdx.x


def _ids(cs):
    return [c.name for c in cs]


def slabs_expected(rows, per_row, C):
    """cvvae_pass_gn_slabs, restated (disc_kernels.hip:512-519)"""
    run = RUN_TRIPS * (WG // (C // VEC))
    return min((per_row + run - 1) // run, max(MAX_BLOCKS // rows, 1))


def sub_for(cpg):
    """disc_kernels.hip:442"""
    return 8 if cpg % 8 == 0 else 4 if cpg % 4 == 0 else 2


def _lib():
    from cvvae_amd import _lib as L
    return L.load()


def test_case_table_holds_the_edges_it_claims():
    """(c)"""
    names = [c.name for c in LC.all_cases()]
    assert len(set(names)) == len(names)
    S = lambda op, k, **f: {c.get(k) for c in BY_OP[op] if all(c.get(a) == b for a, b in f.items()) and not c.raises}
    # --- scale_in: all nine pairs on one shape; vector counts; pad vectors; the slice
    assert {(c["src"], c.dtypes[0]) for c in BY_OP["scale_in"] if (c["H"], c["W"]) == (15, 17)} == {(a, b) for a in PC.ALL for b in PC.ALL}
    assert {c["N"] * c["H"] * c["W"] * c["cpad"] // 8 for c in BY_OP["scale_in"]} >= {1, WG - 1, WG, WG + 1}
    assert S("scale_in", "cpad") == {8, 16, 32} and S("scale_in", "sliced") == {0, 1}
    assert {(c["N"] * c["H"] * c["W"], c["ps"]) for c in BY_OP["scale_in_bwd"]} >= {(n, ps) for n in (WG - 1, WG, WG + 1) for ps in (8, 32)}
    # --- relu, maxpool, relu_pool_bwd
    assert S("relu", "v") >= {1, WG - 1, WG, WG + 1} and {c.recipe for c in BY_OP["relu"]} == {"normal", "special", "nan"}
    mp = BY_OP["maxpool"]
    assert {(c["N"], c["H"], c["W"], c["C"]) for c in mp} >= {(1, 2, 2, 8), (2, 3, 3, 8), (1, 2, 5, 16), (3, 7, 9, 64)}
    assert {c["N"] * (c["H"] // 2) * (c["W"] // 2) * c["C"] // 8 for c in mp} >= {WG - 1, WG, WG + 1}
    assert {c.recipe for c in mp} == {"normal", "neg", "tie", "inf", "nan"}
    assert {c["pos"] for c in mp if c.recipe == "inf"} == {0, 1, 2, 3} == {c["pos"] for c in mp if c.recipe == "nan"}
    rb = [c for c in BY_OP["relu_pool_bwd"] if not c.raises]
    shapes = {(c["N"], c["H"], c["W"], c["C"]) for c in rb}
    for shp in shapes:
        modes = {c["mode"] for c in rb if (c["N"], c["H"], c["W"], c["C"]) == shp}
        assert modes == (set(LC.MODES) if min(shp[1], shp[2]) >= 2 else {"tap"}), shp
    assert shapes >= {(1, 2, 2, 8), (1, 3, 3, 8), (2, 1, 5, 16), (2, 5, 1, 16)}
    assert {c["N"] * ((c["H"] + 1) // 2) * ((c["W"] + 1) // 2) * c["C"] // 8 for c in rb} >= {WG - 1, WG, WG + 1}
    assert {c.recipe for c in rb} == {"normal", "tie", "zero", "negy"}
    assert sorted((c["H"], c["W"]) for c in BY_OP["relu_pool_bwd"] if c.raises) == [(1, 5), (5, 1)]
    # --- the head: PB = 256 / (C / 8) pixels per block; the pixel loops; the final kernel's second block
    hd = [c for c in BY_OP["head"] if not c.raises]
    for C in LC.HEAD_C:
        pb = WG // (C // VEC)
        assert S("head", "HW", C=C) >= {1, pb - 1, pb, pb + 1}, C
    blocks = lambda c: (c["HW"] + WG // (c["C"] // VEC) - 1) // (WG // (c["C"] // VEC))
    fwd = sorted((c["C"], blocks(c) / HEAD_FWD_BLOCKS) for c in hd if blocks(c) > HEAD_FWD_BLOCKS)
    assert any(C == 512 and r > 1 for C, r in fwd) and any(C == 64 and r > 2 for C, r in fwd)
    c512 = [c for c in hd if (c["C"], c["HW"]) == (512, 1025)][0]
    assert blocks(c512) == HEAD_FWD_BLOCKS + 1                                  # one extra trip, for block 0 only
    c64 = [c for c in hd if (c["C"], c["HW"]) == (64, 16417)][0]
    assert 2 * HEAD_FWD_BLOCKS < blocks(c64) < 3 * HEAD_FWD_BLOCKS and c64["HW"] % 32  # two trips, a third for some, a ragged tail
    bwd = {c["C"] for c in hd if blocks(c) > HEAD_BWD_BLOCKS}
    assert bwd == {64, 512} and all(blocks(c) <= HEAD_BWD_BLOCKS + 1 for c in hd)
    assert S("head", "N") >= {1, 3, HEAD_FINAL_WG, HEAD_FINAL_WG + 1}
    assert {c.recipe for c in hd} == {"normal", "zero0", "zero01", "tiny", "same", "big"}
    assert sorted(c["C"] for c in BY_OP["head"] if c.raises) == [192, 1024]
    for c in hd:  # the cotangent holds a negative entry (N >= 3) and a zero (N >= 64)
        g = LR.inputs(c, c.dtypes[0])["gout"]
        assert (c["N"] < 3 or bool((g < 0).any())) and (c["N"] < 64 or bool((g == 0).any()))
    # --- the 3-D pool
    p3 = BY_OP["pool3d"]
    assert {(c["T"], c["H"], c["W"]) for c in p3 if c["C"] == 8 and c["B"] == 2} == {(T, H, W) for T in (1, 2, 3, 4, 5) for H, W in ((2, 2), (3, 2), (2, 3), (3, 3))}
    assert 40 in S("pool3d", "C")
    og = {c["B"] * ((c["T"] + 1) // 2) * (c["H"] // 2) * (c["W"] // 2) * c["C"] // VEC for c in p3}
    ig = {c["B"] * c["T"] * c["H"] * c["W"] * c["C"] // VEC for c in p3}
    assert og >= {WG - 1, WG, WG + 1} and ig >= {WG - 1, WG, 2 * WG + 2}
    # --- gn_leaky_apply, leaky_bwd
    la = BY_OP["leaky_apply"]
    assert all(c["rows"] >= 2 and (c["per_row"] * c["C"] // VEC) % WG for c in la)
    assert {(c["affine"], c["slope"]) for c in la} == {(a, s) for a in (0, 1) for s in (0.2, 0.01)}
    assert {c.recipe for c in la} == {"normal", "inf", "nan"}
    assert S("leaky_bwd", "n") == {1, 7, 8, 9, 2047, 2048, 2049, 2055} and S("leaky_bwd", "slope") == {0.2, 0.01}
    assert {n % VEC for n in S("leaky_bwd", "n")} >= {0, 1, 7} and max(S("leaky_bwd", "n")) > WG * VEC
    # --- the statistics forms
    sl = [c for c in BY_OP["stats_leaky"] if not c.raises]
    assert {(c["C"], c["G"]) for c in sl} == set(LC.STATS_CG)
    assert {sub_for(C // G) for C, G in LC.STATS_CG} == {2, 4, 8}
    assert sub_for(192 // 32) == 2 and 192 // 32 == 6 and 192 // 8 == 24 and 512 // 32 == 16           # 6-, 24- and 16-channel groups
    assert WG // (8 // VEC) == 256 and WG // (2048 // VEC) == 1 and 2048 == MAX_STAT_C                  # 256 pixel lanes, and one
    for C, G in LC.STATS_CG:
        ppp = WG // (C // VEC)
        per = {c["per_row"] for c in sl if (c["C"], c["G"]) == (C, G) and c["rows"] == 2}
        assert per == {1, max(ppp - 1, 1), ppp, ppp + 1, RUN_TRIPS * ppp, RUN_TRIPS * ppp + 1, 3 * RUN_TRIPS * ppp + 5}, (C, G)
        assert {slabs_expected(2, p, C) for p in per} == {1, 2, 4}                                     # one slab, the step to two, three + ragged
        assert any(p < ppp for p in per) or ppp == 1                                                    # per_row below the pixel lanes
    empty = [c for c in sl if c["rows"] == 108]
    assert len(empty) == 1 and slabs_expected(108, empty[0]["per_row"], 2048) == 18 and 17 * 17 >= empty[0]["per_row"] == 289
    capped = {c["rows"]: slabs_expected(c["rows"], c["per_row"], c["C"]) for c in sl if c["rows"] >= 1024}
    assert capped == {1024: 2, 1025: 1} and all((c["per_row"] + RUN_TRIPS * 256 - 1) // (RUN_TRIPS * 256) == 3 for c in sl if c["rows"] >= 1024)
    assert sorted((c["C"], c["G"]) for c in BY_OP["stats_leaky"] if c.raises) == [(24, 8), (2048, 257), (2056, 8)]
    assert (24 // 8) % 2 == 1 and 2056 > MAX_STAT_C and 257 > WG
    sp = BY_OP["stats_pool"]
    assert {(c["C"], c["G"]) for c in sp} == set(LC.STATS_CG) and {c["T"] % 2 for c in sp} == {0, 1}
    crosses = 0
    for c in sp:   # a slab whose run crosses a frame boundary: several slabs whose length does not divide a frame's pixels
        rows, per_row = LR.stats_rows(c)
        n = slabs_expected(rows, per_row, c["C"])
        per = (per_row + n - 1) // n
        crosses += n > 1 and c["T"] > 2 and (c["Ho"] * c["Wo"]) % per != 0
    assert crosses >= len(LC.STATS_CG)
    # --- the small-Cin input gradient
    dg = [c for c in BY_OP["dgrad"] if not c.raises]
    assert {(c["T"], c["H"], c["W"]) for c in dg if c["B"] == 2 and c["Cout"] == 8} == {(t, h, w) for t in (1, 2, 3) for h in (1, 2, 3) for w in (1, 2, 3)}
    chunks = {c["W"]: (((c["W"] + 1) // 2) + 63) // 64 for c in dg if c["W"] > 100}
    assert chunks == {127: 1, 128: 1, 129: 2}
    assert {c["Cin"] for c in dg if c["Cout"] == 16 and not c.get("ps")} == {1, 3, 4, 5, 8}
    lds = lambda c: 27 * c["Cout"] * (4 if c["Cin"] <= 4 else 8) * 4
    assert sorted(lds(c) for c in dg if c["Cout"] > 64) == [62208, 62208] and max(lds(c) for c in dg) <= DG_MAX_LDS
    assert sorted(lds(c) for c in BY_OP["dgrad"] if c.raises) == [65664, 69120] and min(lds(c) for c in BY_OP["dgrad"] if c.raises) > DG_MAX_LDS
    assert any(c.get("ps", 0) > c["Cout"] for c in dg)
    # --- the capped grids: above the cap, no multiple of 256, each half at or below the cap
    kernels = set()
    for c in BY_OP["split"]:
        cap = {LC.DISC_CAP: MAX_BLOCKS * WG, LC.LPIPS_CAP: LPIPS_MAX_BLOCKS * 256}[c["cap"]]
        assert cap == c["cap"]
        items = LC.split_items(c)
        assert items > cap and items % 256 and c["shape"][0] == 2 and items // 2 <= cap and items % 2 == 0, (c.name, items)
        kernels.add((c["kernel"], cap))
    assert kernels == {(k, MAX_BLOCKS * WG) for k in ("avgpool3d_down", "avgpool3d_down_bwd", "gn_leaky_apply", "leaky_bwd")} | \
        {(k, LPIPS_MAX_BLOCKS * 256) for k in ("relu", "maxpool2x2", "relu_pool_bwd")}


def test_slab_counts_against_the_library():
    """(c): cvvae_pass_gn_slabs itself on every statistics case (host code: the library loads without a GPU)"""
    f = _lib().cvvae_pass_gn_slabs
    for c in BY_OP["stats_leaky"] + BY_OP["stats_pool"]:
        rows, per_row = LR.stats_rows(c)
        got = int(f(rows, per_row, c["C"], c["G"]))
        if c.raises:
            assert got < 0, (c.name, got)
        else:
            assert got == slabs_expected(rows, per_row, c["C"]), (c.name, got)
    # the empty last slab: slab 17 of 18 starts at 17 * 17 = 289 >= per_row
    c = [c for c in BY_OP["stats_leaky"] if c.name.endswith("emptyslab")][0]
    slabs = int(f(c["rows"], c["per_row"], c["C"], c["G"]))
    per = (c["per_row"] + slabs - 1) // slabs
    assert (c["rows"], c["per_row"], c["C"], c["G"], c.dtypes, c["affine"]) == (108, 289, 2048, 32, (PC.BF16,), 0)
    assert slabs == 18 == MAX_BLOCKS // 108 and per == 17 and (slabs - 1) * per >= c["per_row"]


def _pair_err(mine, theirs):
    a, b = torch.nan_to_num(LR.canon(mine.double()), nan=12345.0, posinf=1e300, neginf=-1e300), \
        torch.nan_to_num(LR.canon(theirs.double()), nan=12345.0, posinf=1e300, neginf=-1e300)
    return (a - b).abs().max().item(), max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_reference_agrees_with_torch_fp64(case):
    """(a)"""
    for dt in case.dtypes:
        for name, mine, theirs in LR.torch_pairs(case, dt):
            err, mag = _pair_err(mine, theirs)
            assert err <= 1e-12 * mag, (case.name, dt, name, err)


def _checks_and_emulation(case, dt):
    emu = LR.emulate(case, dt)
    if case.op in LR.STATS_OPS:   # the tables of the tensor the emulation stores
        y = emu["y"].to(PR.DTYPE[dt])
        return LR.stats_reference(case, y), LR.stats_emulate(case, y), None
    return LR.reference(case, dt), emu, LR.round_emu(case, dt, emu)


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_fp32_evaluation_sits_inside_the_bound(case):
    """(b), and (d)"""
    for dt in case.dtypes:
        checks, emu, rounded = _checks_and_emulation(case, dt)
        for name, chk in checks.items():
            if chk.bound is not None:
                fin = torch.isfinite(chk.ref)
                assert torch.isfinite(chk.bound[fin]).all() and (chk.before_store()[fin] > 0).all(), (case.name, dt, name)
                small = int((chk.ref.abs() <= PR.TINY).sum())
                assert small <= 0.1 * chk.ref.numel(), (case.name, dt, name, f"{small} of {chk.ref.numel()} reference elements are below TINY")
        half = dt != PC.F32 and case.op not in LR.STATS_OPS
        w32, at32, _ = LR.worst(checks, emu, before_store=half)
        line = f"LOSSNET-EDGE-HOST {case.name} {dt}: fp32 evaluation err/bound = {w32:.4f} at {at32}"
        assert w32 <= 0.5, (case.name, dt, w32, at32)
        if rounded is not None:
            w, at, bad = LR.worst(checks, rounded)
            line += f"; rounded to {dt}: {w:.4f} at {at}"
            assert w <= (0.5 if dt == PC.F32 else 1.0) and bad == 0, (case.name, dt, w, at)
        print(line)


def test_exact_comparison_ignores_the_sign_of_zero_and_flags_one_bit():
    z = torch.zeros(4, dtype=torch.bfloat16)
    assert LR.check_one(-z, PR.Check(z, None))[2] == 0
    nan = torch.full((4,), float("nan"), dtype=torch.float16)
    assert LR.check_one(-nan, PR.Check(nan, None))[2] == 0
    one = torch.ones(4, dtype=torch.bfloat16)
    bad = one.clone()
    bad[2] = 1.0078125
    assert LR.check_one(bad, PR.Check(one, None))[1:] == ((2,), 1)
    # a bounded output with a non-finite reference element: that element exactly, the others under their bound
    ref = torch.tensor([1.0, float("inf"), float("nan")], dtype=torch.float64)
    chk = PR.Check(ref, torch.full((3,), 0.1, dtype=torch.float64))
    assert LR.check_one(torch.tensor([1.05, float("inf"), float("nan")]), chk)[2] == 0
    assert LR.check_one(torch.tensor([1.05, 3.0e38, float("nan")]), chk)[2] == 1
    assert LR.check_one(torch.tensor([1.05, float("inf"), 0.0]), chk)[2] == 1
    assert LR.check_one(torch.tensor([float("nan"), float("inf"), float("nan")]), chk)[2] == 1


def test_nan_recipes_hold_a_nan_in_every_window_position():
    for c in BY_OP["maxpool"]:
        if c.recipe == "nan":
            x = LR.inputs(c, PC.BF16)["x"]
            y0, x0 = 0 + (c["pos"] >> 1), 0 + (c["pos"] & 1)
            assert bool(torch.isnan(x[0, y0, x0, :4]).all()) and not bool(torch.isnan(x[0, y0, x0, 4:]).any())
            ref = LR.reference(c, PC.BF16)["y"].ref
            assert bool(torch.isnan(ref[0, 0, 0, :4]).all()) and bool(torch.isnan(ref[0, 1, 1]).all()) and bool(torch.isnan(ref[0, 1, 0]).all())
            assert not bool(torch.isnan(ref[0, 0, 1]).any())
    c = [c for c in BY_OP["relu"] if c.recipe == "nan"][0]
    assert int(torch.isnan(LR.reference(c, PC.F16)["y"].ref).sum()) == 3


def test_tie_recipe_has_more_than_one_maximum_per_window():
    c = [c for c in BY_OP["relu_pool_bwd"] if c.recipe == "tie" and c["mode"] == "both"][0]
    y = LR.inputs(c, PC.BF16)["y"].float()
    Ho, Wo = c["H"] // 2, c["W"] // 2
    win = torch.stack([y[:, (d >> 1):2 * Ho:2, (d & 1):2 * Wo:2] for d in range(4)])
    assert float((win == win.max(0).values).sum(0).float().mean()) > 1.5
