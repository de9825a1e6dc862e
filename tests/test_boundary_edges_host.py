"""CPU checks of the network-boundary edge tests' own parts (tests/boundary_ref.py, tests/boundary_edge_cases.py): no GPU, no library.

  (a) every reference agrees with a second, independent statement of the op: tests/emu_ops.py, the kernels' op-by-op fp32 reading of
      the uint8 chains, plain integer arithmetic with ops.resize_tables, torch autograd of the nearest upsampling, scalar loops;
  (b) for the three summing ops that second statement is a correct fp32 evaluation (emu_ops), and it stays within the format-derived
      bound: worst err / bound <= 1 over every case, so the bound is no tighter than correct fp32 arithmetic;
  (c) the table reaches what its comments claim, by the kernels' own launch arithmetic;
  (d) every case that names an edge can tell the wrong readings of that edge from the right one."""
import math

import pytest
import torch
import torch.nn.functional as F

import boundary_edge_cases as BC
import boundary_ref as BR
from pass_edge_cases import BF16, F16, F32
from pass_ref import DTYPE

ALL_CASES = BC.all_cases()
CASES = [c for c in ALL_CASES if not c.raises]
BY_OP = BC.by_op()
GRIDCAP = [c for c in BY_OP["upsum"] if c.recipe == "tiled_ints"]


def _ids(cs):
    return [c.name for c in cs]


# ---------------------------------------------------------------------------------------------------------------------------- (c)
def test_case_table_reaches_the_edges_its_comments_name():
    assert set(BY_OP) == {"n2c", "c2n", "rowpack_n", "rowpack_c", "u8_in", "u8_out", "resize", "resize_axis", "gather", "blend", "upsum"}
    names = [c.name for c in ALL_CASES]
    assert len(set(names)) == len(names)
    # a work-item count % 256 of 255, 0 and 1 in every op whose grid is sized from one
    for op in ("n2c", "c2n", "rowpack_n", "rowpack_c", "u8_in", "u8_out", "resize_axis", "blend", "upsum"):
        rem = {BR.threads(c) % BC.BLOCK for c in BY_OP[op] if not c.raises}
        assert rem >= {255, 0, 1}, (op, sorted(rem))
        assert any(BR.threads(c) > BC.BLOCK for c in BY_OP[op]), op       # more than one block
    S = lambda op, k: {c.get(k) for c in BY_OP[op] if not c.raises}
    # the moves
    assert all(len(c.dtypes) == 9 for c in BY_OP["n2c"]) and S("n2c", "Cpad") == {8, 16, 32}
    assert any(c["C"] == c["Cpad"] for c in BY_OP["n2c"]) and any(c["C"] % 8 and c["C"] > 8 for c in BY_OP["n2c"])
    assert (1, 8) in {(c["C"], c["Cpad"]) for c in BY_OP["n2c"]}
    assert {(c["c"], c["Cs"]) for c in BY_OP["c2n"]} >= {(8, 8), (16, 16), (3, 8), (1, 8), (4, 16), (16, 32)}
    assert sum(c["B"] == 2 for c in BY_OP["c2n"]) >= 2
    for op in ("rowpack_n", "rowpack_c"):
        grid = {(c["W"], c["C"], c["pad"]) for c in BY_OP[op] if (c["B"], c["T"], c["H"]) == (2, 2, 3) and not c.raises}
        assert grid == {(W, C, p) for W in (1, 2, 5, 13, 61) for C in (1, 3, 4) for p in (0, 1)}
        assert any((c["B"], c["T"], c["H"], c["W"]) == (1, 1, 16, 13) for c in BY_OP[op])
        assert [c.dtypes for c in BY_OP[op] if c.raises] in ([BC.PAIRS32], [(F32,)])
    assert all(len(c.dtypes) == 6 for c in BY_OP["rowpack_n"] if not c.raises)
    # the pixel conversions
    assert {(c["npix"], c["Cpad"]) for c in BY_OP["u8_in"]} == {(n, cp) for n in (1, 255, 256, 257) for cp in (8, 16, 32)}
    for c in BY_OP["u8_in"]:
        f = BR.inputs(c, F32)["frames"].reshape(-1, 3)
        if c["npix"] >= 256:
            assert all(len(set(f[:, ch].tolist())) == 256 for ch in range(3)), c.name
    nbits = {dt: BR.inputs(BY_OP["u8_out"][0], dt)["x"] for dt in (F16, BF16)}
    assert len(set(BR.bits(nbits[F16]).flatten().tolist())) >= 65536 - 2046 and len(set(BR.bits(nbits[BF16]).flatten().tolist())) >= 65536 - 254
    assert not any(torch.isnan(BR.inputs(c, dt)["x"]).any() for c in BY_OP["u8_out"] for dt in c.dtypes)
    steps = BR.inputs(BY_OP["u8_out"][1], F32)["x"].flatten()
    k = (torch.arange(256, dtype=torch.float64) / 127.5 - 1.0).float()
    for probe in (k, torch.nextafter(k, torch.tensor(9.0)), torch.nextafter(k, torch.tensor(-9.0)),
                  torch.tensor([float("inf"), float("-inf"), 3e38, -3e38, 2.0 ** -149])):
        assert torch.isin(probe, steps).all()
    assert (BR.bits(steps) == BR.bits(torch.tensor([-0.0]))).any()
    # the gather: nblk, nblk // 8 and the tail of each shape
    got = {(c["B"], c["T"], c["H"], c["W"]): BR.gather_blocks(c) for c in BY_OP["gather"]}
    assert got == {(1, 1, 1, 1): (1, 0, 1), (1, 1, 8, 32): (1, 0, 1), (1, 1, 9, 33): (4, 0, 4), (2, 2, 9, 33): (16, 2, 0),
                   (1, 3, 9, 65): (18, 2, 2), (2, 5, 7, 31): (10, 1, 2), (1, 1, 17, 97): (12, 1, 4)}
    assert len(BY_OP["gather"]) == 7 * 12 + 5 * 12
    assert {(c["pad"], c["ldv"], c.recipe) for c in BY_OP["gather"]} == {(p, l, r) for p in (0, 1) for l in (28, 32, 40) for r in ("normal", "ints")}
    assert all(c["B"] == 1 for c in BY_OP["gather"] if c["u8"]) and sum(c["u8"] for c in BY_OP["gather"]) == 5 * 12
    for c in BY_OP["gather"]:
        assert torch.isnan(BR.inputs(c, F32)["V"][..., 27:]).all()
    # the blend: o = 1, o = the whole tile, unequal tiles, on both axes
    for ax, (full_a, full_b, other_a, other_b) in ((0, ("Ha", "Hb", "Wa", "Wb")), (1, ("Wa", "Wb", "Ha", "Hb"))):
        cs = [c for c in BY_OP["blend"] if c["axis"] == ax]
        assert any(c["o"] == 1 for c in cs) and any(c["o"] == c[full_a] == c[full_b] for c in cs)
        assert any(c[full_a] != c[full_b] and c["o"] < min(c[full_a], c[full_b]) for c in cs)
        assert all(c[other_a] == c[other_b] for c in cs)
    assert any(c["Wb"] == 13 and c["axis"] == 0 for c in BY_OP["blend"]) and any(c["Hb"] % 2 and c["axis"] == 1 for c in BY_OP["blend"])
    # the 2x2 sum: only the grid-cap case runs the grid-stride loop, by 2048 vectors
    over = [c for c in BY_OP["upsum"] if BR.threads(c) > BC.GRID_CAP * BC.BLOCK]
    assert over == GRIDCAP and BR.threads(GRIDCAP[0]) - BC.GRID_CAP * BC.BLOCK == 2048 and GRIDCAP[0].dtypes == (BF16,)
    assert {c["C"] // 8 for c in BY_OP["upsum"]} >= {1, 3, 65}


def test_resize_cases_reach_their_filter_supports():
    from cvvae_amd import ops
    tab = lambda n_in, n_out: ops.resize_tables(n_in, n_out)
    shapes = {(c["T"], c["H"], c["W"], c["oh"], c["ow"]) for c in BY_OP["resize"]}
    assert shapes == {(1, 1, 1, 5, 7), (2, 5, 7, 1, 7), (2, 5, 7, 5, 1), (2, 2, 3, 7, 11), (1, 64, 64, 63, 65), (1, 300, 5, 7, 5),
                      (3, 17, 31, 40, 33), (2, 7, 9, 7, 20)}
    assert (1, 1) not in {(oh, ow) for _, _, _, oh, ow in shapes}          # torch's CPU kernel asserts there: no yardstick
    assert {c.recipe for c in BY_OP["resize"]} == {"bytes", "binary"}
    for n_in, n_out, ks, xs_max in ((1, 5, 3, 1), (1, 7, 3, 1),            # from one pixel: one tap of three
                                    (5, 1, 11, 5), (7, 1, 15, 7),          # to one pixel: the whole axis, below ksize
                                    (2, 7, 3, 2), (3, 11, 3, 2),           # upscale: two taps
                                    (64, 63, 5, None), (64, 65, 3, None),
                                    (300, 7, 87, None)):                   # ceil(300 / 7) = 43 pixels of support on each side
        xmin, xsize, wi, ksize, prec = tab(n_in, n_out)
        assert ksize == ks == int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1 and max(xsize) == (xs_max or max(xsize)), (n_in, n_out, ksize, max(xsize))
        assert min(xsize) < ksize and all(a + b <= n_in for a, b in zip(xmin, xsize)) and 1 <= prec <= 22
    assert max(tab(300, 7)[1]) >= 85                                       # 2 * 300 / 7 = 85.7 input pixels under one filter
    for c in BY_OP["resize_axis"]:
        xmin, xsize, _, ksize, _ = tab(c["n_in"], c["n_out"])
        assert min(xsize) < ksize and all(a + b <= c["n_in"] for a, b in zip(xmin, xsize))
    for c in BY_OP["resize"]:
        if c.recipe == "binary":
            assert set(BR.inputs(c, BC.U8)["frames"].flatten().tolist()) <= {0, 255}


def test_rounding_recipe_holds_ties_overflow_and_subnormals():
    pool = BR.rounding_pool()
    h, b = pool.to(torch.float16).float(), pool.to(torch.bfloat16).float()
    assert torch.isinf(h).any() and torch.isinf(b).any() and not torch.isinf(pool).any()          # beyond both maxima
    tie16 = pool[(pool.abs() > 1) & (pool.abs() < 2) & (pool.double() * 2 ** 11 % 2 == 1)]         # odd multiples of 2^-11 in (1, 2)
    tie_b = pool[(pool.abs() > 1) & (pool.abs() < 2) & (pool.double() * 2 ** 8 % 2 == 1)]
    assert tie16.numel() >= 4 and tie_b.numel() >= 4
    for ties, dt in ((tie16, torch.float16), (tie_b, torch.bfloat16)):
        r = ties.to(dt).float()
        assert ((r - ties) > 0).any() and ((r - ties) < 0).any()                                   # ties to even go both ways
    sub = pool[(pool.abs() < 2.0 ** -14) & (pool != 0)]
    assert (sub.to(torch.float16) != 0).any() and (sub.to(torch.float16) == 0).any()              # fp16 subnormals, and below them
    assert (BR.bits(pool) == BR.bits(torch.tensor([-0.0]))).any() and (BR.bits(pool) == 0).any()
    for c in BY_OP["n2c"]:
        for dt in c.dtypes:
            s, d = BR.src_dst(dt)
            x = BR.inputs(c, dt)["x"]
            assert torch.isfinite(x).all()
            if x.numel() >= 2 * pool.numel() and s == F32:
                assert torch.isin(pool, x.flatten()).all(), (c.name, dt)
            if x.numel() >= 2 * pool.numel() and s == F32 and d == F16:
                out = BR.reference(c, dt)["out"].ref
                assert torch.isinf(out).any() and ((out != 0) & (out.abs() < 2.0 ** -14)).any()


# ---------------------------------------------------------------------------------------------------------------------- (a), (b)
SMALL = [c for c in CASES if c not in GRIDCAP]   # (the grid-cap case has 0.27 GB of input: test_tiled_ints_recipe checks its recipe and
#                                                    reference at a small shape instead)


@pytest.mark.parametrize("case", SMALL, ids=_ids(SMALL))
def test_reference_agrees_with_a_second_statement(case):
    for dt in case.dtypes:
        got = BR.emulate(case, dt)
        w, where, bad = BR.worst(case, dt, got)
        kind = "exact" if BR.exact(case, dt) else f"fp32 evaluation err/bound = {w:.4f} at {where}"
        print(f"BOUNDARY-EDGE-HOST {case.name} {dt}: {kind}")
        assert w <= 1.0 and bad == 0, (case.name, dt, w, where, bad)
        if case.op in BR.BANDED and not BR.exact(case, dt):
            for chk in BR.reference(case, dt).values():
                assert chk.bound is None or (torch.isfinite(chk.bound).all() and (chk.bound > 0).all())


def test_tiled_ints_recipe():
    """the grid-cap case's input formula and its integer reference, at a shape small enough for the CPU"""
    for N, H, W, C in ((2, 3, 5, 8), (1, 4, 7, 16)):
        g = BR.tiled_ints(N, 2 * H, 2 * W, C, torch.bfloat16)
        assert g.min() == -8 and g.max() == 8 and g.shape == (N, 1, 2 * H, 2 * W, C)
        sums = BR.tiled_ints_sums(N, H, W, C)
        assert torch.equal(sums.double(), g.double().reshape(N, 1, H, 2, W, 2, C).sum((3, 5)))
        assert torch.equal(sums.to(torch.bfloat16).double(), sums.double())         # exact in bf16
    # neighbouring outputs differ, so an output written from the wrong vector shows
    s = BR.tiled_ints_sums(1, 4, 7, 16)
    assert (s[:, :, :, 1:] != s[:, :, :, :-1]).float().mean() > 0.8 and (s[:, :, 1:] != s[:, :, :-1]).float().mean() > 0.8


def test_upsum_reference_is_the_adjoint_of_nearest_upsampling():
    for case in BY_OP["upsum"]:
        if case in GRIDCAP:
            continue
        g = BR.inputs(case, F32)["g"].double()                                      # [N,1,2H,2W,C]
        x = torch.zeros(case["N"], case["C"], case["H"], case["W"], dtype=torch.float64, requires_grad=True)
        F.interpolate(x, scale_factor=2, mode="nearest").backward(g[:, 0].permute(0, 3, 1, 2))
        ref = BR.reference(case, F32)["out"].ref
        assert torch.equal(x.grad.permute(0, 2, 3, 1)[:, None], ref) or (x.grad.permute(0, 2, 3, 1)[:, None] - ref).abs().max() <= 1e-15


def test_gather_reference_against_a_scalar_loop():
    for case in BY_OP["gather"]:
        if (case["H"], case["W"]) not in ((1, 1), (9, 33)) or case["u8"] or case["B"] != 1:
            continue
        t = BR.inputs(case, F32)
        V, bias, H, W = t["V"].double(), t["bias"].double(), case["H"], case["W"]
        ref = BR.reference(case, F32)["out"].ref
        for y in range(H):
            for x in range(W):
                for co in range(3):
                    acc = float(bias[co])
                    for dy in range(3):
                        for dx in range(3):
                            yy, xx = y + dy - 1, x + dx - 1
                            if case["pad"] == BC.PAD_REPLICATE:
                                yy, xx = min(max(yy, 0), H - 1), min(max(xx, 0), W - 1)
                            elif not (0 <= yy < H and 0 <= xx < W):
                                continue
                            acc += float(V[0, 0, yy, xx, (dy * 3 + dx) * 3 + co])
                    assert abs(acc - float(ref[0, co, 0, y, x])) <= 1e-12, (case.name, co, y, x)


def test_blend_and_rowpack_references_against_scalar_loops():
    case = [c for c in BY_OP["blend"] if c["o"] == 3 and c["axis"] == 1][0]
    t = BR.inputs(case, F32)
    a, b, o = t["a"].double(), t["b"].double(), 3
    ref = BR.reference(case, F32)["b_overlap"].ref
    for i in range(o):
        w = float(torch.tensor(float(i)) / torch.tensor(float(o)))
        want = (1.0 - w) * a[..., case["Wa"] - o + i] + w * b[..., i]
        assert (want - ref[..., i]).abs().max() <= 1e-15
    for case in BY_OP["rowpack_n"]:
        if case.raises or case["W"] > 2:
            continue
        x = BR.inputs(case, "f32>f16")["x"]
        out = BR.reference(case, "f32>f16")["out"].ref[:-BR.READ_AHEAD].reshape(case["B"], case["T"], case["H"], case["W"] + 3, 4)
        W, C = case["W"], case["C"]
        for xp in range(W + 3):
            for ch in range(4):
                xs = xp - 1
                zero = xp == W + 2 or ch >= C or (case["pad"] == BC.PAD_ZERO and not 0 <= xs < W)
                want = torch.zeros_like(out[..., xp, ch]) if zero else x[:, ch, :, :, min(max(xs, 0), W - 1)].to(torch.float16)
                assert torch.equal(BR.bits(out[..., xp, ch]), BR.bits(want)), (case.name, xp, ch)


def test_no_reference_element_of_a_move_equals_the_sentinel():
    """so an element the kernel never wrote (it keeps the prefilled bytes) cannot pass the comparison of the bits"""
    for case in CASES:
        if case.op in BR.MOVES:
            for dt in case.dtypes:
                raw = BR.bits(BR.reference(case, dt)["out"].ref)
                filled = int.from_bytes(bytes([BR.SENTINEL]) * raw.element_size(), "little", signed=True)
                assert not (raw == filled).any(), (case.name, dt)


# ---------------------------------------------------------------------------------------------------------------------------- (d)
def _differs(case, dt, variant):
    a, b = BR.reference(case, dt), BR.reference(case, dt, variant)
    return any(not torch.equal(a[k].ref, b[k].ref) or (a[k].hi is not None and not torch.equal(a[k].hi, b[k].hi)) for k in a)


def test_every_case_tells_the_wrong_readings_of_its_edge_apart():
    for case in BY_OP["rowpack_n"] + BY_OP["rowpack_c"]:
        if case.raises:
            continue
        for dt in case.dtypes:
            assert _differs(case, dt, "pad_swap") and _differs(case, dt, "xp_shift"), (case.name, dt)
            # ... and at the very columns: xp = 0 and xp = W + 1 of the two pad modes differ in every row
            a = BR.reference(case, dt)["out"].ref[:-BR.READ_AHEAD].reshape(-1, case["W"] + 3, 4)[..., :case["C"]]
            b = BR.reference(case, dt, "pad_swap")["out"].ref[:-BR.READ_AHEAD].reshape(-1, case["W"] + 3, 4)[..., :case["C"]]
            assert (a[:, 0] != b[:, 0]).all() and (a[:, case["W"] + 1] != b[:, case["W"] + 1]).all(), (case.name, dt)
    for case in BY_OP["gather"]:
        for dt in case.dtypes:
            assert _differs(case, dt, "pad_swap"), (case.name, dt)
    # truncating against rounding: every case of the uint8 store and of the gather's uint8 arm, the one-pixel frames included
    for case in BY_OP["u8_out"] + [c for c in BY_OP["gather"] if c["u8"]]:
        for dt in case.dtypes:
            assert _differs(case, dt, "u8_round"), (case.name, dt)
    for case in BY_OP["gather"]:
        if case["u8"] and case["H"] * case["W"] >= 8:
            for dt in case.dtypes:
                ref = BR.reference(case, dt)["out"]
                assert ((ref.ref > 0) & (ref.ref < 255)).float().mean() > 0.5, (case.name, dt)   # most pixels inside the clamp
                if case.recipe == "ints":                                                       # ... equality, on many byte values
                    assert torch.equal(ref.ref, ref.hi) and len(set(ref.ref.flatten().tolist())) > 40, (case.name, dt)


def test_compare_flags_one_bad_element_one_bad_bit_and_a_nan():
    case = [c for c in BY_OP["blend"] if c["o"] == 3 and c["axis"] == 0][0]
    chk = BR.reference(case, F16)["b_overlap"]
    good = chk.ref.to(torch.float16)
    assert BR.compare(good, chk)[2] == 0
    bad = good.clone().double()
    bad[0, 0, 0, 1, 2] = chk.ref[0, 0, 0, 1, 2] + 1.5 * chk.bound[0, 0, 0, 1, 2]
    w, idx, n = BR.compare(bad, chk)
    assert n == 1 and idx == (0, 0, 0, 1, 2) and 1.4 < w < 1.6
    bad[1, 0, 0, 0, 0] = float("nan")
    assert BR.compare(bad, chk)[0] == float("inf")
    z = torch.zeros(2, 3, dtype=torch.float16)
    assert BR.compare(z, BR.Check(z.clone())) == (0.0, (), 0)
    assert BR.compare(-z, BR.Check(z))[2] == 6                        # -0 is not the +0 a padding must hold
    n_ = torch.full((2,), float("nan"), dtype=torch.float16)
    assert BR.compare(n_, BR.Check(n_.clone()))[2] == 0 and BR.compare(z[0, :2], BR.Check(n_))[2] == 2
    lo, hi = torch.tensor([3, 3], dtype=torch.uint8), torch.tensor([3, 4], dtype=torch.uint8)
    assert BR.compare(torch.tensor([3, 4], dtype=torch.uint8), BR.Check(lo, None, hi))[2] == 0
    assert BR.compare(torch.tensor([4, 5], dtype=torch.uint8), BR.Check(lo, None, hi))[1:] == ((0,), 2)


def test_half_ulp_is_the_formats_own():
    for dt, t in ((F16, torch.float16), (BF16, torch.bfloat16)):
        for v in (1.0, 1.5, 0.75, 3.0, 1000.0, 2.0 ** -14, 2.0 ** -20 if dt == F16 else 2.0 ** -100):
            x = torch.tensor([v], dtype=t)
            up = torch.nextafter(x.float(), torch.tensor(float("inf")))   # (torch has no nextafter on 16-bit tensors: step the bits)
            nxt = (BR.bits(x) + 1).view(t)
            assert BR.half_ulp(dt, x.double()).item() == (nxt.double() - x.double()).item() / 2, (dt, v, up)
    assert BR.half_ulp(F32, torch.tensor([1.0], dtype=torch.float64)).item() == 0.0
    assert BR.half_ulp(F16, torch.tensor([0.0], dtype=torch.float64)).item() == 2.0 ** -25
    assert all(DTYPE[k] is v for k, v in ((F32, torch.float32), (F16, torch.float16), (BF16, torch.bfloat16)))
