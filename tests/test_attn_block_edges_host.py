"""The attention-block edge tests' own references, recipes, bound and defects, checked on the CPU (tests/attn_block_ref.py,
tests/attn_block_cases.py): the yardstick equals the oracle, the recipes meet their conditions, the hand-written adjoint equals
autograd, the real engine / grad / grad3d functions over tests/emu_ops.py -- an independent second draw of the rounding process -- stay
within MARGIN x noise on every case and tensor, every seeded defect is seen beyond that bound, and `emulate` is the real
composition bit for bit."""
import pytest
import torch

import attn_block_cases as AC
import attn_block_ref as AR
from attn_block_cases import ALL, BF16, F16, F32, SD3, V3S, V3ST
from conv_instance_cases import XP_ULP
from oracle import cvvae_oracle as O

CASES = AC.all_cases()
RUN = [c for c in CASES if not c.raises]
BY_NAME = AC.by_name()


def _ids(cs):
    return [c.name for c in cs]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


# ----------------------------------------------------------------------------------------------------------------- the table
def test_the_table_reaches_every_edge_with_more_than_one_frame():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names) and len(CASES) <= 64
    spatial = AC.spatial_cases()
    for N in AC.N_EDGES:   # one below, at and one above 16 / 32 / 64 / 128 / 256, the smallest counts, the ragged block
        assert any(AC.tokens(c) == N and AC.frames(c) > 1 for c in spatial), N
    for e in (16, 32, 64, 128, 256):
        assert {e - 1, e, e + 1} <= set(AC.N_EDGES)
    for N in AC.ALL_FRAMES_N:
        assert {(c["B"], c["T"]) for c in spatial if AC.tokens(c) == N} == set(AC.FRAMES), N
    for N in (n for n in AC.N_EDGES if n >= 33):
        assert any(AC.tokens(c) == N and c.recipe == "edgekey" and c["mstar"] == "block" for c in spatial), N
        assert any(AC.tokens(c) == N and c.recipe == "edgekey" and c["mstar"] == "last" for c in spatial), N
    assert {c["C"] for c in CASES} == {128, 256, 512} and {c.op for c in CASES} == set(AC.BLOCKS)
    assert {c.recipe for c in CASES} == {"flat", "sharp", "edgekey"}
    t = [c for c in AC.temporal_cases() if not c.get("fwd_only") and not c.raises]
    assert {c["T"] for c in t} == {1, 2, 5, 8} and {AC.tokens(c) for c in t} == set(AC.TEMPORAL_S)
    assert {c["T"] for c in CASES if c.get("fwd_only")} == {9, 17} and [c["T"] for c in CASES if c.raises] == [9]
    assert max(AC.tokens(c) * c["C"] * AC.frames(c) for c in CASES) == 257 * 512 * 6
    for c in CASES:   # H != W wherever N has such a factorisation
        assert c["H"] != c["W"] or AC.tokens(c) in (1, 4), c.name


# ----------------------------------------------------------------------------------------------------------------- yardstick == oracle
def _oracle(case, dt):
    d = AR.inputs(case, dt)
    B, T, H, W, C = d["x"].shape
    x = d["x"].double().permute(0, 4, 1, 2, 3)   # NCDHW
    P = {k: v.double() for k, v in d["P"].items()}
    if case.op == SD3:
        sd = {f"a.{AR.NAMES[SD3][r]}{'.0' if r == 'proj' else ''}.{s}": P[f"{r}.{s}"] for r in AR.SPATIAL for s in ("weight", "bias")}
        y = O.sd3_attention(x, sd, "a")
    else:
        sd = {}
        for r in AR.roles(case):
            leaf = AR.NAMES[case.op][r].split(".")[-1]
            for s in ("weight", "bias"):
                v = P[f"{r}.{s}"]
                sd[f"a.{leaf}.{s}"] = v.reshape(C, C, 1, 1) if s == "weight" and r in ("q", "k", "v", "proj") else v
        y = (O.v3_attn_spatial if case.op == V3S else O.v3_attn_spatial_temporal)(x, sd, "a")
    return y.permute(0, 2, 3, 4, 1)


ORACLE_CASES = [c for c in RUN if c["C"] == 128 and AC.tokens(c) <= 65] + [c for c in RUN if c["C"] != 128][:3]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=_ids(ORACLE_CASES))
def test_yardstick_equals_the_oracle(case):
    for dt in (F32, BF16):
        y = AR.yardstick(case, dt)[0]["y"]
        ref = _oracle(case, dt).reshape(y.shape)
        assert float((y - ref).norm() / ref.norm()) <= 1e-12, (case.name, dt)


@pytest.mark.parametrize("case", RUN, ids=_ids(RUN))
def test_unrounded_restatement_equals_autograd(case):
    """`rounded` with every rounding switched off is the yardstick: the hand-written backward is the adjoint of the forward"""
    ref, S, _ = AR.yardstick(case, BF16)
    got = AR.rounded(case, BF16, None)
    for k in AR.tensors(case):
        scale = float(S[k].norm()) if k in S else float(ref[k].norm())
        assert float((got[k] - ref[k]).norm()) <= 1e-10 * scale, (case.name, k)


# ----------------------------------------------------------------------------------------------------------------- recipes
@pytest.mark.parametrize("case", RUN, ids=_ids(RUN))
def test_recipes_meet_their_conditions(case):
    for dt in case.dtypes:
        t = AR.yardstick(case, dt)[2]
        N, Fr = AC.tokens(case), AC.frames(case)
        if case.recipe == "sharp":
            if N > 1:
                assert 2.0 <= float(t["s"].std(unbiased=False)) <= 8.0, (case.name, dt)
            if case.op == V3ST and case["T"] > 1:
                assert 2.0 <= float(t["s_t"].std(unbiased=False)) <= 8.0, (case.name, dt)
            assert N > 1 or (case.op == V3ST and case["T"] > 1), case.name
        if case.recipe == "edgekey":
            ms = [AR.mstar(case, f) for f in range(Fr)]
            mass = min(float(t["p"][f, :, ms[f]].min()) for f in range(Fr))
            assert mass >= AR.EDGE_MASS, (case.name, dt, mass)
            assert ms[0] == (N - 1 if case["mstar"] == "last" else 32 * ((N - 1) // 32))
            if Fr > 1 and N > 2 and not (case["mstar"] == "block" and ms[0] == N - 1):
                assert ms[1] != ms[0], case.name   # neighbouring frames differ


# ----------------------------------------------------------------------------------------------------------------- the fp32 product model
def test_split_precision_product_is_within_xp_ulp_of_fp64():
    """the fp32 model of `rounded` (fp16 hi + lo of both operands, lo x lo dropped, as conv_kernel.h stages them) against the project's
    constant: one product of 512 terms is within XP_ULP * S of fp64, and is NOT exact (the model does round)"""
    g = torch.Generator().manual_seed(5)
    a, w = torch.randn(300, 512, generator=g).double(), (torch.rand(512, 512, generator=g).double() * 2 - 1) * 512 ** -0.5
    A = AR.Arith(F32)
    got = A.mm(a, w, AR._ws(w))
    exact, S = a @ w, a.abs() @ w.abs()
    ratio = float(((got - exact).abs() / S).max())
    assert 0.0 < ratio <= XP_ULP, ratio
    # ... and the unscaled form the per-frame "weights" packed from activations take
    ratio = float(((A.mm(a, a.t()) - a @ a.t()).abs() / (a.abs() @ a.abs().t())).max())
    assert 0.0 < ratio <= XP_ULP, ratio


# ----------------------------------------------------------------------------------------------------------------- the bound
def _within(case, dt, got, keys=None):
    bad = []
    for k, m, bound, _ in AR.compare(case, dt, got, keys):
        if not m <= bound:
            bad.append(f"{dt} {k}: {m:.3e} > {bound:.3e} ({m / max(bound, 1e-300):.2f})")
    return bad


def _exact(case, got):
    return [f"{k} is not exactly zero" for k in AR.exact_zero(case) if k in got and bool((got[k] != 0).any())]


@pytest.mark.parametrize("case", RUN, ids=_ids(RUN))
def test_second_draw_stays_within_margin_times_noise(case):
    """the real engine / grad / grad3d functions over emu_ops (fp32 torch arithmetic, autograd-based adjoints) are a second draw of
    the product path's rounding process: MARGIN is held here, on the CPU, on every case, dtype and tensor"""
    bad = []
    bwd = not case.get("fwd_only")
    for dt in case.dtypes:
        got = AR.second_draw(case, dt, backward_pass=bwd, frozen=True)
        bad += _within(case, dt, got) + _exact(case, got)
        if bwd:
            assert _same(got["y"], got["y_taped"]) and (case.op == V3ST or _same(got["dx"], got["dx_frozen"]))
            p = got["p"].view(-1, got["p"].shape[-1])
            assert not bool((p[:, AC.tokens(case):] != 0).any())
        if case["C"] == 512 and dt != F32:   # the five-launch form of the same model
            with AR.fused_switch(False):
                bad += [b + " [five-launch]" for b in _within(case, dt, AR.second_draw(case, dt, backward_pass=bwd))]
    assert not bad, f"{case.name}: " + "; ".join(bad)


def test_noise_is_positive_and_of_the_formats_size():
    """the bound is not vacuous: the noise of a banded tensor is a few roundings of the format, never zero, never of order one"""
    for case in RUN:
        for dt in case.dtypes:
            nz = AR.noise(case, dt)
            u = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}[dt]
            # (fp32 models: the split-precision products stage a gradient operand below fp16's normal range, 6e-5, as a subnormal hi
            #  and a zero lo, so the q / k gradients behind a saturated softmax keep only hi's bits: up to 2^-11 -- DESIGN.md 3.5
            #  -- and the key-bias gradient, all cancellation, peaks there.  16-bit: the worst is bf16 k.weight behind a saturated softmax,
            #  2^-9 of P's rounding over 1 - p.)
            cap = 2.0 ** -10 if dt == F32 else 64 * u
            for k in AR.banded(case):
                assert 0.0 < nz[k] <= cap, (case.name, dt, k, nz[k])


# ----------------------------------------------------------------------------------------------------------------- emulate
EMU_CASES = [c for c in RUN if AC.tokens(c) * c["C"] * AC.frames(c) <= 129 * 128 * 6] + [c for c in RUN if c["C"] == 512][:2]


@pytest.mark.parametrize("case", EMU_CASES, ids=_ids(EMU_CASES))
def test_emulate_is_the_real_composition_bit_for_bit(case):
    bwd = not case.get("fwd_only")
    for dt in case.dtypes:
        with torch.no_grad():
            emu = AR.emulate(case, dt, frozen=True)
        real = AR.second_draw(case, dt, backward_pass=bwd, frozen=True)
        for k in real:
            assert _same(emu[k], real[k].reshape(emu[k].shape)), (case.name, dt, k)


# the cases each defect is looked for on (small ones that reach it: more than one frame, a temporal half, a padded row, ...)
DEFECT_CASES = ["v3s-C128-N33-b1t3-edgekey", "sd3-C128-N64-b1t3-edgekey-block", "v3st-C128-N63-b2t3-edgekey", "v3st-C128-N31-b2t3-edgekey",
                "v3st-C128-T5-S4-b2-flat", "v3st-C128-T8-S5-b1-sharp", "sd3-C128-N16-b2t1-sharp", "v3s-C128-N33-b2t3-sharp"]


def test_defect_cases_exist():
    assert all(n in BY_NAME for n in DEFECT_CASES), [n for n in DEFECT_CASES if n not in BY_NAME]


@pytest.mark.parametrize("defect", AR.DEFECTS)
def test_every_defect_is_seen(defect):
    seen = []
    for name in DEFECT_CASES:
        case = BY_NAME[name]
        for dt in ALL:
            with torch.no_grad():
                got = AR.emulate(case, dt, defect)
            if _within(case, dt, got):
                seen.append((name, dt))
    assert seen, defect
    print(f"\n[defect {defect}] seen on {len(seen)} of {3 * len(DEFECT_CASES)} (case, dtype) pairs: {seen[:4]}")
