"""CPU checks of the conv input-gradient edge tests' own parts (tests/dgrad_edge_cases.py, tests/dgrad_ref.py); the library is loaded
for its host-side kernel-name resolution only, no GPU.

  1. the table is what it claims: unique names, a literal case count, engine's own geometry triples, every geometry x stride
     combination, both parities on every strided axis, the extents' limits, `add` only where the fold sums;
  2. the composition is right and the bound honest: the REAL grad3d.dgrad333, backward.conv_dgrad, backward.dgrad1x1 and
     grad3d.sd3_upsample_backward run under emu_ops.patched() over a WeightCache, every case in every dtype, and every element stays
     within its bound; the result has the stated shape and dtype, zero pad channels, exact zeros where no window reaches; every
     conv launch resolves to a kernel instance; and dgrad_ref.emulate gives the same bits;
  3. TINY is at most 1 % of the median bound of every case;
  4. the check catches errors: each seeded defect of dgrad_ref.DEFECTS, on every case it applies to, puts at least one element
     beyond its bound -- the printed relative L2 error shows which of them a norm tolerance of 1e-1 would have passed -- and where a
     defect cannot change the result, it does not.
Run with -s for the figures."""
import contextlib

import pytest
import torch

import dgrad_edge_cases as DC
import dgrad_ref as DR
from tests import emu_ops

CASES = DC.cases()
BY_NAME = {c.name: c for c in CASES}


def _ids(cs):
    return [c.name for c in cs]


# ------------------------------------------------------------------------------------------------------------ 1. the table
def test_table_is_what_it_claims():
    from cvvae_amd import engine
    names = _ids(CASES)
    assert len(set(names)) == len(names)
    assert len(CASES) == 54
    # the triples are engine's own
    assert DC.GEO["sd3-causal"] == engine.SD3_GEO.conv(True) and DC.GEO["sd3-sym"] == engine.SD3_GEO.conv(False)
    assert DC.GEO["v3-causal"] == engine.V3_GEO.conv(True) and DC.GEO["zero"] == engine.V3_GEO.conv(False)
    assert DC.GEO["v3-down"] == engine.V3_GEO.down and DC.GEO["v3-up"] == engine.V3_GEO.up
    assert engine.SD3_GEO.down is None and engine.SD3_GEO.up is None          # (the sd3 family's own conv triples)
    assert DC.GEO["frame"] == (engine.P2D, engine.ZERO, engine.ZERO) and (DC.REP, DC.ZERO) == (engine.REP, engine.ZERO)
    from cvvae_amd import grad3d
    assert DR.FULL == grad3d.FULL
    d3 = [c for c in CASES if c.path == DC.DGRAD333]
    combos = {(c.geo, c.stride) for c in d3}
    want = {(g, DC.S1) for g in ("sd3-causal", "sd3-sym", "v3-causal", "zero")} | {(g, s) for g in DC.STRIDED_GEO for s in (DC.S222, DC.S122)}
    assert combos == want, combos ^ want
    assert {c.geo for c in CASES if c.path == DC.UPCHAIN} >= {"v3-up"} and {c.path for c in CASES} == set(DC.KERNEL)
    # both parities of every strided axis under every strided combination; under (2,2,2) an even and an odd T out of {2, 3, 5}
    for g in DC.STRIDED_GEO:
        for s in (DC.S222, DC.S122):
            cs = [c for c in d3 if (c.geo, c.stride) == (g, s)]
            for axis in (1, 2, 3):
                if s[axis - 1] == 2:
                    assert {c.dims[axis] % 2 for c in cs} == {0, 1}, (g, s, axis)
            if s == DC.S222:
                ts = {c.dims[1] for c in cs} & {2, 3, 5}
                assert {t % 2 for t in ts} == {0, 1}, (g, ts)
    assert {c.dims[1] for c in d3} >= {1, 2, 3, 5}
    assert any(c.dims[1] == 1 and c.geo == "sd3-causal" and c.stride == DC.S1 for c in d3)
    assert any(c.dims[1] == 1 and c.stride == DC.S222 for c in d3)
    # one row / one column under replicate pad 1; a row wider than the widest forward tile, at front pad 2
    assert any(c.dims[2] == 1 and c.mode_hw == DC.REP for c in d3) and any(c.dims[3] == 1 and c.mode_hw == DC.REP for c in d3)
    assert any(c.dims[3] == 70 and c.mode_hw == DC.REP for c in d3) and any(c.dims[3] == 70 and c.mode_hw == DC.ZERO for c in d3)
    for c in CASES:
        B, T, H, W = c.dims
        assert B <= 2 and T <= 5 and H <= 9 and (W <= 12 or W == 70 or c.path == DC.DGRAD1X1), c.name
        assert all(n >= 1 for n in c.out_grid), c.name
        assert not c.add or (c.path == DC.DGRAD333 and c.folds), c.name
        assert not c.residual or c.path == DC.DGRAD1X1, c.name
    # the channel pairs the networks launch
    pairs = {(c.path, c.cout, c.cin) for c in CASES}
    assert pairs >= {(DC.DGRAD333, 128, 128), (DC.DGRAD333, 256, 128), (DC.DGRAD333, 128, 256), (DC.DGRAD1X1, 512, 512),
                     (DC.DGRAD333, 128, 3), (DC.DGRAD333, 3, 128), (DC.DGRAD333, 32, 512), (DC.DGRAD333, 512, 16), (DC.UPCHAIN, 256, 128)}
    ups = [c for c in CASES if c.path == DC.UPCHAIN]
    assert {c.up_time for c in ups} == {True, False} and any(c.up_time and c.dims[1] == 1 for c in ups)
    assert all(c.g_shape[1] == 2 * c.dims[1] - 1 for c in ups if c.up_time)
    d2 = [c for c in CASES if c.path == DC.DGRAD133]
    assert any(c.cin_pad == 32 and c.g_store == 32 and c.cout == 3 for c in d2) and any(c.ncdhw for c in d2)
    assert {c.cout_pad for c in d2} >= {8, 128}
    d1 = [c for c in CASES if c.path == DC.DGRAD1X1]
    px = lambda c: c.dims[1] * c.dims[2] * c.dims[3]  # noqa: E731
    assert {px(c) for c in d1} == {1, 37, 150} and {(px(c), c.residual) for c in d1} >= {(1, True), (1, False), (37, True), (37, False), (150, True), (150, False)}
    assert {n: sum(1 for c in CASES if DR.n_stored(c) == n) > 0 for n in (0, 1, 2)} == {0: True, 1: True, 2: True}


# ------------------------------------------------------------------------------------------------------------ 2. product under emu_ops
@contextlib.contextmanager
def _patched_with_kernel_names(seen: list):
    """emu_ops.patched(), and every conv launch is first resolved to a kernel instance as ops.conv's descriptor would be"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    with emu_ops.patched():
        emu_conv = ops.conv

        def conv(x, pw, *, pad=((0, 0), (0, 0), (0, 0)), out_mode=L.OUT_NDHWC, cout_pad=None, **kw):
            assert kw.get("pad_mode_t", DC.ZERO) == DC.ZERO and kw.get("pad_mode_hw", DC.ZERO) == DC.ZERO and "stride" not in kw
            name = ops.conv_kernel_name(DR.conv_desc(x, pw, pad, out_mode, cout_pad))
            assert name, f"no kernel instance: input {tuple(x.shape)} {x.dtype}, k {pw.k}, K {pw.cin}, Cout {pw.cout}, pad {pad}"
            seen.append(name)
            return emu_conv(x, pw, pad=pad, out_mode=out_mode, cout_pad=cout_pad, **kw)
        ops.conv = conv
        yield


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_product_composition_under_emulated_ops_sits_inside_the_bound(case):
    from cvvae_amd.engine import WeightCache
    for dt in case.dtypes:
        t = DR.inputs(case, dt)
        before = {k: v.clone() for k, v in t.items()}
        seen = []
        with _patched_with_kernel_names(seen):
            got = DR.call(case, t, WeightCache(DR.holder(t["w"])))
        assert len(seen) == 1, seen
        assert all(torch.equal(DR.inputs(case, dt)[k], v) for k, v in before.items())
        dead = DR.check_result(case, dt, got)
        w, at, bad = DR.worst(case, dt, got)
        print(f"DGRAD-EDGE-HOST {case.name} {dt}: n = {DR.n_stored(case)}, {seen[0]}, emulated ops err/bound = {w:.4f} at {at}, "
              f"{dead} unreached elements")
        assert w <= 1.0 and bad == 0, (case.name, dt, w, at)
        assert torch.equal(got, DR.emulate(case, dt)), (case.name, dt, "dgrad_ref.emulate is not the product's composition")


def test_unreached_positions_exist_in_the_table():
    """causal pad (2, 0) under stride 2 with an even T: no window reaches the last frame -- the exact-zero check has something to check"""
    case = BY_NAME["s222-sd3causal-even"]
    _, S, _ = DR.reference_of(case, DC.BF16)
    assert bool((S[:, -1] == 0).all()) and bool((S[:, :-1] > 0).all())


# ------------------------------------------------------------------------------------------------------------ 3. the floor
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_tiny_is_at_most_a_hundredth_of_the_median_bound(case):
    from conv_instance_cases import TINY
    for dt in case.dtypes:
        ref, S, bound = DR.reference_of(case, dt)
        assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and bool((bound > 0).all())
        med = float(bound[S > 0].median())
        assert TINY <= 0.01 * med, (case.name, dt, med)


# ------------------------------------------------------------------------------------------------------------ 4. the check catches errors
DEFECT_PAIRS = [(d, c) for c in CASES for d in DR.DEFECTS if DR.applies(d, c)]
NOOP_PAIRS = [(d, c) for c in CASES for d in ("no_flip_w", "no_flip_t", "swap_fold_t", "swap_crop")
              if not DR.applies(d, c) and (c.path in (DC.DGRAD333, DC.UPCHAIN) or (d == "no_flip_w" and c.path == DC.DGRAD133))]


def test_every_defect_has_cases_and_no_ops():
    assert {d for d, _ in DEFECT_PAIRS} == set(DR.DEFECTS)
    assert all(sum(1 for d, _ in DEFECT_PAIRS if d == name) >= 2 for name in DR.DEFECTS)
    assert {d for d, _ in NOOP_PAIRS} == {"no_flip_w", "no_flip_t", "swap_fold_t", "swap_crop"}


@pytest.mark.parametrize("defect,case", DEFECT_PAIRS, ids=[f"{d}-{c.name}" for d, c in DEFECT_PAIRS])
def test_seeded_defect_exceeds_the_bound(defect, case):
    dt = case.dtypes[-1]               # bf16: the widest bound, the hardest for the check
    got = DR.emulate(case, dt, defect=defect)
    w, at, bad = DR.worst(case, dt, got)
    l2 = DR.rel_l2(case, dt, got)
    print(f"DGRAD-EDGE-HOST defect {defect} on {case.name} {dt}: err/bound = {w:.1f} at {at} ({bad} elements); relative L2 = {l2:.3e}"
          f"{'  (inside a 1e-1 norm tolerance)' if l2 <= 1e-1 else ''}")
    assert w > 1.0 and bad >= 1, (defect, case.name, w)


@pytest.mark.parametrize("defect,case", NOOP_PAIRS, ids=[f"{d}-{c.name}" for d, c in NOOP_PAIRS])
def test_defect_is_no_defect_where_it_cannot_act(defect, case):
    """one column (or frame): the three taps along that axis meet the same pixels; symmetric pads: front and back ARE exchanged"""
    dt = case.dtypes[-1]
    good, bad = DR.emulate(case, dt), DR.emulate(case, dt, defect=defect)
    (tf, tb), (hf, hb), (wf, wb) = case.pad
    if (defect == "swap_fold_t" and tf == tb) or (defect == "swap_crop" and (hf, wf) == (hb, wb)):
        assert torch.equal(good, bad), (defect, case.name)
    else:  # the same summands in another order: the same value up to the fp32 accumulation
        assert DR.worst(case, dt, bad)[0] <= 1.0 and (good.float() - bad.float()).abs().max() <= 2.0 ** -6 * good.float().abs().max()


def test_checker_flags_nan_and_one_bad_element():
    case = BY_NAME["s1-conv-in-sd3causal-128to3"]
    ref, _, bound = DR.reference_of(case, DC.F32)
    got = torch.zeros(case.out_shape, dtype=torch.float32)
    got[..., :3] = ref.float()
    assert DR.worst(case, DC.F32, got)[0] <= 0.01
    got[0, 2, 3, 4, 1] = float("nan")
    assert DR.worst(case, DC.F32, got)[0] == float("inf")
    got[0, 2, 3, 4, 1] = float(ref[0, 2, 3, 4, 1] + 1.5 * bound[0, 2, 3, 4, 1])
    w, at, bad = DR.worst(case, DC.F32, got)
    assert 1.4 < w < 1.6 and bad == 1 and at == (0, 2, 3, 4, 1)
