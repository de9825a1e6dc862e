"""CPU side of the conv instance sweep (tests/conv_instance_cases.py, tests/test_gpu_conv_instances.py):
  * every (instance, dtype) the default build registers has a case, and no case names a kernel that is not built;
  * every case's descriptor, under its environment, resolves through the library's own selection to exactly the declared kernel
    (CVVAE_CONV_FORCE silently falls back to the normal choice when nothing matches);
  * the per-element checker flags the defects tiled kernels make (a dropped halo tap, the last K chunk left out, ...)."""
import re

import pytest
import torch

from tests import conv_instance_cases as CI


def test_every_built_kernel_has_a_case():
    insts = CI.instances()
    cases = CI.cases(insts)
    declared = {(n, c.dtype) for c in cases for s in c.shapes for n in s.names}
    assert declared == CI.expected_kernels(insts)
    assert len({(c.inst.name, c.dtype) for c in cases}) == len(cases)
    assert all(len(c.shapes) >= 2 for c in cases)


def test_parser_follows_the_default_build_and_fails_on_an_uncovered_row():
    text = open(CI.TABLE_H).read()
    base = CI.instances(text)
    assert not any(e.family == "NB2" for e in base)  # CVVAE_BUILD_NB2 is off by default
    assert sum(1 for e in base if e.wm * e.wn * e.kg == 4) == 1  # CVVAE_BUILD_NW4 off: only the per-frame four-wave instance
    # a row added to a copy of the table is a kernel the cases do not cover
    fake = re.sub(r"(#define CVVAE_CONV_G2\(X\) \\\n)", r"\1  X(3,3,3, 1,1,1, 1,8,64, 1,4,2, 2, 0,0) \\\n", text)
    more = CI.instances(fake)
    assert len(more) == len(base) + 1
    declared = {(n, c.dtype) for c in CI.cases(base) for s in c.shapes for n in s.names}
    assert CI.expected_kernels(more) - declared == {("conv_k333_s111_t1x8x64_w1x4x2_c32_pro0_ups0", "f16"),
                                                     ("conv_k333_s111_t1x8x64_w1x4x2_c32_pro0_ups0", "bf16")}


def test_each_case_resolves_to_its_declared_kernel(monkeypatch):
    from cvvae_amd import _lib as L
    lib = L.load()
    insts = CI.instances()
    reached = set()
    for c in CI.cases(insts):
        for k, v in c.env().items():
            monkeypatch.setenv(k, v)
        for s in c.shapes:
            d = CI.conv_desc(L, c, s, lib)
            n = lib.cvvae_conv_kernel_name(d)
            assert n is not None and n.decode() == s.names[0], (c.id, s, n)
            if s.gn_out:  # the instance can carry fused statistics for this launch
                assert lib.cvvae_conv_gn_slabs(d, s.gn_out) > 0, (c.id, s)
            reached.update((nm, c.dtype) for nm in s.names)
    # 166 (instance, dtype) kernels in the default build of this table; the number follows the parse when the table changes
    assert len(reached) == len(CI.expected_kernels(insts))


# ---------------------------------------------------------------------------------------------- the checker can fail
def _small(inst_pred, dt=CI.BF16, shape_index=0):
    insts = CI.instances()
    e = next(e for e in insts if inst_pred(e))
    c = CI.make_case(insts, e, dt)
    return c, c.shapes[shape_index]


def _stored(case, s, y):
    """the reference as the kernel would store it (rounded to the output dtype)"""
    return y.to(torch.float32 if s.out_f32 else CI.torch_dtype(case.dtype)).double()


def _flagged(case, s, t, y_def):
    ref, S = CI.reference(case, s, t)
    a, b = CI.tolerance(case, s)
    worst, _, nbad = CI.compare(_stored(case, s, y_def), ref, S, a, b)
    return nbad > 0, worst


# G1's 3x3x3 prologue-free tile with a register-staged 8 x 32 tile; shape 1: zero padding
_G = lambda e: e.family == "G" and (e.kt, e.kh, e.kw) == (3, 3, 3) and e.pro == 0 and e.ups == 0 and e.sh == 1 and e.th == 8 and e.tw == 32


def test_checker_passes_the_exact_result():
    c, s = _small(_G, shape_index=1)
    t = CI.make_tensors(c, s, 0)
    ref, _ = CI.reference(c, s, t)
    assert not _flagged(c, s, t, ref)[0]


def test_checker_flags_a_tap_dropped_at_the_halo_edge():
    c, s = _small(_G, shape_index=1)
    t = CI.make_tensors(c, s, 0)
    ref, _ = CI.reference(c, s, t)
    w = t["w"].clone()
    w[:, :, :, 2, :] = 0  # the bottom halo row's taps (the next tile's first row) ...
    y_drop, _ = CI.reference(c, s, t, defect={"w": w})
    y = ref.clone()
    r = c.inst.th - 1
    y[:, :, :, r] = y_drop[:, :, :, r]  # ... dropped for the last output row of the first tile only
    assert _flagged(c, s, t, y)[0]


def test_checker_flags_the_last_k_chunk_left_out():
    c, s = _small(_G, shape_index=1)
    t = CI.make_tensors(c, s, 0)
    ck = 16 * c.inst.ksub
    w = t["w"].clone()
    w[:, -ck:] = 0
    y, _ = CI.reference(c, s, t, defect={"w": w})
    assert _flagged(c, s, t, y)[0]


def test_checker_flags_the_partial_tiles_last_column_left_at_zero():
    c, s = _small(_G, shape_index=1)
    t = CI.make_tensors(c, s, 0)
    ref, _ = CI.reference(c, s, t)
    y = ref.clone()
    y[..., -1] = 0
    assert _flagged(c, s, t, y)[0]


def test_checker_flags_replicate_padding_at_one_zero_border():
    c, s = _small(_G, shape_index=1)
    assert s.mode_hw == 0 and s.pad[2][0] == 1
    t = CI.make_tensors(c, s, 0)
    y, _ = CI.reference(c, s, t, defect={"mode_w_left": 1})
    assert _flagged(c, s, t, y)[0]


def test_checker_flags_the_residual_added_twice_for_one_block():
    c, s = _small(lambda e: e.family == "G" and (e.kt, e.kh, e.kw) == (1, 3, 3) and e.kg == 2 and e.pro == 0)
    assert s.residual and not s.sc_cin
    t = CI.make_tensors(c, s, 0)
    ref, _ = CI.reference(c, s, t)
    y = ref.clone()
    y[:, 32:64] += t["res"].double()[:, 32:64]
    assert _flagged(c, s, t, y)[0]


def test_checker_flags_one_statistics_record_off_by_one_percent():
    c, s = _small(_G, shape_index=1)
    assert s.gn_out == 32
    t = CI.make_tensors(c, s, 0)
    ref, _ = CI.reference(c, s, t)
    y = _stored(c, s, ref)
    m_ref, r_ref = CI.group_stats(y, s.gn_out)
    assert CI.compare_stats(m_ref, r_ref, m_ref, r_ref) == 0.0
    # one record = one tile's pixels of one wave slab and a 4-channel slot: its values 1 % off
    e = c.inst
    y2 = y.clone()
    y2[0, 4:8, 0, :e.th // e.wm, :e.tw] *= 1.01
    m, r = CI.group_stats(y2, s.gn_out)
    assert CI.compare_stats(m, r, m_ref, r_ref) > 1.0
