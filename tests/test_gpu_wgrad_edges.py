"""The weight-gradient kernels, the per-channel sums and the padding adjoint against fp64 at their edges (needs the MI355X).

Every case of tests/wgrad_edge_cases.py runs on the HIP kernels in each of its dtypes, twice on the same inputs: the two results
must be bit-identical, and the first is compared PER ELEMENT with the fp64 reference of tests/wgrad_ref.py (computed from the
dtype-rounded operands) under that element's own bound.  A line per (case, dtype) reports `worst err/bound` and where; any ratio
above 1 fails.  Cases eligible for the scalar-base wave-loads also run with CVVAE_WGRAD_FAST=1 and =0, each against fp64 and the
two bit for bit.  The 16-bit kH = 3 register-staged kernel (CVVAE_WGRAD_DMA=0, read once per process) runs in one child process.
profiles/wgrad_edges_parity.log holds the lines of one run (pytest -s).

tests/test_wgrad_edges_host.py checks the cases' plans, the references and the bounds themselves on the CPU."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import wgrad_edge_cases as WC  # noqa: E402
import wgrad_ref as WR  # noqa: E402
from conv_instance_cases import XP_ULP  # noqa: E402

pytestmark = pytest.mark.gpu

CONV = WC.conv_cases()
CHAN = WC.chan_cases()
FOLD = WC.fold_cases()
FAST = [c for c in CONV if c.fast]


def _ids(cs):
    return [c.name for c in cs]


def _log(line):
    print(line, flush=True)


def _same(a, b):
    return all(torch.equal(WR._bits(x), WR._bits(y)) for x, y in zip(a, b))


def _conv(case: WC.Conv, dt: str):
    from cvvae_amd import ops
    t = WR.conv_inputs(case, dt)
    dw, db = ops.conv_wgrad(t["a"].cuda(), t["gy"].cuda(), case.k, stride=case.stride, pad=case.pad, pad_mode_t=case.mode_t,
                            pad_mode_hw=case.mode_hw, cin=case.cin, cout=case.cout, bias=True)
    torch.cuda.synchronize()
    assert tuple(dw.shape) == (case.cout, case.cin) + case.k and dw.dtype == torch.float32 and tuple(db.shape) == (case.cout,)
    return dw.cpu(), db.cpu()


def _conv_line(case, dt, tag, raw, same=True):
    """log one (case, dtype) line; -> the failures it shows"""
    w, where, bad = WR.conv_worst(case, dt, raw)
    note = ""
    if dt == WC.F32:  # (the figure under the forward convs' split-precision term, for the record: see wgrad_ref's docstring)
        note = f"  [with XP_ULP = 4e-6 in place of 3 * 2^-16: {WR.conv_worst(case, dt, raw, xp=XP_ULP)[0]:.4f}]"
    _log(f"WGRAD-EDGE {case.name}{tag} {dt}: worst err/bound = {w:.4f} at {where}{note}{'' if same else '  NOT REPRODUCIBLE'}")
    out = [] if same else [f"{dt}{tag}: two runs on the same inputs differ"]
    if not w <= 1.0:
        out.append(f"{dt}{tag}: worst err/bound = {w:.4f} at {where} ({bad} elements beyond their bound)")
    return out


@pytest.mark.parametrize("case", CONV, ids=_ids(CONV))
def test_conv_wgrad(case):
    failures = []
    for dt in case.dtypes:
        raw, again = _conv(case, dt), _conv(case, dt)
        failures += _conv_line(case, dt, "", raw, _same(raw, again))
    assert not failures, f"{case.name} ({case.edge}): " + "; ".join(failures)


@pytest.mark.parametrize("case", FAST, ids=_ids(FAST))
def test_scalar_base_and_per_lane_wave_loads(case, monkeypatch):
    """both address forms of wgrad_dma_kernel's wave-loads against fp64, and against each other bit for bit"""
    failures = []
    for dt in case.dtypes:
        monkeypatch.setenv("CVVAE_WGRAD_FAST", "1")
        fast = _conv(case, dt)
        monkeypatch.setenv("CVVAE_WGRAD_FAST", "0")
        lane = _conv(case, dt)
        monkeypatch.delenv("CVVAE_WGRAD_FAST")
        failures += _conv_line(case, dt, "[FAST=1]", fast) + _conv_line(case, dt, "[FAST=0]", lane)
        if not _same(fast, lane):
            failures.append(f"{dt}: the scalar-base and the per-lane form differ")
    assert not failures, f"{case.name}: " + "; ".join(failures)


def _simple(case, inputs, call, worst):
    from cvvae_amd import ops
    failures = []
    for dt in case.dtypes:
        t = {k: v.cuda() for k, v in inputs(case, dt).items()}
        raw, again = [tuple(r.cpu() for r in call(ops, case, t)) for _ in range(2)]
        same = _same(raw, again)
        w, where, bad = worst(case, dt, raw)
        _log(f"WGRAD-EDGE {case.name} {dt}: worst err/bound = {w:.4f} at {where}{'' if same else '  NOT REPRODUCIBLE'}")
        if not same:
            failures.append(f"{dt}: two runs on the same inputs differ")
        if not w <= 1.0:
            failures.append(f"{dt}: worst err/bound = {w:.4f} at {where} ({bad} elements beyond their bound)")
    assert not failures, f"{case.name}: " + "; ".join(failures)


@pytest.mark.parametrize("case", CHAN, ids=_ids(CHAN))
def test_channel_sums(case):
    _simple(case, WR.chan_inputs, WR.chan_call, WR.chan_worst)


@pytest.mark.parametrize("case", FOLD, ids=_ids(FOLD))
def test_pad_fold(case):
    _simple(case, WR.fold_inputs, WR.fold_call, WR.fold_worst)


# ------------------------------------------------------------------------------------------------------------ CVVAE_WGRAD_DMA=0
def _child() -> int:
    """the four REG16_K3_CHILD cases in bf16 on the register-staged kernel; prints their lines; exit status 1 on any failure"""
    from cvvae_amd import _lib as L
    by_name = {c.name: c for c in CONV}
    failures = []
    for name in WC.REG16_K3_CHILD:
        case = by_name[name]
        if L.load().cvvae_conv_wgrad_fuses_bias(WR.conv_desc(L, case, WC.BF16)) != 0:
            failures.append(f"{name}: CVVAE_WGRAD_DMA=0 did not take the launch off the DMA kernel")
            continue
        raw, again = _conv(case, WC.BF16), _conv(case, WC.BF16)
        failures += _conv_line(case, WC.BF16, "[DMA=0]", raw, _same(raw, again))
    for f in failures:
        print("FAIL " + f)
    return 1 if failures else 0


def test_register_staged_16bit_3x3_kernel_in_a_child_process():
    env = dict(os.environ, CVVAE_WGRAD_DMA="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ratios = re.findall(r"^WGRAD-EDGE (\S+)\[DMA=0\] bf16: worst err/bound = (\S+) at", r.stdout, flags=re.M)
    assert [n for n, _ in ratios] == list(WC.REG16_K3_CHILD), ratios
    assert all(float(v) <= 1.0 for _, v in ratios) and "NOT REPRODUCIBLE" not in r.stdout, ratios


if __name__ == "__main__":
    assert sys.argv[1:] == ["--child"]
    sys.exit(_child())
