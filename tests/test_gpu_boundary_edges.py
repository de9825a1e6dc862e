"""The passes at the networks' boundary, bit for bit at their edges (needs the MI355X): the layout moves, the row-packers, the uint8
pixel conversions, the uint8 resize, the last layer's gather and the tile blend of cvvae_amd/csrc/misc_kernels.hip, and the 2x2 sum
of cvvae_amd/csrc/bwd_kernels.hip.

Every case of tests/boundary_edge_cases.py runs on the HIP kernels in each of its dtypes, twice on the same inputs: the two results
must be bit-identical, and the first is held PER ELEMENT to the reference of tests/boundary_ref.py -- equality of the bits for the
moves, the pixel conversions, the resize and every integer-valued case of the summing ops; the format-derived bound of that module
for the gather, the blend and the 2x2 sum on other inputs.  The four moves are called through the C ABI into a buffer prefilled with
a sentinel byte and followed by a guard band: equality with the reference over the whole contract region shows an element that was
never written (it still holds the sentinel, which no reference value equals), and the guard band must come back untouched.
A line per (case, dtype) reports `exact`, `within [lo, hi]` (the gather's uint8 arm on non-integer inputs) or `worst err/bound` and
where; any mismatch or any ratio above 1 fails.
profiles/boundary_edges_parity.log holds those lines from one run (pytest -s).

tests/test_boundary_edges_host.py checks the references, bounds and input recipes themselves on the CPU."""
import pytest
import torch

import boundary_edge_cases as BC
import boundary_ref as BR
from pass_ref import DTYPE

pytestmark = pytest.mark.gpu

BY_OP = BC.by_op()


def _ids(cs):
    return [c.name for c in cs]


def _guarded(nbytes: int):
    """-> (the whole device buffer, sentinel-filled; its first nbytes, the region the contract names)"""
    buf = torch.full((nbytes + BR.GUARD_BYTES,), BR.SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[:nbytes]


def _move(case: BC.Case, dt: str, t):
    """the four moves through the C ABI, as cvvae_amd.ops calls them -> {"out", "guard"}"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    lib = L.load()
    s, d = BR.src_dst(dt)
    sd, dd = DTYPE[s], DTYPE[d]
    x = t["x"].cuda()
    p = dict(case.p)
    es = torch.empty((), dtype=dd).element_size()
    if case.op == "n2c":
        n = p["B"] * p["T"] * p["H"] * p["W"] * p["Cpad"]
        buf, out = _guarded(n * es)
        L.check(lib.cvvae_ncdhw_to_ndhwc(ops._DT[sd], ops._dt(dd), x.data_ptr(), p["B"], p["C"], p["T"], p["H"], p["W"], p["Cpad"],
                                         out.data_ptr(), ops._stream(x)), "cvvae_ncdhw_to_ndhwc")
        shape = (p["B"], p["T"], p["H"], p["W"], p["Cpad"])
    elif case.op == "c2n":
        n = p["B"] * p["c"] * p["T"] * p["H"] * p["W"]
        buf, out = _guarded(n * es)
        L.check(lib.cvvae_ndhwc_to_ncdhw(ops._dt(dd), x.data_ptr(), p["B"], p["c"], p["T"], p["H"], p["W"], p["Cs"], out.data_ptr(),
                                         ops._stream(x)), "cvvae_ndhwc_to_ncdhw")
        shape = (p["B"], p["c"], p["T"], p["H"], p["W"])
    else:
        n = p["B"] * p["T"] * p["H"] * (p["W"] + 3) * 4 + BR.READ_AHEAD
        buf, out = _guarded(n * es)
        if case.op == "rowpack_n":
            L.check(lib.cvvae_ncdhw_to_rowpack(ops._DT[sd], ops._dt(dd), x.data_ptr(), p["B"], p["C"], p["T"], p["H"], p["W"], p["pad"],
                                               out.data_ptr(), ops._stream(x)), "cvvae_ncdhw_to_rowpack")
        else:
            L.check(lib.cvvae_ndhwc_to_rowpack(ops._dt(dd), x.data_ptr(), p["B"], p["C"], p["T"], p["H"], p["W"], p["Cs"], p["pad"],
                                               out.data_ptr(), ops._stream(x)), "cvvae_ndhwc_to_rowpack")
        shape = (n,)
    torch.cuda.synchronize()
    host = buf.cpu()
    return {"out": host[:n * es].view(dd).reshape(shape), "guard": host[n * es:]}


def _run(case: BC.Case, dt: str, t):
    """one call of the op under test -> its named outputs as CPU tensors"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    op = case.op
    if op in BR.MOVES:
        return _move(case, dt, t)
    if op == "u8_in":
        got = {"out": ops.frames_u8_to_ndhwc(t["frames"].cuda(), case["Cpad"], DTYPE[dt])}
    elif op == "u8_out":
        got = {"out": ops.ncdhw_to_frames_u8(t["x"].cuda())}
    elif op == "resize":
        got = {"out": ops.resize_frames_u8(t["frames"].cuda(), (case["oh"], case["ow"]))}
    elif op == "resize_axis":  # the C ABI with inner = 1
        lib = L.load()
        f = t["frames"].cuda()
        xmin, xsize, wi, ksize, prec = ops.resize_tables(case["n_in"], case["n_out"])
        tabs = [torch.tensor(v, dtype=torch.int32, device="cuda").contiguous() for v in (xmin, xsize, wi)]
        out = torch.empty((case["outer"], case["n_out"]), dtype=torch.uint8, device="cuda")
        L.check(lib.cvvae_resize_u8_axis(f.data_ptr(), out.data_ptr(), case["outer"], case["n_in"], case["n_out"], 1, tabs[0].data_ptr(),
                                         tabs[1].data_ptr(), tabs[2].data_ptr(), ksize, prec, ops._stream(f)), "cvvae_resize_u8_axis")
        got = {"out": out}
    elif op == "gather":
        got = {"out": ops.conv_out_gather(t["V"].cuda(), 3, t["bias"].cuda(), case["pad"], DTYPE[dt], u8=bool(case["u8"]))}
    elif op == "blend":
        a, b = t["a"].cuda(), t["b"].cuda()
        ops.blend_(a, b, case["o"], case["axis"])
        torch.cuda.synchronize()
        return BR.blend_post(case, a.cpu(), b.cpu())
    elif op == "upsum":
        if case.recipe == "tiled_ints":
            g = BR.tiled_ints(case["N"], 2 * case["H"], 2 * case["W"], case["C"], DTYPE[dt], device="cuda")
        else:
            g = t["g"].cuda()
        got = {"out": ops.upsample2x_sum(g)}
    else:
        raise AssertionError(op)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}


def _check(case: BC.Case):
    failures = []
    for dt in case.dtypes:
        t = BR.inputs(case, dt)
        if case.raises:
            with pytest.raises(NotImplementedError):
                _run(case, dt, t)
            print(f"BOUNDARY-EDGE {case.name} {dt}: raises (unsupported dtype)")
            continue
        got, again = _run(case, dt, t), _run(case, dt, t)
        same = all(torch.equal(BR.bits(got[k]), BR.bits(again[k])) for k in got)
        w, where, bad = BR.worst(case, dt, got)
        guard = got.get("guard")
        touched = guard is not None and bool((guard != BR.SENTINEL).any())
        if w == 0.0 and BR.exact(case, dt):
            verdict = "exact"
        elif w == 0.0 and BR.open_intervals(case, dt)[1]:  # the gather's uint8 arm on non-integer inputs (boundary_ref.py says why)
            verdict = "within [lo, hi] (lo < hi at %d of %d elements)" % BR.open_intervals(case, dt)
        else:
            verdict = f"worst err/bound = {w:.4f} at {where}"
        print(f"BOUNDARY-EDGE {case.name} {dt}: {verdict}{'' if same else '  NOT REPRODUCIBLE'}{'  GUARD BAND WRITTEN' if touched else ''}")
        if not same:
            failures.append(f"{dt}: two runs on the same inputs differ")
        if touched:
            failures.append(f"{dt}: byte {int(torch.nonzero(guard != BR.SENTINEL)[0])} behind the output was written")
        if not w <= 1.0:
            failures.append(f"{dt}: worst err/bound = {w:.4f} at {where} ({bad} bad elements)")
    assert not failures, f"{case.name}: " + "; ".join(failures)


@pytest.mark.parametrize("case", BY_OP["n2c"], ids=_ids(BY_OP["n2c"]))
def test_ncdhw_to_ndhwc(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["c2n"], ids=_ids(BY_OP["c2n"]))
def test_ndhwc_to_ncdhw(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["rowpack_n"], ids=_ids(BY_OP["rowpack_n"]))
def test_ncdhw_to_rowpack(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["rowpack_c"], ids=_ids(BY_OP["rowpack_c"]))
def test_ndhwc_to_rowpack(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["u8_in"], ids=_ids(BY_OP["u8_in"]))
def test_frames_u8_to_ndhwc(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["u8_out"], ids=_ids(BY_OP["u8_out"]))
def test_ncdhw_to_frames_u8(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["resize"] + BY_OP["resize_axis"], ids=_ids(BY_OP["resize"] + BY_OP["resize_axis"]))
def test_resize_u8(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["gather"], ids=_ids(BY_OP["gather"]))
def test_conv_out_gather(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["blend"], ids=_ids(BY_OP["blend"]))
def test_blend(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["upsum"], ids=_ids(BY_OP["upsum"]))
def test_upsample2x_sum(case):
    _check(case)
