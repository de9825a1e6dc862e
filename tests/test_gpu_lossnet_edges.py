"""The LPIPS and discriminator passes against fp64 at their edges (needs the MI355X).

Every case of tests/lossnet_edge_cases.py runs on the HIP kernels of cvvae_amd/csrc/lpips_kernels.hip and disc_kernels.hip in each of
its dtypes, twice on the same inputs: the two results must be bit-identical, and the first is compared PER ELEMENT with the fp64
reference of tests/lossnet_ref.py (computed from the dtype-rounded operands) under that element's own bound, or bit for bit where the
output is a selection, an exact scaling or memory that must stay untouched.  A line per (case, dtype) reports `worst err/bound` and
where; any ratio above 1 fails.  profiles/lossnet_edges_parity.log holds those lines from one run (pytest -s).

Beyond the per-element check a case also holds, where it applies: the in-place call and the one-sided head gradients are bit-equal to
the plain call; the statistics forms store the plain entry point's bits, count every element once, give the plain pass through the C
entry with out_groups = 0 or NULL partials, and their records merge (ops.gn_finalize) to the fp64 statistics of the stored tensor
under STATS_TOL.  The capped grids are checked by split invariance: a launch above the cap (the grid-stride loop runs) must be
bit-equal to the two un-looped launches on the halves of its batch, the path the small cases hold against fp64.

tests/test_lossnet_edges_host.py checks the references, bounds and input recipes themselves on the CPU.
"""
import pytest
import torch

import lossnet_edge_cases as LC
import lossnet_ref as LR
import pass_edge_cases as PC
import pass_ref as PR

pytestmark = pytest.mark.gpu

BY_OP = LC.by_op()
EPS = PR.GN_EPS


def _ids(cs):
    return [c.name for c in cs]


def _dev(t):
    return {k: v.cuda() for k, v in t.items()}


def _same(a, b):
    return torch.equal(PR._bits(a), PR._bits(b))


def _stats_tables(case, y, part, fails):
    """y: the stored tensor (GPU), part: its GNPartials -> the (mean, rstd) tables and the record bits; counts every element once"""
    from cvvae_amd import ops
    rows, C, G = y.shape[0], y.shape[-1], case["G"]
    n = part.buf[..., 0].double().sum(-1)
    if not bool((n == y[0].numel() // G).all()):
        fails.append("the records do not count every stored element once")
    scale, shift = ops.gn_finalize(part, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), EPS)
    return PR._tables_post(case, (scale.cpu(), shift.cpu()), False)


def _run(case: PC.Case, dt: str, t):
    """one call of the op under test -> (its named outputs as CPU tensors, failures of the checks that need no reference)"""
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    d = _dev(t)
    op, tdt, fails = case.op, PR.DTYPE[dt], []
    if op == "scale_in":
        N, H, W, cpad = case["N"], case["H"], case["W"], case["cpad"]
        if case["sliced"]:  # the second half of a [1, 2N, H, W, cpad] buffer, 64 elements behind it
            half = N * H * W * cpad
            buf = torch.full((2 * half + 64,), LR.CANARY, dtype=tdt, device="cuda")
            out = buf[:2 * half].view(1, 2 * N, H, W, cpad)[0, N:]
            y = ops.lpips_scale_in(d["x"], d["shift"], d["scale"], cpad, tdt, out=out)
            assert y.data_ptr() == buf.data_ptr() + half * buf.element_size()
            got = {"y": y[..., :3], "pad": y[..., 3:], "canary": torch.cat([buf[:half], buf[2 * half:]])}
        else:
            y = ops.lpips_scale_in(d["x"], d["shift"], d["scale"], cpad, tdt)
            got = {"y": y[..., :3], "pad": y[..., 3:]}
    elif op == "scale_in_bwd":
        N = case["N"]
        big = torch.full((2 * N, case["H"], case["W"], case["ps"]), 5.0, dtype=d["g"].dtype, device="cuda")
        big[N:] = d["g"]
        got = {"gx": ops.lpips_scale_in_bwd(big[N:], d["scale"], tdt)}
    elif op == "relu":
        got = {"y": ops.relu_(d["x"].clone())}
    elif op == "maxpool":
        got = {"y": ops.maxpool2x2(d["x"])}
    elif op == "relu_pool_bwd":
        got = {"gx": ops.relu_pool_bwd(d["y"], d.get("g_tap"), d.get("g_pool"))}
    elif op == "head":
        N = case["N"]
        # the features are samples N .. 2N-1 of a [2N, HW, C] tensor, as the network's are
        f0 = torch.cat([d["f1"], d["f0"]])[N:]
        f1 = torch.cat([d["f0"], d["f1"]])[N:]
        out = d["out0"].clone()
        ops.lpips_head(f0, f1, d["w"], out)
        g0, g1 = torch.full_like(f0, float("nan")), torch.full_like(f1, float("nan"))   # (an element left unwritten is caught)
        ops.lpips_head_bwd(f0, f1, d["w"], d["gout"], g0, g1)
        only0, only1 = torch.full_like(f0, 7.0), torch.full_like(f1, 7.0)
        ops.lpips_head_bwd(f0, f1, d["w"], d["gout"], only0, None)
        ops.lpips_head_bwd(f0, f1, d["w"], d["gout"], None, only1)
        if not (_same(only0, g0) and _same(only1, g1)):
            fails.append("a one-sided gradient differs from the two-sided run")
        got = {"out": out, "g0": g0, "g1": g1}
    elif op == "pool3d":
        got = {"y": ops.avgpool3d_down(d["x"]), "gx": ops.avgpool3d_down_bwd(d["gy"], tuple(t["x"].shape))}
    elif op == "leaky_apply":
        rows, per, C = t["x"].shape
        x5 = d["x"].reshape(rows, 1, 1, per, C)
        tabs = (d["scale"], d["shift"]) if case["affine"] else None
        y = ops.gn_leaky_apply(x5, tabs, case["slope"])
        xin = x5.clone()
        if not (ops.gn_leaky_apply(xin, tabs, case["slope"], out=xin) is xin and _same(xin, y) and _same(x5.cpu(), t["x"].reshape(x5.shape))):
            fails.append("the in-place call differs, or the out-of-place call touched x")
        got = {"y": y.reshape(rows, per, C)}
    elif op == "leaky_bwd":
        gv = ops.leaky_bwd(d["y"], d["gy"], case["slope"])
        gin = d["gy"].clone()
        if not (ops.leaky_bwd(d["y"], gin, case["slope"], out=gin) is gin and _same(gin, gv) and _same(d["gy"].cpu(), t["gy"])):
            fails.append("the in-place call differs, or the out-of-place call touched gy")
        got = {"gv": gv}
    elif op == "stats_leaky":
        rows, per, C = t["x"].shape
        x5 = d["x"].reshape(rows, 1, 1, per, C)
        tabs = (d["scale"], d["shift"]) if case["affine"] else None
        plain = ops.gn_leaky_apply(x5, tabs, 0.2)
        y, part = ops.gn_leaky_apply(x5, tabs, 0.2, gn_out=case["G"])
        if not _same(y, plain):
            fails.append("the stored tensor differs from the plain entry point's")
        lib = L.load()
        for groups, buf in ((case["G"], None), (0, part.buf.data_ptr())):   # through the C entry: the plain pass
            o = torch.full_like(x5, 7.0)
            rc = lib.cvvae_gn_leaky_apply_stats(ops._dt(tdt), x5.data_ptr(), tabs[0].data_ptr() if tabs else None,
                                                tabs[1].data_ptr() if tabs else None, o.data_ptr(), rows, per, C, 0.2, groups, buf,
                                                ops._stream(x5))
            if rc != 0 or not _same(o, plain):
                fails.append(f"out_groups = {groups}, partials {'NULL' if buf is None else 'given'}: not the plain pass")
        got = dict(_stats_tables(case, y, part, fails), _stored=y, _records=part.buf)
    elif op == "stats_pool":
        plain = ops.avgpool3d_down(d["x"])
        y, part = ops.avgpool3d_down(d["x"], gn_out=case["G"])
        if not _same(y, plain):
            fails.append("the stored tensor differs from the plain entry point's")
        lib = L.load()
        B, T, H, W, C = t["x"].shape
        for groups, buf in ((case["G"], None), (0, part.buf.data_ptr())):
            o = torch.full_like(plain, 7.0)
            rc = lib.cvvae_avgpool3d_down_stats(ops._dt(tdt), d["x"].data_ptr(), o.data_ptr(), B, T, H, W, C, groups, buf, ops._stream(d["x"]))
            if rc != 0 or not _same(o, plain):
                fails.append(f"out_groups = {groups}, partials {'NULL' if buf is None else 'given'}: not the plain pass")
        got = dict(_stats_tables(case, y, part, fails), _stored=y, _records=part.buf)
    elif op == "dgrad":
        gy, cin = d["gy"], case["Cin"]
        if case.get("ps"):  # a pixel stride above Cout with NaN in the gap
            wide = torch.full((*gy.shape[:4], case["ps"]), float("nan"), dtype=tdt, device="cuda")
            wide[..., :case["Cout"]] = gy
            gy = wide
        out = ops.conv333_s2_dgrad_small(gy, d["w"], (case["B"], case["T"], case["H"], case["W"]), cin)
        got = {"gx": out[..., :cin], "pad": out[..., cin:]}
    else:
        raise AssertionError(op)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}, fails


def _device_inputs(case, dt):
    """the `device` recipe: operands too large to build on the host, drawn on the GPU"""
    g = torch.Generator(device="cuda").manual_seed(case.seed)
    x = torch.randn(case["rows"], case["per_row"], case["C"], generator=g, device="cuda").to(PR.DTYPE[dt])
    return {"x": (x * 1.3 + 0.25).to(PR.DTYPE[dt])}


def _check(case: PC.Case):
    failures = []
    for dt in case.dtypes:
        if case.raises:
            t = LR.inputs(case, dt)
            with pytest.raises((NotImplementedError, ValueError)):
                _run(case, dt, t)
            print(f"LOSSNET-EDGE {case.name} {dt}: raises (unsupported shape)")
            continue
        t = _device_inputs(case, dt) if case.recipe == "device" else LR.inputs(case, dt)
        (got, fails), (again, _) = _run(case, dt, t), _run(case, dt, t)
        same = all(_same(got[k], again[k]) for k in got)
        if case.recipe == "device":   # fp64 statistics of the stored tensor, on the device (64 M and 100 M elements)
            y = got["_stored"].cuda()
            mean, _, rstd = PR._moments(y.reshape(y.shape[0], -1, y.shape[-1]), case["G"], EPS)
            checks = PR._table_checks(mean.cpu(), rstd.cpu(), None, None, case["C"], False)
        elif case.op in LR.STATS_OPS:
            checks = LR.stats_reference(case, got["_stored"])
        else:
            checks = LR.reference(case, dt)
        w, where, bad = LR.worst(checks, got)
        print(f"LOSSNET-EDGE {case.name} {dt}: worst err/bound = {w:.4f} at {where}{'' if same else '  NOT REPRODUCIBLE'}"
              + "".join(f"  [{f}]" for f in fails))
        if not same:
            failures.append(f"{dt}: two runs on the same inputs differ")
        if not w <= 1.0:
            failures.append(f"{dt}: worst err/bound = {w:.4f} at {where} ({bad} elements beyond their bound)")
        failures += [f"{dt}: {f}" for f in fails]
    assert not failures, f"{case.name}: " + "; ".join(failures)


@pytest.mark.parametrize("case", BY_OP["scale_in"], ids=_ids(BY_OP["scale_in"]))
def test_lpips_scale_in(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["scale_in_bwd"], ids=_ids(BY_OP["scale_in_bwd"]))
def test_lpips_scale_in_bwd(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["relu"], ids=_ids(BY_OP["relu"]))
def test_relu(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["maxpool"], ids=_ids(BY_OP["maxpool"]))
def test_maxpool2x2(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["relu_pool_bwd"], ids=_ids(BY_OP["relu_pool_bwd"]))
def test_relu_pool_bwd(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["head"], ids=_ids(BY_OP["head"]))
def test_lpips_head_and_its_backward(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["pool3d"], ids=_ids(BY_OP["pool3d"]))
def test_avgpool3d_down_and_its_backward(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["leaky_apply"], ids=_ids(BY_OP["leaky_apply"]))
def test_gn_leaky_apply(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["leaky_bwd"], ids=_ids(BY_OP["leaky_bwd"]))
def test_leaky_bwd(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["stats_leaky"], ids=_ids(BY_OP["stats_leaky"]))
def test_gn_leaky_apply_stats(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["stats_pool"], ids=_ids(BY_OP["stats_pool"]))
def test_avgpool3d_down_stats(case):
    _check(case)


@pytest.mark.parametrize("case", BY_OP["dgrad"], ids=_ids(BY_OP["dgrad"]))
def test_conv333_s2_dgrad_small(case):
    _check(case)


# ------------------------------------------------------------------------------------------------------------ capped grids
def _split_launch(kernel, ops):
    """-> (draw the device operands of a [B, ...] shape, run the kernel on operands, slice operands to one sample)"""
    bf = torch.bfloat16

    def rnd(g, *shape):
        return torch.randn(*shape, generator=g, device="cuda").to(bf)

    if kernel == "avgpool3d_down":
        return (lambda g, s: (rnd(g, *s),)), (lambda a: ops.avgpool3d_down(a[0]))
    if kernel == "avgpool3d_down_bwd":
        return (lambda g, s: (rnd(g, *ops.avgpool3d_down_shape(s)), s)), \
               (lambda a: ops.avgpool3d_down_bwd(a[0], (a[0].shape[0],) + tuple(a[1][1:])))
    if kernel == "gn_leaky_apply":
        return (lambda g, s: (rnd(g, *s), 1.0 + 0.3 * torch.randn(s[0], s[4], generator=g, device="cuda"),
                              0.5 * torch.randn(s[0], s[4], generator=g, device="cuda"))), \
               (lambda a: ops.gn_leaky_apply(a[0], (a[1].contiguous(), a[2].contiguous()), 0.2))
    if kernel == "leaky_bwd":
        return (lambda g, s: (rnd(g, *s), rnd(g, *s))), (lambda a: ops.leaky_bwd(a[0], a[1], 0.2))
    if kernel == "relu":
        return (lambda g, s: (rnd(g, *s),)), (lambda a: ops.relu_(a[0].clone()))
    if kernel == "maxpool2x2":
        return (lambda g, s: (rnd(g, *s),)), (lambda a: ops.maxpool2x2(a[0]))
    if kernel == "relu_pool_bwd":
        return (lambda g, s: (torch.relu(rnd(g, *s)), rnd(g, *s), rnd(g, s[0], s[1], s[2] // 2, s[3] // 2, s[4]))), \
               (lambda a: ops.relu_pool_bwd(a[0], a[1], a[2]))
    raise AssertionError(kernel)


def _fp64_of_split(kernel, args, whole):
    """the looped launch of a disc kernel against the small cases' own reference (about 4.2 M elements: fractions of a second)"""
    cpu = [a.cpu() if isinstance(a, torch.Tensor) else a for a in args]
    if kernel == "avgpool3d_down":
        x = cpu[0].double()
        y, mean_abs = LR.pool3d_fwd(x), LR.pool3d_fwd(x.abs())
        arith = 8 * PR.U32 * mean_abs + 1e-300
        chk = PR.Check(y, arith + LR.half_ulp(y.abs() + arith, PC.BF16))
    elif kernel == "avgpool3d_down_bwd":
        chk = PR.Check(LR.pool3d_bwd(cpu[0].double(), tuple(whole.shape)).to(torch.bfloat16), None)
    elif kernel == "gn_leaky_apply":
        c = LC._case("split", "leaky_apply", affine=1, slope=0.2)
        B, C = cpu[0].shape[0], cpu[0].shape[-1]
        chk = LR._leaky_apply_reference(c, PC.BF16, {"x": cpu[0].reshape(B, -1, C), "scale": cpu[1], "shift": cpu[2]})["y"]
        whole = whole.reshape(B, -1, C)
    else:
        c = LC._case("split", "leaky_bwd", slope=0.2)
        chk = LR._leaky_bwd_reference(c, PC.BF16, {"y": cpu[0], "gy": cpu[1]})["gv"]
    return LR.check_one(whole.cpu(), chk)


@pytest.mark.parametrize("case", BY_OP["split"], ids=_ids(BY_OP["split"]))
def test_looped_launch_equals_the_two_unlooped_halves(case):
    from cvvae_amd import ops
    kernel, shape = case["kernel"], tuple(case["shape"])
    assert LC.split_items(case) > case["cap"] >= LC.split_items(case) // 2
    draw, launch = _split_launch(kernel, ops)
    args = draw(torch.Generator(device="cuda").manual_seed(case.seed), shape)
    whole = launch(args)
    again = launch(args)
    halves = [launch(tuple(a[i:i + 1].contiguous() if isinstance(a, torch.Tensor) else a for a in args)) for i in (0, 1)]
    torch.cuda.synchronize()
    same, split_ok = _same(whole, again), all(_same(whole[i:i + 1], halves[i]) for i in (0, 1))
    w, where = 0.0, "-"
    if case["cap"] == LC.DISC_CAP:
        w, idx, _ = _fp64_of_split(kernel, args, whole)
        where = f"out{list(idx)}"
    print(f"LOSSNET-EDGE {case.name} bf16: worst err/bound = {w:.4f} at {where}; looped launch "
          f"{'==' if split_ok else '!='} the two un-looped halves{'' if same else '  NOT REPRODUCIBLE'}")
    assert same and split_ok and w <= 1.0, (case.name, same, split_ok, w, where)
