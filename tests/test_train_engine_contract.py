"""The contract of the training engines (cvvae_amd/autoencoder.py) and of cvvae_recon_panels that holds without a GPU: import paths,
constructor parameter names and defaults (tests/golden/engine_signatures.json: names only, taken from the reference's
lvdm/models/autoencoder.py and re-derived with `ast` where that file is present), state-dict key prefixes, the symbol, its
prototype and its refusals, the kernel's arithmetic plan against eager torch on the CPU, and the `frame_maps` switch of the
domain-constraint loss."""
import ast
import ctypes
import inspect
import json
import os

import pytest
import torch
import torch.nn as nn

from tests import engine_cases as EC
from tests import panel_edge_cases as PC
from tests import panel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = os.path.join(ROOT, "tests", "golden", "engine_signatures.json")
REFERENCE = "/root/reference/lvdm/models/autoencoder.py"
CLASSES = ["AbstractAutoencoder", "AutoencodingEngine", "AutoencodingEngineWithLatentConstraint", "AutoencodingEngineWithAllConstraint"]
REQUIRED = "<required>"
EINVAL, EUNSUPPORTED = -1, -2


def test_import_paths_resolve_to_one_set_of_classes():
    import cvvae_amd.autoencoder as B
    import lvdm.models.autoencoder as A
    import lvdm.util as U
    for n in CLASSES + ["build_from_config"]:
        assert getattr(A, n) is getattr(B, n), n
    assert not hasattr(A, "AutoencodingEngineWithEncoderConstraint")
    assert U.default(None, 3) == 3 and U.default(0, 3) == 0 and U.default(None, lambda: 5) == 5
    assert U.get_obj_from_str("torch.nn.Identity") is nn.Identity
    assert isinstance(U.instantiate_from_config({"target": "torch.nn.Linear", "params": {"in_features": 2, "out_features": 3}}), nn.Linear)
    assert U.instantiate_from_config("__is_first_stage__") is None and U.instantiate_from_config("__is_unconditional__") is None
    with pytest.raises(KeyError, match="target"):
        U.instantiate_from_config({"params": {}})
    for mod in ("pytorch_lightning", "omegaconf"):
        assert mod not in inspect.getsource(B).replace("pytorch_lightning did", "")


def _signature(cls):
    out = {"positional": [], "vararg": None, "kwonly": [], "kwarg": None}
    for name, p in list(inspect.signature(cls.__init__).parameters.items())[1:]:
        d = REQUIRED if p.default is inspect.Parameter.empty else p.default
        if p.kind == p.VAR_POSITIONAL:
            out["vararg"] = name
        elif p.kind == p.VAR_KEYWORD:
            out["kwarg"] = name
        elif p.kind == p.KEYWORD_ONLY:
            out["kwonly"].append([name, d])
        else:
            out["positional"].append([name, d])
    return out


def _from_source(path):
    tree = ast.parse(open(path).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in CLASSES:
            a = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == "__init__").args
            pos = [x.arg for x in a.args][1:]
            pd = [REQUIRED] * (len(pos) - len(a.defaults)) + [ast.literal_eval(d) for d in a.defaults]
            out[node.name] = {"positional": [[n, d] for n, d in zip(pos, pd)], "vararg": a.vararg.arg if a.vararg else None,
                              "kwonly": [[x.arg, REQUIRED if d is None else ast.literal_eval(d)] for x, d in zip(a.kwonlyargs, a.kw_defaults)],
                              "kwarg": a.kwarg.arg if a.kwarg else None}
    return out


def test_constructor_names_and_defaults_are_the_recorded_ones():
    import cvvae_amd.autoencoder as B
    want = json.load(open(SIGNATURES))
    assert sorted(want) == sorted(CLASSES)
    for n in CLASSES:
        assert _signature(getattr(B, n)) == want[n], n


def test_recorded_names_are_the_references():
    if not os.path.isfile(REFERENCE):
        pytest.skip("the reference's source is not on this machine")
    assert _from_source(REFERENCE) == json.load(open(SIGNATURES))


@pytest.fixture(scope="module")
def engines():
    return {(k, ema): EC.build(k, False, ema_decay=ema) for k in ("latent", "all") for ema in (None, 0.999)}


def test_state_dict_prefixes_and_optimizer_split(engines):
    for (kind, ema), e in engines.items():
        pre = {k.split(".", 1)[0] for k in e.state_dict()}
        want = {"encoder", "decoder", "loss", "constraint_decoder"} | ({"constraint_encoder"} if kind == "all" else set()) | \
               ({"model_ema"} if ema else set())
        assert pre == want, (kind, ema, pre)
        assert all(not p.requires_grad for p in e.constraint_decoder.parameters())
        assert {"loss.logvar", "loss.logvar_2d", "loss.discriminator.main.0.weight", "encoder.conv_in.weight",
                "decoder.conv_out.weight"} <= set(e.state_dict())
        assert e.learning_rate == EC.BASE_LR and e.input_key == "frames" and e.global_step == 0
        opts, sches = e.optimizers(), e.lr_schedulers()
        assert len(opts) == 2 and len(sches) == 2 and e.optimizers() is opts
        ae = [id(p) for g in opts[0].param_groups for p in g["params"]]
        assert ae == [id(p) for p in e.get_autoencoder_params()]
        assert ae[:2] == [id(e.loss.logvar), id(e.loss.logvar_2d)]
        assert [id(p) for g in opts[1].param_groups for p in g["params"]] == [id(p) for p in e.loss.discriminator.parameters()]
        assert opts[0].param_groups[0]["lr"] == 0.0 and opts[0].param_groups[0]["initial_lr"] == 2 * EC.BASE_LR   # the warm-up's step 0
        assert opts[1].param_groups[0]["lr"] == EC.BASE_LR
        assert e.get_last_layer() is e.decoder.conv_out.weight
        if ema:
            shadows = dict(e.model_ema.named_buffers())
            trainable = [n for n, p in e.named_parameters() if p.requires_grad]
            assert len(shadows) == len(trainable) + 2 and "encoderconv_inweight" in shadows and "losslogvar" in shadows
            assert torch.equal(shadows["decoderconv_outweight"], e.decoder.conv_out.weight)


def test_trainable_switch_and_param_groups():
    for trainable, frozen in ((False, ("encoder", "decoder", "loss")), ("encoder", ("decoder",)), ("decoder", ("encoder",))):
        e = EC.build("latent", False, trainable=trainable, ema_decay=0.9)
        for n in ("encoder", "decoder"):
            assert all(p.requires_grad != (n in frozen) for p in getattr(e, n).parameters()), (trainable, n)
        assert len(dict(e.model_ema.named_buffers())) == 2 + sum(p.requires_grad for p in e.parameters())
    with pytest.raises(AssertionError, match="trainable"):
        EC.build("latent", False, trainable="both")
    e = EC.build("latent", False, trainable_ae_params=[["encoder\\.conv_in\\..*"], ["decoder\\.conv_out\\.weight"]],
                 ae_optimizer_args=[{"weight_decay": 0.0}, {}])
    groups, n = e.get_param_groups(e.trainable_ae_params, e.ae_optimizer_args)
    assert [len(g["params"]) for g in groups] == [2, 1] and groups[0]["weight_decay"] == 0.0
    assert n == e.encoder.conv_in.weight.numel() + e.encoder.conv_in.bias.numel() + e.decoder.conv_out.weight.numel()
    assert [len(g["params"]) for g in e.optimizers()[0].param_groups] == [2, 1]
    e = EC.build("latent", False)
    e.learning_rate = None
    with pytest.raises(RuntimeError, match="learning_rate"):
        e.optimizers()


def test_toggle_model_restores_on_an_exception(engines):
    e = engines[("latent", None)]
    opts = e.optimizers()
    before = {n: p.requires_grad for n, p in e.named_parameters()}
    with pytest.raises(ZeroDivisionError):
        with e.toggle_model(opts[0]):
            assert not any(p.requires_grad for p in e.loss.discriminator.parameters())
            assert all(p.requires_grad for p in e.encoder.parameters()) and e.loss.logvar.requires_grad
            1 / 0
    assert before == {n: p.requires_grad for n, p in e.named_parameters()}
    with e.toggle_model(opts[1]):
        assert all(p.requires_grad for p in e.loss.discriminator.parameters())
        assert not any(p.requires_grad for p in list(e.encoder.parameters()) + list(e.decoder.parameters()) + [e.loss.logvar])
    assert before == {n: p.requires_grad for n, p in e.named_parameters()}


# ---- cvvae_recon_panels ----
def test_entry_point_is_exported_typed_and_declared_and_the_abi_version_stays():
    from cvvae_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(os.path.join(ROOT, "include", "cvvae.h")).read()
    assert "#define CVVAE_ABI_VERSION 14" in header and "cvvae_recon_panels(" in header
    n = "cvvae_recon_panels"
    assert n in _lib.PROTOTYPES and hasattr(lib, n) and getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1]
    assert _lib.PROTOTYPES[n][1][8] is ctypes.c_float and len(_lib.PROTOTYPES[n][1]) == 14
    assert "panel_kernels.hip" in open(os.path.join(_lib._HERE, "csrc", "Makefile")).read()
    assert "panel_kernels.hip" in _lib.TRAINING_ONLY_SOURCES
    src = open(os.path.join(_lib._HERE, "csrc", "panel_kernels.hip")).read()
    assert "__shared__" not in src and "atomic" not in src.replace("no atomics", "")


def test_every_refusal_is_reached_before_any_launch():
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL, aligned HOST pointer: the checks never dereference it or launch
    W = 13

    def view(**kw):
        v = L.ClipView()
        v.layout, v.dtype, v.sb, v.sc, v.st, v.sy = L.CLIP_NCTHW, L.BF16, 3 * 2 * 12 * W, 2 * 12 * W, 12 * W, W
        for k, val in kw.items():
            setattr(v, k, val)
        return v
    names = ["x", "vx", "xrec", "vr", "B", "T", "H", "W", "boost", "inputs", "reconstructions", "diff", "diff_boost", "stream"]
    vx, vr = view(), view()

    def call(**kw):
        args = [p, ctypes.byref(vx), p, ctypes.byref(vr), 1, 2, 12, W, 3.0, p, p, p, p, None]
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.cvvae_recon_panels(*args)

    for k in ("x", "vx", "xrec", "vr", "inputs", "reconstructions", "diff", "diff_boost"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("B", "T", "H", "W"):
        for bad in (0, -1):
            assert call(**{k: bad}) == EINVAL, (k, bad)
    for k in ("sb", "sc", "st", "sy"):
        nv = view(**{k: -1})
        assert call(vx=ctypes.byref(nv)) == EINVAL and call(vr=ctypes.byref(nv)) == EINVAL, k
    nv = view(sy=W - 1)
    assert call(vx=ctypes.byref(nv)) == EINVAL and call(vr=ctypes.byref(nv)) == EINVAL
    odd = ctypes.c_void_p(p.value + 1)
    for k in ("x", "xrec", "inputs", "diff_boost"):
        assert call(**{k: odd}) == EINVAL, k
    half = ctypes.c_void_p(p.value + 2)
    f32x, f32r = view(dtype=L.F32), view(dtype=L.F32)
    assert call(vx=ctypes.byref(f32x), vr=ctypes.byref(f32r), diff=half) == EINVAL      # a float output on a 2-byte boundary
    for bad in (L.F32Q, L.F32Q6, 9, -1):
        nv = view(dtype=bad)
        assert call(vx=ctypes.byref(nv)) == EUNSUPPORTED and call(vr=ctypes.byref(nv)) == EUNSUPPORTED, bad
    assert call(vr=ctypes.byref(f32r)) == EUNSUPPORTED and call(vx=ctypes.byref(f32x)) == EUNSUPPORTED     # two dtypes
    for bad in (L.CLIP_THWC_U8, 2, -1):
        nv = view(layout=bad)
        assert call(vx=ctypes.byref(nv)) == EUNSUPPORTED and call(vr=ctypes.byref(nv)) == EUNSUPPORTED, bad
    wide, wide_r = view(sy=(1 << 20) + 1), view(sy=(1 << 20) + 1)
    assert call(W=(1 << 20) + 1, vx=ctypes.byref(wide), vr=ctypes.byref(wide_r)) == EUNSUPPORTED
    assert call(H=(1 << 20) + 1) == EUNSUPPORTED and call(B=1 << 11, T=1 << 10) == EUNSUPPORTED


def test_wrapper_has_no_cpu_path_and_checks_its_operands_first(monkeypatch):
    from cvvae_amd import ops
    x = torch.zeros(1, 3, 2, 4, 5)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.recon_panels(x, x, 3.0)
    monkeypatch.setattr(ops, "_need_gpu", lambda t: None)
    for a, b, msg in ((x, x.half(), "one dtype"), (x, x[:, :, :1], "shapes"), (x[0], x[0], r"\[B,3,T,H,W\]"),
                      (x.double(), x.double(), "fp16 / bf16 / fp32"), (x[:, :, :0], x[:, :, :0], "empty")):
        with pytest.raises(ValueError, match=msg):
            ops.recon_panels(a, b, 3.0)


def test_case_list_covers_what_it_says():
    assert len(PC.CASES) == 3 * 6 * 4 and len({c.name for c in PC.CASES}) == len(PC.CASES)
    for case in PC.CASES:
        x, r = PC.bases(case)
        v = PC.view_of(case, x)
        assert torch.equal(v, x) and v.stride(4) == 1 and v.stride(3) >= x.shape[4]
        if case.view != "none":
            assert not v.is_contiguous() or v.storage_offset()
        if x.numel() >= 3 * 32:
            xf, rf = x.float(), r.float()
            assert bool((xf.abs() > 1).any()) and bool((rf.abs() > 1).any()) and bool((xf == -3).any())
            assert bool(((xf == 0) & xf.signbit()).any()) and bool(((rf == 0) & rf.signbit()).any())
            assert bool((xf.abs() == 1).any()) and bool((rf.abs() == 1).any())


@pytest.mark.parametrize("case", [c for c in PC.CASES if c.view == "none"], ids=lambda c: c.name)
def test_the_kernels_arithmetic_plan_is_the_eager_expression_bit_for_bit(case):
    """fp32 arithmetic with one rounding per stored tensor == torch's own evaluation in the dtype (CPU)"""
    x, r = PC.bases(case)
    for f in PC.BOOSTS:
        for name, a, b in zip(("inputs", "reconstructions", "diff", "diff_boost"), R.kernel_model(x, r, f), R.panels(x, r, f)):
            assert R.same_bits(a, b), (f, name)
    d = R.panels(x, r, 3.0)
    i = (x.float().flatten() == -3).nonzero()
    if len(i):   # x = -3 against xrec = 1: the upper clamp, both panels at +1
        xf = R.frames(x).flatten().float()
        j = int((xf == -3).nonzero()[0])
        assert float(d[2].flatten()[j]) == 1.0 and float(d[3].flatten()[j]) == 1.0


# ---- the domain-constraint loss's frame maps ----
def test_domain_class_refuses_without_frame_maps_and_builds_with_it():
    from cvvae_amd.loss import LPIPSWithDiscriminatorAndAllConstraint as A
    from cvvae_amd.loss import LPIPSWithDiscriminatorAndDomainConstraint as D
    disc = nn.Identity()
    for t in ("mean", "random"):
        with pytest.raises(NotImplementedError, match=f'target_type="{t}".*frame_maps=True'):
            D(disc_start=0, dims=3, target_type=t, discriminator=disc)
        m = D(disc_start=0, dims=3, target_type=t, discriminator=disc, frame_maps=True)
        assert m.target_type == t and m.frame_maps
    assert not D(disc_start=0, dims=3, discriminator=disc).frame_maps
    p = inspect.signature(D.__init__).parameters["frame_maps"]
    assert p.kind == p.KEYWORD_ONLY and p.default is False
    fw = inspect.signature(D.forward).parameters
    assert fw["generator"].kind == fw["frame_indices"].kind == inspect.Parameter.KEYWORD_ONLY
    assert D.draw_frame_indices is A.draw_frame_indices and D._rec2d_sum is A._rec2d_sum        # shared, not copied
    g = torch.Generator().manual_seed(4)
    idx = D(disc_start=0, dims=3, target_type="random", discriminator=disc, frame_maps=True).draw_frame_indices(9, g)
    assert idx.tolist()[0] == 0 and 1 <= idx[1] <= 4 and 5 <= idx[2] <= 8
