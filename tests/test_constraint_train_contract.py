"""What holds without a GPU for the frame-mapped pixel sums (csrc/loss_kernels.hip: cvvae_reduce_sum_frames / _bwd) and the
all-constraint loss class: the three entry points are exported, typed and declared, the ABI version and the existing structs stay,
every refusal returns its code from HOST pointers before any launch, the Python wrappers describe clips as the header says and
refuse what cannot be read in place, and the class carries the reference's names (tests/golden/loss_names_allconstraint.json)."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = json.load(open(os.path.join(HERE, "golden", "loss_names_allconstraint.json")))
ENTRIES = ["cvvae_reduce_frames_workspace_bytes", "cvvae_reduce_sum_frames", "cvvae_reduce_sum_frames_bwd"]
EINVAL, EUNSUPPORTED = -1, -2


def test_entry_points_are_exported_with_prototypes_and_the_abi_version_stays():
    from cvvae_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 and lib.cvvae_abi_version() == 14
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "cvvae.h")).read()
    assert "#define CVVAE_ABI_VERSION 14" in header
    for n in ENTRIES:
        assert n in _lib.PROTOTYPES and hasattr(lib, n) and (n + "(") in header, n
    assert (_lib.FMAP_GATHER, _lib.FMAP_GROUP_MEAN, _lib.FMAP_MAX_FRAMES) == (0, 1, 256)
    assert "CVVAE_FMAP_GATHER = 0" in header and "CVVAE_FMAP_GROUP_MEAN = 1" in header and "#define CVVAE_FMAP_MAX_FRAMES 256" in header
    assert ctypes.sizeof(_lib.ReduceShape) == 80                     # the existing struct did not move
    assert ctypes.sizeof(_lib.FrameMap) == 2 * 4 + 6 * 8 + ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in _lib.FrameMap._fields_] == ["mode", "group", "rows", "frames_in", "frames_out", "HW", "row_stride",
                                                      "frame_stride", "index"]


def _map(mode=0, group=1, rows=2, fin=9, fout=3, hw=16, row_stride=None, frame_stride=None, index=(0, 4, 8)):
    from cvvae_amd import _lib as L
    m = L.FrameMap()
    m.mode, m.group, m.rows, m.frames_in, m.frames_out, m.HW = mode, group, rows, fin, fout, hw
    m.frame_stride = hw if frame_stride is None else frame_stride
    m.row_stride = fin * m.frame_stride if row_stride is None else row_stride
    if index is not None:
        m._keep = (ctypes.c_int32 * len(index))(*index)
        m.index = ctypes.cast(m._keep, ctypes.POINTER(ctypes.c_int32))
    return m


def test_frame_entry_points_refuse_bad_arguments_before_any_launch():
    from cvvae_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # a non-NULL (host) pointer: the checks below never dereference or launch
    A, S = L.RED_ABS_DIFF, L.RED_SQ_DIFF
    good = _map()
    g = ctypes.byref(good)

    def fwd(m, op=A, da=L.F32, a=p, db=L.BF16, clip=p, ws=p, out=p):
        return lib.cvvae_reduce_sum_frames(op, da, a, db, clip, ctypes.byref(m) if m is not None else None, ws, out, None)

    def bwd(m, op=S, da=L.F16, a=p, db=L.F32, clip=p, coef=p, ga=p):
        return lib.cvvae_reduce_sum_frames_bwd(op, da, a, db, clip, ctypes.byref(m) if m is not None else None, coef, ga, None)

    # every NULL pointer
    assert fwd(good, a=None) == EINVAL and fwd(good, clip=None) == EINVAL and fwd(None) == EINVAL
    assert fwd(good, ws=None) == EINVAL and fwd(good, out=None) == EINVAL
    assert bwd(good, a=None) == EINVAL and bwd(good, clip=None) == EINVAL and bwd(None) == EINVAL
    assert bwd(good, coef=None) == EINVAL and bwd(good, ga=None) == EINVAL
    assert fwd(_map(index=None)) == EINVAL and bwd(_map(index=None)) == EINVAL          # GATHER without its table
    # ops and dtypes
    for op in (L.RED_SQ, L.RED_IDENT, L.RED_HINGE_NEG, L.RED_SOFTPLUS_POS, 8, -1):
        assert fwd(good, op=op) == EUNSUPPORTED and bwd(good, op=op) == EUNSUPPORTED, op
    assert fwd(good, da=7) == EUNSUPPORTED and fwd(good, db=L.F32Q) == EUNSUPPORTED
    assert bwd(good, da=L.F32Q6) == EUNSUPPORTED and bwd(good, db=9) == EUNSUPPORTED
    # extents, indices, strides, the group rule, the table's length
    bad = [_map(rows=0), _map(fin=0), _map(fout=0, index=()), _map(hw=0), _map(rows=-1), _map(hw=-16),
           _map(index=(0, 4, 9)), _map(index=(0, -1, 8)),
           _map(frame_stride=15), _map(row_stride=9 * 16 - 1), _map(frame_stride=20, row_stride=8 * 20 + 15),
           _map(mode=1, group=0, index=None), _map(mode=1, group=-4, index=None), _map(mode=1, group=4, fin=8, index=None),
           _map(mode=1, group=3, fin=9, index=None), _map(mode=2), _map(mode=-1)]
    for m in bad:
        assert fwd(m) == EINVAL and bwd(m) == EINVAL, (m.mode, m.group, m.rows, m.frames_in, m.frames_out, m.HW)
        assert lib.cvvae_reduce_frames_workspace_bytes(ctypes.byref(m)) == 0
    many = _map(fin=300, fout=257, index=tuple(range(257)))
    assert fwd(many) == EUNSUPPORTED and bwd(many) == EUNSUPPORTED
    assert lib.cvvae_reduce_frames_workspace_bytes(None) == 0
    del g


def test_workspace_bytes_follow_the_grid_rule_of_the_plain_reduction():
    """one fp32 partial per workgroup pass of 2048 target elements, capped at 2048: the grid of cvvae_reduce_sum over the target"""
    from cvvae_amd import _lib as L
    lib = L.load()
    ws = lambda m: lib.cvvae_reduce_frames_workspace_bytes(ctypes.byref(m))  # noqa: E731
    assert ws(_map()) == 4                                                   # 2 x 3 x 16 = 96 elements
    assert ws(_map(rows=6, hw=256)) == 4 * 3                                 # 4608
    assert ws(_map(rows=3, hw=1024, fin=9, fout=3, mode=1, group=4, index=None)) == 4 * 5      # 9216 -> 5 passes
    assert ws(_map(rows=3, fin=1, fout=1, hw=2049, index=(0,))) == 4 * 4
    assert ws(_map(rows=4096, hw=4096, fin=1, fout=1, index=(0,))) == 4 * 2048
    # strides of extent-1 dimensions are not read
    assert ws(_map(rows=1, fin=1, fout=1, hw=64, row_stride=0, frame_stride=0, index=(0,))) == 4


def test_python_wrapper_describes_clips_in_place_and_refuses_the_rest(monkeypatch):
    from cvvae_amd import _lib as L
    from cvvae_amd import ops
    monkeypatch.setattr(ops, "_need_gpu", lambda t: None)
    x = torch.zeros(2, 3, 9, 6, 5)
    a = torch.zeros(2, 3, 3, 6, 5, dtype=torch.bfloat16)
    m = ops._frame_map(L.RED_ABS_DIFF, a, x, L.FMAP_GATHER, [0, 3, 7], None)
    assert (m.mode, m.rows, m.frames_in, m.frames_out, m.HW, m.row_stride, m.frame_stride) == (0, 6, 9, 3, 30, 270, 30)
    assert [m.index[i] for i in range(3)] == [0, 3, 7]
    m = ops._frame_map(L.RED_SQ_DIFF, a, x, L.FMAP_GATHER, torch.tensor([0, 1, 5]), None)
    assert [m.index[i] for i in range(3)] == [0, 1, 5]
    m = ops._frame_map(L.RED_SQ_DIFF, a, x, L.FMAP_GROUP_MEAN, None, 4)
    assert (m.mode, m.group, m.frames_in, m.frames_out) == (1, 4, 9, 3)
    big = torch.zeros(2, 3, 9, 8, 5)
    m = ops._frame_map(L.RED_ABS_DIFF, a, big[:, :, :, 1:-1], L.FMAP_GROUP_MEAN, None, 4)       # a row-strided view: H sliced
    assert (m.HW, m.frame_stride, m.row_stride, m.rows) == (30, 40, 360, 6)
    m = ops._frame_map(L.RED_ABS_DIFF, a[:1], x[:1], L.FMAP_GROUP_MEAN, None, 4)
    assert (m.rows, m.row_stride) == (3, 270)
    with pytest.raises(ValueError, match="contiguous"):
        ops._frame_map(L.RED_ABS_DIFF, a, torch.zeros(2, 3, 9, 6, 7)[..., 1:-1], L.FMAP_GROUP_MEAN, None, 4)   # W sliced
    with pytest.raises(ValueError, match="row stride"):
        ops._frame_map(L.RED_ABS_DIFF, a, torch.zeros(2, 4, 9, 6, 5)[:, :3], L.FMAP_GROUP_MEAN, None, 4)       # B, C do not merge
    with pytest.raises(ValueError, match="contiguous"):
        ops._frame_map(L.RED_ABS_DIFF, torch.zeros(2, 3, 6, 6, 5)[:, :, ::2], x, L.FMAP_GROUP_MEAN, None, 4)
    with pytest.raises(ValueError, match="frame indices"):
        ops._frame_map(L.RED_ABS_DIFF, a, x, L.FMAP_GATHER, [0, 4], None)
    with pytest.raises(ValueError, match="ABS_DIFF / SQ_DIFF"):
        ops._frame_map(L.RED_SQ, a, x, L.FMAP_GATHER, [0, 4, 8], None)
    with pytest.raises(ValueError, match=r"\[B,C,T',H,W\]"):
        ops._frame_map(L.RED_ABS_DIFF, a, torch.zeros(2, 3, 9, 6, 6), L.FMAP_GATHER, [0, 4, 8], None)


def test_cpu_tensors_raise_the_no_cpu_path_error():
    from cvvae_amd import _lib as L
    from cvvae_amd import loss, ops
    x, a = torch.zeros(1, 3, 5, 8, 8), torch.zeros(1, 3, 2, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.reduce_sum_frames(L.RED_ABS_DIFF, a, x, L.FMAP_GROUP_MEAN, group=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.reduce_sum_frames_bwd(L.RED_ABS_DIFF, a, x, torch.zeros(()), L.FMAP_GATHER, index=[0, 2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.reduce_frames(L.RED_ABS_DIFF, a, x, L.FMAP_GATHER, index=[0, 2])
    m = loss.LPIPSWithDiscriminatorAndAllConstraint(disc_start=0, dims=3, target_type="random", discriminator=nn.Identity())
    for idx in (0, 1):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(x, torch.zeros(2, 3, 5, 8, 8, requires_grad=True), a, regularization_log={}, optimizer_idx=idx, global_step=1,
              last_layer=None)


class TinyDisc3d(nn.Module):
    def __init__(self, ch: int = 4):
        super().__init__()
        self.conv = nn.Conv3d(3, ch, 1)
        self.norm = nn.BatchNorm3d(ch)


@pytest.mark.parametrize("learn", [False, True])
@pytest.mark.parametrize("target_type", ["slice", "random", "mean"])
def test_names_parameters_and_forward_keys_are_the_references(target_type, learn):
    import cvvae_amd.loss as loss
    from cvvae_amd.lpips import LPIPS
    from lvdm.modules.autoencoding.losses import LPIPSWithDiscriminatorAndAllConstraint
    assert LPIPSWithDiscriminatorAndAllConstraint is loss.LPIPSWithDiscriminatorAndAllConstraint
    assert issubclass(LPIPSWithDiscriminatorAndAllConstraint, loss.GeneralLPIPSWithDiscriminator)
    torch.manual_seed(0)
    m = LPIPSWithDiscriminatorAndAllConstraint(
        disc_start=5, logvar_init=0.25, dims=3, learn_logvar=learn, target_type=target_type, time_n_compress=2, rec2d_weight=0.5,
        discriminator_config={"target": "tests.test_constraint_train_contract.TinyDisc3d", "params": {"ch": 6}})
    want = NAMES["LPIPSWithDiscriminatorAndAllConstraint"]
    keys = list(m.state_dict())
    assert sorted(k for k in keys if not k.startswith("discriminator.")) == sorted(want["state_dict"])
    assert sorted(k for k in keys if k.startswith("discriminator.")) == sorted("discriminator." + k for k in TinyDisc3d().state_dict())
    assert m.forward_keys == want["forward_keys"]
    assert (m.target_type, m.time_n_compress, m.rec2d_weight) == (target_type, 2, 0.5)
    for p in (m.logvar, m.logvar_2d):
        assert p.dim() == 0 and float(p.detach()) == 0.25 and p.requires_grad == learn
    assert [id(p) for p in m.get_trainable_autoencoder_parameters()] == ([id(m.logvar), id(m.logvar_2d)] if learn else [])
    assert [id(p) for p in m.get_trainable_parameters()] == [id(p) for p in m.discriminator.parameters()]
    assert isinstance(m.perceptual_loss, LPIPS) and not m.perceptual_loss.training
    assert type(m.discriminator).__name__ == "TinyDisc3d" and m.discriminator.conv.out_channels == 6


def test_unsupported_options_raise_as_for_the_sibling_classes():
    from cvvae_amd.loss import LPIPSWithDiscriminatorAndAllConstraint as A
    disc = nn.Identity()
    with pytest.raises(NotImplementedError, match="no discriminator network ships yet"):
        A(disc_start=0, dims=3)
    with pytest.raises(NotImplementedError, match="scale_input_to_tgt_size"):
        A(disc_start=0, dims=3, scale_input_to_tgt_size=True, discriminator=disc)
    with pytest.raises(AssertionError):
        A(disc_start=0, dims=3, target_type="median", discriminator=disc)
    with pytest.raises(ValueError, match="not both"):
        A(disc_start=0, dims=3, discriminator=disc, discriminator_config={"target": "torch.nn.Identity"})
    assert not hasattr(A, "log_images")
