"""Test infrastructure for the LPIPS perceptual loss (cvvae_amd/lpips.py): the state-dict layout written out literally, seeded
weights, and a plain-PyTorch restatement of the reference's LPIPS.forward that every parity test is measured against.

The restatement follows lvdm/modules/autoencoding/lpips/loss/lpips.py of the reference line by line (cited below) with
torchvision's VGG16 `features` layout (configuration D: 64 64 M 128 128 M 256 256 256 M 512 512 512 M 512 512 512, every conv 3x3
with padding 1 followed by ReLU, M = MaxPool2d(2, 2); indices 0..29 used).  The reference module itself cannot be run here: it
imports torchvision and downloads its weights.  Pretrained VGG / LPIPS weights are not available either, so all parity is on
seeded weights."""
import torch
import torch.nn.functional as F

from oracle.seeded import seeded_state_dict

# (slice, starts with a pool, conv indices): lpips.py:103-118 over torchvision's numbering
PLAN = (("slice1", False, (0, 2)), ("slice2", True, (5, 7)), ("slice3", True, (10, 12, 14)), ("slice4", True, (17, 19, 21)),
        ("slice5", True, (24, 26, 28)))

# the reference's state dict, key -> shape (LPIPS(use_dropout=True): lin weights at model.1, the Dropout is model.0)
STATE_DICT_SHAPES = {
    "scaling_layer.shift": (1, 3, 1, 1),
    "scaling_layer.scale": (1, 3, 1, 1),
    "net.slice1.0.weight": (64, 3, 3, 3), "net.slice1.0.bias": (64,),
    "net.slice1.2.weight": (64, 64, 3, 3), "net.slice1.2.bias": (64,),
    "net.slice2.5.weight": (128, 64, 3, 3), "net.slice2.5.bias": (128,),
    "net.slice2.7.weight": (128, 128, 3, 3), "net.slice2.7.bias": (128,),
    "net.slice3.10.weight": (256, 128, 3, 3), "net.slice3.10.bias": (256,),
    "net.slice3.12.weight": (256, 256, 3, 3), "net.slice3.12.bias": (256,),
    "net.slice3.14.weight": (256, 256, 3, 3), "net.slice3.14.bias": (256,),
    "net.slice4.17.weight": (512, 256, 3, 3), "net.slice4.17.bias": (512,),
    "net.slice4.19.weight": (512, 512, 3, 3), "net.slice4.19.bias": (512,),
    "net.slice4.21.weight": (512, 512, 3, 3), "net.slice4.21.bias": (512,),
    "net.slice5.24.weight": (512, 512, 3, 3), "net.slice5.24.bias": (512,),
    "net.slice5.26.weight": (512, 512, 3, 3), "net.slice5.26.bias": (512,),
    "net.slice5.28.weight": (512, 512, 3, 3), "net.slice5.28.bias": (512,),
    "lin0.model.1.weight": (1, 64, 1, 1),
    "lin1.model.1.weight": (1, 128, 1, 1),
    "lin2.model.1.weight": (1, 256, 1, 1),
    "lin3.model.1.weight": (1, 512, 1, 1),
    "lin4.model.1.weight": (1, 512, 1, 1),
}
SHIFT = (-0.030, -0.088, -0.188)   # lpips.py:70-75
SCALE = (0.458, 0.448, 0.450)


def lpips_state_dict(seed: int = 0) -> dict:
    """seeded fp32 weights in the reference's layout.  oracle.seeded draws conv weights uniform in +-1/sqrt(fan_in) (variance
    1 / (3 fan_in)); times sqrt(6) that is He scaling (variance 2 / fan_in), which keeps the ReLU features' magnitude level
    across the 13 layers.  The lin weights are made non-negative, as the trained ones are; the buffers hold the constants."""
    sd = seeded_state_dict(STATE_DICT_SHAPES, seed)
    for k in sd:
        if k.startswith("net.") and k.endswith(".weight"):
            sd[k] = sd[k] * 6.0 ** 0.5
        elif k.startswith("lin"):
            sd[k] = sd[k].abs()
    sd["scaling_layer.shift"] = torch.tensor(SHIFT)[None, :, None, None]
    sd["scaling_layer.scale"] = torch.tensor(SCALE)[None, :, None, None]
    return sd


def normalize_tensor(x, eps=1e-10):
    """lpips.py:141-143"""
    norm_factor = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True) + eps)
    return x / (norm_factor + eps)


def vgg_taps(x, p):
    """vgg16.forward, lpips.py:123-138: the five tapped ReLU outputs"""
    outs = []
    for name, pool, convs in PLAN:
        if pool:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
        for i in convs:
            x = F.relu(F.conv2d(x, p[f"net.{name}.{i}.weight"], p[f"net.{name}.{i}.bias"], stride=1, padding=1))
        outs.append(x)
    return outs


def lpips_forward(inp, tgt, sd, dtype=torch.float64):
    """LPIPS.forward, lpips.py:46-64, evaluated op by op in `dtype` on the tensors' device (autograd-capable) -> [N,1,1,1]"""
    p = {k: v.to(dtype) for k, v in sd.items()}

    def scaling(x):  # ScalingLayer.forward, lpips.py:77-78
        return (x - p["scaling_layer.shift"]) / p["scaling_layer.scale"]

    outs0, outs1 = vgg_taps(scaling(inp.to(dtype)), p), vgg_taps(scaling(tgt.to(dtype)), p)
    val = None
    for kk in range(5):
        diff = (normalize_tensor(outs0[kk]) - normalize_tensor(outs1[kk])) ** 2                   # :52-55
        res = F.conv2d(diff, p[f"lin{kk}.model.1.weight"]).mean([2, 3], keepdim=True)            # :57-60 (Dropout = identity in eval)
        val = res if val is None else val + res                                                  # :61-63
    return val


def lpips_with_grads(inp, tgt, sd, cot, dtype=torch.float64, wrt=(False, True)):
    """(value, d/d inp or None, d/d tgt or None) of sum(cot * LPIPS(inp, tgt)) with torch.autograd, everything in `dtype`"""
    a = inp.detach().to(dtype).clone().requires_grad_(wrt[0])
    b = tgt.detach().to(dtype).clone().requires_grad_(wrt[1])
    with torch.enable_grad():
        val = lpips_forward(a, b, sd, dtype)
        (val * cot.to(dtype)).sum().backward()
    return val.detach(), a.grad, b.grad
