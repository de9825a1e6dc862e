"""`lvdm.util` as the reference's engines and configs import it: the three helpers every `*_config` entry of the training YAML goes
through.  A config is a mapping `{"target": "dotted.path.Name", "params": {...}}`; the rest of that file (logging of tensors as
images, the diffusion helpers) is not on the codec's path."""
import importlib
from inspect import isfunction

__all__ = ["default", "get_obj_from_str", "instantiate_from_config"]


def default(val, d):
    """val unless it is None; else d (called first when d is a plain function)"""
    if val is not None:
        return val
    return d() if isfunction(d) else d


def get_obj_from_str(string: str, reload: bool = False, invalidate_cache: bool = True):
    """"pkg.module.Name" -> the object `Name` of the imported module"""
    module, name = string.rsplit(".", 1)
    if invalidate_cache:
        importlib.invalidate_caches()
    if reload:
        importlib.reload(importlib.import_module(module))
    return getattr(importlib.import_module(module, package=None), name)


def instantiate_from_config(config):
    """target(**params).  The two marker strings of the diffusion configs give None; anything else without a target is a KeyError."""
    if "target" not in config:
        if config in ("__is_first_stage__", "__is_unconditional__"):
            return None
        raise KeyError("Expected key `target` to instantiate.")
    return get_obj_from_str(config["target"])(**config.get("params", dict()))
