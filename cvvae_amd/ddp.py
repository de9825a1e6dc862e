"""Data-parallel training for the engines: the gradient exchange between `manual_backward` and the clip, as ONE pack launch and ONE
all-reduce of a flat bucket.

`torch.nn.parallel.DistributedDataParallel` hooks a wrapper's `forward`; the engines (cvvae_amd/autoencoder.py) optimise by hand --
zero, toggle `requires_grad` between two optimizers, backward, clip, step -- so the exchange is a call of its own, `GradientSync.sync()`,
which `training_step` makes once `engine.data_parallel()` has been called.

Layout.  One persistent flat fp32 buffer per GradientSync.  Every fp32 parameter of `params` has a slot of its element count whose
start is a multiple of 4 elements (16 bytes: the pack kernel and the passes that read the slot afterwards move 16-byte vectors); a
parameter of another dtype has an empty slot (its gradients take the torch path below).  Slots follow list order and are disjoint;
the gaps between them are zeroed once and never written.  `layout()` returns the offsets (pure host code).

sync().  `ops.mt_pack` (include/cvvae.h cvvae_mt_pack) writes g / world into the slots -- a correctly rounded fp32 division, what
DistributedDataParallel applies before its sum, so a replica's sum is sum_r(g_r / world) -- and zeros into the slot of a parameter
without a gradient.  The buffer is all-reduced (SUM), and `p.grad` becomes the slot's view for every parameter that had a gradient
on this rank (the others keep None).  There is no unpack pass: the views are dense contiguous fp32 device tensors, so cvvae_mt_grad_norm
and cvvae_mt_adamw read the bucket in place, and `optimizer.last_grad_norm` is the norm of the AVERAGED gradient on every rank.  With a
world size of 1 the all-reduce is skipped; the pack and the views still run.

Gradients the kernel does not take (not fp32, not contiguous, not on a ROCm device) are exchanged per dtype by plain torch calls:
flatten, div_, all-reduce, copy back.

transport.  "device": the buffer is all-reduced where it lies, on the group's backend (RCCL for an `nccl` group).  "host": the
buffer goes to a pinned host tensor, is all-reduced over a `gloo` group and comes back -- two ranks can then drive the real kernels on
ONE card, and CPU tensors work.  Its all-reduce is an all-gather followed by the sum in RANK ORDER on every rank: the result is
sum_r(g_r / world) added in rank order, bit for bit, for any number of ranks (gloo's own ring all-reduce adds in another order per
chunk from three ranks on).  It is a test and bring-up transport, not a fast one.  "auto": "device" for an `nccl` group, "host"
otherwise.

wide_gradients=True (off by default: nothing above changes).  A dense bf16 / fp16 parameter gets an fp32 slot of its element count
under the same alignment rule; `slot_layout` is the same function.  sync() packs with one launch per source dtype present -- `ops.mt_pack`
for the fp32 gradients, `ops.mt_pack_wide` (cvvae_mt_pack_wide: float(g) / world, widened exactly, divided in fp32) per 16-bit dtype --
and reduces the bucket once: the ranks are summed in fp32, the all-reduce moves 4 bytes instead of 2 per 16-bit parameter.  torch
refuses an fp32 `.grad` on a 16-bit parameter, so the averaged gradient of a 16-bit parameter is `p.main_grad` (the name Megatron and
Apex use), the slot's view in the parameter's shape, and `p.grad` becomes None, which frees the 16-bit gradient; a 16-bit parameter
without a gradient this iteration gets `main_grad = None` and a zeroed slot.  `cvvae_amd.optim.AdamW(master_weights=True)` reads
`main_grad` in place (cvvae_mt_adamw_master_wide); no other optimizer does.  A 16-bit gradient the kernel cannot take keeps the torch path.

bucket_bytes splits the buffer at slot boundaries into consecutive ranges, each all-reduced with async_op=True in order and all
waited for before sync() returns.  The default, None, is ONE range: RCCL has not been measured on this path, so there is no tuned
default to offer.  Overlapping the exchange with the backward is not attempted.

Agreement.  Which parameters have a gradient (and which path each takes) must be the same on every rank, or the replicas diverge
silently.  On the first `check_first` calls every rank takes part in one all_gather_object of that map; when the maps differ every
rank raises RuntimeError naming the first differing parameter index.  The check is counted by call number, so all ranks enter the
collective together.  After those calls sync() on the device transport does not synchronise with the host.
"""
from typing import List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import ops
from .optim import _MASTER_DTYPES, _kernel_tensor

__all__ = ["GradientSync", "slot_layout", "bucket_ranges", "all_reduce_sum", "broadcast", "world_size"]

ALIGN = 4  # elements: a slot starts on a 16-byte boundary


def slot_layout(numels: Sequence[int]) -> Tuple[List[int], int]:
    """-> (the slots' first elements, the buffer's length): list order, every start a multiple of ALIGN, an empty tensor an empty slot"""
    offsets, at = [], 0
    for n in numels:
        offsets.append(at)
        at += -(-int(n) // ALIGN) * ALIGN
    return offsets, at


def bucket_ranges(offsets: Sequence[int], total: int, bucket_bytes: Optional[int]) -> List[Tuple[int, int]]:
    """consecutive element ranges [a, b) that cover [0, total) and are cut at slot starts only: a range is closed before the slot that
    would take it past bucket_bytes (a slot larger than that is a range of its own).  None: one range"""
    if total == 0:
        return []
    if bucket_bytes is None:
        return [(0, total)]
    if int(bucket_bytes) <= 0:
        raise ValueError(f"bucket_bytes must be positive, got {bucket_bytes}")
    cap = max(int(bucket_bytes) // 4, 1)
    ends = list(offsets[1:]) + [total]
    out, a = [], 0
    for start, end in zip(offsets, ends):
        if start > a and end - a > cap:
            out.append((a, start))
            a = start
    out.append((a, total))
    return out


def world_size(group=None) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _on_device_backend(group) -> bool:
    """does the group's backend take device tensors where they lie (nccl = RCCL)?"""
    return dist.is_available() and dist.is_initialized() and str(dist.get_backend(group)).lower() == "nccl"


def all_reduce_sum(t: torch.Tensor, group=None) -> torch.Tensor:
    """t summed over the group, in place; a device tensor on a backend that takes none goes through the host.  Not for the hot path"""
    if world_size(group) == 1:
        return t
    if t.device.type == "cpu" or _on_device_backend(group):
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    else:
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        t.copy_(h)
    return t


def broadcast(t: torch.Tensor, group=None, src: int = 0) -> None:
    """rank `src` OF THE GROUP's values into t on every rank, in place (through the host where the backend takes no device tensors)"""
    if world_size(group) == 1:
        return
    src = dist.get_global_rank(group, src) if group is not None else src
    if t.device.type == "cpu" or _on_device_backend(group):
        dist.broadcast(t, src=src, group=group)
    else:
        h = t.cpu()
        dist.broadcast(h, src=src, group=group)
        t.copy_(h)


NONE, KERNEL, TORCH = 0, 1, 2  # the agreement map's entries


class GradientSync:
    def __init__(self, params, group=None, transport: str = "auto", bucket_bytes: Optional[int] = None, check_first: int = 4,
                 wide_gradients: bool = False):
        self.params: List[torch.Tensor] = list(params)
        if len({id(p) for p in self.params}) != len(self.params):
            raise ValueError("GradientSync: a parameter is listed twice")
        if transport not in ("auto", "device", "host"):
            raise ValueError(f"GradientSync: transport={transport!r}: 'auto', 'device' or 'host'")
        self.group = group
        self.world = world_size(group)
        if transport == "auto":
            transport = "device" if _on_device_backend(group) else "host"
        self.transport = transport
        self.check_first = int(check_first)
        self.calls = 0
        self.wide_gradients = bool(wide_gradients)
        self.slot_dtypes = (torch.float32,) + (_MASTER_DTYPES if self.wide_gradients else ())   # parameter dtypes that have a slot
        self.numels = [p.numel() if p.dtype in self.slot_dtypes else 0 for p in self.params]
        self.offsets, self.total = slot_layout(self.numels)
        self.ranges = bucket_ranges(self.offsets, self.total, bucket_bytes)
        self.flat: Optional[torch.Tensor] = None      # the bucket, made on the first sync() that has a gradient for the kernel
        self.slots: List[torch.Tensor] = []           # per parameter: its slot as a view of the parameter's shape
        self._mtl: Optional[ops.MultiTensorList] = None   # the fp32 gradients' pack list (a 16-bit parameter: no elements)
        self._wide: list = []                         # wide_gradients: (16-bit dtype, parameter indices, its pack list) per dtype present
        self._host: Optional[torch.Tensor] = None     # transport "host": the pinned staging buffer

    def layout(self) -> List[int]:
        """the first element of every parameter's slot in the flat buffer, in list order"""
        return list(self.offsets)

    # ---- the bucket ----
    def _make(self, device: torch.device) -> None:
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=device)   # the gaps are zero from here on
        self.slots = [self.flat[o:o + n].view(p.shape if p.dtype in self.slot_dtypes else (0,)) for p, o, n in zip(self.params, self.offsets, self.numels)]
        self._mtl = ops.MultiTensorList([n if p.dtype == torch.float32 else 0 for p, n in zip(self.params, self.numels)], device)
        by = [(dt, [i for i, p in enumerate(self.params) if p.dtype == dt]) for dt in self.slot_dtypes[1:]]
        self._wide = [(dt, sel, ops.MultiTensorList([self.numels[i] for i in sel], device, dt)) for dt, sel in by if sel]
        if self.transport == "host" and device.type != "cpu":
            self._host = torch.empty(self.total, dtype=torch.float32, pin_memory=True)

    def _takes(self, i: int, g: torch.Tensor) -> bool:
        p = self.params[i]
        return (self.numels[i] == g.numel() and g.shape == p.shape and p.dtype in self.slot_dtypes and _kernel_tensor(g, (p.dtype,))
                and (self.flat is None or g.device == self.flat.device))

    def _all_reduce(self, t: torch.Tensor, ranges) -> None:
        works = [dist.all_reduce(t[a:b], op=dist.ReduceOp.SUM, group=self.group, async_op=True) for a, b in ranges]
        for w in works:
            w.wait()

    def _exchange(self, t: torch.Tensor, ranges, staging: Optional[torch.Tensor] = None) -> None:
        """t <- its sum over the group, range by range"""
        if self.world == 1:
            return
        if self.transport == "device":
            self._all_reduce(t, ranges)
            return
        h = t
        if t.device.type != "cpu":
            h = staging if staging is not None else torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t)                  # (a blocking copy: the host reads it next)
        self._sum_in_rank_order(h, ranges)
        if h is not t:
            t.copy_(h, non_blocking=True)

    def _sum_in_rank_order(self, h: torch.Tensor, ranges) -> None:
        """the host transport's all-reduce: every rank gathers all ranks' buffers and adds them in rank order.  gloo's ring adds each
        chunk of a buffer in another rotation of the ranks, which from three ranks on is another fp32 sum per chunk (measured here:
        up to 2 ulp from the rank-order sum); this transport is the one the tests compare bit for bit, so it pays world x the
        buffer in host memory for a sum that is a function of the ranks' values alone"""
        rows = torch.empty((self.world,) + tuple(h.shape), dtype=h.dtype)
        works = [dist.all_gather([rows[r, a:b] for r in range(self.world)], h[a:b], group=self.group, async_op=True) for a, b in ranges]
        for w in works:
            w.wait()
        h.copy_(rows[0])
        for r in range(1, self.world):
            h.add_(rows[r])

    # ---- the agreement check ----
    def _check(self, codes: List[int]) -> None:
        mine = bytes(codes)
        maps = [None] * self.world
        dist.all_gather_object(maps, mine, group=self.group)
        if all(m == maps[0] for m in maps):
            return
        k = next(i for i in range(max(len(m) for m in maps))
                 if len({m[i] if i < len(m) else -1 for m in maps}) > 1)
        names = {NONE: "no gradient", KERNEL: "a gradient for the pack kernel", TORCH: "a gradient for the torch path", -1: "no such parameter"}
        raise RuntimeError(
            f"GradientSync: the ranks disagree about parameter {k} (call {self.calls}): "
            + ", ".join(f"rank {r}: {names[m[k] if k < len(m) else -1]}" for r, m in enumerate(maps))
            + "; every rank must produce gradients for the same parameters, or the replicas diverge")

    # ---- one exchange ----
    @torch.no_grad()
    def sync(self) -> None:
        self.calls += 1
        grads = [p.grad for p in self.params]
        if self.flat is None:
            first = next((g for i, g in enumerate(grads) if g is not None and self._takes(i, g)), None)
            if first is not None and self.total:
                self._make(first.device)
        codes = [NONE if g is None else (KERNEL if self.flat is not None and self._takes(i, g) else TORCH) for i, g in enumerate(grads)]
        if self.world > 1 and self.calls <= self.check_first:
            self._check(codes)
        if self.flat is not None:
            # every call packs every slot (zeros where there is no gradient for the kernel): the buffer's content never depends on an
            # earlier iteration, and all ranks reduce the same ranges whatever their maps were
            if self._mtl.n_chunks:              # (none: a list of 16-bit parameters alone under wide_gradients)
                fp32 = [p.dtype == torch.float32 for p in self.params]
                mtl = self._mtl.set(g=[g if c == KERNEL and f else None for g, c, f in zip(grads, codes, fp32)], shadow=self.slots)
                ops.mt_pack(mtl, float(self.world))
                mtl.release("g")
            for dt, sel, mtl in self._wide:     # one more launch per 16-bit dtype present: float(g) / world into the fp32 slots
                mtl.set(g=[grads[i] if codes[i] == KERNEL else None for i in sel], shadow=[self.slots[i] for i in sel])
                ops.mt_pack_wide(mtl, float(self.world))
                mtl.release("g")
            self._exchange(self.flat, self.ranges, self._host)
            for p, c, s in zip(self.params, codes, self.slots):
                if p.dtype == torch.float32:
                    if c == KERNEL:
                        p.grad = s
                elif self.wide_gradients and p.dtype in _MASTER_DTYPES:
                    # an fp32 .grad on a 16-bit parameter is refused by torch: the slot is `main_grad`, the 16-bit gradient is freed
                    p.main_grad = s if c == KERNEL else None
                    if c == KERNEL:
                        p.grad = None
        elif self.wide_gradients:
            for p in self.params:      # no bucket yet (no gradient for the kernels so far): nothing stale may stay
                if p.dtype in _MASTER_DTYPES:
                    p.main_grad = None
        rest = {}
        for g, c in zip(grads, codes):
            if c == TORCH:
                rest.setdefault((g.dtype, g.device), []).append(g)
        for gs in rest.values():
            flat = torch.cat([g.reshape(-1) for g in gs])
            flat.div_(self.world)
            self._exchange(flat, [(0, flat.numel())])
            for g, part in zip(gs, flat.split([g.numel() for g in gs])):
                g.copy_(part.view(g.shape))
