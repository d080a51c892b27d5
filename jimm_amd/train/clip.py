"""Global-norm gradient clipping (optax.clip_by_global_norm /
torch.nn.utils.clip_grad_norm_ semantics).

On GPU the norm is a two-stage multi-tensor reduction over the same chunk
descriptors the fused Adam uses (csrc/adam.hip): one fp32 partial per 65536-
element chunk, then one block that adds every partial in fp64 and writes the
device stats buffer ``[norm, coef, finite, skipped]``. Nothing comes back to the
host, so the whole thing captures into a hipGraph. The plain-torch path below
is the numerics oracle.
"""

from __future__ import annotations

from typing import Iterable

import torch

from jimm_amd.ops import _backend

STATS_LEN = 4  # [pre-clip norm, coef, finite flag, skipped-step count]


def ref_clip_coef(gs: list[torch.Tensor], max_norm: float) -> tuple[torch.Tensor, torch.Tensor]:
    """Oracle: per-tensor fp32 L2 norms, combined; coef = min(1, c / (norm + 1e-6)).

    Returns 0-d fp32 tensors (norm, coef). A non-finite norm leaves coef
    unclamped (0 for inf, NaN for NaN), as torch's clip_grad_norm_ does."""
    # each per-tensor norm is an fp32 number, but summed in fp64: torch's fp32
    # accumulation is up to 1e-6 off over 1e5 elements, which is more than the
    # device reduction (fp64 over the chunk partials) that this is the oracle for
    norms = [torch.linalg.vector_norm(g, dtype=torch.float64).float() for g in gs]
    norm = torch.linalg.vector_norm(torch.stack(norms), dtype=torch.float64).float()
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return norm, coef


# descriptor table of the latest gradient list, keyed by its storage: repeated
# calls on the same buffers (the usual training loop) do no host work
_cache: dict = {}


def _device_tables(gs: list[torch.Tensor]):
    key = tuple((g.data_ptr(), g.numel(), g.dtype) for g in gs)
    if _cache.get("key") != key:
        ext = _backend.ext()
        desc, nchunks = ext.grad_desc_prepare(gs)
        n = int(nchunks.item())
        _cache.clear()
        _cache.update(
            key=key,
            desc=desc,
            nchunks=n,
            partials=torch.zeros(n, dtype=torch.float32, device=gs[0].device),
            stats=torch.zeros(STATS_LEN, dtype=torch.float32, device=gs[0].device),
        )
    return _cache["desc"], _cache["nchunks"], _cache["partials"], _cache["stats"]


@torch.no_grad()
def clip_grad_norm_(parameters: torch.Tensor | Iterable[torch.Tensor], max_norm: float) -> torch.Tensor:
    """Scale the gradients of ``parameters`` in place so that their global L2
    norm is at most ``max_norm``; return the pre-clip norm as a 0-d fp32 tensor
    on the gradients' device (no host sync).

    For users who bring their own optimizer; ``Adam(max_grad_norm=...)`` folds
    the scale into the update instead and never rewrites the gradients."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    gs = [p.grad for p in parameters if p.grad is not None]
    if not gs:
        return torch.zeros((), dtype=torch.float32)
    if gs[0].is_cuda and not _backend.force_eager():
        ext = _backend.ext()
        desc, nchunks, partials, stats = _device_tables(gs)
        ext.grad_sqnorm(desc, nchunks, partials, 0)
        ext.clip_finalize(partials, stats, float(max_norm))
        ext.grad_scale(desc, nchunks, stats)
        return stats[0].clone()
    norm, coef = ref_clip_coef(gs, float(max_norm))
    for g in gs:
        g.mul_(coef)
    return norm
