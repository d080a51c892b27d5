"""Counter-based dropout: the keep decision is a pure function of
``(seed, step, site, row, column)``.

No mask is ever stored. The forward computes it in registers (the standalone
kernel in csrc/elementwise.hip, or the fc1 / fc2 epilogues of the 8-phase
GEMM), the backward and a checkpoint recompute regenerate it, and a captured
graph advances it through one device-side integer.

Definition (every layer and every test agrees on it):

* Generator: Philox4x32, 10 rounds, the standard constants.
* A tensor is rows x columns ``(m, n)``, leading dimensions flattened into
  ``m``. Element ``(m, n)`` takes
  counter ``{m >> 1, (n >> 6) * 16 + (n & 15), site, step & 0xffffffff}``,
  key ``{seed & 0xffffffff, seed >> 32}``, output word ``(n >> 4) & 3`` and of
  that word the low 16 bits for even ``m``, the high 16 bits for odd ``m``:
  ``u``.
* ``t = round(p * 65536)``; keep iff ``u >= t``; kept values are multiplied by
  ``s = float32(65536 / (65536 - t))``, the exact inverse of the keep rate.

The functions in this file that take plain integers are the CPU reference:
they are the CPU path of :func:`dropout` and the oracle of the GPU tests.

State: one int64[2] tensor ``{seed, step}`` per device. Kernels read both
values through its pointer, so a captured graph never bakes them in;
:func:`next_dropout_rng` hands out a 16-byte snapshot and advances ``step``
with an in-stream add.
"""

from __future__ import annotations

import math

import torch

from jimm_amd.ops import _backend

_MASK32 = 0xFFFFFFFF
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85


def _mulhilo(a: int, b: torch.Tensor):
    """(hi, lo) 32-bit halves of a * b for a 32-bit constant a and an int64
    tensor b of 32-bit values, in 16-bit limbs so no int64 product overflows."""
    lo16 = a * (b & 0xFFFF)   # < 2^48
    hi16 = a * (b >> 16)      # < 2^48
    lo = (lo16 + ((hi16 & 0xFFFF) << 16)) & _MASK32
    hi = (hi16 + (lo16 >> 16)) >> 16
    return hi, lo


def philox4x32(counter, key):
    """Philox4x32-10. counter: 4 int64 tensors (or ints) of 32-bit values,
    key: 2 ints. Returns the 4 output words as int64 tensors."""
    c0, c1, c2, c3 = (torch.as_tensor(c, dtype=torch.int64) & _MASK32 for c in counter)
    k0, k1 = int(key[0]) & _MASK32, int(key[1]) & _MASK32
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return c0, c1, c2, c3


def dropout_threshold(p: float) -> int:
    """t = round(p * 65536), halves up (the kernels' host code does the same)."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    return min(int(math.floor(p * 65536.0 + 0.5)), 65535)


def dropout_scale(t: int) -> float:
    """float32(65536 / (65536 - t)) as a Python float."""
    return torch.tensor(65536.0 / (65536.0 - t), dtype=torch.float32).item()


def dropout_u(rows: int, cols: int, seed: int, step: int, site: int,
              device: torch.device | str = "cpu") -> torch.Tensor:
    """The 16-bit uniforms u(m, n) of a rows x cols tensor, int64."""
    m = torch.arange(rows, dtype=torch.int64, device=device).view(-1, 1)
    n = torch.arange(cols, dtype=torch.int64, device=device).view(1, -1)
    c0 = (m >> 1).expand(rows, cols)
    c1 = ((n >> 6) * 16 + (n & 15)).expand(rows, cols)
    c2 = torch.full((), int(site) & _MASK32, dtype=torch.int64, device=device)
    c3 = torch.full((), int(step) & _MASK32, dtype=torch.int64, device=device)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = philox4x32((c0, c1, c2, c3), (seed & _MASK32, seed >> 32))
    word = ((n >> 4) & 3).expand(rows, cols)
    w = torch.where(word == 0, out[0], torch.where(word == 1, out[1],
                    torch.where(word == 2, out[2], out[3])))
    return torch.where((m & 1) == 1, w >> 16, w & 0xFFFF)


def keep_mask(rows: int, cols: int, p: float, seed: int, step: int, site: int,
              device: torch.device | str = "cpu") -> torch.Tensor:
    """bool (rows, cols): True where the element is kept."""
    return dropout_u(rows, cols, seed, step, site, device) >= dropout_threshold(p)


def _dropout_ref(x: torch.Tensor, p: float, rng: torch.Tensor, site: int) -> torch.Tensor:
    seed, step = rng.tolist()
    x2 = x.reshape(-1, x.shape[-1])
    keep = keep_mask(x2.shape[0], x2.shape[1], p, seed, step, site, x.device)
    s = dropout_scale(dropout_threshold(p))
    ref_dtype = torch.float64 if x.dtype == torch.float64 else torch.float32
    y = torch.where(keep, x2.to(ref_dtype) * s, torch.zeros((), dtype=ref_dtype, device=x.device))
    return y.to(x.dtype).view(x.shape)


class _DropoutFn(torch.autograd.Function):
    """y = x * mask * s; the backward is the same map applied to dy."""

    @staticmethod
    def forward(ctx, x, p, rng, site):
        ctx.save_for_backward(rng)
        ctx.p, ctx.site = p, site
        return _apply(x, p, rng, site)

    @staticmethod
    def backward(ctx, dy):
        (rng,) = ctx.saved_tensors
        return _apply(dy, ctx.p, rng, ctx.site), None, None, None


def _apply(x: torch.Tensor, p: float, rng: torch.Tensor, site: int) -> torch.Tensor:
    if _backend.use_hip(x):
        x2 = x.contiguous().view(-1, x.shape[-1])
        return _backend.ext().dropout_fwd(x2, p, rng, site).view(x.shape)
    return _dropout_ref(x, p, rng, site)


def dropout(x: torch.Tensor, p: float, rng: torch.Tensor | None, site: int = 0) -> torch.Tensor:
    """Dropout of ``x`` (rows = all leading dimensions, columns = the last) at
    ``site`` under the ``{seed, step}`` snapshot ``rng``. ``p`` that rounds to
    a zero threshold returns ``x`` itself."""
    if dropout_threshold(p) == 0:
        return x
    if rng is None:
        raise ValueError("dropout with p > 0 needs an rng snapshot (next_dropout_rng)")
    return _DropoutFn.apply(x, p, rng, site)


# ---------------------------------------------------------------------------
# per-device {seed, step}
# ---------------------------------------------------------------------------

_SEED = 0
_STATES: dict[torch.device, torch.Tensor] = {}


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def dropout_state(device) -> torch.Tensor:
    """The live int64[2] ``{seed, step}`` tensor of ``device`` (created at
    step 0 with the current seed). It is updated in place only, so a captured
    graph keeps pointing at it."""
    device = _device(device)
    st = _STATES.get(device)
    if st is None:
        st = torch.tensor([_SEED, 0], dtype=torch.int64, device=device)
        _STATES[device] = st
    return st


def set_dropout_seed(seed: int) -> None:
    """Seed every device's dropout state and restart its step count at 0."""
    global _SEED
    _SEED = int(seed) & 0x7FFFFFFFFFFFFFFF
    for st in _STATES.values():
        st.copy_(torch.tensor([_SEED, 0], dtype=torch.int64))


def get_dropout_state(device) -> tuple[int, int]:
    """``(seed, step)`` of ``device`` as Python ints (synchronises)."""
    seed, step = dropout_state(device).tolist()
    return seed, step


def set_dropout_state(device, seed: int, step: int) -> None:
    """Overwrite ``{seed, step}`` of ``device`` in place (checkpoint restore)."""
    dropout_state(device).copy_(torch.tensor([int(seed), int(step)], dtype=torch.int64))


def next_dropout_rng(device) -> torch.Tensor:
    """Snapshot ``{seed, step}`` for one forward pass and advance ``step``.
    Both are in-stream device operations, so they capture into a graph and
    every replay sees the next step."""
    st = dropout_state(device)
    snap = st.clone()
    st[1:].add_(1)
    return snap


__all__ = [
    "dropout",
    "dropout_state",
    "dropout_threshold",
    "dropout_scale",
    "dropout_u",
    "get_dropout_state",
    "keep_mask",
    "next_dropout_rng",
    "philox4x32",
    "set_dropout_seed",
    "set_dropout_state",
]
