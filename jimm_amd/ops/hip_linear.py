"""GPU linear / patch-embed path, and the GEMM engine layer the fused encoder
block (ops/block.py) shares with it.

Two engines run a GEMM:
  * the in-house MFMA bf16 kernels: forward and dX on the NT kernels behind
    ``ext.linear_fwd`` (the 8-phase 256-tile kernel of csrc/gemm8p.hip where
    N % 256 == 0, K % 64 == 0 and K >= 128, else the 128-tile kernels of
    csrc/gemm.hip for any K % 64 == 0), with the bias / activation / residual /
    dropout epilogues and the activation backward fused into the GEMM; where
    none of those takes a shape that ran on rocBLAS so far (dX and fc2-dX off
    the 8-phase grid, a forward with K % 64 != 0, the fused block at widths
    off the 256 grid), the 128-tile NT kernel of csrc/gemm_nt128.hip for any
    N % 8 == 0, K % 8 == 0 with M >= 256 and K <= 576 (``_nt128_ok``); what
    that leaves, the ragged form of the 8-phase kernel (gemm_nt_8p_ragged:
    any N % 8 == 0, K % 8 == 0, K >= 128) with M >= 32768 and N filling at
    least 98% of its 256-wide tile columns (``_nt8pr_ok``: so400m's fc1 and
    fc2-dX, 8% ahead of rocBLAS + its epilogue pass as a pair at M = 46656;
    every other so400m site measured level or behind and stays on rocBLAS,
    profiles/nt_ragged_NOTES.md); dW on
    the split-M TN kernels (fp32 accumulate), which can fold the bias
    gradient out of their operands: the 256-tile kernel of csrc/gemm_tn8p.hip
    where N % 256 == 0 and K % 256 == 0, else the 128-tile kernel of
    csrc/gemm_tn128.hip for any N % 8 == 0, K % 8 == 0 with M >= 256 and at
    most 162 output tiles of 128 x 128, 243 with the bias fold (ViT-S,
    so400m's proj and qkv, class heads); beyond those caps the ragged form
    of the 256-tile kernel (gemm_tn_8p_ragged) with M >= 16384 where N x K
    fills 89% of its 256 x 256 tiles and N 98% of its tile rows (``_tn8pr_ok``:
    so400m's fc1; fc2 and qkv without a bias gradient measured level with
    rocBLAS and stay there, profiles/dw_ragged_NOTES.md; JIMM_AMD_DW_RAGGED=1
    sends every off-grid dW to it, 0 none); every other dW goes to
    torch.matmul;
  * hipBLASLt/rocBLAS through torch (with the committed MI355X TunableOp
    table) + the separate fused bias+act(+residual) elementwise kernel.

How an engine runs a GEMM is written once, in ``gemm_fwd`` / ``gemm_dx`` /
``gemm_dx_act`` / ``gemm_dw_db`` below. Which engine runs is each call site's
own rule: ``JIMM_AMD_GEMM`` (``hip``, the default, or ``blas``; read by
``_gemm_mode`` alone) and the shape predicates of the extension.
``gemm_fwd`` and ``gemm_dx_act`` take the caller's choice as ``hip=``;
``gemm_dx`` and ``gemm_dw_db`` gate per shape themselves.

fp8 (``jimm_amd.ops.set_fp8(True)``): e4m3 scaled_mm forward GEMMs with
per-tensor dynamic device-side scales (graph-capturable); the backward GEMMs,
LN and losses stay bf16/fp32. The fused block has its own producer-fused
fp8 arm (ops/block.py). ``set_fp8(True, gemm="hip")`` (or
``JIMM_AMD_FP8_GEMM=hip``; default ``blas``) runs those e4m3 GEMMs on the
in-house 16x16x128 MFMA kernel (csrc/gemm8p_f8.hip) with the bias /
activation / residual / e4m3-emission epilogues fused in, where
``ext.gemm_f8_supported`` takes the shape (``gemm_fwd_f8`` below).
"""

from __future__ import annotations

import os

import torch

from jimm_amd.ops import _backend


# ---------------------------------------------------------------------------
# fp8 forward path (BASELINE config 5): per-tensor dynamic-scaled e4m3 GEMM
# via torch._scaled_mm (hipBLASLt fp8 MFMA — measured 1.4-3.0 PF/s on the
# model shapes, benchmarks/fp8_probe.py, vs ~1.0 PF/s bf16). Backward stays
# bf16 (dX/dW GEMMs on the saved bf16 activations); LN/softmax/losses are
# bf16/fp32 throughout. Enable with jimm_amd.ops.set_fp8(True).
# ---------------------------------------------------------------------------

_FP8_STATE = {"enabled": False, "gemm": None}
_FP8_MAX = 448.0  # e4m3 (OCP) max normal


def set_fp8(on: bool = True, gemm: str | None = None) -> None:
    """Switch the e4m3 forward path. gemm: the engine of its GEMMs, "blas"
    (torch._scaled_mm + separate epilogue passes) or "hip" (the in-house e4m3
    MFMA kernel, epilogues fused); None leaves the choice to
    JIMM_AMD_FP8_GEMM (default blas)."""
    if gemm not in (None, "blas", "hip"):
        raise ValueError(f"set_fp8: gemm must be 'blas' or 'hip', got {gemm!r}")
    _FP8_STATE["enabled"] = bool(on)
    _FP8_STATE["gemm"] = gemm


def fp8_enabled() -> bool:
    return _FP8_STATE["enabled"]


def _fp8_ok(x2: torch.Tensor, w: torch.Tensor) -> bool:
    # _scaled_mm needs K % 16 == 0 and fp8-capable torch; bf16 inputs only
    return (
        x2.dtype == torch.bfloat16
        and x2.shape[1] % 16 == 0
        and w.shape[0] % 16 == 0
        and hasattr(torch, "_scaled_mm")
    )


def _quant_e4m3(t: torch.Tensor, transpose: bool = False):
    """Per-tensor e4m3 copy of t and its scale. transpose: the bytes of t^T,
    row-major — the column-major b operand a scaled_mm dX GEMM (dz @ W) needs
    is the .t() view of that."""
    scale = (t.abs().amax().float() / _FP8_MAX).clamp(min=1e-12)
    t8 = (t * scale.reciprocal().to(t.dtype)).to(torch.float8_e4m3fn)
    return (t8.t().contiguous() if transpose else t8), scale


def _gemm_nt_fp8(x2: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    x8, sx = _quant_e4m3(x2)
    w8, sw = _quant_e4m3(w)
    return torch._scaled_mm(
        x8, w8.t(), scale_a=sx.view(1, 1), scale_b=sw.view(1, 1), out_dtype=torch.bfloat16
    )


def _gemm_mode() -> str:
    # "hip" (default): the in-house MFMA GEMMs with fused epilogues;
    # JIMM_AMD_GEMM=blas: hipBLASLt/rocBLAS + separate elementwise passes.
    return os.environ.get("JIMM_AMD_GEMM", "hip")


def _fp8_gemm_mode() -> str:
    # engine of the e4m3 GEMMs under set_fp8: its gemm= argument, else
    # JIMM_AMD_FP8_GEMM ("blas", the default, or "hip").
    return _FP8_STATE["gemm"] or os.environ.get("JIMM_AMD_FP8_GEMM", "blas")


def _deterministic() -> bool:
    return os.environ.get("JIMM_AMD_DETERMINISTIC", "0") == "1"


# ---------------------------------------------------------------------------
# GEMM engine layer
# ---------------------------------------------------------------------------


# Fewest rows at which a forward / dX GEMM off the 8-phase grid goes to the
# 128-tile NT kernel (csrc/gemm_nt128.hip). At the floor itself the call is
# two row tiles and launch-bound: (256 | 1024, 1152, 384) and (256, 384, 384)
# measured 0.010 ms against addmm's 0.021. Below it the traces the route
# tests pin at M = 80 and M = 8 stay as they are; not measured there.
_NT128_MIN_M = 256
# Longest contraction at which it does. Its K loop runs at 0.55-0.75 PF/s
# where rocBLAS reaches 0.8-1.15, and what it saves is the separate epilogue
# pass and rocBLAS's weaker short-K tiles: at M = 201728 / 46656 every site
# with K <= 576 measured level or ahead (up to 1.45x) and every site with
# K >= 768 but one behind (1.03-1.68x the time), under either staging design
# that was built; profiles/nt_offgrid_NOTES.md.
_NT128_MAX_K = 576


def nt128_rows_k_ok(M: int, K: int) -> bool:
    """The two routing conditions above, and nothing under set_fp8(True):
    every route of that mode stays what it was."""
    return M >= _NT128_MIN_M and K <= _NT128_MAX_K and not _FP8_STATE["enabled"]


def _nt128_ok(ext, x2: torch.Tensor, w: torch.Tensor | None, N: int) -> bool:
    """Whether x2 (M, K) @ w (N, K)^T may run the 128-tile NT kernel: its
    domain (N and K multiples of 8, contiguous 16-byte-aligned bf16 operands)
    and the routing conditions of nt128_rows_k_ok. w is None where the
    caller is about to make the weight operand itself (the transposed copy
    of a dX GEMM)."""
    M, K = x2.shape
    return (
        nt128_rows_k_ok(M, K)
        and x2.dtype == torch.bfloat16
        and ext.gemm_nt_128_supported(M, N, K)
        and x2.is_contiguous()
        and x2.data_ptr() % 16 == 0
        and (w is None or (w.dtype == torch.bfloat16 and w.is_contiguous()
                           and w.data_ptr() % 16 == 0))
    )


# Fewest rows at which a forward / dX GEMM that neither the 8-phase grid kernel
# nor the 128-tile NT kernel takes goes to the ragged 8-phase kernel
# (gemm_nt_8p_ragged, csrc/gemm8p.hip). The fc1 ladder of
# profiles/nt_ragged_NOTES.md is behind rocBLAS up to 8192 rows and the routed
# pair (below) level at 16384 and ahead from 32768.
_NT8PR_MIN_M = 32768
# Least share of its ceil(N / 256) tile columns that N must fill. The partial
# last n-tile costs a whole tile's time: at N = 1152 (5 tile columns for 4.5
# tiles of work, 90%) and 3456 (96%) the kernel measured level with or behind
# rocBLAS at one or more of M = 16384 / 46656 / 65536, at N = 4304 (98.9%:
# so400m's fc1 and, with the saved derivative, fc2-dX) ahead as a pair at
# 46656 and 65536; same notes.
_NT8PR_MIN_FILL = 0.98


def nt8pr_rows_ok(M: int) -> bool:
    """The row floor, and nothing under set_fp8(True)."""
    return M >= _NT8PR_MIN_M and not _FP8_STATE["enabled"]


def _nt8pr_ok(ext, x2: torch.Tensor, w: torch.Tensor | None, N: int) -> bool:
    """Whether x2 (M, K) @ w (N, K)^T may run the ragged 8-phase kernel: its
    domain (N and K multiples of 8, K >= 128, contiguous 16-byte-aligned bf16
    operands) and the measured rule above (row floor, n-tile fill). w is None where the caller is about
    to make the weight operand itself (the transposed copy of a dX GEMM).
    Callers ask the 8-phase grid kernel and the 128-tile kernel first."""
    M, K = x2.shape
    return (
        nt8pr_rows_ok(M)
        and N >= _NT8PR_MIN_FILL * 256 * -(-N // 256)
        and x2.dtype == torch.bfloat16
        and ext.gemm_nt_8p_ragged_supported(M, N, K)
        and x2.is_contiguous()
        and x2.data_ptr() % 16 == 0
        and (w is None or (w.dtype == torch.bfloat16 and w.is_contiguous()
                           and w.data_ptr() % 16 == 0))
    )


_SAVE_NAMES = {None: "none", "z": "pre", "g": "grad"}


def gemm_fwd(ext, x2, w, b, act, res2, *, hip: bool, save=None, drop=None, nt128: bool = False):
    """y = act(x2 @ w^T + b) [+ res2] -> (y, saved). save: None, "z" (the
    bf16 pre-activation) or "g" (the fp16 derivative act'(pre), in-house
    engine only). drop = (p, rng, site): dropout fused into the in-house
    epilogue. hip is the caller's engine choice; with nt128 a shape the
    8-phase kernel does not take runs the 128-tile NT kernel (no dropout
    form) where _nt128_ok admits it, then the ragged 8-phase kernel (none
    either) where _nt8pr_ok does, and rocBLAS otherwise, instead of the
    kernels behind linear_fwd."""
    act = act or ""
    if hip and nt128 and not ext.gemm8p_supported(x2.shape[0], w.shape[0], w.shape[1]):
        if drop is None and _nt128_ok(ext, x2, w, w.shape[0]):
            return tuple(ext.gemm_nt_128(x2, w, b, act, res2, _SAVE_NAMES[save]))
        if drop is None and _nt8pr_ok(ext, x2, w, w.shape[0]):
            return tuple(ext.gemm_nt_8p_ragged(x2, w, b, act, res2, _SAVE_NAMES[save]))
        hip = False
    if hip:
        drop = drop or ()
        if save == "g":
            y, saved = ext.linear_fwd_actgrad(x2, w, b, act, res2, *drop)
        else:
            y, saved = ext.linear_fwd(x2, w, b, act, res2, save == "z", *drop)
        return y, saved
    if save == "g" or drop is not None:
        raise RuntimeError("gemm_fwd: the saved derivative and fused dropout need the HIP GEMMs")
    if not act and res2 is None and b is not None:
        # bias-only: hipBLASLt fuses the bias epilogue into the GEMM —
        # no separate full-tensor bias pass
        return torch.addmm(b, x2, w.t()), None
    z = torch.matmul(x2, w.t())
    # fused bias+act(+residual): z is updated in place to hold the
    # pre-activation (z+bias); y aliases z when there is no act.
    y = ext.bias_act_fwd(z, b, act, res2)
    return y, (z if save else None)


def fp8_hip(ext, M: int, N: int, K: int) -> bool:
    """True when an (M, K) x (N, K)^T e4m3 GEMM runs on the in-house kernel."""
    return _fp8_gemm_mode() == "hip" and ext.gemm_f8_supported(M, N, K)


def gemm_fwd_f8(ext, a8, sa, w8, sw, b=None, act=None, res2=None, scale_out=None, amax_out=None):
    """y = act((sa*sw) * a8 @ w8^T + b) [+ res2] on e4m3 bytes with device
    scales, one launch of the in-house e4m3 kernel -> (y, z, y8): z the bf16
    pre-activation (saved exactly when there is an activation), y8 the e4m3
    copy of y under scale_out with its amax folded into amax_out (fc1 form:
    activation + bias, no residual). The caller has checked fp8_hip."""
    return ext.linear_fwd_f8(a8, sa, w8, sw, b, act or "", res2, bool(act), scale_out, amax_out)


def gemm_dx(ext, dz: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dX = dz @ w — in-house NT kernel on a pre-transposed weight copy.

    (Per-call-quantized fp8 dX was measured NET-NEGATIVE at config 5: the
    w.t().contiguous() + two quantization passes cost more than the fp8
    GEMM saves. The fused-block path instead runs fc1-dX on fp8 with a
    producer-emitted e4m3 operand — see ops/block.py.)"""
    if _gemm_mode() == "hip" and dz.dtype == torch.bfloat16:
        if ext.gemm8p_supported(dz.shape[0], w.shape[1], w.shape[0]):
            wt = w.t().contiguous()
            y, _ = ext.linear_fwd(dz, wt, None, "", None, False)
            return y
        # off the 8-phase grid: the 128-tile NT kernel
        if w.dtype == torch.bfloat16 and _nt128_ok(ext, dz, None, w.shape[1]):
            return ext.gemm_nt_128(dz, w.t().contiguous())[0]
        # neither: the ragged 8-phase kernel, where its measured rule admits
        if w.dtype == torch.bfloat16 and _nt8pr_ok(ext, dz, None, w.shape[1]):
            return ext.gemm_nt_8p_ragged(dz, w.t().contiguous())[0]
    return torch.matmul(dz, w)


def gemm_dx_act(ext, dy2, w, saved, act, *, hip: bool) -> torch.Tensor:
    """dz = (dy2 @ w) * act'(pre), the dX of an activated linear, from what
    its forward saved: the fp16 derivative (one multiply in the epilogue), or
    the bf16 pre-activation — the derivative recomputed in the epilogue where
    the caller's engine is the in-house one (hip) and the 8-phase, the
    128-tile NT or the ragged 8-phase kernel takes the shape (asked in that
    order), else rocBLAS + a separate act_bwd pass."""
    p8 = ext.gemm8p_supported(dy2.shape[0], w.shape[1], w.shape[0])
    nt128 = not p8 and w.dtype == torch.bfloat16 and _nt128_ok(ext, dy2, None, w.shape[1])
    nt8pr = (not p8 and not nt128 and w.dtype == torch.bfloat16
             and _nt8pr_ok(ext, dy2, None, w.shape[1]))
    if saved.dtype == torch.float16:
        # the forward saved the derivative because one of the three takes
        # this shape (the same (M, N, K) as fc1 itself)
        gradmul = (ext.gemm_nt_8p_gradmul if p8 else
                   ext.gemm_nt_8p_ragged_gradmul if nt8pr else ext.gemm_nt_128_gradmul)
        return gradmul(dy2, w.t().contiguous(), saved)
    if hip and p8:
        return ext.gemm_nt_8p_gradact(dy2, w.t().contiguous(), saved, act)
    if hip and nt128:
        return ext.gemm_nt_128_gradact(dy2, w.t().contiguous(), saved, act)
    if hip and nt8pr:
        return ext.gemm_nt_8p_ragged_gradact(dy2, w.t().contiguous(), saved, act)
    return ext.act_bwd(torch.matmul(dy2, w), saved, act)


def _colsum(ext, dz: torch.Tensor) -> torch.Tensor:
    """The bias gradient on its own: one fp32-accumulating pass over dz."""
    if dz.is_cuda and dz.shape[-1] % 8 == 0:
        return ext.colsum(dz).to(dz.dtype)
    return dz.sum(dim=0)


# Fewest rows at which an off-grid dW goes to the 128-tile TN kernel: below
# four 64-row m-steps the call is launch-bound on either engine.
_TN128_MIN_M = 256
# Most 128x128 output tiles at which it does: with more, rocBLAS fills the
# device with larger tiles and is ahead (measured crossover at M = 46656:
# between 162 and 192 tiles for dW alone, beyond 243 and before 306 with the
# bias fold, which saves the separate colsum pass;
# profiles/dw_offgrid_NOTES.md).
_TN128_MAX_TILES = 162
_TN128_MAX_TILES_DB = 243


def _tn128_ok(ext, dz, x2, fold: bool) -> bool:
    """Whether an off-grid dW runs the 128-tile TN kernel: its domain (N and
    K multiples of 8, contiguous 16-byte-aligned bf16 operands) and the two
    routing conditions above. fold: the call will use the bias fold."""
    M, N, K = dz.shape[0], dz.shape[1], x2.shape[1]
    return (
        M >= _TN128_MIN_M
        and ext.gemm_tn_128_supported(M, N, K)
        and -(-N // 128) * -(-K // 128) <= (_TN128_MAX_TILES_DB if fold else _TN128_MAX_TILES)
        and x2.dtype == torch.bfloat16
        and dz.is_contiguous()
        and x2.is_contiguous()
        and dz.data_ptr() % 16 == 0
        and x2.data_ptr() % 16 == 0
    )


def _dw_ragged_mode() -> str:
    # JIMM_AMD_DW_RAGGED: "1" sends every off-grid dW in the domain of the
    # ragged 256-tile TN kernel to it, "0" none; unset: the measured rule of
    # _tn8pr_ok.
    return os.environ.get("JIMM_AMD_DW_RAGGED", "")


# The ragged 256-tile TN kernel (gemm_tn_8p_ragged, csrc/gemm_tn8p.hip) by
# default, among the shapes beyond the 128-tile kernel's tile caps (which ran
# torch.matmul so far): the fewest rows, the least share of its
# ceil(N/256) x ceil(K/256) output tiles that N x K must fill, and the least
# share of its ceil(N/256) tile rows that N must. Of so400m's sites beyond the
# caps, fc1 (4304 x 1152: 89% of 85 tiles, N 98.9%) took 5-14% less time
# than rocBLAS (dW + db: 4-18% less than rocBLAS + colsum) at M = 46656 and
# 65536 and about half its time at 16384, beyond the spread in both runs;
# fc2 (1152 x 4304: the same 89%, N 90%) was level or behind with db at
# 46656, and qkv without db (3456 x 1152, 87%) behind at 16384 and level at
# 65536 in one run: both stay on rocBLAS.
# benchmarks/dw_ragged_bench.py; profiles/dw_ragged_NOTES.md.
_TN8PR_MIN_M = 16384
_TN8PR_MIN_FILL = 0.89
_TN8PR_MIN_FILL_N = 0.98


def _tn8pr_ok(ext, dz, x2, fold: bool, forced: bool) -> bool:
    """Whether an off-grid dW runs the ragged 256-tile TN kernel: its domain
    (N and K multiples of 8, contiguous 16-byte-aligned bf16 operands), nothing
    under set_fp8(True), and either JIMM_AMD_DW_RAGGED=1 (forced) or the
    measured rule: what the 128-tile kernel's row floor admits and its tile
    caps decline, at or above the row floor and the fill above. fold: the call
    will use the bias fold."""
    M, N, K = dz.shape[0], dz.shape[1], x2.shape[1]
    if not (
        not _FP8_STATE["enabled"]
        and ext.gemm_tn8p_ragged_supported(M, N, K)
        and x2.dtype == torch.bfloat16
        and dz.is_contiguous()
        and x2.is_contiguous()
        and dz.data_ptr() % 16 == 0
        and x2.data_ptr() % 16 == 0
    ):
        return False
    return forced or (
        M >= max(_TN128_MIN_M, _TN8PR_MIN_M)
        and -(-N // 128) * -(-K // 128) > (_TN128_MAX_TILES_DB if fold else _TN128_MAX_TILES)
        and N * K >= _TN8PR_MIN_FILL * 65536 * -(-N // 256) * -(-K // 256)
        and N >= _TN8PR_MIN_FILL_N * 256 * -(-N // 256)
    )


def gemm_dw_db(ext, dz, x2, out_dtype, need_dw: bool = True, need_db: bool = True):
    """(dW = dz^T @ x2 | None, db = colsum(dz) | None). The in-house split-M
    TN kernels (fp32 accumulate, deterministic fixed-order combine of the
    splits; bf16 weights: the combine rounds to bf16 itself, no cast pass)
    fold db out of the dz fragments they already hold in registers instead
    of a separate full re-read of dz. That fold adds fp32 atomically, so
    deterministic mode does not take it. Shapes on the 256 grid run the
    256-tile kernel; any other N % 8 == 0, K % 8 == 0 shape with M >= 256 and
    few enough output tiles the 128-tile kernel; of what that leaves, the
    ragged 256-tile kernel what its measured rule admits (_tn8pr_ok); the rest
    torch.matmul + colsum. JIMM_AMD_DW_RAGGED=1 puts the ragged kernel ahead
    of the 128-tile one, for every shape of its domain; 0 turns it off."""
    tn = need_dw and _gemm_mode() == "hip" and dz.dtype == torch.bfloat16
    fold = need_db and not _deterministic()
    ragged = _dw_ragged_mode()
    if tn and ext.gemm_tn8p_supported(dz.shape[0], dz.shape[1], x2.shape[1]):
        tn_dw, tn_dw_db = ext.gemm_tn_8p, ext.gemm_tn_8p_db
    elif tn and ragged == "1" and _tn8pr_ok(ext, dz, x2, fold, True):
        tn_dw, tn_dw_db = ext.gemm_tn_8p_ragged, ext.gemm_tn_8p_ragged_db
    elif tn and _tn128_ok(ext, dz, x2, fold):
        tn_dw, tn_dw_db = ext.gemm_tn_128, ext.gemm_tn_128_db
    elif tn and ragged != "0" and _tn8pr_ok(ext, dz, x2, fold, False):
        tn_dw, tn_dw_db = ext.gemm_tn_8p_ragged, ext.gemm_tn_8p_ragged_db
    else:
        tn = False
    if tn and fold:
        dw, db = tn_dw_db(dz, x2, 0, out_dtype == torch.bfloat16)
        return dw.to(out_dtype), db.to(dz.dtype)
    dw = db = None
    if tn and not need_db:
        dw = tn_dw(dz, x2, 0, out_dtype == torch.bfloat16).to(out_dtype)
    elif need_dw:
        dw = torch.matmul(dz.t(), x2)
    if need_db:
        db = _colsum(ext, dz)
    return dw, db


class _LinearActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, act, residual):
        in_f, out_f = w.shape[1], w.shape[0]
        x2 = x.contiguous().reshape(-1, in_f)
        res2 = residual.contiguous().reshape(-1, out_f) if residual is not None else None
        ext = _backend.ext()
        if _FP8_STATE["enabled"] and _fp8_ok(x2, w):
            if fp8_hip(ext, x2.shape[0], out_f, in_f):
                y, z, _ = gemm_fwd_f8(ext, *_quant_e4m3(x2), *_quant_e4m3(w), b, act, res2)
            else:
                z = _gemm_nt_fp8(x2, w)
                y = ext.bias_act_fwd(z, b, act or "", res2)
        else:
            hip = _gemm_mode() == "hip" and ext.gemm_supported(x2.shape[0], out_f, in_f, str(x2.dtype))
            # a contraction length off the 64 grid is served by no kernel
            # behind linear_fwd: the 128-tile NT kernel, within its K cap
            # ((201728, 384, 328) measured 0.158 ms against addmm's 0.168;
            # so400m's 4304 is beyond the cap and stays on rocBLAS)
            nt128 = (not hip and _gemm_mode() == "hip" and in_f % 64 != 0
                     and _nt128_ok(ext, x2, w, out_f))
            # the ragged 8-phase kernel takes what is left of that (K beyond
            # the cap: so400m's 4304) and the N % 256 != 0 shapes that
            # linear_fwd runs on the 128-tile kernels of gemm.hip, at or above
            # its row floor (profiles/nt_ragged_NOTES.md)
            nt8pr = (_gemm_mode() == "hip" and not nt128
                     and not ext.gemm8p_supported(x2.shape[0], out_f, in_f)
                     and _nt8pr_ok(ext, x2, w, out_f))
            if nt8pr:
                y, z = ext.gemm_nt_8p_ragged(x2, w, b, act or "", res2,
                                             "pre" if act is not None else "none")
            else:
                y, z = gemm_fwd(ext, x2, w, b, act, res2, hip=hip or nt128, nt128=nt128,
                                save="z" if act is not None else None)
        if act is not None:
            ctx.save_for_backward(x2, w, z)
        else:
            ctx.save_for_backward(x2, w)
        ctx.act = act
        ctx.has_bias = b is not None
        ctx.has_res = residual is not None
        ctx.res_shape = residual.shape if residual is not None else None
        ctx.x_shape = x.shape
        return y.view(*x.shape[:-1], out_f)

    @staticmethod
    def backward(ctx, dy):
        if ctx.act is not None:
            x2, w, z = ctx.saved_tensors
        else:
            x2, w = ctx.saved_tensors
        ext = _backend.ext()
        dy2 = dy.contiguous().reshape(-1, dy.shape[-1])
        dz = ext.act_bwd(dy2, z, ctx.act) if ctx.act is not None else dy2
        dx = gemm_dx(ext, dz, w).view(ctx.x_shape) if ctx.needs_input_grad[0] else None
        dw, db = gemm_dw_db(ext, dz, x2, w.dtype, ctx.needs_input_grad[1],
                            ctx.has_bias and ctx.needs_input_grad[2])
        dres = dy.view(ctx.res_shape) if (ctx.has_res and ctx.needs_input_grad[4]) else None
        return dx, dw, db, None, dres


def linear_act(x, w, b, act, residual):
    return _LinearActFn.apply(x, w, b, act, residual)


class _PatchEmbedFn(torch.autograd.Function):
    """K1: stride=kernel conv == im2col (pure gather) + NT GEMM + bias.

    im2col for kernel==stride is a permute-gather:
      img (B,C,h*P,w*P) -> cols (B*h*w, C*P*P), patch-major rows.
    The HIP kernel does the gather with coalesced writes; the GEMM against
    weight (hidden, C*P*P) reuses the linear path.
    """

    @staticmethod
    def forward(ctx, img, w, b, patch):
        B, C, H, W = img.shape
        h, wn = H // patch, W // patch
        ext = _backend.ext()
        cols = ext.im2col_patch(img.contiguous(), patch)  # (B*h*w, C*P*P)
        w2 = w.reshape(w.shape[0], -1).contiguous()  # (hidden, C*P*P)
        hip = (
            _gemm_mode() == "hip"
            and cols.dtype == torch.bfloat16
            and ext.gemm8p_supported(cols.shape[0], w2.shape[0], w2.shape[1])
        )
        if hip:
            y, _ = gemm_fwd(ext, cols, w2, b, None, None, hip=True)
        else:
            # not gemm_fwd's rocBLAS arm, whose bias-only case is addmm: this
            # path adds the bias in a separate pass, and its numbers stay
            y = ext.bias_act_fwd(torch.matmul(cols, w2.t()), b, "", None)
        ctx.save_for_backward(cols, w2)
        ctx.img_shape = img.shape
        ctx.patch = patch
        ctx.has_bias = b is not None
        ctx.w_shape = w.shape
        return y.view(B, h * wn, w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        cols, w2 = ctx.saved_tensors
        patch = ctx.patch
        ext = _backend.ext()
        dy2 = dy.contiguous().reshape(-1, dy.shape[-1])
        dimg = None
        if ctx.needs_input_grad[0]:
            dcols = gemm_dx(ext, dy2, w2)
            dimg = ext.col2im_patch(dcols, list(ctx.img_shape), patch)
        # dW alone, db by the separate colsum: this path does not use the
        # TN kernel's db fold
        dw, _ = gemm_dw_db(ext, dy2, cols, w2.dtype, ctx.needs_input_grad[1], need_db=False)
        db = _colsum(ext, dy2) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dimg, dw.view(ctx.w_shape) if dw is not None else None, db, None


def patch_embed(img, w, b, patch):
    return _PatchEmbedFn.apply(img, w, b, patch)
