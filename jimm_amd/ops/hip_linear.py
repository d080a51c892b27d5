"""GPU linear / patch-embed path, and the GEMM engine layer the fused encoder
block (ops/block.py) shares with it.

Two engines run a GEMM:
  * the in-house MFMA bf16 kernels: forward and dX on the NT kernels behind
    ``ext.linear_fwd`` (the 8-phase 256-tile kernel of csrc/gemm8p.hip where
    N % 256 == 0, K % 64 == 0 and K >= 128, else the 128-tile kernels of
    csrc/gemm.hip for any K % 64 == 0), with the bias / activation / residual /
    dropout epilogues and the activation backward fused into the GEMM; dW on
    the split-M TN kernel (csrc/gemm_tn8p.hip, fp32 accumulate, N % 256 == 0
    and K % 256 == 0), which can fold the bias gradient out of its operands;
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
fp8 arm (ops/block.py).
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

_FP8_STATE = {"enabled": False}
_FP8_MAX = 448.0  # e4m3 (OCP) max normal


def set_fp8(on: bool = True) -> None:
    _FP8_STATE["enabled"] = bool(on)


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


def _deterministic() -> bool:
    return os.environ.get("JIMM_AMD_DETERMINISTIC", "0") == "1"


# ---------------------------------------------------------------------------
# GEMM engine layer
# ---------------------------------------------------------------------------


def gemm_fwd(ext, x2, w, b, act, res2, *, hip: bool, save=None, drop=None):
    """y = act(x2 @ w^T + b) [+ res2] -> (y, saved). save: None, "z" (the
    bf16 pre-activation) or "g" (the fp16 derivative act'(pre), in-house
    engine only). drop = (p, rng, site): dropout fused into the in-house
    epilogue. hip is the caller's engine choice."""
    act = act or ""
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


def gemm_dx(ext, dz: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dX = dz @ w — in-house NT kernel on a pre-transposed weight copy.

    (Per-call-quantized fp8 dX was measured NET-NEGATIVE at config 5: the
    w.t().contiguous() + two quantization passes cost more than the fp8
    GEMM saves. The fused-block path instead runs fc1-dX on fp8 with a
    producer-emitted e4m3 operand — see ops/block.py.)"""
    if (
        _gemm_mode() == "hip"
        and dz.dtype == torch.bfloat16
        and ext.gemm8p_supported(dz.shape[0], w.shape[1], w.shape[0])
    ):
        wt = w.t().contiguous()
        y, _ = ext.linear_fwd(dz, wt, None, "", None, False)
        return y
    return torch.matmul(dz, w)


def gemm_dx_act(ext, dy2, w, saved, act, *, hip: bool) -> torch.Tensor:
    """dz = (dy2 @ w) * act'(pre), the dX of an activated linear, from what
    its forward saved: the fp16 derivative (one multiply in the epilogue), or
    the bf16 pre-activation — the derivative recomputed in the epilogue where
    the caller's engine is the in-house one (hip) and the 8-phase kernel
    takes the shape, else rocBLAS + a separate act_bwd pass."""
    if saved.dtype == torch.float16:
        return ext.gemm_nt_8p_gradmul(dy2, w.t().contiguous(), saved)
    if hip and ext.gemm8p_supported(dy2.shape[0], w.shape[1], w.shape[0]):
        return ext.gemm_nt_8p_gradact(dy2, w.t().contiguous(), saved, act)
    return ext.act_bwd(torch.matmul(dy2, w), saved, act)


def _colsum(ext, dz: torch.Tensor) -> torch.Tensor:
    """The bias gradient on its own: one fp32-accumulating pass over dz."""
    if dz.is_cuda and dz.shape[-1] % 8 == 0:
        return ext.colsum(dz).to(dz.dtype)
    return dz.sum(dim=0)


def gemm_dw_db(ext, dz, x2, out_dtype, need_dw: bool = True, need_db: bool = True):
    """(dW = dz^T @ x2 | None, db = colsum(dz) | None). The in-house split-M
    TN kernel (fp32 accumulate, deterministic fixed-order combine of the
    splits; bf16 weights: the combine rounds to bf16 itself, no cast pass)
    folds db out of the dz fragments it already holds in registers instead
    of a separate full re-read of dz. That fold adds fp32 atomically, so
    deterministic mode does not take it."""
    tn = (
        need_dw
        and _gemm_mode() == "hip"
        and dz.dtype == torch.bfloat16
        and ext.gemm_tn8p_supported(dz.shape[0], dz.shape[1], x2.shape[1])
    )
    if tn and need_db and not _deterministic():
        dw, db = ext.gemm_tn_8p_db(dz, x2, 0, out_dtype == torch.bfloat16)
        return dw.to(out_dtype), db.to(dz.dtype)
    dw = db = None
    if tn and not need_db:
        dw = ext.gemm_tn_8p(dz, x2, 0, out_dtype == torch.bfloat16).to(out_dtype)
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
            z = _gemm_nt_fp8(x2, w)
            y = ext.bias_act_fwd(z, b, act or "", res2)
        else:
            hip = _gemm_mode() == "hip" and ext.gemm_supported(x2.shape[0], out_f, in_f, str(x2.dtype))
            y, z = gemm_fwd(ext, x2, w, b, act, res2, hip=hip, save="z" if act is not None else None)
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
        dcols = gemm_dx(ext, dy2, w2)
        dimg = ext.col2im_patch(dcols, list(ctx.img_shape), patch) if ctx.needs_input_grad[0] else None
        # dW alone, db by the separate colsum: this path does not use the
        # TN kernel's db fold
        dw, _ = gemm_dw_db(ext, dy2, cols, w2.dtype, ctx.needs_input_grad[1], need_db=False)
        db = _colsum(ext, dy2) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dimg, dw.view(ctx.w_shape) if dw is not None else None, db, None


def patch_embed(img, w, b, patch):
    return _PatchEmbedFn.apply(img, w, b, patch)
