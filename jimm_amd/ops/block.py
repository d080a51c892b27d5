"""Whole-encoder-block autograd Function (GPU fast path).

The composite EncoderBlock (models/common/transformer.py) is numerically
identical but lets autograd insert two full-tensor grad-accumulation adds
per block (the residual branches: x feeds both LN1 and the attention
residual; a feeds both LN2 and the MLP residual — ~1.1 ms/step for ViT-B
bs256, profiles/r01_NOTES.md). Here the block is one Function and those
adds ride the ln_bwd kernel's fused ``addend`` input for free. The default
path runs every GEMM on the in-house MFMA kernels with the bias / act /
residual / act-backward epilogues fused in; under ``set_fp8(True)`` (and
past the M*H size gate) the forward GEMMs and fc1-dX run e4m3 with
producer-fused quantization and per-block delayed scaling.

Active dropout (training, p > 0) stays on this path where the bf16 HIP GEMMs
take both MLP shapes: the fc1 and fc2 epilogues compute the counter-based
masks (ops/philox_dropout.py) in registers, fc1 saves the masked derivative,
and the backward regenerates the fc2-site mask on dy with one elementwise
pass. Otherwise the composite path (the reference and the CPU path) runs
with ops.dropout. JIMM_AMD_FUSED_BLOCK=0 disables.
"""

from __future__ import annotations

import os

import torch

from jimm_amd.ops import _backend
from jimm_amd.ops.functional import _split_heads
from jimm_amd.ops.hip_linear import (
    _FP8_STATE,
    _gemm_mode,
    _quant_e4m3,
    gemm_dw_db,
    gemm_dx,
    gemm_dx_act,
    gemm_fwd,
)
from jimm_amd.ops.philox_dropout import dropout_threshold


def _hip_gemms(H: int, mlp_dim: int) -> bool:
    """True when the encoder block's forward GEMMs run on the in-house MFMA
    kernels (JIMM_AMD_GEMM=hip, the default): H % 256 == 0 puts qkv, proj and
    fc2 (N = 3H, H, H) on the 8-phase kernel, and every K (H or mlp_dim)
    must be a multiple of 64 for any of them. fc1 (N = mlp_dim) takes the
    128-tile kernels where mlp_dim % 256 != 0."""
    return _gemm_mode() == "hip" and H % 256 == 0 and mlp_dim % 64 == 0


def _act_save_g() -> bool:
    """What the bf16 HIP path keeps of fc1 for the backward: the fp16
    activation derivative g = act'(z1), computed by the forward epilogue from
    values it already holds, so that fc2-dX is left with one multiply
    (default), or, with JIMM_AMD_ACT_SAVE=z, the bf16 pre-activation z1,
    from which the fc2-dX epilogue recomputes the derivative (A/B)."""
    return os.environ.get("JIMM_AMD_ACT_SAVE", "g") != "z"


# minimum rows x hidden for the fp8 block path (tests lower it to force fp8)
_FP8_MIN_MH = 1 << 26


def _fp8_block_state(mod: torch.nn.Module, device: torch.device):
    """Per-block delayed-scaling state, 4 sites: [0] h1->qkv, [1] h2->fc1,
    [2] f->fc2 (forward), [3] dz1->fc1-dX (backward). scale8 is what this
    step's producers divide by; amax collected this step becomes next
    step's scale (scale8[0:3] updated at forward end, [3] at backward
    end). The grad site starts at 1/448 (assume amax~1; adapts in one
    step) so first-step gradients are not flushed to zero."""
    st = getattr(mod, "_fp8_state", None)
    if st is None or st[0].device != device:
        scale = torch.ones(4, device=device, dtype=torch.float32)
        scale[3] = 1.0 / 448.0
        st = (scale, torch.zeros(4, device=device, dtype=torch.float32))
        mod._fp8_state = st
    return st


def _mm_fp8q(y8: torch.Tensor, s: torch.Tensor, w: torch.Tensor,
             bias: torch.Tensor | None = None) -> torch.Tensor:
    """GEMM on a producer-emitted e4m3 activation (uint8 bytes + its scale)
    against a per-call-quantized e4m3 weight; bias fused in the hipBLASLt
    epilogue; bf16 out."""
    w8, sw = _quant_e4m3(w)
    return torch._scaled_mm(
        y8.view(torch.float8_e4m3fn), w8.t(), scale_a=s.view(1, 1),
        scale_b=sw.view(1, 1), bias=bias, out_dtype=torch.bfloat16,
    )


def _fused_dropout_ok(x: torch.Tensor, dropout_p: float, mlp_dim: int | None) -> bool:
    """Active dropout stays on the fused block where both MLP GEMMs run the
    8-phase kernel (its fc1 / fc2 epilogues compute the masks) and fc1 saves
    the fp16 derivative, which then carries the activation-site mask to the
    backward. p so close to 1 that s * act' leaves fp16 is not taken."""
    if mlp_dim is None or _gemm_mode() != "hip" or not _act_save_g() or _FP8_STATE["enabled"]:
        return False
    if dropout_threshold(dropout_p) > 65000:
        return False
    M, H = x.numel() // x.shape[-1], x.shape[-1]
    ext = _backend.ext()
    return ext.gemm8p_supported(M, mlp_dim, H) and ext.gemm8p_supported(M, H, mlp_dim)


def fused_block_enabled(x: torch.Tensor, dropout_p: float, mlp_dim: int | None = None) -> bool:
    """dropout_p is the ACTIVE probability (0 in eval mode); with p > 0 the
    caller passes the MLP width so the GEMM shapes can be checked."""
    return (
        x.is_cuda
        and x.dtype == torch.bfloat16
        and _backend.use_hip(x)
        and os.environ.get("JIMM_AMD_FUSED_BLOCK", "1") == "1"
        and (dropout_threshold(dropout_p) == 0 or _fused_dropout_ok(x, dropout_p, mlp_dim))
    )


class EncoderBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(
        ctx, x, ln1w, ln1b, wqkv, bqkv, wproj, bproj, ln2w, ln2b, w1, b1, w2, b2,
        scale8, amax8,
        num_heads: int, act: str, eps: float, causal: bool, scale: float,
        p: float = 0.0, rng: torch.Tensor | None = None, site0: int = 0,
    ):
        ext = _backend.ext()
        B, L, H = x.shape
        x = x.contiguous()
        x2 = x.view(-1, H)
        # the engine of every bf16 GEMM below: the in-house MFMA kernels with
        # the bias / act / residual epilogues fused into the GEMM kernel
        # itself, or rocBLAS + the fused elementwise pass (gemm_fwd)
        hip = _hip_gemms(H, w1.shape[0])
        # active dropout: site0 after the activation, site0 + 1 after fc2,
        # both under the {seed, step} snapshot rng (fused_block_enabled has
        # checked that the bf16 HIP save-g path below takes these shapes)
        drop = dropout_threshold(p) > 0
        if not drop:
            p, rng = 0.0, None

        # Producer-fused fp8 (BASELINE config 5): LN / bias-act kernels emit
        # the e4m3 copy of their output alongside bf16 (one extra store, no
        # standalone quantization pass) using last step's per-site scale;
        # this step's amax feeds next step's scale (delayed scaling, all
        # device-side — graph-safe). Backward stays bf16 on the saved
        # activations. Sites: h1->qkv, h2->fc1, f->fc2; proj keeps the bf16
        # fused-residual GEMM (its input o comes from attention, not from a
        # producer kernel we control cheaply).
        # fp8 pays only when the tower's GEMMs are big enough to amortize
        # the per-call weight quantization and producer-kernel emission.
        # M*H separates the measured winners from the losers: ViT-L
        # 73856x1024 (+5%) and ViT-B 201728x768 (+8%) win; CLIP-B/32
        # vision 51200x768, CLIP text 78848x512 and SigLIP text 32768x768
        # all lose — those towers stay on the fused bf16 path even under
        # set_fp8(True).
        fp8 = (
            scale8 is not None
            and x.dtype == torch.bfloat16
            and H % 64 == 0
            and H <= 2048
            and B * L * H > _FP8_MIN_MH
            and hasattr(torch, "_scaled_mm")
        )
        if drop and (fp8 or not hip):
            raise RuntimeError("fused block: dropout runs on the bf16 HIP GEMM path only")
        if fp8:
            amax8.zero_()
            h1, h1q, mean1, rstd1 = ext.layernorm_fwd_fp8(
                x, ln1w, ln1b, eps, scale8[0:1], amax8[0:1]
            )
            qkv2 = _mm_fp8q(h1q, scale8[0:1], wqkv, bias=bqkv)
        else:
            h1, mean1, rstd1 = ext.layernorm_fwd(x, ln1w, ln1b, eps)
            qkv2, _ = gemm_fwd(ext, h1.view(-1, H), wqkv, bqkv, None, None, hip=hip)  # (M, 3H)
        qkv = qkv2.view(B, L, 3, num_heads, H // num_heads)
        o, lse = ext.attn_fwd(*_split_heads(qkv), causal, scale)  # (B,nh,L,d), (B,L,nh,d) storage
        o2 = o.transpose(1, 2).reshape(-1, H)                    # free view
        a, _ = gemm_fwd(ext, o2, wproj, bproj, None, x2, hip=hip)  # + bias + residual
        a3 = a.view(B, L, H)
        if fp8:
            h2, h2q, mean2, rstd2 = ext.layernorm_fwd_fp8(
                a3, ln2w, ln2b, eps, scale8[1:2], amax8[1:2]
            )
            z1 = _mm_fp8q(h2q, scale8[1:2], w1, bias=b1)  # z1 = pre-act (bias fused)
            f, f8 = ext.bias_act_fwd_fp8(z1, None, act, scale8[2:3], amax8[2:3])
            y = ext.bias_act_fwd(_mm_fp8q(f8, scale8[2:3], w2, bias=b2), None, "", a)
            # next step's forward scales (delayed); grad sites [3:5] are
            # updated at backward end, after their amax is collected
            scale8[0:3].copy_(torch.clamp(amax8[0:3] / 448.0, min=1e-12))
        else:
            h2, mean2, rstd2 = ext.layernorm_fwd(a3, ln2w, ln2b, eps)
            # fc2-dX runs as (M, mlp, H); where the 8-phase kernel takes it,
            # z1 holds the fp16 derivative act'(pre) instead of the
            # pre-activation (nothing else reads z1)
            save_g = hip and _act_save_g() and ext.gemm8p_supported(B * L, w1.shape[0], H)
            if drop and not save_g:
                raise RuntimeError("fused block: dropout needs the saved-derivative fc1 path")
            # with dropout f = act(z)*m*s and z1 = act'(z)*m*s: the mask of
            # site0 reaches the backward inside the saved derivative
            f, z1 = gemm_fwd(ext, h2.view(-1, H), w1, b1, act, None, hip=hip,
                             save="g" if save_g else "z", drop=(p, rng, site0) if drop else None)
            # y = a + m*s*(f @ w2^T + b2) at site0 + 1
            y, _ = gemm_fwd(ext, f, w2, b2, None, a, hip=hip,
                            drop=(p, rng, site0 + 1) if drop else None)
        ctx.save_for_backward(x, ln1w, wqkv, wproj, ln2w, w1, w2,
                              h1, qkv, o, lse, a, mean1, rstd1, mean2, rstd2, h2, z1, f, rng)
        ctx.dims = (B, L, H, num_heads)
        ctx.meta = (act, causal, scale)
        ctx.drop = (p, site0)
        ctx.fp8_state = (scale8, amax8) if fp8 else None
        return y.view(B, L, H)

    @staticmethod
    def backward(ctx, dy):
        ext = _backend.ext()
        (x, ln1w, wqkv, wproj, ln2w, w1, w2,
         h1, qkv, o, lse, a, mean1, rstd1, mean2, rstd2, h2, z1, f, rng) = ctx.saved_tensors
        B, L, H, nh = ctx.dims
        act, causal, scale = ctx.meta
        p, site0 = ctx.drop
        dy2 = dy.contiguous().view(-1, H)
        # dropout after fc2: its backward regenerates the mask on dy. dyd
        # feeds fc2's dX, dW and db; the residual branch (the LN2 addend
        # below) keeps the undropped dy.
        dyd = ext.dropout_fwd(dy2, p, rng, site0 + 1) if rng is not None else dy2
        h1_2 = h1.view(-1, H)
        h2_2 = h2.view(-1, H)
        hip = _hip_gemms(H, w1.shape[0])
        fp8 = ctx.fp8_state is not None and hip

        # MLP fc2 (+residual into a)
        if fp8:
            scale8, amax8 = ctx.fp8_state
            # gradact dX with fused e4m3 emission of dz1; the fc1-dX GEMM
            # (dh2 = dz1 @ W1) then runs on the fp8 MFMA pipe
            dz1, dz18 = ext.gemm_nt_8p_gradact_fp8(
                dy2, w2.t().contiguous(), z1, act, scale8[3:4], amax8[3:4]
            )
        else:
            # z1 is the saved fp16 g = act'(pre) (times the activation-site
            # dropout mask, if any): dz1 = (dyd @ W2) * g; or the bf16
            # pre-activation: dz1 = (dy @ W2) * act'(z1), recomputed in the
            # GEMM epilogue or in a separate act_bwd pass
            dz1 = gemm_dx_act(ext, dyd, w2, z1, act, hip=hip)
        dw2, db2 = gemm_dw_db(ext, dyd, f, w2.dtype)
        if fp8:
            w1t8, sw1 = _quant_e4m3(w1, transpose=True)
            dh2 = torch._scaled_mm(
                dz18.view(torch.float8_e4m3fn), w1t8.t(), scale_a=scale8[3:4].view(1, 1),
                scale_b=sw1.view(1, 1), out_dtype=torch.bfloat16,
            )
        else:
            dh2 = gemm_dx(ext, dz1, w1)
        dw1, db1 = gemm_dw_db(ext, dz1, h2_2, w1.dtype)
        # LN2 backward with the MLP residual grad (dy) fused into dx
        da3, dln2w, dln2b = ext.layernorm_bwd(
            dh2.view(B, L, H), a.view(B, L, H), ln2w, mean2, rstd2, dy.contiguous()
        )
        da2 = da3.view(-1, H)

        # attention out-projection
        do2 = gemm_dx(ext, da2, wproj)
        dwproj, dbproj = gemm_dw_db(ext, da2, o.transpose(1, 2).reshape(-1, H), wproj.dtype)
        do_v = do2.view(B, L, nh, H // nh).permute(0, 2, 1, 3)   # (B,nh,L,d) strided view

        # fused flash attention backward straight into the strided dqkv
        dqkv = torch.empty_like(qkv)
        ext.attn_bwd_fused(*_split_heads(qkv), o, do_v, lse, *_split_heads(dqkv), causal, scale)
        dqkv2 = dqkv.view(-1, 3 * H)

        # QKV projection. (qkv-dX stays bf16: quantizing dqkv needs a
        # standalone cast pass — measured a wash vs the fp8 GEMM saving,
        # and it costs dx accuracy. fc1-dX gets its e4m3 operand free from
        # the gradact epilogue, so only that dX runs fp8.)
        dh1 = gemm_dx(ext, dqkv2, wqkv)
        dwqkv, dbqkv = gemm_dw_db(ext, dqkv2, h1_2, wqkv.dtype)
        # LN1 backward with the attention residual grad (da) fused into dx
        dx, dln1w, dln1b = ext.layernorm_bwd(
            dh1.view(B, L, H), x, ln1w, mean1, rstd1, da3
        )
        if fp8:
            # next step's backward scale (delayed)
            scale8[3:4].copy_(torch.clamp(amax8[3:4] / 448.0, min=1e-12))
        return (dx, dln1w, dln1b, dwqkv, dbqkv, dwproj, dbproj, dln2w, dln2b,
                dw1, db1, dw2, db2, None, None, None, None, None, None, None,
                None, None, None)


def encoder_block(x, norm1, qkv, proj, norm2, fc1, fc2, *, num_heads, act, eps, causal, scale,
                  p=0.0, rng=None, site0=0):
    scale8 = amax8 = None
    if _FP8_STATE["enabled"] and x.is_cuda and x.dtype == torch.bfloat16:
        scale8, amax8 = _fp8_block_state(norm1, x.device)
    return EncoderBlockFn.apply(
        x, norm1.weight, norm1.bias, qkv.weight, qkv.bias, proj.weight, proj.bias,
        norm2.weight, norm2.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias,
        scale8, amax8,
        num_heads, act, eps, causal, scale, p, rng, site0,
    )
