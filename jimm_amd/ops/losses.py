"""Training losses (K13) with the distributed variants (C3) and the fused
similarity-head kernels (K12).

The reference ships only the classification CE (examples/vit_training.py:76);
the contrastive / sigmoid losses are implied by the CLIP/SigLIP similarity
heads (models/clip.py:180-188, models/siglip.py:166-174) and the papers.

GPU path: row L2-normalize, softmax-CE over the contrastive logit block and
the SigLIP pairwise sigmoid loss run as HIP kernels (csrc/losses.hip); the
logit GEMMs run through rocBLAS. CPU path is the fp32 torch reference.

fused=True (off by default) takes the logit GEMM in-house as well: the block
is computed on MFMA tiles and consumed in the epilogue (csrc/simloss.hip), so
no logits are stored, in either direction.
"""

from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn.functional as F

from jimm_amd.ops import _backend, hip_linear
from jimm_amd.parallel.gather import all_gather_with_grad


def softmax_cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Mean CE with integer labels (examples/vit_training.py:60-78)."""
    if _backend.use_hip(logits):
        return _XentRowsFn.apply(logits.float(), labels)
    return F.cross_entropy(logits.float(), labels)


# ---------------------------------------------------------------------------
# K12 — row L2 normalize
# ---------------------------------------------------------------------------


class _L2NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y, rinv = _backend.ext().l2norm_fwd(x)
        ctx.save_for_backward(x, rinv)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, rinv = ctx.saved_tensors
        return _backend.ext().l2norm_bwd(dy, x, rinv)


def l2norm(x: torch.Tensor) -> torch.Tensor:
    if _backend.use_hip(x) and x.dim() == 2:
        return _L2NormFn.apply(x)
    return x / x.norm(dim=-1, keepdim=True)


# ---------------------------------------------------------------------------
# K13 — fused softmax-CE over logit rows (HIP fwd/bwd, mean over rows)
# ---------------------------------------------------------------------------


class _XentRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        logits = logits.contiguous()
        loss, lse = _backend.ext().xent_rows_fwd(logits, labels)
        ctx.save_for_backward(logits, labels, lse)
        return loss.mean()

    @staticmethod
    def backward(ctx, g):
        logits, labels, lse = ctx.saved_tensors
        dlogits = _backend.ext().xent_rows_bwd(logits, labels, lse, 1.0 / logits.shape[0])
        return dlogits * g, None


class _SigmoidLossFn(torch.autograd.Function):
    """loss_sum = sum_ij -logsigmoid(z_ij * logits_ij), z = +1 at col diag0+i."""

    @staticmethod
    def forward(ctx, logits, diag0):
        logits = logits.contiguous()
        loss, dlogits = _backend.ext().sigmoid_loss_ew(logits, diag0)
        ctx.save_for_backward(dlogits)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None


# ---------------------------------------------------------------------------
# K12 — fused similarity head: loss over scale * a @ b_all^T (+ bias) without
# a stored logit block (csrc/simloss.hip)
# ---------------------------------------------------------------------------

_SIM_MODES = {"softmax": 0, "sigmoid": 1}


def _sim_residual(x: torch.Tensor, lse, diag0: int, start: int, mode: str) -> torch.Tensor:
    """r = dloss/dx of the column chunk starting at `start` (torch arm):
    softmax - onehot, or -z * sigmoid(-z * x); labels at column diag0 + m."""
    m = torch.arange(x.shape[0], device=x.device)
    col = m + (diag0 - start)
    own = (col >= 0) & (col < x.shape[1])
    if mode == "softmax":
        r = torch.exp(x - lse[:, None])
        r[m[own], col[own]] -= 1.0
        return r
    z = torch.full_like(x, -1.0)
    z[m[own], col[own]] = 1.0
    return -z * torch.sigmoid(-z * x)


class _SimLossFn(torch.autograd.Function):
    """The loss of the (M, N) block x = scale * a @ b_all^T (+ bias), row m's
    label at column diag0 + m: mean over rows of the softmax CE ("softmax"), or
    sum_mn -logsigmoid(z * x) ("sigmoid"). Nothing of size M x N is kept: the
    forward reduces the block tile by tile, the backward recomputes it in
    column chunks of chunk_size, one bf16 G = coef * scale * r per chunk, and
    feeds G to the two backward GEMMs of the engine layer (ops/hip_linear.py).

    Inputs outside ext.sim_supported (CPU tensors, fp32, D % 64 != 0) run the
    torch arm: the same chunk algorithm in fp32 torch ops."""

    @staticmethod
    def forward(ctx, a, b_all, scale, bias, diag0, mode, chunk_size):
        M, D = a.shape
        N = b_all.shape[0]
        hip = (
            _backend.use_hip(a)
            and a.dtype == b_all.dtype
            and _backend.ext().sim_supported(M, N, D, str(a.dtype))
        )
        ctx.hip, ctx.diag0, ctx.mode, ctx.chunk = hip, int(diag0), mode, max(int(chunk_size), 1)
        ctx.has_bias = bias is not None
        a = a.contiguous()
        b_all = b_all.contiguous()
        # fp32 device scalars: what the kernels read through a pointer
        s32 = scale.detach().float().reshape(1)
        b32 = bias.detach().float().reshape(1) if bias is not None else None
        lse = None
        if hip:
            ext = _backend.ext()
            if mode == "softmax":
                lse, pos = ext.sim_lse_fwd(a, b_all, s32, ctx.diag0)
                out = (lse - pos).mean()
            else:
                out = ext.sim_sigmoid_fwd(a, b_all, s32, b32, ctx.diag0)[0]
        else:
            out, lse = _SimLossFn._torch_fwd(a, b_all, s32, b32, ctx.diag0, mode, ctx.chunk)
        ctx.save_for_backward(a, b_all, scale, bias, lse)
        return out

    @staticmethod
    def _torch_fwd(a, b_all, s32, b32, diag0, mode, chunk):
        M, N = a.shape[0], b_all.shape[0]
        a32 = a.float()
        rows = torch.arange(M, device=a.device)
        if mode == "sigmoid":
            total = a32.new_zeros(())
            for start in range(0, N, chunk):
                x = s32 * (a32 @ b_all[start : start + chunk].float().t()) + b32
                z = torch.full_like(x, -1.0)
                col = rows + (diag0 - start)
                own = (col >= 0) & (col < x.shape[1])
                z[rows[own], col[own]] = 1.0
                total = total - F.logsigmoid(z * x).sum()
            return total, None
        if diag0 < 0 or diag0 + M > N:
            raise ValueError(f"labels {diag0} .. {diag0 + M - 1} outside the {N} columns")
        # running (max, sum exp) over the chunks, merged as the kernels merge
        # their 64-column groups
        mx = a32.new_full((M,), float("-inf"))
        sm = a32.new_zeros((M,))
        pos = a32.new_zeros((M,))
        for start in range(0, N, chunk):
            x = s32 * (a32 @ b_all[start : start + chunk].float().t())
            cm = x.max(dim=1).values
            nm = torch.maximum(mx, cm)
            sm = sm * torch.exp(mx - nm) + torch.exp(x - nm[:, None]).sum(dim=1)
            mx = nm
            col = rows + (diag0 - start)
            own = (col >= 0) & (col < x.shape[1])
            pos[own] = x[rows[own], col[own]]
        lse = mx + torch.log(sm)
        return (lse - pos).mean(), lse

    @staticmethod
    def backward(ctx, g):
        a, b_all, scale, bias, lse = ctx.saved_tensors
        M, N = a.shape[0], b_all.shape[0]
        mode = ctx.mode
        s32 = scale.detach().float().reshape(1)
        b32 = bias.detach().float().reshape(1) if ctx.has_bias else None
        # upstream gradient -> per-element coefficient, on the device
        coef = (g.float() / M if mode == "softmax" else g.float()).reshape(1)
        starts = range(0, N, ctx.chunk)
        dB = torch.empty_like(b_all)
        dA32 = None
        dscale = coef.new_zeros(1)
        dbias = coef.new_zeros(1)
        ext = _backend.ext() if ctx.hip else None
        for start in starts:
            b_chunk = b_all[start : start + ctx.chunk]
            if ctx.hip:
                G, ds, db = ext.sim_grad(a, b_chunk, s32, b32, lse, coef, ctx.diag0 - start,
                                         _SIM_MODES[mode])
                dA = hip_linear.gemm_dx(ext, G, b_chunk)
                dB[start : start + ctx.chunk] = hip_linear.gemm_dw_db(
                    ext, G, a, b_all.dtype, need_db=False)[0]
            else:
                acc = a.float() @ b_chunk.float().t()
                x = s32 * acc if b32 is None else s32 * acc + b32
                r = _sim_residual(x, lse, ctx.diag0, start, mode)
                G = (coef * s32) * r
                ds, db = coef * (r * acc).sum(), coef * r.sum()
                dA = G @ b_chunk.float()
                dB[start : start + ctx.chunk] = (G.t() @ a.float()).to(dB.dtype)
            if len(starts) == 1:
                dA32 = dA
            else:  # fp32 accumulation across the chunks
                dA32 = dA.float() if dA32 is None else dA32.add_(dA)
            dscale = dscale + ds
            dbias = dbias + db
        dscale = dscale.reshape(scale.shape).to(scale.dtype)
        dbias = dbias.reshape(bias.shape).to(bias.dtype) if ctx.has_bias else None
        return dA32.to(a.dtype), dB, dscale, dbias, None, None, None


def fused_similarity_loss(a, b_all, scale, bias, diag0: int, mode: str, chunk_size: int = 8192):
    """See _SimLossFn. mode: "softmax" (bias must be None) or "sigmoid"."""
    if mode not in _SIM_MODES:
        raise ValueError(f"mode must be one of {sorted(_SIM_MODES)}, got {mode!r}")
    if (bias is None) != (mode == "softmax"):
        raise ValueError("the softmax mode takes no bias, the sigmoid mode needs one")
    return _SimLossFn.apply(a, b_all, scale, bias, diag0, mode, chunk_size)


# ---------------------------------------------------------------------------
# C3 — distributed contrastive / sigmoid losses
# ---------------------------------------------------------------------------


def clip_contrastive_loss(
    img_emb: torch.Tensor,
    txt_emb: torch.Tensor,
    logit_scale: torch.Tensor,
    *,
    group=None,
    gather: bool = True,
    fused: bool = False,
    chunk_size: int = 8192,
) -> torch.Tensor:
    """Symmetric InfoNCE over the GLOBAL batch.

    Both towers' embeddings are all-gathered (with grad); each rank computes
    its local-rows x global-cols logit blocks; CE is averaged over local
    rows, so the DP gradient average yields the global-batch mean loss.

    fused: the two logit blocks are never stored (K12, _SimLossFn); the
    backward recomputes them in column chunks of chunk_size.
    """
    img = l2norm(img_emb)
    txt = l2norm(txt_emb)
    scale = logit_scale.exp()
    b_local = img.shape[0]
    do_gather = gather and dist.is_initialized()
    rank = dist.get_rank(group) if do_gather else 0
    img_all = all_gather_with_grad(img, group) if do_gather else img
    txt_all = all_gather_with_grad(txt, group) if do_gather else txt
    if fused:
        diag0 = rank * b_local
        loss_i = fused_similarity_loss(img, txt_all, scale, None, diag0, "softmax", chunk_size)
        loss_t = fused_similarity_loss(txt, img_all, scale, None, diag0, "softmax", chunk_size)
        return 0.5 * (loss_i + loss_t)
    labels = torch.arange(b_local, device=img.device) + rank * b_local
    logits_i = scale * img @ txt_all.t()  # (B_local, B_global)
    logits_t = scale * txt @ img_all.t()
    return 0.5 * (softmax_cross_entropy(logits_i, labels) + softmax_cross_entropy(logits_t, labels))


def siglip_sigmoid_loss(
    img_emb: torch.Tensor,
    txt_emb: torch.Tensor,
    logit_scale: torch.Tensor,
    logit_bias: torch.Tensor,
    *,
    group=None,
    gather: bool = True,
    chunk_size: int = 8192,
    fused: bool = False,
) -> torch.Tensor:
    """SigLIP pairwise sigmoid loss over the global batch.

    loss = -1/B_global * sum_{i,j} log sigmoid(z_ij * (s*sim_ij + b)),
    z_ij = +1 for matching pairs else -1. Per rank we compute the
    (B_local, B_global) block in column chunks (global batch 32k per
    BASELINE.json config 4 would otherwise materialize 4 GB fp32 logits),
    normalized by B_local so the DP mean reproduces the paper's 1/B_global.

    fused: no logit chunk is stored either (K12, _SimLossFn): one forward
    launch over the whole block, and chunk_size chunks the backward only.
    """
    img = l2norm(img_emb)
    txt = l2norm(txt_emb)
    scale = logit_scale.exp()
    b_local = img.shape[0]
    do_gather = gather and dist.is_initialized()
    rank = dist.get_rank(group) if do_gather else 0
    txt_all = all_gather_with_grad(txt, group) if do_gather else txt
    if fused:
        total = fused_similarity_loss(img, txt_all, scale, logit_bias, rank * b_local, "sigmoid",
                                      chunk_size)
        return total / b_local
    b_global = txt_all.shape[0]
    use_hip = _backend.use_hip(img)
    diag = torch.arange(b_local, device=img.device)
    total = img.new_zeros((), dtype=torch.float32)
    for start in range(0, b_global, chunk_size):
        cols = txt_all[start : start + chunk_size]
        logits = scale * img @ cols.t() + logit_bias  # (B_local, <=chunk)
        if use_hip:
            total = total + _SigmoidLossFn.apply(logits.float(), rank * b_local - start)
            continue
        z = torch.full_like(logits, -1.0)
        # own positives live at global columns rank*b_local + i
        lo, hi = rank * b_local, rank * b_local + b_local
        if start < hi and lo < start + cols.shape[0]:
            i0 = max(lo, start) - lo
            i1 = min(hi, start + cols.shape[0]) - lo
            z[diag[i0:i1], diag[i0:i1] + lo - start] = 1.0
        total = total - F.logsigmoid(z * logits.float()).sum()
    return total / b_local
